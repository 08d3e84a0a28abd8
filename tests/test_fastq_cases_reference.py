"""The yardstick of tests/test_gpu_fastq_cases.py, checked without a GPU: the byte-level FASTQ reference of
tests/fastq_cases_common.py against hand-written records, against the oracle's reader and the package's Python reader, and -- for
every case and container of the table -- against the native host parser (kv_fastx.hip); the packing rules on hand-packed reads; and
that the table holds the edges it says it holds, computed from the constants of kv_fastq.hip."""
import gzip
import os

import numpy as np
import pytest

import fastq_cases_common as fc

C = fc.C
CASES = fc.cases()

LITERALS = [
    (b'@r1\nACGT\n+\nIIII\n', [(b'r1', b'ACGT', b'IIII')]),
    (b'@r1\nACGT\n+\nIIII', [(b'r1', b'ACGT', b'IIII')]),                                        # no newline behind the last line
    (b'@r1 x\nAC\n+r1 x\nII\n\n', [(b'r1 x', b'AC', b'II')]),                                    # the tails: one blank line,
    (b'@r1\nAC\n+\nII\n\r\n \n', [(b'r1', b'AC', b'II')]),                                       # blank lines of \r and blanks,
    (b'@r1\nAC\n+\nII\n\n\n\n\n', [(b'r1', b'AC', b'II')]),                                      # four of them,
    (b'@r1\nAC\n+\nII\n \t\n\r\n\n\t\t \r\n@r2\nG\n+\nJ\n', [(b'r1', b'AC', b'II'), (b'r2', b'G', b'J')]),   # and between records
    (b'@r1\nAC\n+\nII\n@r2\n', [(b'r1', b'AC', b'II'), (b'r2', b'', b'')]),                      # the file stops after a name,
    (b'@r1\nAC\n+\nII\n@r2\nGG', [(b'r1', b'AC', b'II'), (b'r2', b'GG', b'')]),                  # a sequence,
    (b'@r1\nAC\n+\nII\n@r2\nGG\n+\n', [(b'r1', b'AC', b'II'), (b'r2', b'GG', b'')]),             # a plus line
    (b'@r1\r\nAC\r\n+\r\nII\r\n@r2\r\nG\r\n+\r\nJ\r\n', [(b'r1', b'AC', b'II'), (b'r2', b'G', b'J')]),       # CRLF
    (b'@r1\nAC\r\n+\nII\n', [(b'r1', b'AC', b'II')]),                                            # \r on one line only
    (b'@r1\nAC\r\r\n+\nII\n', [(b'r1', b'AC\r', b'II')]),                                        # one \r goes, not two
    (b'@r1\nAC\n+\n@I\n@r2\nG\n+\n+\n', [(b'r1', b'AC', b'@I'), (b'r2', b'G', b'+')]),           # '@' and '+' open a quality line
    (b'@r1\n\n+\n\n@\n\r\n+\n\n', [(b'r1', b'', b''), (b'', b'', b'')]),                         # no bases; no name either
    (b'@\xff\x0b\x8a\nacgtN\n+\n!~\x1a\n', [(b'\xff\x0b\x8a', b'acgtN', b'!~\x1a')]),            # bytes pass as they are
    (b'', []),
    (b'\n \n', []),
]


@pytest.mark.parametrize('data,want', LITERALS)
def test_reference_gives_the_hand_written_records(data, want):
    assert fc.parse_fastx(data) == want


def test_reference_refuses_what_opens_no_record():
    with pytest.raises(ValueError):
        fc.parse_fastx(b'@r1\nAC\n+\nII\nAC\n')


def test_packing_rules_on_hand_packed_reads():
    # base j in bits 2 (j mod 16): ACGT = 0 1 2 3
    assert list(fc.pack_words([b'ACGT'])) == [0 | 1 << 2 | 2 << 4 | 3 << 6]
    # seventeen bases take two words; lower case codes as upper case, N and '.' as A
    assert list(fc.pack_words([b'TTTTTTTTTTTTTTTTG'])) == [0xffffffff, 2]
    assert list(fc.pack_words([b'acgtN.-T', b'', b'C' * 16])) == [0 | 1 << 2 | 2 << 4 | 3 << 6 | 3 << 14, 0x55555555]
    # a read without bases takes no word and is not flagged; lower case is flagged although it codes
    assert len(fc.pack_words([b'', b''])) == 0
    assert fc.flagged([b'ACGT', b'acgt', b'', b'ACGN', b'AC-T', b'TTTT']) == [1, 3, 4]
    assert fc.num_kmers([b'A' * 21, b'A' * 20, b'', b'A' * 31], 21) == 1 + 0 + 0 + 11
    assert fc.num_kmers([b'A' * 21, b''], 1) == 21


def as_text(records):
    return [tuple(field.decode('latin-1') for field in rec) for rec in records]


def plain_text_readers_apply(data):
    """the oracle's reader and the package's Python reader open files in text mode: ASCII only, and a \\r that no \\n follows is a
    line end of its own there"""
    return all(byte < 128 for byte in data) and data.count(b'\r') == data.count(b'\r\n')


@pytest.mark.parametrize('name', [case[0] for case in CASES])
def test_reference_equals_the_oracle_and_the_python_reader(ok, name, tmp_path):
    from kevlar_amd import khmer as hk
    data = fc.by_name()[name][1]
    if not plain_text_readers_apply(data):
        assert name in ('D_names_high_bytes',), name         # (the only case those readers cannot take)
        return
    want = as_text(fc.reference(name))
    path = fc.write_case(tmp_path, data, 'plain')
    assert [(r.name, r.sequence, r.quality) for r in ok.ReadParser(path)] == want
    assert [(r.name, r.sequence, r.quality) for r in hk._iter_fastx(path)] == want


def host_records(path, max_reads):
    """every record of the file through the native host parser, and what it counted"""
    from kevlar_amd import khmer as hk
    os.environ['KV_INGEST'] = 'host'
    try:
        parser = hk.ReadParser(path)
        out = []
        for tb in parser.text_batches(max_reads, upload=False):
            assert type(tb).__name__ == 'TextBatch' and 1 <= tb.n <= max_reads
            for i in range(tb.n):
                r = tb.record(i)
                out.append((r.name, r.sequence, r.quality))
        return out, parser.num_reads
    finally:
        os.environ.pop('KV_INGEST', None)


@pytest.mark.parametrize('name,container', [(case[0], container) for case in CASES for container in case[3]])
def test_host_parser_equals_the_reference(name, container, tmp_path):
    _, data, max_reads, _, _ = fc.by_name()[name]
    want = as_text(fc.reference(name))
    path = fc.write_case(tmp_path, data, container)
    if container != 'plain':
        assert gzip.decompress(open(path, 'rb').read()) == data
    got, num_reads = host_records(path, max_reads)
    assert num_reads == len(want)
    assert got == want


# ---- the ledger: the table holds the edges it names
def test_constants_and_names():
    assert C['FQ_CHUNK'] % (16 * C['FQ_THREADS']) == 0 and C['FQ_THREADS'] % 64 == 0
    names = [case[0] for case in CASES]
    assert len(set(names)) == len(names)
    for name, data, max_reads, containers, route in CASES:
        assert len(data) <= fc.MAX_FILE, name
        assert containers[0] == 'plain' and set(containers) <= set(fc.ALL3) and route in ('device', 'handover', 'any')
        assert max_reads >= 1 and b'\0' not in data
    # every case is run by exactly one test of the GPU module
    single = fc.single_file_params()
    grouped = [(name, 'plain') for name in fc.e_sweep() + fc.e_crlf()]
    assert len(set(single + grouped)) == len(single) + len(grouped) == sum(len(case[3]) for case in CASES)


def line_end_table(data):
    """{offset of a \\n: kind of the line it ends} by the reference's reading of the file (no blank lines in these files)"""
    out, at = {}, 0
    for name, seq, qual in fc.parse_fastx(data):
        lines = data[at:].split(b'\n', 4)[:4]
        assert lines[0] == b'@' + name and lines[1] == seq and lines[3] == qual
        for kind, line in zip(fc.KINDS, lines):
            at += len(line) + 1
            out[at - 1] = kind
    assert at == len(data)
    return out


def test_group_a_puts_a_line_end_on_both_sides_of_every_boundary():
    group = [case for case in CASES if case[0].startswith('A_')]
    bounds = fc.boundaries()
    assert bounds == sorted(set(bounds)) and len(group) == 4 * len(bounds)
    assert bounds[:3] == [16, 16 * 64, 16 * C['FQ_THREADS']] and bounds[3:] == [m * C['FQ_CHUNK'] for m in (1, 2, 3)]
    seen = {b: [] for b in bounds}
    for (name, data, max_reads, containers, route), (b, delta) in zip(group, [(b, d) for b in bounds for d in (-2, -1, 0, 1)]):
        kind = name.rsplit('_', 1)[1]
        assert name == 'A_at{}{:+d}_{}'.format(b, delta, kind)
        assert line_end_table(data)[b + delta] == kind, name
        assert len(data) > bounds[-1] + C['FQ_CHUNK'] and max_reads > len(fc.reference(name)) and route == 'device'
        assert ('gzip' in containers) == ('bgzf' in containers) == (b % C['FQ_CHUNK'] == 0)
        seen[b].append((delta, kind))
    for b, hits in seen.items():
        assert sorted(kind for _, kind in hits) == sorted(fc.KINDS), b
        assert [delta for delta, _ in hits] == [-2, -1, 0, 1]          # two in front of the boundary, one on it, one behind


def test_group_b_is_dense_and_sparse():
    dense = fc.by_name()['B_dense'][1]
    vectors = np.frombuffer(dense[:len(dense) // 16 * 16], dtype=np.uint8).reshape(-1, 16)
    per_vector = (vectors == 10).sum(axis=1)
    assert per_vector.max() >= 10 and per_vector.min() >= 8
    for name in ('B_dense', 'B_dense_crlf'):
        recs = fc.reference(name)
        assert len(recs) == 10000 and not any(seq or qual for _, seq, qual in recs)
        assert sum(1 for rec in recs if rec[0] == b'a') == 9200
    assert fc.by_name()['B_dense_crlf'][1].count(b'\r\n') == 40000 == fc.by_name()['B_dense_crlf'][1].count(b'\n')
    lens = [len(seq) for _, seq, _ in fc.reference('B_dense_some_bases')]
    assert sorted(set(lens)) == [0] + list(fc.DENSE_BASES) and sum(1 for n in lens if n) == 200
    # chunks without a newline
    data = fc.by_name()['B_long40k'][1]
    chunks = [data[at:at + C['FQ_CHUNK']] for at in range(0, len(data), C['FQ_CHUNK'])]
    assert sum(1 for chunk in chunks if b'\n' not in chunk) >= 2
    # a batch of one read whose first stretch holds no whole record, at the start of the file and behind a carry
    for name, at in (('B_long150k_first', 0), ('B_long150k_second', 1), ('B_long150k_20th', 19)):
        _, data, max_reads, _, _ = fc.by_name()[name]
        recs = fc.reference(name)
        assert max_reads == 1 and len(recs[at][1]) == 150000 and max(len(r[1]) for r in recs[:at] + recs[at + 1:]) <= 60
        start = data.index(b'@long\n')
        # what the reader holds when the read's batch comes: the first stretch, and min_fresh bytes more for every batch before it
        held = fc.first_stretch(1) + at * C['min_fresh']
        assert start < fc.first_stretch(1) and (start + 150000 > held) == (at < 2)


def test_group_c_ends_files_every_way():
    m = 4
    sizes = {}
    for name, data, _, _, _ in CASES:
        if name.startswith('C_size{}'.format(m * C['FQ_CHUNK'])):
            sizes.setdefault(len(data), set()).add(data.endswith(b'\n'))
    assert sizes == {m * C['FQ_CHUNK'] + d: {True, False} for d in (-1, 0, 1)}
    assert sorted(len(fc.by_name()['C_size_mod16_{}'.format(r)][1]) % 16 for r in (0, 1, 15)) == [0, 1, 15]
    body = fc.by_name()['C_tail_nl'][1]
    assert body.endswith(b'\n') and not body.endswith(b'\n\n')
    want = fc.reference('C_tail_nl')
    for label, tail, _, route in fc.tails():
        name, data, max_reads, containers, case_route = fc.by_name()['C_tail_' + label]
        assert data == body[:-1] + tail and fc.reference(name) == want and containers == fc.ALL3 and case_route == route
    assert fc.by_name()['C_tail_four_blank'][1][-6:-5] != b'\n' and fc.by_name()['C_tail_four_blank'][1].endswith(5 * b'\n') and fc.by_name()['C_tail_four_blank'][4] == 'handover'
    assert 1 <= fc.by_name()['C_tail_four_blank'][2] < len(want)            # the device serves a batch before it meets them
    assert len(fc.by_name()['C_tail_blanks5000'][1]) - len(body) == 5000 > 4096
    for label, last in (('name', (b'last', b'', b'')), ('sequence', (b'last', b'ACGTACGTAC', b'')), ('plus', (b'last', b'ACGTACGTAC', b''))):
        name, data, _, _, route = fc.by_name()['C_stops_after_' + label]
        assert fc.reference(name) == want + (last,) and route == 'handover' and data.startswith(body)
    assert len(fc.by_name()['C_one_record_{}'.format(C['min_file'] - 1)][1]) == C['min_file'] - 1
    assert len(fc.by_name()['C_one_record_{}'.format(C['min_file'])][1]) == C['min_file']
    assert fc.by_name()['C_one_record_{}'.format(C['min_file'])][4] == 'device'


def test_group_d_holds_the_bytes():
    near = fc.by_name()['D_names_near_newline'][1]
    high = fc.by_name()['D_names_high_bytes'][1]
    assert all(near.count(bytes([b])) > 100 for b in (0x0b, 0x1a, 0x2a)) and all(high.count(bytes([b])) > 100 for b in (0x8a, 0xff))
    # each of them at every position of a 16-byte vector
    for data, probes in ((near, (0x0b, 0x1a, 0x2a)), (high, (0x8a, 0xff))):
        arr = np.frombuffer(data, dtype=np.uint8)
        for b in probes:
            assert set(np.flatnonzero(arr == b) % 16) == set(range(16))
    quals = [q for _, _, q in fc.reference('D_quality_starts_at_or_plus')]
    assert sum(q.startswith(b'@') for q in quals) > 50 and sum(q.startswith(b'+') for q in quals) > 50
    data = fc.by_name()['D_plus_repeats_name'][1]
    assert all(data.count(b'\n+' + name + b'\n') >= 1 for name, _, _ in fc.reference('D_plus_repeats_name')[:50])
    letters = set(b''.join(seq for _, seq, _ in fc.reference('D_sequence_alphabet')))
    assert letters >= set(b'acgtnNRYKMSWBDHV.-')
    crlf = fc.by_name()['D_crlf'][1]
    assert crlf.count(b'\r\n') == crlf.count(b'\n') == 4 * len(fc.reference('D_crlf'))
    some = fc.by_name()['D_cr_on_sequence_only'][1]
    assert some.count(b'\r') == len(fc.reference('D_cr_on_sequence_only')) and not any(b'\r' in f for rec in fc.reference('D_cr_on_sequence_only') for f in rec)
    assert fc.by_name()['D_sequence_just_cr'][1].count(b'\n\r\n+') > 100
    assert sum(1 for _, seq, _ in fc.reference('D_sequence_just_cr') if seq == b'') > 100


def test_group_e_moves_the_cut_across_every_byte_of_a_record():
    cut = fc.first_stretch(fc.E_BATCH)
    sweep = fc.e_sweep()
    assert len(sweep) == fc.E_L
    residues = set()
    for p, name in enumerate(sweep):
        _, data, max_reads, containers, route = fc.by_name()[name]
        ends = sorted(line_end_table(data))
        starts = [0] + [e + 1 for e in ends[3::4]]                           # where records start
        assert len(data) > cut + fc.E_L and max_reads == fc.E_BATCH and route == 'device'
        assert {b - a for a, b in zip(starts[1:], starts[2:])} == {fc.E_L}         # all records but the padded first: one length
        inside = max(s for s in starts if s <= cut)
        residues.add(cut - inside)
        assert cut - inside == (cut - p) % fc.E_L
        # the first stretch holds more records than a batch takes, and the file ends with the second stretch
        assert inside // fc.E_L > max_reads and len(data) - cut <= C['slack']
        assert set(containers) == set(fc.ALL3 if p == 0 else ('plain', 'bgzf') if p in (fc.E_L // 2, fc.E_L - 1) else fc.PLAIN)
    assert residues == set(range(fc.E_L))
    crlf = {label: fc.by_name()['E_crlf_' + label][1] for label, _ in fc.e_crlf_pads()}
    assert len(crlf) == 8
    for label, data in crlf.items():
        assert data.count(b'\r\n') == data.count(b'\n') == data.count(b'\r') and len(data) > cut + 64
        around = data[cut - 2:cut + 2]
        if label.startswith('between_'):
            assert around[1:3] == b'\r\n'
        elif label.startswith('before_cr_'):
            assert around[2:4] == b'\r\n'
        else:
            assert around[0:2] == b'\r\n'
    # which line the cut falls in: the label says it
    for label, data in crlf.items():
        kind = label.rsplit('_', 1)[1]
        newlines_before = data[:cut + (2 if label.startswith('before_cr_') else 1 if label.startswith('between_') else 0)].count(b'\n')
        assert fc.KINDS[(newlines_before - 1) % 4] == kind, label
    one = fc.by_name()['E_300_batches_of_one']
    sizes = {len(n) + len(s) + len(q) + 6 for n, s, q in fc.reference(one[0])}
    assert one[2] == 1 and len(fc.reference(one[0])) == 300 and min(sizes) >= 240 and max(sizes) <= 260
    small = [case for case in CASES if case[0].startswith('E_batch')]
    assert [case[2] for case in small] == [4, 5, 64]
    for case in small:
        assert case[1] == fc.by_name()[case[0].split('_', 2)[2]][1]           # a file of group A
        # the last line the first batch may take ends inside a 16-byte vector that holds further newlines
        ends = sorted(line_end_table(case[1]))
        last = ends[4 * case[2] - 1]
        vector = case[1][last // 16 * 16:last // 16 * 16 + 16]
        assert vector[last % 16 + 1:].count(b'\n') >= 1, case[0]
