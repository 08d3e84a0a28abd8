"""The device FASTQ parser (kevlar_amd/csrc/kv_fastq.hip: k_count_lines, k_line_starts, k_records, k_pack_text, k_terminate,
k_record_extents + k_record_copy, and the carry between batches) against the byte-level reference of tests/fastq_cases_common.py,
on its table of files -- every batch's packed words, flags, k-mer numbers and every record's text, exactly; the file's count tables
against the oracle's.  tests/test_fastq_cases_reference.py holds the reference and the table themselves, without a GPU."""
import functools

import numpy as np
import pytest

import fastq_cases_common as fc

pytestmark = pytest.mark.gpu

K = 21
ROUTES = {'DeviceTextBatch': 'device', 'TextBatch': 'host'}


@functools.lru_cache(maxsize=None)
def oracle_tables(name):
    """the oracle's count tables of the case's reads, or None where a read holds a byte outside ACGT (the oracle's rule for
    those is its own)"""
    from oracle import okhmer as ok
    seqs = [seq for _, seq, _ in fc.reference(name)]
    if fc.flagged(seqs):
        return None
    table = ok.Counttable(K, 5e4, 4)
    bases, offs = ok.concat_reads([s.decode('ascii') for s in seqs])
    n_kmers = ok.consume_reads(table, bases, offs, len(seqs))
    assert n_kmers == fc.num_kmers(seqs, K)
    return n_kmers, [table.table_bytes(t) for t in range(4)]


def check_batch(tb, want):
    """one batch against the records of the reference that it covers"""
    seqs = [seq for _, seq, _ in want]
    words = fc.pack_words(seqs)
    assert tb.batch.n_reads == len(want)
    assert np.array_equal(tb.batch.packed_words(0, len(words)), words)
    with pytest.raises(Exception):
        tb.batch.packed_words(0, len(words) + 1)               # and not a word more
    assert list(tb.batch.flagged_reads()) == fc.flagged(seqs)
    for k in (1, 21, 31):
        assert tb.batch.num_kmers(k) == fc.num_kmers(seqs, k)
    tb.prefetch(range(tb.n))
    got = []
    for i in range(tb.n):
        r = tb.record(i)
        got.append((r.name.encode('latin-1'), r.sequence.encode('latin-1'), r.quality.encode('latin-1')))
    assert got == list(want)


def check_file(hk, name, container, folder):
    """walk the case's file a batch at a time with no ingest knob set; returns who served each batch"""
    _, data, max_reads, _, route = fc.by_name()[name]
    want = fc.reference(name)
    path = fc.write_case(folder, data, container)
    parser = hk.ReadParser(path)
    table = hk.Counttable(K, 5e4, 4)
    served, done, n_kmers = [], 0, 0
    for tb in parser.text_batches(max_reads):
        assert 1 <= tb.n <= max_reads
        served.append(ROUTES[type(tb).__name__])
        check_batch(tb, want[done:done + tb.n])
        n_kmers += table.consume_batch(tb.batch)
        done += tb.n
        tb.batch.close()
    print('{} {}: {} batches, served by {}'.format(name, container, len(served), sorted(set(served))))
    assert done == len(want) and parser.num_reads == len(want)
    if route == 'device':
        assert set(served) == {'device'}
    elif route == 'handover':
        assert served[0] == 'device' and served[-1] == 'host'
    tables = oracle_tables(name)
    if tables is not None:
        assert n_kmers == tables[0]
        for t in range(4):
            assert table.table_bytes(t) == tables[1][t]
    return served


@pytest.mark.parametrize('name,container', fc.single_file_params())
def test_file_equals_the_reference(hk, tmp_path, name, container):
    check_file(hk, name, container, tmp_path)


SWEEP = fc.e_sweep()


@pytest.mark.parametrize('part', range(4))
def test_cut_between_stretches_at_every_byte_of_a_record(hk, tmp_path, part):
    """group E: the first record's name padded by p = 0 .. L-1 moves the cut behind the first stretch across a record"""
    step = (len(SWEEP) + 3) // 4
    for name in SWEEP[part * step:(part + 1) * step]:
        folder = tmp_path / name
        folder.mkdir()
        assert len(check_file(hk, name, 'plain', folder)) >= 2


def test_cut_between_stretches_around_a_crlf(hk, tmp_path):
    for name in fc.e_crlf():
        folder = tmp_path / name
        folder.mkdir()
        assert len(check_file(hk, name, 'plain', folder)) >= 2


def line_counts_and_batches(hk, path, max_reads):
    """how often the reader counted the lines of a stretch (k_count_lines: once per attempt at a batch), and the batches it made"""
    import ctypes
    from kevlar_amd import _lib
    lib = _lib.load()
    lib.kv_prof_reset()
    lib.kv_prof_enable(1)
    try:
        batches = 0
        for tb in hk.ReadParser(path).text_batches(max_reads):
            assert type(tb).__name__ == 'DeviceTextBatch'
            batches += 1
            tb.batch.close()
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        lib.kv_prof_get(b'k_count_lines', ctypes.byref(ms), ctypes.byref(n))
        return n.value, batches
    finally:
        lib.kv_prof_enable(0)


@pytest.mark.parametrize('container', ['plain', 'bgzf'])
def test_a_stretch_without_a_whole_record_is_asked_for_again(hk, tmp_path, container):
    """the read of 150 000 bases as the first and as the second record does reach the arm it is in the table for: its batch takes
    more than one attempt (the input goes back and the budget doubles), where a file of records that fit takes one attempt a batch"""
    for name in ('B_long150k_first', 'B_long150k_second', 'E_300_batches_of_one'):
        _, data, max_reads, _, _ = fc.by_name()[name]
        folder = tmp_path / name
        folder.mkdir()
        counted, batches = line_counts_and_batches(hk, fc.write_case(folder, data, container), max_reads)
        assert batches == len(fc.reference(name))
        if name.startswith('B_long'):
            assert counted > batches, name
        else:
            assert counted == batches, name


@pytest.mark.parametrize('name', ['E_batch64_A_at{}-1_name'.format(fc.C['FQ_CHUNK']), 'E_cut_p00'])
def test_fetching_is_random_access(hk, tmp_path, name):
    """records come in any order, together or one at a time; a batch that has been followed by another no longer answers"""
    _, data, max_reads, _, _ = fc.by_name()[name]
    want = [tuple(f.decode('latin-1') for f in rec) for rec in fc.reference(name)]
    parser = hk.ReadParser(fc.write_case(tmp_path, data, 'plain'))
    rng = np.random.default_rng(len(name))
    batches, done = [], 0
    for tb in parser.text_batches(max_reads):
        assert type(tb).__name__ == 'DeviceTextBatch'
        order = [int(i) for i in rng.permutation(tb.n)]
        together = parser._fetch_records(order)
        assert [(together.record(j).name, together.record(j).sequence, together.record(j).quality) for j in range(tb.n)] == \
            [want[done + i] for i in order]
        for i in order:
            one = parser._fetch_records([i]).record(0)
            assert (one.name, one.sequence, one.quality) == want[done + i]
        batches.append(tb)
        done += tb.n
    assert done == len(want) and len(batches) >= 2
    earlier, last = batches[-2], batches[-1]
    assert last.n < earlier.n
    # an index of the batch before that the current one does not have: refused, not answered
    for i in (last.n, earlier.n - 1):
        with pytest.raises(Exception):
            earlier.record(i)
    r = last.record(last.n - 1)
    assert (r.name, r.sequence, r.quality) == want[-1]
