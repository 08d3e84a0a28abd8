"""CPU check of the rule the device FASTA splitter must reproduce (kevlar_amd/csrc/kv_genome.hip): the
byte-level restatement of tests/genome_common.py against today's host path (seqio.parse_seq_dict + localize.Genome) on the
hand-built files, the files cut at segment ends and 300 seeded ones, and against the reader that holds the localize tests to the
reference's recorded cutouts; that every reference FASTA fixture the end-to-end tests read is one the device may take; and the
host rules of kevlar_amd/csrc/kv_genome_plan.h -- the per-line rule and the carry between segments, run a line at a time
(gn_model_segment) over files cut at every offset -- behind tests/harness/genome_plan_host.cpp.  No GPU involved."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import genome_common as gc

ROOT = gc.ROOT
SRC = os.path.join(ROOT, 'tests', 'harness', 'genome_plan_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libgenome_plan_host.so')
U64 = ctypes.c_uint64
KV_OK, KV_ERR_TYPE = 0, -3

HAND = gc.hand_built()
SEGMENT_SIZES = (1024, 4096)


# ---- the restatement against the host path
@pytest.mark.parametrize('name', sorted(HAND))
def test_rule_equals_host_on_hand_built(name):
    assert gc.device_eligible(HAND[name])
    gc.rule_equals_host(HAND[name])


def test_hand_built_files_hold_what_they_say():
    ids = lambda name: gc.split_rule(HAND[name])[0]                   # noqa: E731
    seqs = lambda name: gc.split_rule(HAND[name])[1]                  # noqa: E731
    assert gc.split_rule(b'') == ([], []) and ids('no_defline') == [] and ids('text_in_front') == [b's1']
    assert seqs('text_in_front') == [b'ACGT'] and seqs('no_trailing_newline') == [b'ACGT', b'GGCC']
    assert seqs('crlf_mixed') == [b'ACGTGG', b'TTAA'] and seqs('interior_blanks') == [b'AC GT G\tG\x0bTT']
    assert ids('defline_runs') == [b'a', b'b', b'c', b'd', b'e'] and seqs('defline_runs') == [b'', b'', b'ACGT', b'', b'']
    assert ids('gt_alone') == [b'', b'x'] and seqs('gt_mid_line') == [b'AC>GTGG> >not_a_defline']
    assert ids('id_space_vs_tab') == [b'id1', b'id2', b'id3\x0bstill']
    assert len(ids('records_3000')) == 3000 and set(seqs('empty_records_3000')) == {b''}
    assert [len(s) for s in seqs('one_line_100000')] == [100000, 4]
    for width in (1, 59, 60, 61, gc.CHUNK - 1, gc.CHUNK, gc.CHUNK + 1):
        assert max(len(line) for line in HAND['width_%d' % width].split(b'\n')) == max(width, 2)
    for name, data in HAND.items():                                   # every id of a file once: the duplicate check has its own test
        assert len(set(ids(name))) == len(ids(name)), name


@pytest.mark.parametrize('S', SEGMENT_SIZES)
def test_rule_equals_host_on_segment_cases(S):
    for name, data in gc.segment_cases(S).items():
        assert gc.device_eligible(data), name
        gc.rule_equals_host(data)
    assert gc.device_eligible(gc.over_bound(S))
    gc.rule_equals_host(gc.over_bound(S))


def test_rule_equals_host_on_seeded_files():
    shapes = set()
    for seed in range(gc.N_SEEDED):
        data = gc.seeded(seed)
        assert gc.device_eligible(data), seed
        ids, seqs = gc.rule_equals_host(data)
        shapes.add((len(ids) > 0, b'\r\n' in data, data[-1:] == b'\n', any(len(s) == 0 for s in seqs), len(data) > gc.CHUNK))
    assert len(shapes) >= 12


def test_declines_are_not_eligible_and_differ_or_could():
    for name, data in gc.declines().items():
        assert not gc.device_eligible(data), name
    # what the text layer does with two of them: a lone CR ends a line, 0x1c-0x1f are stripped like blanks
    genome = gc.host_genome(gc.declines()['lone_cr'])
    assert genome.seqs == ['ACGT'] and gc.split_rule(gc.declines()['lone_cr'])[1] == [b'AC\rGT']
    genome = gc.host_genome(gc.declines()['sep_1f_trailing'])
    assert genome.seqs == ['ACGT'] and gc.split_rule(gc.declines()['sep_1f_trailing'])[1] == [b'ACGT\x1f']


def test_duplicate_ids_are_the_host_s_assertion():
    with pytest.raises(AssertionError, match='^dup$'):
        gc.host_genome(b'>dup a\nAC\n>other\nGG\n>dup b\nTT\n')


# ---- the reference's fixtures
def test_rule_equals_the_fixture_reader_on_the_golden_references():
    import localize_common as lc
    expected_declines = []                                            # golden references the device is NOT expected to take: none
    for path in gc.golden_references():
        data = gc.file_text(path)
        assert gc.device_eligible(data) != (path in expected_declines), path
        ids, seqs = gc.rule_equals_host(data)
        records = lc.read_fasta(path)
        assert [(i.decode(), s.decode()) for i, s in zip(ids, seqs)] == records and len(records) > 0


# ---- kv_genome_plan.h
@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in (SRC, gc.PLAN)):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_last_error.restype = ctypes.c_char_p
    for name in ('h_byte_flags', 'h_check_bytes', 'h_out_bytes'):
        getattr(L, name).restype = ctypes.c_uint32
    for name in ('h_segment_text', 'h_plain_take', 'h_bgzf_take', 'h_grow'):
        getattr(L, name).restype = U64
    L.h_constants.argtypes = [ctypes.c_void_p]
    L.h_is_strip.argtypes = L.h_ends_id.argtypes = L.h_byte_flags.argtypes = [ctypes.c_uint32]
    L.h_check_bytes.argtypes = [ctypes.c_char_p, U64]
    L.h_classify.argtypes = [ctypes.c_char_p, U64, U64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.h_out_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, U64]
    L.h_model.argtypes = [ctypes.c_char_p, U64, ctypes.c_void_p, U64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.h_segment_text.argtypes = [U64]
    L.h_plain_take.argtypes = [U64, U64, U64]
    L.h_bgzf_take.argtypes = [ctypes.c_void_p, U64, U64, U64, ctypes.c_void_p]
    L.h_grow.argtypes = [U64, U64]
    L.h_scan_plan.argtypes = [U64, U64, U64, ctypes.c_void_p]
    return L


def model(lib, data, cuts):
    """(code, ids, seqs' joined text, starts, scalars) of the header's model over data cut at `cuts`"""
    n = len(data)
    cut_arr = (U64 * max(len(cuts), 1))(*cuts)
    text, ids = ctypes.create_string_buffer(n + 1), ctypes.create_string_buffer(n + 1)
    seq_start, id_off, scalars = (U64 * (n + 2))(), (U64 * (n + 2))(), (U64 * 6)()
    rc = lib.h_model(data, n, cut_arr, len(cuts), text, ids, seq_start, id_off, scalars)
    if rc != KV_OK:
        return rc, None, None, None, None
    n_text, n_ids, n_rec = int(scalars[0]), int(scalars[1]), int(scalars[2])
    offs = [int(id_off[r]) for r in range(n_rec)] + [n_ids]
    return rc, [ids.raw[offs[r]:offs[r + 1]] for r in range(n_rec)], text.raw[:n_text], [int(seq_start[r]) for r in range(n_rec)], [int(v) for v in scalars]


def check_model(lib, data, cuts):
    want_ids, want_seqs = gc.split_rule(data)
    want_text, want_starts, _ = gc.joined(want_seqs)
    rc, ids, text, starts, scalars = model(lib, data, cuts)
    assert rc == KV_OK, (lib.h_last_error(), cuts)
    assert (ids, text, starts) == (want_ids, want_text, want_starts), cuts
    assert scalars[3] == len(data) and scalars[5] <= gc.MAX_TRAIL
    return scalars


def test_harness_and_test_share_their_constants(lib):
    out = (U64 * 8)()
    lib.h_constants(out)
    assert [int(v) for v in out] == [gc.CHUNK, 256, gc.MAX_TRAIL, gc.MAX_ID, 256 << 20, 1 << 30, ord('>'), 63]
    assert (gc.CHUNK, gc.MAX_TRAIL, gc.MAX_ID) == (16384, 4096, 4096)
    from kevlar_amd.localize import SEPARATOR
    assert SEPARATOR == gc.SEPARATOR == bytes([int(out[6])])


def test_byte_classes(lib):
    for c in range(256):
        assert bool(lib.h_is_strip(c)) == (bytes([c]) in (b' ', b'\t', b'\x0b', b'\x0c', b'\r')), c
        assert bool(lib.h_ends_id(c)) == (c in (0x20, 0x09))
        assert bool(lib.h_byte_flags(c)) == (c >= 0x80 or c == 0 or 0x1c <= c <= 0x1f), c
        # the strippable bytes and the declined ones are together what str.rstrip() takes from a line (LF ends it), and NUL
        stripped_by_python = chr(c).isspace() if c < 0x80 else False
        assert stripped_by_python == (bool(lib.h_is_strip(c)) or 0x1c <= c <= 0x1f or c == 0x0a), c
    for data, flags in ((b'AC\r\nGT', 0), (b'AC\rGT', 8), (b'ACGT\r', 64), (b'\r\r\n', 8), (b'\r\n\r', 64), (b'\xc3', 1), (b'\x1d', 2), (b'a\x00', 4)):
        assert lib.h_check_bytes(data, len(data)) == flags, data
    for name, data in gc.declines().items():
        if name not in ('long_trail', 'long_id'):             # (a CR on the very end: flag 64, a decline once the file has ended)
            assert lib.h_check_bytes(data, len(data)) & (63 | 64), name


def classify(lib, line, cont=0, cont_def=0, cont_id=0, lead=b'xx\n', tail=b'\nyy'):
    out = (ctypes.c_uint32 * 8)()
    text = lead + line + tail
    lib.h_classify(text, len(lead), len(lead) + len(line), cont, cont_def, cont_id, out)
    return dict(zip(('kind', 'pay_off', 'pay_len', 'is_def', 'defline', 'id_open', 'held', 'flags'), (int(v) for v in out)))


def test_one_line(lib):
    NONE, SEQ, ID = 0, 1, 2
    got = classify(lib, b'ACGT \t\r')
    assert (got['kind'], got['pay_off'], got['pay_len'], got['is_def'], got['held'], got['flags']) == (SEQ, 0, 4, 0, 3, 0)
    assert classify(lib, b'')['pay_len'] == 0 and classify(lib, b' \t ')['pay_len'] == 0 and classify(lib, b' \t ')['held'] == 3
    assert classify(lib, b' AC G')['pay_len'] == 5 and classify(lib, b' >x')['kind'] == SEQ
    got = classify(lib, b'>id rest \t')
    assert (got['kind'], got['pay_off'], got['pay_len'], got['is_def'], got['defline'], got['id_open'], got['held']) == (ID, 1, 2, 1, 1, 0, 2)
    got = classify(lib, b'>id\x0bx')
    assert (got['pay_len'], got['id_open']) == (4, 1)
    got = classify(lib, b'>')
    assert (got['kind'], got['pay_len'], got['is_def'], got['id_open']) == (ID, 0, 1, 1)
    got = classify(lib, b'>  ')
    assert (got['pay_len'], got['id_open'], got['held']) == (0, 1, 2)                # (the blanks are held: the id may go on behind them)
    # continuations of a line cut by a segment end
    got = classify(lib, b'>AC', cont=1)
    assert (got['kind'], got['is_def'], got['pay_len']) == (SEQ, 0, 3)                # '>' in mid-line means nothing
    got = classify(lib, b'more rest', cont=1, cont_def=1, cont_id=1)
    assert (got['kind'], got['pay_off'], got['pay_len'], got['is_def'], got['defline'], got['id_open']) == (ID, 0, 4, 0, 1, 0)
    got = classify(lib, b' more', cont=1, cont_def=1, cont_id=1)
    assert (got['kind'], got['pay_len'], got['id_open']) == (ID, 0, 0)
    got = classify(lib, b'more rest', cont=1, cont_def=1, cont_id=0)
    assert (got['kind'], got['defline'], got['is_def']) == (NONE, 1, 0)
    # the bounds: MAX_TRAIL strippable bytes and MAX_ID id bytes pass, one more declines; a lane walks no further
    assert classify(lib, b'AC' + b' ' * gc.MAX_TRAIL)['flags'] == 0 and classify(lib, b'AC' + b' ' * (gc.MAX_TRAIL + 1))['flags'] == 16
    assert classify(lib, b' ' * (gc.MAX_TRAIL + 500))['flags'] == 16
    assert classify(lib, b'>' + b'i' * gc.MAX_ID)['flags'] == 0 and classify(lib, b'>' + b'i' * gc.MAX_ID + b' d')['flags'] == 0
    assert classify(lib, b'>' + b'i' * (gc.MAX_ID + 1))['flags'] == 32
    assert classify(lib, b'>i ' + b'd' * (3 * gc.MAX_ID))['flags'] == 0
    # what a line owns of the joined text
    assert [lib.h_out_bytes(SEQ, 0, 9, before) for before in (0, 1, 7)] == [0, 9, 9]
    assert [lib.h_out_bytes(ID, 1, 9, before) for before in (0, 1, 7)] == [0, 1, 1]
    assert lib.h_out_bytes(ID, 0, 9, 3) == 0 and lib.h_out_bytes(NONE, 0, 0, 3) == 0


def test_model_on_whole_files(lib):
    for name, data in HAND.items():
        check_model(lib, data, [])
    for seed in range(gc.N_SEEDED):
        check_model(lib, gc.seeded(seed), [])


def test_model_cut_at_every_offset(lib):
    """every small hand-built file cut in two at every byte, and in three at every pair of a sample"""
    rng = random.Random(5)
    for name, data in HAND.items():
        if not 1 <= len(data) <= 80:
            continue
        for cut in range(len(data) + 1):
            check_model(lib, data, [cut])
        for _ in range(60):
            check_model(lib, data, sorted(rng.sample(range(len(data) + 1), 2)))


def test_model_on_seeded_files_in_segments(lib):
    rng = random.Random(6)
    held = 0
    for seed in range(gc.N_SEEDED):
        data = gc.seeded(seed)
        for S in (1, 7, 64, 1024):
            if S == 1 and len(data) > 3000:
                continue
            scalars = check_model(lib, data, list(range(S, len(data), S)))
            held = max(held, scalars[5])
        cuts = sorted(rng.sample(range(len(data) + 1), min(len(data), rng.randint(1, 9))))
        check_model(lib, data, cuts)
    assert held >= 2


@pytest.mark.parametrize('S', SEGMENT_SIZES)
def test_model_on_segment_cases(lib, S):
    for name, data in gc.segment_cases(S).items():
        scalars = check_model(lib, data, list(range(S, len(data), S)))
        assert scalars[4] == -(-len(data) // S), name
        if name.startswith('blanks_') or name == 'two_cuts_in_blanks':
            assert scalars[5] >= 3, name
    # an interior run longer than the bound: taken in one piece, declined where segments end in it
    data = gc.over_bound(S)
    check_model(lib, data, [])
    rc = model(lib, data, list(range(S, len(data), S)))[0]
    assert rc == KV_ERR_TYPE and b'blanks' in lib.h_last_error()


def test_model_declines(lib):
    for name, data in gc.declines().items():
        for cuts in ([], [len(data) // 2], list(range(1, len(data)))[:5000:7]):
            if name == 'long_id' and cuts:
                check_model(lib, data, cuts)          # (the bound is on the id bytes of one line part: cut, the id is taken)
            else:
                assert model(lib, data, cuts)[0] == KV_ERR_TYPE, (name, cuts)
    # a CR as a segment's last byte is judged with the next segment's first
    assert model(lib, b'>s\nAC\r\nGT\n', [6])[0] == KV_OK and model(lib, b'>s\nAC\rGT\n', [6])[0] == KV_ERR_TYPE


def test_takes_growth_and_scan_chunks(lib):
    assert lib.h_segment_text(0) == 256 << 20 and lib.h_segment_text(1024) == 1024 and lib.h_segment_text(1 << 40) == 1 << 30
    assert [lib.h_plain_take(pos, 2500, 1024) for pos in (0, 1024, 2048, 2500)] == [1024, 1024, 452, 0]
    isize = (ctypes.c_uint32 * 6)(500, 600, 0, 65280, 10, 0)
    got, m, text = [], 0, U64()
    while m < 6:
        m1 = lib.h_bgzf_take(isize, 6, m, 1100, ctypes.byref(text))
        got.append((m, m1, text.value))
        assert m1 > m
        m = m1
    assert got == [(0, 3, 1100), (3, 4, 65280), (4, 6, 10)]
    assert lib.h_grow(0, 1) == 4096 and lib.h_grow(4096, 4097) == 8192 and lib.h_grow(1 << 20, 5 << 20) == 8 << 20 and lib.h_grow(8192, 100) == 8192

    def plan(total, z, chunk):
        out = (U64 * 3)()
        lib.h_scan_plan(total, z, chunk, out)
        return tuple(int(v) for v in out)
    assert plan(1000, 13, 0) == (1000, 1000, 1) and plan(1000, 13, 5000) == (1000, 1000, 1) and plan(12, 13, 0)[2] == 0
    assert plan(1000, 13, 13) == (1, 13, 988) and plan(1000, 13, 14) == (2, 14, 494) and plan(1000, 13, 4) == (1, 13, 988)
    assert plan(10000, 13, 4096) == (4080, 4092, 3) and plan(10000, 51, 27 + 50) == (16, 66, 622)
    for total, z, chunk in ((1000, 13, 13), (1000, 13, 14), (10000, 13, 4096), (10000, 128, 200), (5000, 51, 4999), (99999, 51, 65536)):
        step, length, n = plan(total, z, chunk)
        assert length == step + z - 1 <= max(chunk, z) and (step % 16 == 0 or step < 16)
        starts = [w for k in range(n) for w in range(k * step, min(k * step + length, total) - z + 1)]
        assert starts == list(range(total - z + 1))                   # every window in exactly one chunk
