"""`kevlar varfilter` without a GPU: the plain-Python restatement of tests/varfilter_common.py held to what the reference's own
tests state (kevlar/tests/test_varfilter.py, on the fixtures it uses), its error cases, the host generators parse_bed and bedstream
held to the restatement, the command line's new entry, and the host rules of kevlar_amd/csrc/kv_varfilter_plan.h at their edges
(the header compiles for the host; tests/harness/varfilter_plan_host.cpp wraps it in a C ABI)."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import varfilter_common as vc

ROOT = vc.ROOT
CSRC = os.path.join(ROOT, 'kevlar_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'harness', 'varfilter_plan_host.cpp')
SO = os.path.join(ROOT, 'tests', 'harness', 'libvarfilter_plan_host.so')
HEADERS = [os.path.join(CSRC, name) for name in ('kv_require.h', 'kv_varfilter_plan.h')]
KV_OK, KV_ERR_ARG = 0, -1
U8P, U32, U64, I64 = ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64


def calls_of(path):
    import kevlar_amd
    from kevlar_amd.vcf import VCFReader
    with kevlar_amd.open(path, 'r') as stream:
        reader = VCFReader(stream)
        reader.suppress_filter_warnings = True
        return [(call.region[0].encode(), call.region[1], call.region[2]) for call in reader]


def flagged(calls, text):
    flags, _ = vc.expected(calls, text)
    return [call for call, flag in zip(calls, flags) if flag]


# ---- what the reference's tests state -----------------------------------------------------------------------------------------------
def test_single_region_flags_one_call():
    """test_varfilter_single: five calls, one of them filtered, position 36385017"""
    calls = calls_of(vc.VCF_FIVE)
    assert len(calls) == 5 and {call[0] for call in calls} == {b'chr17'}
    assert flagged(calls, open(vc.BED_SINGLE, 'rb').read()) == [(b'chr17', 36385017, 36385018)]


def test_two_regions_flag_two_calls_and_skip_comment_and_blank():
    """test_varfilter_main: the calls at VCF POS 36385018 and 3547691"""
    calls = calls_of(vc.VCF_FIVE)
    text = open(vc.BED_TWO, 'rb').read()
    flags, counters = vc.expected(calls, text)
    assert sorted(call[1] + 1 for call, flag in zip(calls, flags) if flag) == [3547691, 36385018]
    assert counters == {'lines': 4, 'skipped': 2, 'regions': 2, 'known': 2, 'overlaps': 2, 'flagged': 2}


def test_queries_of_the_reference_s_index_tests():
    """test_load_predictions and test_load_predictions_multi_chrom; a point query p is the region (p, p + 1)"""
    five = calls_of(vc.VCF_FIVE)
    assert flagged(five, b'chr1\t1\t1000000\n') == []
    assert flagged(five, b'chr17\t1\t1000000\n') == []
    assert flagged(five, b'chr17\t36385017\t36385018\n') == [(b'chr17', 36385017, 36385018)]
    low = calls_of(vc.VCF_LOW_ABUND)
    assert len(low) == 5 and {call[0] for call in low} == {b'1', b'9', b'14'}
    assert flagged(low, b'chr1\t1\t1000000\n') == []
    assert flagged(low, b'1\t1\t1000000\n') == []
    assert set(flagged(low, b'1\t91850000\t91860000\n')) == {(b'1', 91853096, 91853097), (b'1', 91853110, 91853111)}
    assert flagged(low, b'14\t82461000\t82462000\n') == [(b'14', 82461856, 82461857)]


def test_overlap_rule_edges():
    call = (100, 110)
    for region, hit in (((90, 100), False), ((90, 101), True), ((110, 120), False), ((109, 120), True), ((103, 104), True), ((0, 1000), True),
                        ((105, 105), False), ((108, 103), False), ((-5, 101), True)):
        assert vc.overlaps(region, call) is hit, region


# ---- the restatement's grammar ------------------------------------------------------------------------------------------------------
def test_grammar_of_a_line():
    parse = lambda text: vc.parse_text(text)[0]
    assert parse(b'chr1\t1\t2\n') == parse(b'chr1 1 2') == parse(b' \tchr1 \t 1\x0b2\x1f\n') == parse(b'chr1\t1\t2\r\n') == [(b'chr1', 1, 2)]
    assert parse(b'chr1\t+5\t007\textra\tcolumns\n') == [(b'chr1', 5, 7)]
    assert parse(b'chr1\t-3\t-0\n') == [(b'chr1', -3, 0)]
    assert parse(b'c\r1\r2\n') == [(b'c', 1, 2)]                                    # a lone \r separates tokens
    assert parse(b'c\xc2\xa01 1 2\n') == [(b'c\xc2\xa01', 1, 2)]                    # a no-break space is two token bytes
    assert parse(b'%d %d %d' % (7, -2 ** 63, 2 ** 63 - 1)) == [(b'7', -2 ** 63, 2 ** 63 - 1)]
    assert vc.parse_text(b'#c\t1\t2\n\n \t\n\x1c\n# x') == ([], {'lines': 5, 'skipped': 5})
    assert vc.parse_text(b'') == ([], {'lines': 0, 'skipped': 0})
    assert vc.parse_text(b'\n') == ([], {'lines': 1, 'skipped': 1})
    regions, counters = vc.parse_text(b' #c\t1\t2\n')                               # the comment test comes before stripping
    assert regions == [(b'#c', 1, 2)] and counters == {'lines': 1, 'skipped': 0}


@pytest.mark.parametrize('line', [b'chr1\t5', b'chr1', b'chr1\tabc\t5', b'chr1\t5\tabc', b'chr1\t1_000\t2000', b'chr1\t1\t%d' % 2 ** 63,
                                  b'chr1\t%d\t5' % (-2 ** 63 - 1), b'chr1\t1.0\t5', b'chr1\t+\t5', b'chr1\t1\t--5', b'chr1\t0x10\t5',
                                  b'chr1\t1\t5e3'])
def test_lines_outside_the_grammar(line):
    with pytest.raises(vc.BadLine) as err:
        vc.parse_text(b'chr1\t1\t2\n# fine\n' + line + b'\nchr1\tabc\tdef\n')
    assert err.value.number == 3 and err.value.offset == 16 and err.value.line == line


def test_fuzz_cases_are_what_they_say():
    for seed in (1, 5, 7, 35, 36):
        calls, regions, text = vc.fuzz_case(seed)
        assert 1 <= len(calls) <= 2000 and len(regions) <= 20000 and 1 <= len(vc.distinct(calls)) <= 40
        assert all(1 <= b - a <= 10000 for _, a, b in calls)
        assert vc.parse_text(text)[0] == regions
        pieces = vc.cut_lines(text, 7)
        assert b''.join(pieces) == text and all(piece.endswith(b'\n') for piece in pieces[:-1])
    flags, counters = vc.brute_force(calls, regions)
    assert counters['flagged'] == int(flags.sum()) > 0 and counters['overlaps'] >= counters['flagged']


# ---- the host generators ------------------------------------------------------------------------------------------------------------
def test_parse_bed_is_the_restated_grammar():
    import kevlar_amd
    assert list(kevlar_amd.parse_bed(open(vc.BED_TWO, 'r'))) == [('chr17', 3000000, 4000000, []), ('chr17', 36385017, 36385018, [])]
    assert list(kevlar_amd.parse_bed(open(vc.BED_INTERVALS, 'r'))) == [('1', 10, 100, []), ('2', 20, 200, []), ('3', 30, 300, []),
                                                                       ('4', 40, 400, []), ('4', 44, 444, [])]
    assert list(kevlar_amd.parse_bed(['chr1\t+5\t007\tname\t0\n', '#x\n', ' \t\n', ' #c 1 2'])) == [('chr1', 5, 7, ['name', '0']), ('#c', 1, 2, [])]
    assert list(kevlar_amd.parse_bed([b'chr1 1 2\r\n'])) == [('chr1', 1, 2, [])]
    for seed in (3, 11):
        _, regions, text = vc.fuzz_case(seed)
        assert [(c.encode(), s, e) for c, s, e, _ in kevlar_amd.parse_bed(text.split(b'\n'))] == regions
    for line in ('chr1\t5', 'chr1\tabc\t5', 'chr1\t1_000\t5', 'chr1\t1\t{}'.format(2 ** 63), 'chr1\t\xa01\t5'):
        with pytest.raises(ValueError):
            list(kevlar_amd.parse_bed([line]))


def test_bedstream_reads_plain_and_gzip_files():
    import kevlar_amd
    found = list(kevlar_amd.bedstream([vc.BED_SINGLE, vc.BED_SEGDUPS]))
    text = gzip.open(vc.BED_SEGDUPS, 'rb').read()
    assert found[0] == ('chr17', 36385017, 36385018, [])
    assert [(c.encode(), s, e) for c, s, e, _ in found[1:]] == vc.parse_text(text)[0] and len(found) > 20


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_parser_flags_and_defaults():
    import kevlar_amd
    from kevlar_amd import varfilter
    args = kevlar_amd.cli.parser().parse_args(['varfilter', 'mask.bed', 'a.vcf'])
    assert (args.cmd, args.filt, args.vcf, args.out) == ('varfilter', 'mask.bed', ['a.vcf'], None)
    args = kevlar_amd.cli.parser().parse_args(['varfilter', '--out', 'x.vcf', 'mask.bed', 'a.vcf', 'b.vcf.gz'])
    assert (args.filt, args.vcf, args.out) == ('mask.bed', ['a.vcf', 'b.vcf.gz'], 'x.vcf')
    own = varfilter.parser().parse_args(['-o', 'y.vcf', 'mask.bed', 'a.vcf'])
    assert (own.filt, own.vcf, own.out) == ('mask.bed', ['a.vcf'], 'y.vcf')
    with pytest.raises(SystemExit):
        varfilter.parser().parse_args(['mask.bed'])
    assert varfilter.DEFAULT_CHUNK_BYTES == 256 << 20


def test_fourth_dictionary_and_help_text(capsys):
    import kevlar_amd
    cli = kevlar_amd.cli
    assert list(cli.filtering_mains) == ['varfilter']
    assert not set(cli.filtering_mains) & (set(cli.mains) | set(cli.downstream_mains) | set(cli.calling_mains))
    assert set(cli.subparser_funcs) == set(cli.mains) | set(cli.downstream_mains) | set(cli.calling_mains) | set(cli.filtering_mains)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(['--help'])
    assert '"varfilter"' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.parser().parse_args(['varfilter', '--help'])
    assert 'BED file containing regions to filter out' in capsys.readouterr().out
    from kevlar_amd import varfilter
    assert callable(varfilter.varfilter) and callable(varfilter.varfilter_files) and callable(varfilter.main)


def test_the_build_and_the_binding_know_the_new_files():
    import __graft_entry__ as g
    from kevlar_amd import _lib
    assert 'kv_varfilter.hip' in g.HIP_SOURCES and 'kv_varfilter_plan.h' in g.HIP_HEADERS
    assert {'kv_varfilter_create', 'kv_varfilter_scan', 'kv_varfilter_regions', 'kv_varfilter_hits', 'kv_varfilter_stats',
            'kv_varfilter_destroy'} <= set(_lib.SIGNATURES)


# ---- the plan header ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(clang):
        pytest.skip('clang++ of the ROCm toolchain not found')
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HEADERS):
        subprocess.check_call([clang, '-x', 'c++', '-std=c++17', '-O1', '-fPIC', '-shared', '-o', SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_last_error.restype = ctypes.c_char_p
    for name, args in (('h_table_cap', [U64]), ('h_name_hash', [ctypes.c_char_p, U64]), ('h_tile_bytes', [U64]), ('h_n_tiles', [U64, U32]),
                       ('h_tile_lines', [U32]), ('h_chunk_cut', [ctypes.c_char_p, U64, ctypes.c_int])):
        getattr(L, name).restype = U64
        getattr(L, name).argtypes = args
    L.h_is_sep.argtypes = [U32]
    L.h_overlap.argtypes = [I64, I64, I64, I64]
    L.h_number.argtypes = [ctypes.c_char_p, U64, ctypes.POINTER(I64)]
    L.h_table.argtypes = [ctypes.c_char_p, ctypes.c_void_p, U64, ctypes.c_char_p, ctypes.c_void_p, U64, ctypes.c_void_p, ctypes.POINTER(U64)]
    L.h_check_calls.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, U64, U64]
    L.h_check_regions.argtypes = [ctypes.c_void_p, U64, U64, ctypes.POINTER(U64)]
    return L


def constants(lib):
    out = (U64 * 10)()
    lib.h_constants(out)
    return dict(zip(('threads', 'tile_small', 'tile_large', 'large_from', 'lds_before', 'lds_after', 'max_chunk', 'max_calls', 'no_chrom',
                     'table_least'), out))


def test_plan_separators_numbers_and_overlap(lib):
    assert bytes(c for c in range(256) if lib.h_is_sep(c)) == vc.SEPARATORS
    assert not lib.h_is_sep(0x100 + 9) and not lib.h_is_sep(0xFFFFFFFF)
    value = I64()
    tokens = [b'0', b'-0', b'+5', b'007', b'0' * 40 + b'7', b'%d' % (2 ** 63 - 1), b'%d' % -2 ** 63, b'+%d' % (2 ** 63 - 1), b'%d' % 2 ** 63,
              b'%d' % (-2 ** 63 - 1), b'%d' % 2 ** 64, b'9223372036854775810', b'18446744073709551617', b'1' * 30, b'', b'+', b'-', b'+-5', b'5+',
              b'1_000', b'abc', b'1.0', b' 1', b'0x1', b'1e3', b'\xef\xbc\x95']
    for token in tokens:
        want = vc.number(token)
        assert lib.h_number(token, len(token), ctypes.byref(value)) == (want is not None), token
        if want is not None:
            assert value.value == want, token
    edge = [-2 ** 63, -1, 0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 40, 2 ** 63 - 1]
    for s in edge:
        for e in edge:
            for a, b in ((0, 1), (2 ** 31 - 1, 2 ** 31), (-2 ** 63, 2 ** 63 - 1), (2 ** 40, 2 ** 63 - 1), (5, 5)):
                assert bool(lib.h_overlap(s, e, a, b)) == vc.overlaps((s, e), (a, b))


def offsets_of(names):
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(name) for name in names], out=off[1:])
    return off


def test_plan_name_table(lib):
    c = constants(lib)
    assert [lib.h_table_cap(n) for n in (0, 24, 25, 3000)] == [c['table_least'], 64, 128, 8192]
    names = [b'chr1', b'chr10', b'chr11', b'CHR1', b'Chr1', b'', b'c' * 200] + [b'ctg%d' % i for i in range(3000)]
    queries = names + [b'chr', b'chr100', b'c' * 199, b'c' * 201, b'ctg3000', b'chr1\0']
    ids = np.zeros(len(queries), dtype=np.uint32)
    used = U64()
    off, qoff = offsets_of(names), offsets_of(queries)
    rc = lib.h_table(b''.join(names), off.ctypes.data, len(names), b''.join(queries), qoff.ctypes.data, len(queries), ids.ctypes.data, ctypes.byref(used))
    assert rc == KV_OK and used.value == len(names)
    assert ids.tolist() == list(range(len(names))) + [c['no_chrom']] * 6
    # 3000 names in 8192 slots: some of them share a slot to begin with, so a probe walks
    slots = [lib.h_name_hash(name, len(name)) & 8191 for name in names]
    assert len(set(slots)) < len(slots)
    twice = [b'a', b'b', b'a']
    rc = lib.h_table(b''.join(twice), offsets_of(twice).ctypes.data, 3, b'', qoff.ctypes.data, 0, ids.ctypes.data, ctypes.byref(used))
    assert rc == KV_ERR_ARG and b'repeats' in lib.h_last_error()


def test_plan_argument_checks(lib):
    chrom = np.array([0, 2, 1], dtype=np.uint32)
    start = np.array([5, 6, 7], dtype=np.int64)
    assert lib.h_check_calls(chrom.ctypes.data, start.ctypes.data, start.ctypes.data, 3, 3) == KV_OK
    assert lib.h_check_calls(chrom.ctypes.data, start.ctypes.data, start.ctypes.data, 3, 2) == KV_ERR_ARG
    assert lib.h_check_calls(None, None, None, 0, 0) == KV_OK
    known = U64()
    ids = np.array([0, 0xFFFFFFFF, 2, 0xFFFFFFFF], dtype=np.uint32)
    assert lib.h_check_regions(ids.ctypes.data, 4, 3, ctypes.byref(known)) == KV_OK and known.value == 2
    assert lib.h_check_regions(ids.ctypes.data, 4, 2, ctypes.byref(known)) == KV_ERR_ARG


def test_plan_tiles_and_chunk_cuts(lib):
    c = constants(lib)
    assert (c['threads'], c['tile_small'], c['tile_large']) == (256, 4096, 16384)
    assert c['tile_small'] % (4 * c['threads']) == 0 and c['tile_large'] % (4 * c['threads']) == 0      # four bytes a lane a round
    assert (c['lds_before'] + c['lds_after']) % 16 == 0 and c['lds_before'] >= 4
    assert c['tile_large'] < 2 ** 16                                                                    # line starts are 16-bit in LDS
    for n, tile in ((0, 'tile_small'), (1, 'tile_small'), (c['large_from'] - 1, 'tile_small'), (c['large_from'], 'tile_large'),
                    (2 ** 39, 'tile_large')):
        assert lib.h_tile_bytes(n) == c[tile]
    for tile in (c['tile_small'], c['tile_large']):
        assert [lib.h_n_tiles(n, tile) for n in (0, 1, tile - 1, tile, tile + 1, 7 * tile)] == [0, 1, 1, 1, 2, 7]
        assert lib.h_tile_lines(tile) == tile // 2 + 1
        worst = b'a\n' * (tile // 2)                        # the most lines that are not empty a tile can hold
        assert sum(1 for _, line in vc.lines_of(worst) if line) <= lib.h_tile_lines(tile)
    for buffer in (b'', b'\n', b'a', b'a\n', b'a\nb', b'a\nb\n', b'\n\n', b'ab\ncd\nef', b'no line end in here', b'\nabc'):
        for at_eof in (0, 1):
            assert lib.h_chunk_cut(buffer, len(buffer), at_eof) == vc.chunk_cut(buffer, at_eof), (buffer, at_eof)
    assert lib.h_chunk_cut(b'a\nb', 3, 0) == 2 and lib.h_chunk_cut(b'abc', 3, 0) == 0 and lib.h_chunk_cut(b'abc', 3, 1) == 3
    assert lib.h_chunk_cut(None, 0, 0) == 0
