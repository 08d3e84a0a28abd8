"""`kevlar varfilter` on the device (kevlar_amd/csrc/kv_varfilter.hip) against the plain-Python restatement of
tests/varfilter_common.py: in every case the flags per call, the six counters and the first bad line must be the restatement's.
The join alone through kv_varfilter_regions (overlap edges, coordinates at the ends of int64, a long call in front of many short
ones), the name table, the parser on text at the edges of the grammar and of every workgroup tile the planner can choose, chunked
scans, errors, 300 seeded fuzz cases as text and as regions, and the command end to end on the golden fixtures."""
import ctypes
import gzip
import io
import os

import numpy as np
import pytest

import varfilter_common as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vf(hk):
    from kevlar_amd import varfilter
    return varfilter


def device_text(vf, calls, pieces):
    """(flags, counters) of the chunks of a text scanned one after the other"""
    with vf.CallIndex(calls) as index:
        offset = 0
        for piece in pieces:
            index.scan(piece, offset)
            offset += len(piece)
        return index.hits(), index.stats()


def device_regions(vf, calls, regions):
    with vf.CallIndex(calls) as index:
        index.regions(*vc.region_arrays(vc.distinct(calls), regions))
        return index.hits(), index.stats()


def check_text(vf, calls, text, pieces=None):
    want_flags, want = vc.expected(calls, text)
    flags, got = device_text(vf, calls, [text] if pieces is None else pieces)
    assert got == want
    assert flags.tolist() == want_flags.tolist()
    return want


def check_regions(vf, calls, regions):
    want_flags, want = vc.brute_force(calls, regions)
    flags, got = device_regions(vf, calls, regions)
    assert got == dict(want, lines=0, skipped=0)
    assert flags.tolist() == want_flags.tolist()
    return want


# ---- the join -----------------------------------------------------------------------------------------------------------------------
def test_overlap_edges(vf):
    calls = [(b'c', 100, 110)]
    for region, hit in (((90, 100), 0), ((110, 120), 0), ((109, 120), 1), ((90, 101), 1), ((103, 104), 1), ((0, 1000), 1), ((105, 105), 0),
                        ((108, 103), 0), ((-50, 101), 1), ((-50, -10), 0), ((-2 ** 63, 2 ** 63 - 1), 1)):
        assert check_regions(vf, calls, [(b'c',) + region])['flagged'] == hit, region
    inside = [(b'c', 1000, 2000), (b'c', 1400, 1401)]
    assert check_regions(vf, inside, [(b'c', 1400, 1401)])['flagged'] == 2
    assert check_regions(vf, inside, [(b'c', 1500, 1600)])['flagged'] == 1
    assert check_regions(vf, inside, [(b'c', 0, 10 ** 6)])['overlaps'] == 2


def test_identical_calls_and_shared_starts(vf):
    calls = [(b'c', 50, 60)] * 5 + [(b'c', 50, 51), (b'c', 50, 500), (b'c', 49, 50), (b'd', 50, 60), (b'c', 50, 60)]
    assert check_regions(vf, calls, [(b'c', 55, 56)])['flagged'] == 7
    assert check_regions(vf, calls, [(b'c', 50, 51)])['flagged'] == 8
    assert check_regions(vf, calls, [(b'c', 60, 61)])['flagged'] == 1
    assert check_regions(vf, calls, [(b'c', 49, 50), (b'd', 59, 60), (b'e', 0, 100)]) == {'regions': 3, 'known': 2, 'overlaps': 2, 'flagged': 2}


def test_long_call_in_front_of_many_short_ones(vf):
    """the walk back from the binary search must pass 2000 calls that do not reach the region: no window, no count bounds it"""
    calls = [(b'c', 0, 10000)] + [(b'c', 10 + 3 * i, 11 + 3 * i) for i in range(2000)]
    want = check_regions(vf, calls, [(b'c', 9999, 10000)])
    assert want['flagged'] == 1 and want['overlaps'] == 1
    assert check_regions(vf, calls, [(b'c', 6011, 9000)])['flagged'] == 1
    assert check_regions(vf, calls, [(b'c', 6007, 6008)])['flagged'] == 2
    shuffled = [calls[i] for i in np.random.default_rng(1).permutation(len(calls))]
    assert check_regions(vf, shuffled, [(b'c', 9999, 10000), (b'c', 10, 11)])['flagged'] == 2
    check_text(vf, shuffled, b'c\t9999\t10000\nc\t5000\t5002\n')


def test_no_calls_and_no_regions(vf):
    assert check_regions(vf, [], [(b'c', 0, 10)]) == {'regions': 1, 'known': 0, 'overlaps': 0, 'flagged': 0}
    assert check_regions(vf, [(b'c', 0, 10)], []) == {'regions': 0, 'known': 0, 'overlaps': 0, 'flagged': 0}
    assert check_text(vf, [], b'c\t0\t10\n')['known'] == 0
    assert check_text(vf, [(b'c', 0, 10)], b'')['lines'] == 0
    with vf.CallIndex([(b'c', 0, 10)]) as index:
        with pytest.raises(ValueError):
            index.regions([1], [0], [5])                    # one chromosome: id 1 is neither it nor "none"


def test_coordinates_at_the_ends_of_the_range(vf):
    edge = [0, 2 ** 31 - 1, 2 ** 31, 2 ** 40, 2 ** 63 - 1]
    calls = [(b'c', a, b) for a in edge for b in edge if a < b] + [(b'c', -2 ** 63, -2 ** 63 + 1), (b'c', -5, 5)]
    regions = [(b'c', s, e) for s in edge + [-2 ** 63, -1] for e in edge + [1, -2 ** 63 + 1]]
    want = check_regions(vf, calls, regions)
    assert want['flagged'] == len(calls)
    for region in regions[::5]:
        check_regions(vf, calls, [region])
    check_text(vf, calls, b''.join(b'%s\t%d\t%d\n' % r for r in regions))


# ---- names --------------------------------------------------------------------------------------------------------------------------
def test_names_prefixes_case_length_and_absence(vf):
    long_name = b'scaffold_' + b'N' * 191
    names = [b'chr1', b'chr10', b'chr11', b'CHR1', b'Chr1', long_name]
    calls = [(name, 100 * i, 100 * i + 10) for i, name in enumerate(names)]
    for i, name in enumerate(names):
        want = check_text(vf, calls, b'%s\t0\t10000\n' % name)
        assert want['flagged'] == 1 and want['known'] == 1
    absent = [b'chr', b'chr100', b'chr1 ', long_name[:-1], long_name + b'N', b'chrUn', b'chr1\0']
    text = b''.join(b'%s\t0\t10000\n' % name for name in absent)
    want = check_text(vf, calls, text)
    assert want['known'] == 1 and want['regions'] == len(absent)         # b'chr1 ' is chr1 and a separator
    check_text(vf, calls, b''.join(b'%s\t0\t10000\n' % name for name in names + absent))


def test_three_thousand_names(vf):
    names = [b'ctg%d' % i for i in range(3000)]
    calls = [(name, i, i + 2) for i, name in enumerate(names)]
    text = b''.join(b'%s\t%d\t%d\n' % (name, i + 1, i + 2) for i, name in enumerate(names) if i % 3) + b'ctg3000\t0\t9999\nctg\t0\t9999\n'
    want = check_text(vf, calls, text)
    assert want['flagged'] == 2000 and want['known'] == 2000
    check_regions(vf, calls, [(name, i, i + 1) for i, name in enumerate(names)] + [(b'ctg3000', 0, 10)])


# ---- text ---------------------------------------------------------------------------------------------------------------------------
CALLS = [(b'chr1', 100, 101), (b'chr1', 5, 6), (b'chr2', 100, 130), (b'chr1', 7, 8)]

TEXTS = {
    'tabs': b'chr1\t100\t101\nchr2\t0\t5\n',
    'spaces': b'chr1 100 101\nchr2   129   500\n',
    'mixture': b'chr1 \t100\t \t101\nchr2\x0b0\x0c101\nchr1\x1c5\x1d6\x1e\x1f\n',
    'leading and trailing': b' \tchr1\t100\t101\t \n\t\tchr2 100 101  \n',
    'crlf': b'chr1\t100\t101\r\nchr2\t100\t101\r\n\r\n',
    'lone cr': b'chr1\r100\r101\n',
    'extra columns': b'chr1\t100\t101\tname\t0\t+\nchr2\t100\t101\tabc\tdef\tchr1\t5\t6\n',
    'comment first': b'#chr1\t100\t101\nchr2\t100\t101\n#\n# chr1 5 6',
    'not a comment': b' #chr1\t100\t101\nchr1\t5\t6\t#x\n',
    'separator lines': b'\n \n\t\t\n\x0b\x0c\r\n\x1c\x1d\x1e\x1f \nchr1\t5\t6\n\n\n',
    'no final newline': b'chr2\t100\t101\nchr1\t5\t6',
    'empty': b'',
    'one newline': b'\n',
    'comments only': b'# one\n#two\n#\n',
    'signs and zeros': b'chr1\t+5\t007\nchr1\t-5\t+6\nchr1\t-0\t0000000000000000000000000000000006\n',
    'empty and inverted': b'chr1\t5\t5\nchr1\t8\t5\nchr1\t6\t7\n',
    'unicode space': b'chr1\xc2\xa05\t5\t6\nchr1\t5\t6\n',
}


@pytest.mark.parametrize('name', sorted(TEXTS))
def test_text(vf, name):
    check_text(vf, CALLS, TEXTS[name])


def test_long_extra_column_and_long_separator_runs(vf):
    long_column = b'x' * 100000
    check_text(vf, CALLS, b'chr1\t5\t6\t' + long_column + b'\nchr2\t100\t101\n' + b'chr1\t100\t101\t' + long_column)
    check_text(vf, CALLS, b' ' * 100000 + b'chr1' + b'\t' * 70000 + b'5' + b' ' * 5000 + b'6\nchr2\t100\t101\n' + b' ' * 100000 + b'\n')
    check_text(vf, CALLS, b'#' + long_column + b'\nchr1\t5\t6\n')


def tile_sizes(vf):
    from kevlar_amd import _lib
    plan = (ctypes.c_uint64 * 5)()
    _lib.check(_lib.load().kv_varfilter_plan(0, plan))
    return {int(plan[2]): 1, int(plan[3]): int(plan[4])}            # tile -> the least chunk scanned in it


def planned_tile(n_bytes):
    from kevlar_amd import _lib
    plan = (ctypes.c_uint64 * 5)()
    _lib.check(_lib.load().kv_varfilter_plan(n_bytes, plan))
    return int(plan[0])


def filler(n_bytes):
    """n_bytes of lines that hit nothing, the last one ending the filler: long lines, so that the restatement stays quick"""
    assert n_bytes == 0 or n_bytes >= 2
    unit = b'chrF\t1\t2\t' + b'f' * 4086 + b'\n'                    # 4096 bytes
    whole, rest = divmod(n_bytes, len(unit))
    if rest == 1:
        whole, rest = whole - 1, rest + len(unit)
    return unit * whole + (b'#' * (rest - 1) + b'\n' if rest else b'')


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('edge', ['ends on the last byte', 'starts on the last byte', 'straddles', 'newline first in the next tile',
                                  'name straddles', 'number straddles'])
def test_lines_at_the_tile_edge(vf, which, edge):
    """for both tiles the planner can choose: the line around the end of the third tile"""
    tile, least = sorted(tile_sizes(vf).items())[which]
    line = b'chr2\t100\t101\n'
    front = {'ends on the last byte': 3 * tile - len(line), 'starts on the last byte': 3 * tile - 1, 'straddles': 3 * tile - 7,
             'newline first in the next tile': 3 * tile - len(line) + 1, 'name straddles': 3 * tile - 2, 'number straddles': 3 * tile - 6}[edge]
    text = filler(front) + line + b'chr1\t5\t6\n'
    text += filler(max(least - len(text), 0) + 4096)
    assert planned_tile(len(text)) == tile and text[front:front + len(line)] == line
    want = check_text(vf, CALLS, text)
    assert want['flagged'] == 2
    for cut in (front, front + len(line)):                              # and the same with a chunk that ends or begins there
        if cut and planned_tile(cut) == tile and planned_tile(len(text) - cut) == tile:
            check_text(vf, CALLS, text, [text[:cut], text[cut:]])


@pytest.mark.parametrize('which', [0, 1])
def test_tile_of_empty_lines_and_of_shortest_lines(vf, which):
    """as many line starts as a tile can have"""
    tile, least = sorted(tile_sizes(vf).items())[which]
    n = max(least, 3 * tile)
    for text in (b'\n' * n, (b'#\n' * (n // 2)), b'\n' * (n - 11) + b'chr1\t5\t6\n\n\n'):
        assert planned_tile(len(text)) == tile
        with vf.CallIndex(CALLS) as index:
            index.scan(text)
            stats = index.stats()
        assert stats['lines'] == stats['skipped'] + stats['regions'] == text.count(b'\n') and stats['regions'] == text.count(b'chr1')


@pytest.mark.parametrize('lines_per_chunk', [1, 2, 7])
def test_chunked_scan_equals_whole_scan(vf, lines_per_chunk):
    calls, regions, text = vc.fuzz_case(1003)
    text = b'\n'.join(text.split(b'\n')[:400])
    pieces = vc.cut_lines(text, lines_per_chunk)
    assert len(pieces) > 50 and b''.join(pieces) == text
    check_text(vf, calls, text, pieces)


# ---- errors -------------------------------------------------------------------------------------------------------------------------
BAD_LINES = [b'chr1\t5', b'chr1', b'chr1\tabc\t6', b'chr1\t5\tabc', b'chr1\t1_000\t2000', b'chr1\t5\t%d' % 2 ** 63, b'chr1\t%d\t6' % (-2 ** 63 - 1),
             b'chr1\t5\t99999999999999999999999999', b'chr1\t+\t6', b'chr1\t5\t6x', b'chr1\t5.0\t6', b'chr1 5']


@pytest.mark.parametrize('bad', BAD_LINES)
def test_bad_line_is_named(vf, bad, tmp_path):
    text = b'chr1\t5\t6\n# fine\n\n' + bad + b'\nchr2\t100\t101\n'
    with pytest.raises(vc.BadLine) as want:
        vc.expected(CALLS, text)
    assert want.value.number == 4
    with vf.CallIndex(CALLS) as index:
        with pytest.raises(ValueError):
            index.scan(text, 1000)
        assert index.bad_line() == 1000 + want.value.offset
        index.scan(b'chr1\t5\t6\n')                         # a good chunk behind it: nothing is left of the bad one
        assert index.bad_line() is None
    path = tmp_path / 'bad.bed'
    path.write_bytes(text)
    with pytest.raises(ValueError) as err:
        list(vf.varfilter_files([], [str(path)]))
    assert 'line 4:' in str(err.value) and repr(bad.decode()) in str(err.value)


def test_first_of_several_bad_lines_on_repeated_runs(vf, tmp_path):
    """thousands of bad lines in many workgroups: always the first one in file order, also when chunks are small"""
    rng = np.random.default_rng(12)
    lines = [b'chr1\t%d\t%d' % (i, i + 3) for i in range(30000)]
    bad_at = sorted(rng.choice(np.arange(700, 30000), size=3000, replace=False).tolist())
    for at in bad_at:
        lines[at] = BAD_LINES[at % len(BAD_LINES)]
    text = b'\n'.join(lines) + b'\n'
    with pytest.raises(vc.BadLine) as want:
        vc.expected(CALLS, text)
    assert want.value.number == bad_at[0] + 1
    with vf.CallIndex(CALLS) as index:
        for _ in range(5):
            with pytest.raises(ValueError):
                index.scan(text)
            assert index.bad_line() == want.value.offset
    path = tmp_path / 'bad.bed'
    path.write_bytes(text)
    for chunk_bytes in (1 << 28, 5000, 64):
        with pytest.raises(ValueError) as err:
            list(vf.varfilter_files([], [str(path)], chunk_bytes=chunk_bytes))
        assert 'line {}:'.format(bad_at[0] + 1) in str(err.value)


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', range(10))
def test_fuzz(vf, group):
    """300 seeded cases, thirty a group: each as text and through kv_varfilter_regions"""
    for seed in range(30 * group, 30 * group + 30):
        calls, regions, text = vc.fuzz_case(seed)
        want_flags, want = vc.expected(calls, text)
        flags, got = device_text(vf, calls, [text])
        assert got == want, seed
        assert np.array_equal(flags, want_flags), seed
        flags, got = device_regions(vf, calls, regions)
        assert np.array_equal(flags, want_flags), seed
        assert got == dict(want, lines=0, skipped=0), seed


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def vcf_lines(text):
    return [line for line in text.split('\n') if line and not line.startswith('#')]


@pytest.fixture(scope='module')
def bed_files(tmp_path_factory):
    """every golden BED file plain, as gzip and as this package's blocked gzip"""
    from kevlar_amd import bgzf
    root = tmp_path_factory.mktemp('beds')
    files = {}
    for name, path in (('single', vc.BED_SINGLE), ('two', vc.BED_TWO), ('intervals', vc.BED_INTERVALS), ('segdups', vc.BED_SEGDUPS)):
        text = gzip.open(path, 'rb').read() if path.endswith('.gz') else open(path, 'rb').read()
        plain, zipped, blocked = root / (name + '.bed'), root / (name + '.gzip.bed.gz'), root / (name + '.bgzf.bed.gz')
        plain.write_bytes(text)
        zipped.write_bytes(gzip.compress(text))
        with bgzf.BgzfWriter(str(blocked)) as sink:
            sink.write(text)
        files[name] = [str(plain), str(zipped), str(blocked)]
    return files


@pytest.mark.parametrize('vcf', ['five', 'low'])
@pytest.mark.parametrize('bed', ['single', 'two', 'intervals', 'segdups'])
def test_files_equal_parsed_regions(vf, bed_files, bed, vcf):
    import kevlar_amd
    from kevlar_amd.vcf import VCFWriter, vcfstream
    vcf_path = vc.VCF_FIVE if vcf == 'five' else vc.VCF_LOW_ABUND
    writer = VCFWriter(io.StringIO())
    want = [writer.record_line(call) for call in vf.varfilter(vcfstream([vcf_path]), kevlar_amd.parse_bed(open(bed_files[bed][0], 'rb')))]
    calls = [(line.split('\t')[0].encode(), int(line.split('\t')[1]) - 1, int(line.split('\t')[1]) - 1 + len(line.split('\t')[3])) for line in want]
    flags, _ = vc.expected(calls, open(bed_files[bed][0], 'rb').read())
    assert ['UserFilter' in line.split('\t')[6] for line in want] == [bool(flag) for flag in flags]
    for path in bed_files[bed]:
        for chunk_bytes in (vf.DEFAULT_CHUNK_BYTES, 40):
            got = [writer.record_line(call) for call in vf.varfilter_files(vcfstream([vcf_path]), [path], chunk_bytes=chunk_bytes)]
            assert got == want, (path, chunk_bytes)
    if (bed, vcf) == ('two', 'five'):
        assert sorted(line.split('\t')[1] for line in want if '\tUserFilter\t' in line) == ['3547691', '36385018']
    if (bed, vcf) == ('single', 'five'):
        assert [line.split('\t')[1] for line in want if '\tUserFilter\t' in line] == ['36385018']


def test_output_order_and_calls_without_a_position(vf):
    from kevlar_amd.vcf import Variant
    calls = [Variant('b', 5, 'A', 'C'), Variant('a', 9, 'A', 'C'), Variant('.', '.', '.', '.'), Variant('b', 1, 'ACGT', 'A'), Variant('a', 2, 'A', 'C')]
    out = list(vf.varfilter(iter(calls), [('b', 4, 5, []), ('a', 2, 3, ['x'])]))
    assert [(call.seqid, call.position) for call in out] == [('b', 5), ('b', 1), ('a', 9), ('a', 2), ('.', '.')]
    assert [call.filterstr for call in out] == ['PASS', 'UserFilter', 'PASS', 'UserFilter', '.']


def test_command_line(vf, bed_files, tmp_path, capsys):
    import kevlar_amd
    out = tmp_path / 'filtered.vcf'
    for bed in bed_files['two']:
        kevlar_amd.cli.run(['varfilter', '-o', str(out), bed, vc.VCF_FIVE])
        text = out.read_text()
        assert '##source=kevlar::varfilter\n' in text
        assert '##FILTER=<ID=UserFilter,Description="The user has explicitly filtered this variant out' in text
        assert text.split('\n')[[line.startswith('#CHROM') for line in text.split('\n')].index(True)] == '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO'
        calls = vcf_lines(text)
        assert len(calls) == 5
        assert sorted(line.split('\t')[1] for line in calls if '\tUserFilter\t' in line) == ['3547691', '36385018']
    log = capsys.readouterr().err
    assert '[kevlar::varfilter] Loading predictions to filter' in log and '[kevlar::varfilter] Filtering preliminary variant calls' in log
    args = vf.parser().parse_args([bed_files['two'][0], vc.VCF_FIVE])
    vf.main(args)
    printed = capsys.readouterr().out
    assert vcf_lines(printed) == calls
    kevlar_amd.logstream = None
