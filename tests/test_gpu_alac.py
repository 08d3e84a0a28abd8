"""`kevlar alac` on the device: alac() against the same work done step by step (assemble, localize, call_partitions), the command
line against both, and the calls the reference's kevlar/tests/test_alac.py states (tests/golden/assemble/recorded.json).

Of the 11 stated calls (fiveparts labels 1-5 by position, six pico-var partitions by position, REF and ALT) 10 agree; pico-var/cc2
does not, and what is produced instead is asserted and explained below and in DESIGN.md section 13."""
import filecmp
import os
from collections import defaultdict

import pytest

import kevlar_amd
from kevlar_amd import khmer
from kevlar_amd.alac import alac
from kevlar_amd.assemble import assemble
from kevlar_amd.call import call_partitions
from kevlar_amd.localize import localize

import assemble_common as ac

pytestmark = pytest.mark.gpu

FIVE = ac.fixture_path('fiveparts.augfastq.gz')
FIVE_REFR = ac.fixture_path('fiveparts-refr.fa.gz')
PICO_REFR = ac.fixture_path('human-random-pico.fa.gz')


def stream(path, label=None):
    reads = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(path, 'r'))
    return kevlar_amd.parse_single_partition(reads, label) if label else kevlar_amd.parse_partitioned_reads(reads)


def step_by_step(path, refr, label=None, seedsize=31, delta=50, ksize=31, exclpattern=None):
    """the calls of alac()'s stages run one after the other, sorted as alac() sorts them"""
    contigs = defaultdict(list)
    for partid, contig in assemble(stream(path, label)):
        contigs[partid].append(contig)
    targets = defaultdict(list)
    for partid, gdna in localize(list(contigs.items()), refr, seedsize=seedsize, delta=delta, exclpattern=exclpattern):
        targets[partid].append(gdna)
    calls = [c for partid, c in call_partitions(contigs, [(p, targets[p]) for p in sorted(targets)], ksize=ksize, refrfile=refr)]
    return sorted(calls, key=lambda c: (c.seqid, c.position))


def body(text):
    return [ln for ln in text.split('\n') if ln and not ln.startswith('#')]


@pytest.fixture(scope='module')
def five_calls(hk):
    """alac() over all five partitions, computed once"""
    return list(alac(stream(FIVE), FIVE_REFR))


def test_alac_equals_its_steps(hk, five_calls):
    steps = step_by_step(FIVE, FIVE_REFR)
    assert [c.vcf for c in five_calls] == [c.vcf for c in steps] and len(steps) == 5
    assert [c.position for c in five_calls] == sorted(c.position for c in five_calls)
    one = list(alac(stream(FIVE, '3'), FIVE_REFR))
    assert [c.vcf for c in one] == [c.vcf for c in step_by_step(FIVE, FIVE_REFR, label='3')] == [c.vcf for c in five_calls if c.attribute('PART') == '3']
    # accepted and ignored, accepted and unused
    assert [c.vcf for c in alac(stream(FIVE), FIVE_REFR, threads=8, min_ikmers=3)] == [c.vcf for c in five_calls]
    # the parameters of the assembly rule reach the assembly
    other = list(alac(stream(FIVE), FIVE_REFR, asmk=25, mincount=3))
    assert len(other) == 5 and [c.attribute('CONTIG') for c in other] != [c.attribute('CONTIG') for c in five_calls]


def test_alac_through_the_command_line(hk, five_calls, tmp_path, capsys, kevlar_log):   # (kevlar_log: run() redirects the log; the fixture puts it back)
    out = str(tmp_path / 'calls.vcf')
    kevlar_amd.cli.run(['alac', '--seed-size', '31', '-o', out, FIVE, FIVE_REFR])
    text = open(out).read()
    assert body(text) == [c.vcf for c in five_calls]
    assert '##source=kevlar::alac' in text and FIVE_REFR in text
    kevlar_amd.cli.run(['alac', '--seed-size', '31', '--part-id', '2', FIVE, FIVE_REFR])
    stdout, err = capsys.readouterr()
    assert body(stdout) == [c.vcf for c in five_calls if c.attribute('PART') == '2'] and len(body(stdout)) == 1
    # the command line's own seed size is 51, the function's is 31, as in the reference
    kevlar_amd.cli.run(['alac', FIVE, FIVE_REFR])
    stdout, err = capsys.readouterr()
    assert body(stdout) == [c.vcf for c in step_by_step(FIVE, FIVE_REFR, seedsize=51)]


def test_alac_bad_label_and_exclude_give_nothing(hk, capsys, kevlar_log):
    kevlar_amd.cli.run(['alac', '--part-id', '6', FIVE, FIVE_REFR])
    out, err = capsys.readouterr()
    assert body(out) == [] and '##fileformat' in out
    kevlar_amd.cli.run(['alac', '--exclude', '^seq', FIVE, FIVE_REFR])
    out, err = capsys.readouterr()
    assert body(out) == [] and 'WARNING: no reference matches' in err
    assert step_by_step(FIVE, FIVE_REFR, exclpattern='^seq') == []
    assert 'WARNING: no reference matches' in kevlar_log.getvalue() + capsys.readouterr().err


def test_alac_max_reads(hk, five_calls):
    calls = list(alac(stream(FIVE), FIVE_REFR, maxreads=20))         # kevlar/tests/test_alac.py: test_alac_bigpart states 3
    assert [c.attribute('PART') for c in calls] == [c.attribute('PART') for c in five_calls if c.attribute('PART') in '345']
    assert len(calls) == 3


def test_alac_generates_the_mask(hk, five_calls, tmp_path, capsys, kevlar_log):
    by_function, by_cli, by_hand = (str(tmp_path / name) for name in ('function.nt', 'cli.nt', 'hand.nt'))
    calls = list(alac(stream(FIVE), FIVE_REFR, maskfile=by_function, maskmem=1e6))
    assert [c.vcf for c in calls] == [c.vcf for c in five_calls]
    kevlar_amd.cli.run(['alac', '--seed-size', '31', '--gen-mask', by_cli, '-o', str(tmp_path / 'calls.vcf'), FIVE, FIVE_REFR])
    # the nodetable consumed from the calls' ALTWINDOWs
    mask = khmer.Nodetable(31, 1e6 * khmer._buckets_per_byte['nodegraph'] / 4, 4)
    windows = [c.attribute('ALTWINDOW') for c in five_calls]
    assert len(windows) == 5 and all(len(w) >= 31 for w in windows)
    for window in windows:
        mask.consume(window)
    mask.save(by_hand)
    assert filecmp.cmp(by_function, by_hand, shallow=False) and filecmp.cmp(by_cli, by_hand, shallow=False)
    # kevlar/tests/test_alac.py: test_alac_generate_mask compares with this file: the five ALTWINDOWs are the reference's
    assert filecmp.cmp(by_function, ac.fixture_path('fiveparts-genmask.nodetable'), shallow=False)
    capsys.readouterr()
    list(alac(stream(FIVE), FIVE_REFR, maskfile=by_function, maskmem=100))
    # (kevlar/tests/test_alac.py: test_alac_generate_mask_lowmem)
    assert 'WARNING: mask FPR is 0.8065; exceeds user-specified limit of 0.0100' in capsys.readouterr().err + kevlar_log.getvalue()


# ---- the reference's stated calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ac.recorded()['fiveparts_calls'], ids=lambda row: 'label' + row['label'])
def test_fiveparts_stated_positions(hk, row):
    calls = list(alac(stream(FIVE, row['label']), FIVE_REFR))
    assert len(calls) == 1
    assert calls[0].position == row['position'] and calls[0].attribute('PART') == row['label']


@pytest.mark.parametrize('row', [r for r in ac.recorded()['pico_calls'] if r['cc'] != 2], ids=lambda row: 'cc{}'.format(row['cc']))
def test_pico_stated_calls(hk, row):
    calls = list(alac(stream(ac.fixture_path('pico-var/cc{}.afq.gz'.format(row['cc']))), PICO_REFR, ksize=25, delta=50))
    assert len(calls) == 1
    assert (calls[0]._pos, calls[0]._refr, calls[0]._alt) == (row['pos'], row['ref'], row['alt'])


def test_pico_cc2_is_the_one_that_does_not_agree(hk):
    # The reference states a 160-base insertion behind seq1:834645.  The reads of this partition carry further differences inside
    # the insertion that are seen at least twice, so the graph forks there: five unitigs of 32 to 53 bases, none longer than a
    # read, cover bases 51 to 121 of the insertion, and the two contigs stop on either side of them -- 162 bases (80 of the left
    # flank, the first 81 of the insertion) and 165 bases (the last 69 of the insertion, 96 of the right flank).  Neither spans
    # the insertion with both flanks, no alignment has the shape of a variant, and the result is one no-call at the start of
    # the cutout.  fermi-lite pops such bubbles; the rule has no bubble popping.
    row = [r for r in ac.recorded()['pico_calls'] if r['cc'] == 2][0]
    assert (row['pos'], row['ref'], len(row['alt'])) == (834645, 'A', 161)
    name = 'pico-var/cc2.afq.gz'
    assert [len(c) for c in ac.contigs(ac.all_reads(name))] == [165, 162]
    calls = list(alac(stream(ac.fixture_path(name)), PICO_REFR, ksize=25, delta=50))
    assert [(c.seqid, c._pos, c._refr, c._alt, c.filterstr) for c in calls] == [('seq1', 834515, '.', '.', 'InscrutableCigar')]


def test_pico_4_is_the_reference_s_call(hk, capsys, kevlar_log):
    # kevlar/tests/test_alac.py: test_pico_4 states the whole line; position, alleles, filter and both windows are the same here,
    # the contig is 183 bases where fermi-lite's is 192, and CIGAR and score follow the contig
    kevlar_amd.cli.run(['alac', '--ksize', '25', ac.fixture_path('pico-4.augfastq.gz'), PICO_REFR])
    out, err = capsys.readouterr()
    lines = body(out)
    assert len(lines) == 1
    fields = lines[0].split('\t')
    assert fields[:7] == ['seq1', '1175768', '.', 'T', 'C', '.', 'PASS']
    info = dict(item.split('=') for item in fields[7].split(';'))
    assert info['ALTWINDOW'] == 'CCCTGCCATTATAGATGCTAGATTCACATCTTCATTTATTTTTACTTTT'
    assert info['REFRWINDOW'] == 'CCCTGCCATTATAGATGCTAGATTTACATCTTCATTTATTTTTACTTTT'
    assert info['IKMERS'] == '25' and info['CIGAR'] == '50D183M50D'
    stated = ('ACCTGATTTTGAAGAAGAAAATCAGTTTAAGTCAAAAGGTTACTTTCCTTGTCCTGAACTGGAGAACTGGGGCCCTGCCATTATAGATGCTAGATTCACATCTTCATTTATTTTTACTTTTTGTCT'
              'TGACAGAGTGGGCGCTGGTTTTTTTAATTATTTTTGGCCAATCAAAAAATACTCTCCTTCGTGGGT')
    assert info['CONTIG'] in stated and len(stated) == 192
