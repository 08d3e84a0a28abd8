"""Host-side checks of `kevlar call` behind the alignment.  The yardstick first: the plain-Python restatement of the reference's
calling loops (tests/call_common.py), given the score, CIGAR and strand the reference's own aligner returned, prints the VCF
lines the reference printed for every fixture (tests/golden/call/recorded.json).  Then the product's host modules -- vcf, cigar,
varmap's assembly of calls from scan records, call's de-duplication and ordering -- against the recorded lines and the literal
cases of the reference's test_vcf.py and test_cigar.py, with the two device batches answered by the recorded alignments and the
restatement.  No kernel is launched here."""
import io

import numpy as np
import pytest

import call_common as cc


@pytest.fixture(scope='module')
def records():
    return cc.recorded()


@pytest.fixture(scope='module')
def kevlar():
    import __graft_entry__
    __graft_entry__.build()
    import kevlar_amd
    import kevlar_amd.call  # noqa: F401
    return kevlar_amd


def fixture_pairs(fx, part, kevlar):
    """[(partid, [(contig, cutout, score, cigar, strand)])] of one fixture: the product's parsers and the reference's order,
    checked against the names the reference logged"""
    out = []
    for (partid, cutouts, contigs), rec in zip(cc.load_partitions(fx, kevlar), part):
        assert partid == rec['partid']
        pairs = cc.ordered_pairs(cutouts, contigs)
        assert [[contig.name, cutout.defline] for contig, cutout in pairs] == [row[:2] for row in rec['pairs']]
        out.append((partid, [(contig, cutout, row[2], row[3], row[4]) for (contig, cutout), row in zip(pairs, rec['pairs'])]))
    return out


# ---- the yardstick itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fx', cc.FIXTURES, ids=[fx['name'] for fx in cc.FIXTURES])
def test_restatement_prints_the_recorded_lines(fx, records, kevlar):
    part = records['fixtures'][fx['name']]
    assert len(part) >= 1
    for (partid, pairs), rec in zip(fixture_pairs(fx, part, kevlar), part):
        prelim = cc.restate_partition(partid, pairs, fx['ksize'], fx['mindist'], fx['homopolyfilt'])
        assert [call.vcf for call in prelim] == rec['prelim']
        assert [call.vcf for call in cc.merge_adjacent(cc.dedup(prelim))] == rec['final']


def test_restatement_prints_the_forced_mappings(records, kevlar):
    """kevlar/tests/test_varmap.py:18-115: mappings whose CIGAR the test hands over"""
    assert len(records['forced']) == len(cc.FORCED)
    for (contigs, gdnas, score, cigar, ksize), rec in zip(cc.FORCED, records['forced']):
        contig = next(kevlar.parse_augmented_fastx(kevlar.open(cc.data_file(contigs), 'r')))
        cutout = next(kevlar.reference.load_refr_cutouts(kevlar.open(cc.data_file(gdnas), 'r')))
        notes = [(ikmer.offset, ikmer.ksize) for ikmer in contig.annotations]
        mapping = cc.Mapping(contig.sequence, notes, cutout.sequence, score, cigar, 1, cutout._seqid, cutout._startpos)
        assert (mapping.cigar, mapping.vartype) == (rec['cigar'], rec['vartype'])
        assert [call.vcf for call in mapping.call_variants(ksize, 6)] == rec['lines']
    assert records['forced'][-1]['lines'] == [
        'yourchr\t801\t.\t.\t.\t.\tInscrutableCigar\tCIGAR=25D5M22I5M46D8M13D2M35I;KSW2=1000000.0;CONTIG=AACTGGTGGGCTCAAGA'
        'CTAAAAAGACTTTTTTGGTGACAAGCAGGGCGGCCTGCCCTTCCTGTAGTGCAAGAAAAT']


def test_fuzz_generator_makes_the_shares_it_promises():
    jobs = cc.fuzz_jobs()
    assert len(jobs) == 300
    classes, folds = [], 0
    for target, contig, reverse, cigar, notes, wanted, fold in jobs:
        record = cc.job_record(target, contig, reverse, cigar, notes, cc.FUZZ_KSIZE, cc.FUZZ_MINDIST)
        assert record[1] == cc.CLASS_CODE[wanted] and record[0] == int(fold)
        classes.append(record[1])
        folds += record[0]
    assert [classes.count(c) for c in (0, 1, 2)] == [100, 100, 100]
    assert folds == 75
    assert sum(1 for job in jobs if job[2]) > 60
    assert sum(1 for job in jobs if any(cc.job_record(*job[:5], cc.FUZZ_KSIZE, cc.FUZZ_MINDIST)[16:25])) > 30


# ---- kevlar_amd.vcf ------------------------------------------------------------------------------------------------------------
def test_variant_objects(kevlar):
    """kevlar/tests/test_vcf.py:28-82, 248-256"""
    from kevlar_amd.vcf import Variant, VariantFilter as vf
    snv = Variant('scaffold42', 10773, 'A', 'G')
    assert str(snv) == 'scaffold42:10773:A->G'
    assert snv.vcf == '\t'.join(['scaffold42', '10774', '.', 'A', 'G', '.', 'PASS', '.'])
    assert snv.cigar is None
    snv2 = Variant('chr5', 500, 'T', 'G', CIGAR='10D200M10D')
    assert snv2.cigar == '10D200M10D' and snv2.window is None and snv2.windowlength == 0
    indel1 = Variant('chr3', 8998622, 'GATTACA', 'G')
    assert str(indel1) == 'chr3:8998623:6D'
    assert indel1.vcf == '\t'.join(['chr3', '8998623', '.', 'GATTACA', 'G', '.', 'PASS', '.'])
    indel2 = Variant('chr6', 75522411, 'G', 'GATTACA')
    assert str(indel2) == 'chr6:75522412:I->ATTACA'
    assert indel2.vcf == '\t'.join(['chr6', '75522412', '.', 'G', 'GATTACA', '.', 'PASS', '.'])
    v = Variant('scaffold1', 12345, '.', '.')
    assert v.filterstr == '.'
    v.filter(vf.InscrutableCigar)
    assert v.filterstr == 'InscrutableCigar'
    v = Variant('1', 809768, 'C', 'CAT')
    assert v.filterstr == 'PASS'
    v.filter(vf.PassengerVariant)
    v.filter(vf.Homopolymer)
    assert v.filterstr == 'Homopolymer;PassengerVariant'
    v = Variant('one', 112358, 'T', 'A')
    for junk in ('SNPyMcSNPface', 6.022e23, dict(chicken='waffles')):
        v.filter(junk)
    assert v.filterstr == 'PASS'
    assert Variant('chr12', 1033773, 'A', 'G').region == ('chr12', 1033773, 1033774)
    assert Variant('chr12', 1033773, 'A', 'AGTG').region == ('chr12', 1033773, 1033774)
    assert Variant('chr12', 1033773, 'ATACCG', 'A').region == ('chr12', 1033773, 1033779)
    assert [kind.value for kind in vf] == list(range(1, 12)) and vf.AmbiguousCall.value == 11
    nocall = Variant('.', '.', '.', '.', CONTIG='ACGT', IKMERS='3')
    assert nocall.vcf == '.\t.\t.\t.\t.\t.\t.\tIKMERS=3;CONTIG=ACGT'


def test_info_and_format(kevlar):
    """kevlar/tests/test_vcf.py:85-143"""
    from kevlar_amd.vcf import FormattedList, KevlarMixedDataTypeError, Variant
    values = FormattedList()
    assert str(values) == '.'
    values.append(42)
    values.append(1776)
    assert str(values) == '42,1776'
    values.append('B0gU$')
    with pytest.raises(KevlarMixedDataTypeError, match='mixed data type'):
        str(values)
    v = Variant('1', 12345, 'G', 'C')
    assert v.attribute('VW') is None
    v.annotate('VW', 'GATTACA')
    assert v.attribute('VW') == 'GATTACA' and v.attribute('VW', pair=True) == 'VW=GATTACA'
    v.annotate('VW', 'ATGCCCTAG', replace=False)
    assert v.attribute('VW') == ['GATTACA', 'ATGCCCTAG']
    assert v.attribute('VW', string=True) == 'GATTACA,ATGCCCTAG'
    v.annotate('DROPPED', 3)
    assert v.attribute('DROPPED') == 3 and v.attribute('DROPPED', string=True) == '3'
    v.annotate('DROPPED', 31, replace=False)
    assert v.attribute('DROPPED', pair=True) == 'DROPPED=3,31'
    v.annotate('MATEDIST', 432.1234, replace=False)
    v.annotate('MATEDIST', 8765.4321, replace=False)
    assert v.attribute('MATEDIST', string=True) == '432.123,8765.432'
    v.annotate('LLIH', np.float64(-436.0111857750478))
    assert v.attribute('LLIH', pair=True) == 'LLIH=-436.011'
    v.format('NA19238', 'GT', '0/0')
    assert v.format('NA19238', 'GT') == '0/0'
    assert v.format('NA19238', 'XYZ') is None and v.format('NA19239', 'GT') is None


def test_writer_header_and_sample_columns(records, kevlar):
    """the header is the reference's, byte for byte but for the date; kevlar/tests/test_vcf.py:146-193"""
    from datetime import date
    from kevlar_amd.vcf import Variant, VariantAnnotationError, VCFWriter
    out = io.StringIO()
    VCFWriter(out, source='kevlar::call').write_header()
    lines = out.getvalue().split('\n')
    assert lines[-1] == '' and lines[1] == '##fileDate=' + date.today().isoformat()
    assert lines[:1] + lines[2:-1] == records['header']
    out = io.StringIO()
    VCFWriter(out, source=None, refr='genome.fa').write_header(skipdate=True)
    assert out.getvalue().split('\n')[:2] == ['##fileformat=VCFv4.2', '##reference=genome.fa']

    def writer(stream):
        made = VCFWriter(stream, source='py.test')
        for label in ('NA19238', 'NA19239', 'NA19240'):
            made.register_sample(label)
        made.describe_format('GT', 'String', '1', 'Genotype')
        return made

    out = io.StringIO()
    yrb = writer(out)
    yrb.write_header()
    v = Variant('1', 12345, 'G', 'C')
    v.annotate('PART', '42')
    v.annotate('CONTIG', 'A' * 100)
    for label, gt, abund in (('NA19238', '0/0', '12,9,8'), ('NA19239', '0/0', '0,0,0'), ('NA19240', '0/1', '0,0,0')):
        v.format(label, 'GT', gt)
        v.format(label, 'ALTABUND', abund)
    yrb.write(v)
    lines = out.getvalue().strip().split('\n')
    assert '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">' in lines
    assert len([ln for ln in lines if ln.startswith('##FORMAT')]) == 2
    assert lines[-2].split('\t')[8:] == ['FORMAT', 'NA19238', 'NA19239', 'NA19240']
    assert lines[-1].split('\t')[8:12] == ['ALTABUND:GT', '12,9,8:0/0', '0,0,0:0/0', '0,0,0:0/1']
    bad = Variant('1', 12345, 'G', 'C')
    bad.format('NA19238', 'GT', '0/0')
    bad.format('NA19240', 'GT', '0/1')
    bad.format('NA19239', 'ALTABUND', '0,0,0')
    bad.format('NA19240', 'ALTABUND', '0,0,0')
    with pytest.raises(VariantAnnotationError, match='samples not annotated with the same FORMAT fields'):
        writer(io.StringIO()).write(bad)


def test_reader_and_round_trip(kevlar, kevlar_log):
    """kevlar/tests/test_vcf.py:196-245"""
    from kevlar_amd.vcf import VariantAnnotationError, VCFReader, VCFWriter, vcfstream
    calls = list(VCFReader(kevlar.open(cc.data_file('five-snvs-with-likelihood.vcf.gz'), 'r')))
    assert len(calls) == 5
    assert calls[1].attribute('PART') == '54'
    assert calls[3].format('Kid', 'ALTABUND') == ('21,20,20,19,17,19,20,19,18,17,17,17,17,17,17,17,18,19,19,19,18,18,18,'
                                                  '17,19,18,17,17,17,15,15')
    assert [str(c) for c in vcfstream([cc.data_file('five-snvs-with-likelihood.vcf.gz')])] == [str(c) for c in calls]
    # kevlar/tests/test_vcf.py:209-217: a fourth sample label over three sample columns; a sample column one value short
    lines = kevlar.open(cc.data_file('five-snvs-with-likelihood.vcf.gz'), 'r').read().strip().split('\n')
    at = [n for n, line in enumerate(lines) if line.startswith('#CHROM')][0]
    with pytest.raises(VariantAnnotationError, match='sample number mismatch'):
        list(VCFReader(lines[:at] + [lines[at] + '\tSibling'] + lines[at + 1:]))
    assert lines[at + 2].split('\t')[8].count(':') >= 1
    with pytest.raises(VariantAnnotationError, match='format data mismatch'):
        list(VCFReader(lines[:at + 2] + [lines[at + 2].rsplit(':', 1)[0]] + lines[at + 3:]))
    assert len(list(VCFReader(lines[:at + 1] + ['# a comment'] + lines[at + 1:]))) == 5
    out = io.StringIO()
    writer = VCFWriter(out, source=None, refr='GCA_000001405.15_GRCh38_no_alt_analysis_set.fna.gz')
    for label in ('Kid', 'Mom', 'Dad'):
        writer.register_sample(label)
    writer.describe_format('GT', 'String', '1', 'Genotype')
    writer.write_header(skipdate=True)
    for call in calls:
        writer.write(call)
    again = list(VCFReader(out.getvalue().strip().split('\n')))
    assert [c.position for c in calls] == [c.position for c in again]
    assert [str(c) for c in calls] == [str(c) for c in again]
    assert [c.window for c in calls] == [c.window for c in again]
    assert [c.format('Kid', 'ALTABUND') for c in calls] == [c.format('Kid', 'ALTABUND') for c in again]


def parsed(lines):
    from kevlar_amd.vcf import VCFReader
    reader = VCFReader([])
    reader.suppress_filter_warnings = True
    return [reader._variant_from_vcf_string(line) for line in lines]


def test_recorded_lines_survive_reader_and_writer(records, kevlar):
    from kevlar_amd.vcf import VCFWriter
    for name, part in records['fixtures'].items():
        for rec in part:
            out = io.StringIO()
            writer = VCFWriter(out)
            for call in parsed(rec['prelim']):
                writer.write(call)
            assert out.getvalue() == ''.join(line + '\n' for line in rec['prelim']), name


def test_dedup_and_merge_adjacent_give_the_recorded_final_lines(records, kevlar):
    """the product's dedup and merge_adjacent (and Variant.test_merge under them) on the reference's preliminary calls"""
    from kevlar_amd.call import dedup, merge_adjacent
    merged = shrunk = 0
    for name, part in records['fixtures'].items():
        for rec in part:
            final = [call.vcf for call in merge_adjacent(dedup(parsed(rec['prelim'])))]
            assert final == rec['final'], name
            shrunk += len(rec['final']) < len(rec['prelim'])
            merged += sum(1 for line in rec['final'] if len(line.split('\t')[3]) > 1 and len(line.split('\t')[3]) == len(line.split('\t')[4]))
    assert merged >= 2 and shrunk >= 3        # the mnv and ant fixtures merge, bee-dupl and multibestrc de-duplicate


def test_test_merge_refuses_what_the_reference_refuses(kevlar):
    from kevlar_amd.vcf import Variant
    a = Variant('chr1', 100, 'A', 'C', ALTWINDOW='TTCGG', REFRWINDOW='TTAGG')
    b = Variant('chr1', 101, 'G', 'T', ALTWINDOW='TCTGC', REFRWINDOW='TAGGC')
    assert Variant('.', 100, 'A', 'C').test_merge(b) is None
    assert Variant('chr2', 100, 'A', 'C', ALTWINDOW='TTCGG', REFRWINDOW='TTAGG').test_merge(b) is None
    assert Variant('chr1', 100, 'A', 'CC', ALTWINDOW='TTCGG', REFRWINDOW='TTAGG').test_merge(b) is None
    assert Variant('chr1', 99, 'A', 'C', ALTWINDOW='TTCGG', REFRWINDOW='TTAGG').test_merge(b) is None
    assert Variant('chr1', 100, 'A', 'C').test_merge(b) is None
    assert a.test_merge(Variant('chr1', 101, 'G', 'T', ALTWINDOW='TCTGC')) is None
    assert a.test_merge(b) is None                  # windows that do not continue each other
    c = Variant('chr1', 101, 'G', 'T', ALTWINDOW='TCTGC', REFRWINDOW='TAGGC')
    d = Variant('chr1', 100, 'A', 'C', ALTWINDOW='TTCTG', REFRWINDOW='TTAGG')
    merged = d.test_merge(c)
    assert merged is d and (d._refr, d._alt, d.window, d.refrwindow) == ('AG', 'CT', 'TTCTGC', 'TTAGGC')


def test_alignments_to_report(kevlar):
    from collections import namedtuple
    from kevlar_amd.call import alignments_to_report
    Aln = namedtuple('Aln', 'vartype score')
    assert alignments_to_report([]) == []
    one = [Aln(None, 3)]
    assert alignments_to_report(one) is one
    alns = [Aln(None, 90), Aln('snv', 50), Aln('indel', 70), Aln('snv', 70)]
    assert alignments_to_report(alns) == [alns[2], alns[3]]
    alns = [Aln(None, 90), Aln(None, 50), Aln(None, 90)]
    assert alignments_to_report(alns) == [alns[0], alns[2]]


# ---- kevlar_amd.cigar and the functions of kevlar_amd.varmap -------------------------------------------------------------------
def test_tokenizer_against_the_restatement(records, kevlar):
    """every recorded alignment: blocks, end check and rewritten CIGAR; kevlar/tests/test_cigar.py:52-65 literally"""
    from kevlar_amd.cigar import AlignmentBlock, AlignmentTokenizer
    folded = 0
    for fx in cc.FIXTURES:
        for partid, pairs in fixture_pairs(fx, records['fixtures'][fx['name']], kevlar):
            for contig, cutout, score, cigar, strand in pairs:
                if cigar is None:
                    continue
                query = contig.sequence if strand == 1 else cc.revcom(contig.sequence)
                assert query == (contig.sequence if strand == 1 else kevlar.revcom(contig.sequence))
                blocks = cc.tokenize(query, cutout.sequence, cigar)
                did = cc.endcheck(blocks)
                tok = AlignmentTokenizer(query, cutout.sequence, cigar)
                assert tok.folded == did and tok._origcigar == cigar
                assert tok.blocks == [AlignmentBlock(*block) for block in blocks]
                assert tok._cigar == ''.join('{}{}'.format(block[0], block[1]) for block in blocks)
                assert AlignmentTokenizer(query, cutout.sequence, cigar, folded=did).blocks == tok.blocks
                folded += did
    assert folded >= 5
    for name, newcigar, origcigar, nblocks in (('cigar-b', '41D150M50D', '41D144M50D6M', 3), ('cigar-d', '39D129M4D43M6D', '39D129M4D29M6D14M', 5)):
        (partid, pairs), = fixture_pairs(cc.FIXTURE_BY_NAME[name], records['fixtures'][name], kevlar)
        (contig, cutout, score, cigar, strand), = pairs
        tok = AlignmentTokenizer(contig.sequence, cutout.sequence, cigar)
        assert (tok._cigar, tok._origcigar, len(tok.blocks)) == (newcigar, origcigar, nblocks)


def test_varmap_functions(kevlar):
    from kevlar_amd.varmap import cigar_runs, n_ikmers_present, trim_terminal_snvs
    assert trim_terminal_snvs([0, 4, 5, 50, 95, 96, 99], 100, 5) == (4, [5, 50, 95])
    assert trim_terminal_snvs([1, 2], 10) == (2, [])
    assert trim_terminal_snvs([], 10, 3) == (0, [])
    record = kevlar.Record('r', 'ACGTTGCAAGGCTT')
    record.annotate('GTTGC', 2, (9, 0))
    record.annotate('AAGGC', 7, (9, 0))
    record.annotate('GTTGC', 2, (9, 0))
    assert n_ikmers_present(record, 'TTGTTGCTT') == 2                 # the duplicate counts again
    assert n_ikmers_present(record, 'TTGCCTTAA') == 1                 # only as its reverse complement
    assert n_ikmers_present(record, 'GTTG') == 0
    assert cigar_runs('10D91M69D79M20I') == [10 << 4 | 2, 91 << 4, 69 << 4 | 2, 79 << 4, 20 << 4 | 1]


def test_parser_defaults(kevlar):
    args = kevlar.call.parser().parse_args(['contigs.augfasta', 'targets.fa'])
    assert (args.queryseq, args.targetseq, args.out, args.refr, args.ksize) == ('contigs.augfasta', 'targets.fa', None, None, 31)
    assert (args.match, args.mismatch, args.open, args.extend, args.debug) == (1, 2, 5, 0, False)
    assert (args.no_homopoly_filter, args.max_target_length, args.gen_mask, args.mask_mem, args.mask_max_fpr) == (False, 10000, None, 1e6, 0.01)
    args = kevlar.call.parser().parse_args(['-A', '2', '-B', '3', '-O', '6', '-E', '1', '-d', '--no-homopoly-filter', '--max-target-length', '50',
                                            '--gen-mask', 'm.nt', '--mask-mem', '1M', '--mask-max-fpr', '0.1', '--refr', 'g.fa', '-o', 'o.vcf',
                                            '-k', '25', 'q', 't'])
    assert (args.match, args.mismatch, args.open, args.extend, args.debug, args.no_homopoly_filter) == (2, 3, 6, 1, True, True)
    assert (args.max_target_length, args.gen_mask, args.mask_mem, args.mask_max_fpr, args.refr, args.out, args.ksize) == (
        50, 'm.nt', 1e6, 0.1, 'g.fa', 'o.vcf', 25)
    assert 'call' not in kevlar.cli.mains


# ---- the assembly of calls from scan records, the two device batches answered here ---------------------------------------------
@pytest.fixture
def answered(monkeypatch, records, kevlar):
    """align_partitions answers with the recorded alignments of the fixture set in `answered.fixture`, scan_batch with the
    restatement's records"""
    from kevlar_amd import varmap

    class State(object):
        fixture = None
        scans = 0

    def align_partitions(contigs_by_partition, cutouts_by_partition, match=1, mismatch=2, gapopen=5, gapextend=0, maxtargetlen=10000,
                         z_budget=None):
        wanted = iter(fixture_pairs(State.fixture, records['fixtures'][State.fixture['name']], kevlar))
        cutouts_by_partition = dict(cutouts_by_partition)
        for partid, contigs in contigs_by_partition:
            ref_partid, pairs = next(wanted)
            assert partid == ref_partid
            ours = cc.ordered_pairs(cutouts_by_partition[partid], contigs)
            assert [(a.name, b.defline) for a, b in ours] == [(row[0].name, row[1].defline) for row in pairs]
            for (contig, cutout), row in zip(ours, pairs):
                assert (row[3] is None) == bool(maxtargetlen and len(cutout) > maxtargetlen)
                yield (partid, contig, cutout) + tuple(row[2:])

    def scan_batch(targets, queries, jobs, cigars, annotations, ksize, mindist):
        State.scans += 1
        made = []
        for (t, q, rev), cigar in zip(jobs, cigars):
            words = np.zeros(32, dtype=np.uint32)
            words[:25] = cc.job_record(targets[t], queries[q], rev, cigar, annotations[q], ksize, mindist)
            made.append(varmap.ScanRecord(words))
        return made

    monkeypatch.setattr(kevlar.call, 'align_partitions', align_partitions)
    monkeypatch.setattr(kevlar.call, 'scan_batch', scan_batch)
    return State


@pytest.mark.parametrize('fx', cc.FIXTURES, ids=[fx['name'] for fx in cc.FIXTURES])
def test_calls_assembled_from_records_are_the_recorded_lines(fx, answered, records, kevlar, kevlar_log):
    answered.fixture = fx
    parts = cc.load_partitions(fx, kevlar)
    kwargs = dict(ksize=fx['ksize'], mindist=fx['mindist'], homopolyfilt=fx['homopolyfilt'], maxtargetlen=fx['maxtargetlen'])
    found = list(kevlar.call.call_partitions({partid: contigs for partid, cutouts, contigs in parts},
                                             [(partid, cutouts) for partid, cutouts, contigs in parts], **kwargs))
    assert answered.scans <= 1
    wanted = [(rec['partid'], line) for rec in records['fixtures'][fx['name']] for line in rec['final']]
    assert [(partid, call.vcf) for partid, call in found] == wanted
    for (partid, cutouts, contigs), rec in zip(parts, records['fixtures'][fx['name']]):
        if len(parts) == 1:
            prelim = list(kevlar.call.prelim_call(cutouts, contigs, partid=partid, **kwargs))
            assert [call.vcf for call in prelim] == rec['prelim']


# ---- the library's argument checks: host code, nothing is launched --------------------------------------------------------------
@pytest.mark.parametrize('name,change', cc.ARGUMENT_ERRORS, ids=[name for name, change in cc.ARGUMENT_ERRORS])
def test_scan_refuses_wrong_arguments_before_the_device(name, change, kevlar):
    from kevlar_amd import _lib
    rc, words = cc.raw_scan(_lib.load(), **dict(cc.GOOD_CALL, **change))
    assert rc == _lib.KV_ERR_ARG
    assert (words == cc.UNTOUCHED).all()
    with pytest.raises(_lib.KvArgError):
        _lib.check(rc)
