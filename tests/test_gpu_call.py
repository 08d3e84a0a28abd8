"""`kevlar call` behind the alignment on the device (kevlar_amd/csrc/kv_call.hip through kevlar_amd.varmap and kevlar_amd.call):
the scan's records against the plain-Python restatement of tests/call_common.py, job for job and word for word, and the calls
of every fixture against the VCF lines the reference itself printed (tests/golden/call/recorded.json) -- never against itself."""
import os
import random
import subprocess
import sys

import pytest

import kevlar_amd
import kevlar_amd.call
from kevlar_amd import _lib, varmap

import call_common as cc

pytestmark = pytest.mark.gpu
K, DIST = 31, 5


@pytest.fixture(scope='module', autouse=True)
def device(hk):
    assert varmap.RECORD_WORDS == cc.RECORD_WORDS
    return hk


@pytest.fixture(scope='module')
def records():
    return cc.recorded()


def device_records(jobs, ksize, mindist):
    """jobs: [(target, contig, reverse, cigar, annotations)], each with sequences of its own; one batch"""
    index = [(k, k, job[2]) for k, job in enumerate(jobs)]
    got = varmap.scan_batch([job[0] for job in jobs], [job[1] for job in jobs], index, [job[3] for job in jobs],
                            [job[4] for job in jobs], ksize, mindist)
    assert len(got) == len(jobs)
    return [record.astuple() for record in got]


def agree(jobs, ksize=K, mindist=DIST):
    """every job of one batch against the restatement; returns the records"""
    got = device_records(jobs, ksize, mindist)
    for k, job in enumerate(jobs):
        assert got[k] == cc.job_record(*job[:5], ksize, mindist), (k, job[3], job[2], ksize, mindist)
    return got


def every_kmer(query, reverse, size, step=1):
    """annotations for every `step`-th window of `size` bases of the query as the job reads it"""
    return [cc.contig_coordinates(at, size, len(query), reverse) for at in range(0, len(query) - size + 1, step)]


# ---- 1. the reference's fixtures, end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize('fx', cc.FIXTURES, ids=[fx['name'] for fx in cc.FIXTURES])
def test_fixture_calls_are_the_recorded_lines(fx, records, kevlar_log):
    parts = cc.load_partitions(fx, kevlar_amd)
    kwargs = dict(ksize=fx['ksize'], mindist=fx['mindist'], homopolyfilt=fx['homopolyfilt'], maxtargetlen=fx['maxtargetlen'])
    found = list(kevlar_amd.call.call_partitions({partid: contigs for partid, cutouts, contigs in parts},
                                                 [(partid, cutouts) for partid, cutouts, contigs in parts], **kwargs))
    wanted = [(rec['partid'], line) for rec in records['fixtures'][fx['name']] for line in rec['final']]
    assert [(partid, call.vcf) for partid, call in found] == wanted
    for (partid, cutouts, contigs), rec in zip(parts, records['fixtures'][fx['name']]):
        prelim = list(kevlar_amd.call.prelim_call(cutouts, contigs, partid=partid, **kwargs))
        assert [call.vcf for call in prelim] == rec['prelim']
        final = list(kevlar_amd.call.call(cutouts, contigs, partid=partid, **kwargs))
        assert [call.vcf for call in final] == rec['final']


def test_fixture_alignments_scanned_as_the_restatement_scans_them(records):
    """every recorded alignment of every fixture in one batch, sequences shared between jobs as call_partitions shares them"""
    targets, queries, notes, jobs, cigars, wanted = [], [], [], [], [], []
    for fx in cc.FIXTURES:
        if fx['ksize'] != K or fx['mindist'] != DIST:
            continue
        for (partid, cutouts, contigs), rec in zip(cc.load_partitions(fx, kevlar_amd), records['fixtures'][fx['name']]):
            pairs = cc.ordered_pairs(cutouts, contigs)
            at = {}
            for (contig, cutout), row in zip(pairs, rec['pairs']):
                if row[3] is None:
                    continue
                for item, pool in ((cutout, targets), (contig, queries)):
                    if id(item) not in at:
                        at[id(item)] = len(pool)
                        pool.append(item.sequence)
                        if pool is queries:
                            notes.append(varmap.contig_annotations(contig))
                jobs.append((at[id(cutout)], at[id(contig)], int(row[4] == -1)))
                cigars.append(row[3])
                wanted.append(cc.job_record(cutout.sequence, contig.sequence, row[4] == -1, row[3], notes[at[id(contig)]], K, DIST))
    assert len(jobs) > 40 and len(queries) < len(jobs)
    got = varmap.scan_batch(targets, queries, jobs, cigars, notes, K, DIST)
    assert [record.astuple() for record in got] == wanted
    assert sum(1 for record in wanted if record[0]) >= 3 and {record[1] for record in wanted} == {0, 1, 2}


def test_forced_mappings_and_str(records):
    """kevlar/tests/test_varmap.py: mappings given their CIGAR (a batch of one each), the properties of a no-call, str(mapping)"""
    for (contigs, gdnas, score, cigar, ksize), rec in zip(cc.FORCED, records['forced']):
        contig = next(kevlar_amd.parse_augmented_fastx(kevlar_amd.open(cc.data_file(contigs), 'r')))
        cutout = next(kevlar_amd.reference.load_refr_cutouts(kevlar_amd.open(cc.data_file(gdnas), 'r')))
        mapping = varmap.VariantMapping(contig, cutout, score, cigar)
        assert (mapping.cigar, mapping.vartype) == (rec['cigar'], rec['vartype'])
        assert [call.vcf for call in mapping.call_variants(ksize)] == rec['lines']
    assert mapping.vartype is None
    assert [mapping.offset, mapping.targetshort, mapping.match, mapping.leftflank, mapping.indel, mapping.indeltype, mapping.rightflank] == [None] * 7
    contig = next(kevlar_amd.parse_augmented_fastx(kevlar_amd.open(cc.data_file('wasp-pass.contig.augfasta.gz'), 'r')))
    cutout = next(kevlar_amd.reference.load_refr_cutouts(kevlar_amd.open(cc.data_file('wasp.gdna.fa'), 'r')))
    mapping = varmap.VariantMapping(contig, cutout)
    assert str(mapping) == open(cc.data_file('wasp-align.txt')).read().strip() == records['wasp_str']
    assert mapping.interval == cutout.interval and mapping.seqid == cutout._seqid and mapping.pos == cutout._startpos
    calls = list(mapping.call_variants(29))
    assert [call.filterstr for call in calls] == ['PASS', 'PassengerVariant']
    # kevlar/tests/test_varmap.py:133-153
    for query, target, dist, n, trimcount in (('phony-snv-01b.contig.fa', 'phony-snv-01.gdna.fa', 5, 1, 1), ('phony-snv-02b.contig.fa', 'phony-snv-02.gdna.fa', 5, 1, 1),
                                              ('phony-snv-01b.contig.fa', 'phony-snv-01.gdna.fa', 2, 2, 0), ('phony-snv-02b.contig.fa', 'phony-snv-02.gdna.fa', None, 2, 0)):
        contig = next(kevlar_amd.parse_augmented_fastx(kevlar_amd.open(cc.data_file(query), 'r')))
        cutout = next(kevlar_amd.reference.load_refr_cutouts(kevlar_amd.open(cc.data_file(target), 'r')))
        mapping = varmap.VariantMapping(contig, cutout)
        assert len(list(mapping.call_variants(31, mindist=dist))) == n and mapping.trimmed == trimcount


def fiveparts_lines(records):
    return [line for rec in records['fixtures']['fiveparts'] for line in rec['final']]


def check_vcf_file(path, records, refr=None):
    lines = open(path).read().split('\n')
    assert lines[-1] == ''
    head = [line for line in lines[:-1] if line.startswith('#') and not line.startswith('##fileDate')]
    wanted = list(records['header'])
    if refr:
        wanted.insert(2, '##reference=' + refr)
    assert head == wanted
    assert [line for line in lines[:-1] if not line.startswith('#')] == fiveparts_lines(records)


def test_main_writes_the_recorded_vcf_and_mask(records, tmp_path, kevlar_log, hk):
    """main() on the fiveparts fixture: header and lines; --gen-mask saves the table a Nodetable fed the recorded windows holds"""
    out, mask = str(tmp_path / 'calls.vcf'), str(tmp_path / 'mask.nt')
    args = kevlar_amd.call.parser().parse_args(['--gen-mask', mask, '--mask-mem', '1M', '--refr', 'fiveparts-refr.fa.gz', '-o', out,
                                                cc.data_file('fiveparts.contigs.augfasta.gz'), cc.data_file('fiveparts.gdnas.fa.gz')])
    kevlar_amd.call.main(args)
    check_vcf_file(out, records, refr='fiveparts-refr.fa.gz')
    windows = []
    for line in fiveparts_lines(records):
        info = dict(item.split('=', 1) for item in line.split('\t')[7].split(';') if '=' in item)
        if len(info.get('ALTWINDOW', '')) >= 31:
            windows.append(info['ALTWINDOW'])
    assert len(windows) >= 5
    wanted = hk.Nodetable(31, 1e6 * 8 / 4, 4)
    for window in windows:
        wanted.consume(window)
    saved = hk.Nodetable.load(mask)
    assert saved.hashsizes() == wanted.hashsizes() and saved.ksize() == 31
    for t in range(4):
        assert saved.table_bytes(t) == wanted.table_bytes(t)
    assert saved.n_occupied() == wanted.n_occupied() > 0
    assert 'WARNING: mask FPR' not in kevlar_log.getvalue()
    # kevlar/tests/test_call.py:254-267
    args = kevlar_amd.call.parser().parse_args(['--gen-mask', mask, '--mask-mem', '100', '-o', out, cc.data_file('fiveparts.contigs.augfasta.gz'),
                                                cc.data_file('fiveparts.gdnas.fa.gz')])
    kevlar_amd.call.main(args)
    assert 'WARNING: mask FPR is 0.8065; exceeds user-specified limit of 0.0100' in kevlar_log.getvalue()
    # kevlar/tests/test_call.py:227-236
    args = kevlar_amd.call.parser().parse_args(['--debug', '-o', out, cc.data_file('wasp-pass.contig.augfasta.gz'), cc.data_file('wasp.gdna.fa')])
    kevlar_amd.call.main(args)
    assert records['wasp_str'] in kevlar_log.getvalue()


def test_module_entry_point_writes_the_recorded_vcf(records, tmp_path):
    """python -m kevlar_amd.call contigs targets -o calls.vcf: the public command line for now"""
    out = str(tmp_path / 'calls.vcf')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, '-m', 'kevlar_amd.call', cc.data_file('fiveparts.contigs.augfasta.gz'),
                           cc.data_file('fiveparts.gdnas.fa.gz'), '-o', out], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    check_vcf_file(out, records)


# ---- 2. block edges ------------------------------------------------------------------------------------------------------------
def test_block_lengths_and_mismatch_positions():
    rng = random.Random(11)
    jobs = []
    for length in (1, K - 1, K, K + 1, 63, 64, 65, 255, 256, 257):
        edge = sorted({p for p in (0, DIST - 1, DIST, length - DIST, length - DIST + 1, length - 1) if 0 <= p < length})
        sets = [[]] + [[p] for p in edge] + [edge]
        inner = list(range(DIST, length - DIST + 1))
        for count in (1, 4, 5, 40):
            if len(inner) >= count:
                sets.append(sorted(rng.sample(inner, count)))
            if length >= count:
                sets.append(sorted(rng.sample(range(length), count)))
        if length > 65:
            sets += [[63, 64], [62, 63, 64, 65], [63], [64], [127, 128, 191, 192]][:4 if length < 200 else 5]
        for mismatches in sets:
            for reverse in (False, True):
                target, contig, cigar, query = cc.build_job([('M', length, mismatches)], rng, reverse)
                jobs.append((target, contig, int(reverse), cigar, every_kmer(query, reverse, 13, 7)))
    assert len(jobs) > 300
    with_trimming = agree(jobs, K, DIST)
    without = agree(jobs, K, 0)
    assert device_records(jobs, K, None) == without
    assert agree(jobs, K, 40) != with_trimming
    kept = {record[4] for record in with_trimming}
    assert {0, 1, 4, 5, 40} <= kept
    assert any(record[3] == 4 for record in with_trimming) and all(record[3] == 0 for record in without)
    assert any(record[5:9] == (63, 64, cc.NO_POSITION, cc.NO_POSITION) for record in with_trimming)
    assert any(record[5:9] == (62, 63, 64, 65) for record in with_trimming)
    # a block below ksize is not scanned whatever it holds; other k-mer sizes move that edge
    assert all(record[3:5] == (0, 0) for record, job in zip(with_trimming, jobs) if len(job[0]) < K)
    agree(jobs[::3], 64, 3)
    agree(jobs[1::3], 65, 70)
    agree(jobs[2::3], 1, 1)


def test_bytes_compare_as_they_are():
    """lower case, N and IUPAC codes on either side; the reverse strand reads kevlar_amd.sequence.revcom of the contig"""
    rng = random.Random(12)
    jobs = []
    base = cc.random_bases(rng, 130)

    def put(text, at, what):
        return text[:at] + what + text[at + 1:]

    for at in (0, 7, 63, 64, 100, 129):
        jobs.append((put(base, at, base[at].lower()), base, 0, '130M', [(min(max(at - 5, 0), 117), 13)]))
        jobs.append((base, put(base, at, base[at].lower()), 0, '130M', [(min(max(at - 5, 0), 117), 13)]))
        jobs.append((put(base, at, base[at].lower()), put(base, at, base[at].lower()), 0, '130M', [(50, 31)]))
        jobs.append((put(base, at, 'N'), base, 0, '130M', []))
        jobs.append((base, put(base, at, 'N'), 0, '130M', [(min(max(at - 12, 0), 117), 13)]))
        jobs.append((put(base, at, 'N'), put(base, at, 'N'), 0, '130M', []))
        jobs.append((put(base, at, 'N'), put(base, at, 'n'), 0, '130M', []))
        # reversed: a lower-case base of the contig is read as the upper-case complement
        jobs.append((base, put(cc.revcom(base), 129 - at, cc.revcom(base)[129 - at].lower()), 1, '130M', [(40, 31), (129 - at, 1)]))
        jobs.append((put(base, at, base[at].lower()), cc.revcom(base), 1, '130M', []))
    alphabet = 'ACGTURYSWKMBDHVNacgturyswkmbdhvnXx-*'
    for _ in range(6):
        contig = cc.random_bases(rng, 150, alphabet)
        assert kevlar_amd.revcom(contig) == cc.revcom(contig)
        for reverse in (0, 1):
            target = list(cc.revcom(contig) if reverse else contig)
            for at in rng.sample(range(150), 3):
                target[at] = rng.choice(alphabet)
            jobs.append((''.join(target), contig, reverse, '150M', every_kmer(contig, False, 13, 3) + every_kmer(contig, False, 31, 5)))
    got = agree(jobs, K, DIST)
    assert sum(1 for record in got if record[4] >= 1) > 30 and any(sum(record[16:25]) > 0 for record in got)
    agree(jobs, 13, 0)


# ---- 3. CIGAR shapes -----------------------------------------------------------------------------------------------------------
def shaped(spec, rng, reverse=False, fold=None, sizes=((13, 3), (31, 7))):
    target, contig, cigar, query = cc.build_job(spec, rng, reverse, fold)
    notes = [note for size, step in sizes for note in every_kmer(query, reverse, size, step)]
    return (target, contig, int(reverse), cigar, notes)


def test_cigar_shapes():
    rng = random.Random(13)
    jobs, wanted = [], []

    def add(spec, cls, fold=None, folded=0):
        for reverse in (False, True):
            jobs.append(shaped(spec, rng, reverse, fold))
            wanted.append((folded, cc.CLASS_CODE[cls]))

    assert K == 31
    for spec, cls, fold, folded in cc.CIGAR_SHAPES:
        add(spec, cls, fold, folded)
    got = agree(jobs)
    assert [record[:2] for record in got] == wanted
    assert max(sum(1 for word in record[5:9] + record[12:16] if word != cc.NO_POSITION) for record in got) == 8
    agree(jobs, 13, 2)
    agree(jobs, 1, 0)           # the whole left flank is the window then, as a slice from -0 is
    agree(jobs, 64, 5)


# ---- 4. interesting k-mers -----------------------------------------------------------------------------------------------------
def test_interesting_kmers_in_the_window():
    rng = random.Random(14)
    jobs, wanted = [], []

    def add(target, query, cigar, notes, reverse, count=None):
        contig = cc.revcom(query) if reverse else query
        jobs.append((target, contig, int(reverse), cigar, [cc.contig_coordinates(at, size, len(query), reverse) for at, size in notes]))
        wanted.append(count)

    for reverse in (False, True):
        # one SNV at 100 of a 201-base block: the window is [70, 131)
        target, _, cigar, query = cc.build_job([('M', 201, [100])], rng)
        add(target, query, cigar, [], reverse, 0)
        add(target, query, cigar, [(70, 31)], reverse, 1)                         # at the first window position
        add(target, query, cigar, [(100, 31)], reverse, 1)                        # at the last
        add(target, query, cigar, [(69, 31)], reverse, 0)                         # overhanging by one base
        add(target, query, cigar, [(101, 31)], reverse, 0)
        add(target, query, cigar, [(70, 31), (69, 31), (70, 31), (100, 31), (101, 31), (70, 31)], reverse, 4)     # duplicates count
        for size, inside in ((13, True), (31, True), (32, True), (33, True), (61, True), (62, False), (64, False), (65, False), (128, False)):
            add(target, query, cigar, [(70, size)], reverse, int(inside))         # a k-mer longer than the window is absent
            add(target, query, cigar, [(131 - size, size)] if size <= 131 else [(0, size)], reverse, int(inside))
        for count in (1, 64, 65, 400):
            notes = [(rng.randrange(201 - 31 + 1), 31) for _ in range(count)]
            add(target, query, cigar, notes, reverse, sum(1 for at, size in notes if 70 <= at <= 100))
        # present only as its reverse complement: bases 0..31 of both sequences are the reverse complement of 80..111 of the query
        flipped = cc.revcom(query[80:111])
        add(flipped + target[31:], flipped + query[31:], cigar, [(0, 31), (35, 31)], reverse, 1)
        # its own copy lies outside the window, an equal copy inside
        copied = query[75:106]
        add(target[:150] + copied + target[181:], query[:150] + copied + query[181:], cigar, [(150, 31), (135, 31)], reverse, 1)
        # an insertion's window: 30 + 150 + 30 bases, room for the long k-mers
        target, _, cigar, query = cc.build_job([('M', 100, []), ('I', 150), ('M', 100, [50])], rng, fold=False)
        for size in (13, 31, 32, 33, 64, 65, 128):
            add(target, query, cigar, [(70, size), (280 - size, size), (69, size), (281 - size, size), (120, size)], reverse)
        sizes = [rng.choice([13, 31, 64, 65, 128]) for _ in range(400)]
        add(target, query, cigar, [(rng.randrange(350 - size + 1), size) for size in sizes], reverse)
    got = agree(jobs)
    for record, count in zip(got, wanted):
        if count is not None:
            assert record[17] == count and record[1] == 1
    assert [record[16] for record, count in zip(got, wanted) if count is None and record[1] == 2][:7] == [3] * 7
    agree(jobs, 13, DIST)


# ---- 5. seeded jobs ------------------------------------------------------------------------------------------------------------
def test_seeded_jobs_in_one_batch_and_in_small_ones():
    made = cc.fuzz_jobs()
    jobs = [job[:5] for job in made]
    got = agree(jobs, cc.FUZZ_KSIZE, cc.FUZZ_MINDIST)
    assert [record[1] for record in got] == [cc.CLASS_CODE[job[5]] for job in made]
    assert [record[0] for record in got] == [int(job[6]) for job in made]
    assert [sum(1 for record in got if record[1] == c) for c in (0, 1, 2)] == [100, 100, 100]
    assert sum(record[0] for record in got) == 75
    ones = [device_records(jobs[k:k + 1], cc.FUZZ_KSIZE, cc.FUZZ_MINDIST)[0] for k in range(len(jobs))]
    assert ones == got
    sevens = [record for k in range(0, len(jobs), 7) for record in device_records(jobs[k:k + 7], cc.FUZZ_KSIZE, cc.FUZZ_MINDIST)]
    assert sevens == got


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_are_refused_before_any_launch():
    lib = _lib.load()
    rc, records = cc.raw_scan(lib, **cc.GOOD_CALL)
    assert rc == _lib.KV_OK
    assert tuple(records[0][:25]) == cc.job_record('ACGTACGTAC', 'ACGTTCGTAC', 0, '10M', [(2, 5)], 5, 2)
    for name, change in cc.ARGUMENT_ERRORS:
        rc, records = cc.raw_scan(lib, **dict(cc.GOOD_CALL, **change))
        assert rc == _lib.KV_ERR_ARG, name
        assert (records == cc.UNTOUCHED).all(), name
    with pytest.raises(_lib.KvArgError):
        varmap.scan_batch(['ACGT'], ['ACGT'], [(0, 0, 0)], ['3M'], [[]], 31, 5)
    with pytest.raises(_lib.KvArgError):
        varmap.scan_batch(['ACGT'], ['ACGT'], [(0, 0, 0)], ['4M'], [[(-1, 2)]], 31, 5)
    assert varmap.scan_batch([], [], [], [], [], 31, 5) == []
