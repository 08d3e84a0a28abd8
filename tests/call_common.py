"""What the call tests share: the fixtures of tests/golden/call, a literal plain-Python restatement of the reference's calling
loops (kevlar/cigar.py, kevlar/varmap.py, kevlar/call.py, the VCF line of kevlar/vcf.py) that imports nothing of the product's
call modules, and the generators of the hand-built and seeded jobs.

The restatement walks every base in Python as the reference does.  For one aligned job it gives the fixed record kv_call_scan
returns (include/kvsketch.h) and the calls as VCF lines; tests/test_call_reference.py holds it to the lines the reference itself
printed (tests/golden/call/recorded.json), tests/test_gpu_call.py holds the device to it."""
import json
import os
import random
import re

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'call')

NO_POSITION = 0xFFFFFFFF
CLASS_CODE = {None: 0, 'snv': 1, 'indel': 2}


def fixture(name, contigs, gdnas, ksize=31, mindist=5, flat=False, homopolyfilt=True, maxtargetlen=10000):
    return dict(name=name, contigs=contigs, gdnas=gdnas, ksize=ksize, mindist=mindist, flat=flat, homopolyfilt=homopolyfilt,
                maxtargetlen=maxtargetlen)


# the data of the reference's test_call.py, test_varmap.py and test_cigar.py, partition by partition as main() calls them (flat:
# all contigs against all cutouts as one unlabelled partition).  Inputs of more than 1 KB are stored gzipped (GZIPPED).
FIXTURES = [
    fixture('ssc223', 'ssc223.contig.augfasta.gz', 'ssc223.gdna.fa'),
    fixture('ssc218', 'ssc218.contig.augfasta', 'ssc218.gdna.fa'),
    fixture('ssc107', 'ssc107.contig.augfasta.gz', 'ssc107.gdna.fa.gz'),
    fixture('funkycigar-deletion', 'funkycigar/deletion.contig.fa', 'funkycigar/deletion.gdna.fa'),
    fixture('nodiff', 'nodiff.contig.fa', 'nodiff.gdna.fa'),
    fixture('14153.cc5463', '14153.cc5463.contig.augfasta.gz', '14153.cc5463.gdna.augfasta.gz'),
    fixture('multibestrc', 'multibestrc.contig.fa', 'multibestrc.gdna.fa.gz'),
    fixture('bee-dupl', 'bee-dupl.contigs.augfasta.gz', 'bee-dupl.gdna.fa', ksize=27),
    fixture('wasp-29', 'wasp-pass.contig.augfasta.gz', 'wasp.gdna.fa', ksize=29, mindist=6),
    fixture('fiveparts', 'fiveparts.contigs.augfasta.gz', 'fiveparts.gdnas.fa.gz'),
    fixture('mnv', 'mnv-contig.augfasta.gz', 'mnv-gdna.fa', ksize=49),
    fixture('ant', 'ant.contig.augfasta.gz', 'ant.gdna.fa', ksize=29),
    fixture('homopolymer-14153', 'homopolymer/14153-6parts.contigs.augfasta.gz', 'homopolymer/14153-6parts.targets.fasta.gz'),
    fixture('homopolymer-12175', 'homopolymer/12175-3parts.contigs.augfasta.gz', 'homopolymer/12175-3parts.targets.fasta.gz'),
    fixture('homopolymer-12175-nofilter', 'homopolymer/12175-3parts.contigs.augfasta.gz', 'homopolymer/12175-3parts.targets.fasta.gz',
            homopolyfilt=False),
    fixture('bigtarget', 'bigtarget-contig.augfasta.gz', 'bigtarget-gdna.fasta.gz'),
    fixture('indel-snv', 'indel-snv.contig.augfasta.gz', 'indel-snv.gdna.fa', mindist=6),
    fixture('iktest', 'iktest.contig.fa', 'iktest.gdna.fa', ksize=29, mindist=6),
    fixture('drop-polysnp', 'drop-polysnp-contig.augfasta', 'drop-polysnp-gdna.fa', ksize=21, mindist=6),
    fixture('nomargin-snv', 'nomargin-snv-contigs.augfasta.gz', 'nomargin-gdna.fa', mindist=6),
    fixture('nomargin-indel', 'nomargin-indel-contigs.augfasta', 'nomargin-gdna.fa', mindist=6),
    fixture('nomargin-r-snv', 'nomargin-r-snv-contigs.augfasta.gz', 'nomargin-r-gdna.fa', mindist=6),
    fixture('nomargin-r-indel', 'nomargin-r-indel-contigs.augfasta', 'nomargin-r-gdna.fa', mindist=6),
    fixture('phony-snv-01', 'phony-snv-01.contig.fa', 'phony-snv-01.gdna.fa', ksize=21, mindist=6),
    fixture('phony-snv-02', 'phony-snv-02.contig.fa', 'phony-snv-02.gdna.fa', ksize=21, mindist=6),
    fixture('phony-deletion-01', 'phony-deletion-01.contig.fa', 'phony-deletion-01.gdna.fa', ksize=21, mindist=6),
    fixture('phony-deletion-02', 'phony-deletion-02.contig.fa', 'phony-deletion-02.gdna.fa', ksize=21, mindist=6),
    fixture('phony-insertion-01', 'phony-insertion-01.contig.fa', 'phony-insertion-01.gdna.fa', ksize=21, mindist=6),
    fixture('phony-insertion-02', 'phony-insertion-02.contig.fa', 'phony-insertion-02.gdna.fa', ksize=21, mindist=6),
    fixture('phony-snv-01b', 'phony-snv-01b.contig.fa', 'phony-snv-01.gdna.fa'),
    fixture('phony-snv-01b-dist2', 'phony-snv-01b.contig.fa', 'phony-snv-01.gdna.fa', mindist=2),
    fixture('phony-snv-02b', 'phony-snv-02b.contig.fa', 'phony-snv-02.gdna.fa'),
    fixture('phony-snv-02b-notrim', 'phony-snv-02b.contig.fa', 'phony-snv-02.gdna.fa', mindist=None),
    fixture('cigar-a', 'cigar/a.contig.fa', 'cigar/a.gdna.fa'),
    fixture('cigar-b', 'cigar/b.contig.fa', 'cigar/b.gdna.fa'),
    fixture('cigar-c', 'cigar/c.contig.fa', 'cigar/c.gdna.fa'),
    fixture('cigar-d', 'cigar/d.contig.fa', 'cigar/d.gdna.fa'),
]
FIXTURE_BY_NAME = {fx['name']: fx for fx in FIXTURES}

# mappings with the CIGAR the reference's tests force on them (test_varmap.py:27, 49, 54-73, 100): (contigs, gdnas, score, cigar, ksize)
FORCED = [
    ('ssc218.contig.augfasta', 'ssc218.gdna.fa', 1e6, '50D132M1D125M50D', 31),
    ('ssc107.contig.augfasta.gz', 'ssc107.gdna.fa.gz', 1e6, '25D263M25D', 31),
    ('phony-snv-01.contig.fa', 'phony-snv-01.gdna.fa', 1e6, '25D98M25D', 21),
    ('phony-snv-02.contig.fa', 'phony-snv-02.gdna.fa', 1e6, '24D99M25D', 21),
    ('phony-deletion-01.contig.fa', 'phony-deletion-01.gdna.fa', 1e6, '25D28M8D49M25D', 21),
    ('phony-deletion-02.contig.fa', 'phony-deletion-02.gdna.fa', 1e6, '40D29M3D36M40D', 21),
    ('phony-insertion-01.contig.fa', 'phony-insertion-01.gdna.fa', 1e6, '10D34M7I49M10D1M', 21),
    ('phony-insertion-02.contig.fa', 'phony-insertion-02.gdna.fa', 1e6, '10D33M27I95M10D', 21),
    ('phony-deletion-01.contig.fa', 'phony-insertion-01.gdna.fa', 1e6, '25D5M22I5M46D8M13D2M35I', 21),
]

# the other data files the tests read
EXTRA_FILES = ['wasp-align.txt', 'five-snvs-with-likelihood.vcf.gz']
GZIPPED = 1024          # make_golden_call.py stores a plain-text input of more than this many bytes as NAME.gz


def data_file(rel):
    return os.path.join(GOLDEN, rel)


def fixture_files():
    files = set(EXTRA_FILES)
    for fx in FIXTURES:
        files.update((fx['contigs'], fx['gdnas']))
    for contigs, gdnas, score, cigar, ksize in FORCED:
        files.update((contigs, gdnas))
    return sorted(files)


_recorded = None


def recorded():
    """tests/golden/call/recorded.json, read once.  A final call that is one of the partition's preliminary calls unchanged is
    stored as that call's index; here every final call is its line again."""
    global _recorded
    if _recorded is None:
        with open(os.path.join(GOLDEN, 'recorded.json')) as stream:
            _recorded = json.load(stream)
        for parts in _recorded['fixtures'].values():
            for part in parts:
                part['final'] = [part['prelim'][line] if isinstance(line, int) else line for line in part['final']]
    return _recorded


def load_partitions(fx, kevlar):
    """[(partid, cutouts, contigs)] of a fixture, in the cutout file's order; `kevlar` is the package that parses (the product here,
    the reference in make_golden_call.py)"""
    contigs = list(kevlar.parse_partitioned_reads(kevlar.parse_augmented_fastx(kevlar.open(data_file(fx['contigs']), 'r'))))
    cutouts = list(kevlar.parse_partitioned_reads(kevlar.reference.load_refr_cutouts(kevlar.open(data_file(fx['gdnas']), 'r'))))
    if fx['flat']:
        return [(None, [c for partid, part in cutouts for c in part], [c for partid, part in contigs for c in part])]
    by_partition = dict(contigs)
    return [(partid, part, by_partition[partid]) for partid, part in cutouts if partid in by_partition]


# ---- the restatement ---------------------------------------------------------------------------------------------------------

_COMPLEMENT = {}
for _a, _b in zip('ATUGCYRSWKMBDHVN', 'TAACGRYSWMKVHDBN'):
    _COMPLEMENT[_a] = _b
    _COMPLEMENT[_a.lower()] = _b


def revcom(sequence):
    out = []
    for base in reversed(sequence):
        out.append(_COMPLEMENT.get(base, base))
    return ''.join(out)


def tokenize(query, target, cigar):
    """kevlar/cigar.py:28-44: [[length, type, target bases or None, query bases or None]]"""
    blocks = []
    for found in re.finditer(r'(\d+)([DIM])', cigar):
        length, kind = int(found.group(1)), found.group(2)
        tseq = qseq = None
        if kind in ('M', 'D'):
            tseq, target = target[:length], target[length:]
        if kind in ('M', 'I'):
            qseq, query = query[:length], query[length:]
        blocks.append([length, kind, tseq, qseq])
    assert target == '' and query == ''
    return blocks


def endcheck(blocks):
    """kevlar/cigar.py:46-71: True when the last block was folded into the third-last (the list is changed in place)"""
    if len(blocks) < 3:
        return False
    if blocks[-1][1] != 'M' or blocks[-3][1] != 'M':
        return False
    if blocks[-2][1] == 'D':
        prevseq, lastseq, endseq = blocks[-2][2], blocks[-1][2], blocks[-1][3]
    else:
        prevseq, lastseq, endseq = blocks[-2][3], blocks[-1][3], blocks[-1][2]
    longseq = prevseq + lastseq
    for i in range(len(endseq)):
        if i >= len(longseq) or longseq[i] != endseq[i]:
            return False
    blocks[-3] = [blocks[-3][0] + blocks[-1][0], 'M', blocks[-3][2] + blocks[-1][2], blocks[-3][3] + blocks[-1][3]]
    del blocks[-1]
    return True


def classify(cigar):
    """kevlar/varmap.py:49-54"""
    if re.search(r'^((\d+)([DI]))?(\d+)M((\d+)[DI])?$', cigar):
        return 'snv'
    if re.search(r'^((\d+)([DI]))?(\d+)M(\d+)([ID])(\d+)M((\d+)[DI])?$', cigar):
        return 'indel'
    return None


def n_ikmers_present(contig_sequence, annotations, window):
    """kevlar/varmap.py:309-317; annotations: (offset, ksize) pairs"""
    n = 0
    for offset, ksize in annotations:
        seq = contig_sequence[offset:offset + ksize]
        if seq in window:
            n += 1
        elif revcom(seq) in window:
            n += 1
    return n


def trim_terminal_snvs(mismatches, alnlength, mindist):
    valid, trimcount = [], 0
    for mm in mismatches:
        if mm < mindist or alnlength - mm < mindist:
            trimcount += 1
        else:
            valid.append(mm)
    return trimcount, valid


class Call(object):
    """a variant as far as its VCF line and the de-duplication need it (kevlar/vcf.py:64-140, 235-259)"""

    def __init__(self, seqid, pos, refr, alt, **info):
        self.seqid, self.position, self.refr, self.alt = seqid, pos, refr, alt
        self.info = dict(info)
        self.filters = set()

    @property
    def window(self):
        return self.info.get('ALTWINDOW')

    @property
    def refrwindow(self):
        return self.info.get('REFRWINDOW')

    @property
    def windowlength(self):
        return 0 if self.window is None else len(self.window)

    @property
    def vcf(self):
        pairs = ['{}={}'.format(key, self.info[key]) for key in sorted(self.info) if key != 'CONTIG']
        if 'CONTIG' in self.info:
            pairs.append('CONTIG={}'.format(self.info['CONTIG']))
        filterstr = ';'.join(sorted(self.filters)) if self.filters else ('.' if self.refr == '.' else 'PASS')
        pos = self.position if self.position == '.' else self.position + 1
        return '{}\t{}\t.\t{}\t{}\t.\t{}\t{}'.format(self.seqid, pos, self.refr, self.alt, filterstr, ';'.join(pairs) if pairs else '.')

    def test_merge(self, other):
        if self.seqid == '.' or self.seqid != other.seqid:
            return None
        if len(self.alt) != len(self.refr) or len(other.alt) != len(other.refr):
            return None
        length = len(self.refr)
        if self.position != other.position - length:
            return None
        if self.window is None or other.window is None or self.refrwindow is None or other.refrwindow is None:
            return None
        if self.window[length:] != other.window[:-1] or self.refrwindow[length:] != other.refrwindow[:-1]:
            return None
        self.info['ALTWINDOW'] = self.window + other.window[-length]
        self.info['REFRWINDOW'] = self.refrwindow + other.refrwindow[-length]
        self.alt += other.alt
        self.refr += other.refr
        return self


class Mapping(object):
    """kevlar/varmap.py:19-306 for one aligned pair.  contig_sequence / annotations ((offset, ksize) pairs) / target: plain
    strings; seqid and startpos: of the cutout; strand 1 or -1.  After call_variants(): .record is the 25-word record of the
    device for this job, .calls the calls."""

    def __init__(self, contig_sequence, annotations, target, score, cigar, strand=1, seqid='seq', startpos=0, homopolyfilt=True,
                 nocall=False):
        self.contig_sequence, self.annotations, self.target = contig_sequence, list(annotations), target
        self.seqid, self.startpos, self.homopolyfilt, self.nocall = seqid, startpos, homopolyfilt, nocall
        self.vartype = None
        self.score = 0 if nocall else score
        if nocall:
            return
        self.strand = strand
        self.varseq = contig_sequence if strand == 1 else revcom(contig_sequence)
        self.blocks = tokenize(self.varseq, target, cigar)
        self.folded = endcheck(self.blocks)
        self.cigar = ''.join('{:d}{:s}'.format(block[0], block[1]) for block in self.blocks) if self.folded else cigar
        self.vartype = classify(self.cigar)
        self.trimmed = 0

    def _flanks(self):
        first = 0 if self.blocks[0][1] == 'M' else 1
        if self.vartype == 'snv':
            return self.blocks[first], None, None
        return self.blocks[first], self.blocks[first + 1], self.blocks[-1 if self.blocks[-1][1] == 'M' else -2]

    def call_variants(self, ksize, mindist):
        self.record = [0, 0] + ([0, 0, 0] + [NO_POSITION] * 4) * 2 + [0] * 9
        self.calls = []
        if self.nocall:
            self.calls.append(Call('.', '.', '.', '.', CONTIG=self.contig_sequence, IKMERS=str(len(self.annotations))))
            return self.calls
        self.record[0] = int(self.folded)
        self.record[1] = CLASS_CODE[self.vartype]
        if self.vartype is None:
            nocall = Call(self.seqid, self.startpos, '.', '.', CONTIG=self.varseq, CIGAR=self.cigar, KSW2=str(self.score))
            nocall.filters.add('InscrutableCigar')
            self.calls.append(nocall)
            return self.calls
        left, gap, right = self._flanks()
        offset = 0 if self.blocks[0][1] != 'D' else self.blocks[0][0]       # targetshort (a leading I) counts 0
        if self.vartype == 'snv':
            found = self.call_snv(0, left[3], left[2], offset, ksize, mindist, True)
        else:
            indel = self.call_indel(left, gap, right, offset, ksize)
            if self.is_passenger(indel):
                indel.filters.add('PassengerVariant')
            if self.homopolyfilt and len(right[2]) >= 5 and right[2][0] * 5 in right[2][0:7]:
                indel.filters.add('Homopolymer')
            self.calls.append(indel)
            found = self.call_snv(0, left[3], left[2], offset, ksize, mindist, False)
            offset += left[0]
            if gap[1] == 'D':
                offset += gap[0]
            found += self.call_snv(1, right[3], right[2], offset, ksize, mindist, False)
        for call in found:
            if self.is_passenger(call):
                call.filters.add('PassengerVariant')
            self.calls.append(call)
        return self.calls

    def is_passenger(self, call):
        if call.window is None:
            return False
        ikmers = []
        for offset, ksize in self.annotations:
            seq = self.contig_sequence[offset:offset + ksize]
            ikmers.extend([seq, revcom(seq)])
        return sum(1 for k in ikmers if k in call.window) == 0

    def call_snv(self, which, qseq, tseq, offset, ksize, mindist, donocall):
        length = len(qseq)
        assert len(tseq) == length
        base = 2 + 7 * which
        self.record[base] = length
        if length < ksize:
            return []
        diffs = [i for i in range(length) if tseq[i] != qseq[i]]
        if mindist:
            self.trimmed, diffs = trim_terminal_snvs(diffs, length, mindist)
            self.record[base + 1] = self.trimmed
        self.record[base + 2] = len(diffs)
        self.record[base + 3:base + 3 + min(len(diffs), 4)] = diffs[:4]
        if len(diffs) == 0 or len(diffs) > 4:
            if not donocall:
                return []
            nocall = Call(self.seqid, self.startpos + offset, '.', '.', CONTIG=qseq, CIGAR=self.cigar, KSW2=str(self.score),
                          IKMERS=str(len(self.annotations)))
            nocall.filters.add('PerfectMatch' if len(diffs) == 0 else 'NumerousMismatches')
            return [nocall]
        calls = []
        for n, pos in enumerate(diffs):
            minpos, maxpos = max(pos - ksize + 1, 0), min(pos + ksize, length)
            altwindow, refrwindow = qseq[minpos:maxpos], tseq[minpos:maxpos]
            nikmers = n_ikmers_present(self.contig_sequence, self.annotations, altwindow)
            self.record[17 + 4 * which + n] = nikmers
            calls.append(Call(self.seqid, self.startpos + pos + offset, tseq[pos].upper(), qseq[pos].upper(), CONTIG=qseq,
                              CIGAR=self.cigar, KSW2=str(self.score), IKMERS=str(nikmers), ALTWINDOW=altwindow, REFRWINDOW=refrwindow))
        return calls

    def call_indel(self, left, gap, right, offset, ksize):
        if gap[1] == 'D':
            refrwindow = left[2][-(ksize - 1):] + gap[2] + right[2][:(ksize - 1)]
            refrallele = left[2][-1] + gap[2]
            altwindow = left[3][-(ksize - 1):] + right[3][:(ksize - 1)]
            altallele = left[3][-1]
        else:
            refrwindow = left[2][-(ksize - 1):] + right[2][:(ksize - 1)]
            refrallele = left[2][-1]
            altwindow = left[3][-(ksize - 1):] + gap[3] + right[3][:(ksize - 1)]
            altallele = left[3][-1] + gap[3]
        nikmers = n_ikmers_present(self.contig_sequence, self.annotations, altwindow)
        self.record[16] = nikmers
        return Call(self.seqid, self.startpos + offset + left[0] - 1, refrallele, altallele, CONTIG=self.varseq, CIGAR=self.cigar,
                    KSW2=str(self.score), IKMERS=str(nikmers), ALTWINDOW=altwindow, REFRWINDOW=refrwindow)


def job_record(target, contig, reverse, cigar, annotations, ksize, mindist):
    """the 25 words the device owes for one job"""
    mapping = Mapping(contig, annotations, target, 0, cigar, -1 if reverse else 1)
    mapping.call_variants(ksize, mindist)
    return tuple(mapping.record)


def alignments_to_report(alignments):
    """kevlar/call.py:18-35"""
    if len(alignments) <= 1:
        return alignments
    scrtbl = [aln for aln in alignments if aln.vartype is not None]
    finallist = scrtbl if scrtbl else alignments
    bestscore = max(aln.score for aln in finallist)
    return [aln for aln in finallist if aln.score == bestscore]


def dedup(calls):
    """kevlar/call.py:38-50 (the reference keeps the calls of a position in a set; of equally long windows the first made is taken
    here)"""
    table = {}
    for call in calls:
        table.setdefault(call.seqid, {}).setdefault(call.position, []).append(call)
    for seqid in sorted(table):
        for position in sorted(table[seqid]):
            yield sorted(table[seqid][position], key=lambda call: call.windowlength, reverse=True)[0]


def merge_adjacent(calls):
    """kevlar/call.py:53-64"""
    prev = None
    for call in calls:
        if prev is not None:
            trymerge = prev.test_merge(call)
            if trymerge is not None:
                call = trymerge
                prev = None
        if prev is not None:
            yield prev
        prev = call
    yield prev


def restate_partition(partid, pairs, ksize, mindist, homopolyfilt=True):
    """kevlar/call.py:67-93 with the alignments given: pairs = [(contig record, cutout, score, cigar, strand)] in the order of the
    reference's loops (contigs longest first, cutouts by defline; cigar None = a cutout over the length limit).  Returns the
    preliminary calls."""
    calls, at = [], 0
    while at < len(pairs):
        contig = pairs[at][0]
        alignments = []
        while at < len(pairs) and pairs[at][0] is contig:
            contig, cutout, score, cigar, strand = pairs[at]
            notes = [(ikmer.offset, ikmer.ksize) for ikmer in contig.annotations]
            alignments.append(Mapping(contig.sequence, notes, cutout.sequence, score, cigar, strand, cutout._seqid, cutout._startpos,
                                      homopolyfilt, nocall=cigar is None))
            at += 1
        for alignment in alignments_to_report(alignments):
            for call in alignment.call_variants(ksize, mindist):
                if partid is not None:
                    call.info['PART'] = partid
                calls.append(call)
    return calls


def ordered_pairs(cutouts, contigs):
    """(contig, cutout) in the order of kevlar/call.py:71-73"""
    return [(contig, cutout) for contig in sorted(contigs, reverse=True, key=len)
            for cutout in sorted(cutouts, key=lambda cutout: cutout.defline)]


# ---- jobs built by construction ----------------------------------------------------------------------------------------------

def random_bases(rng, n, alphabet='ACGT'):
    return ''.join(rng.choice(alphabet) for _ in range(n))


def other_base(rng, base):
    return rng.choice([b for b in 'ACGT' if b != base.upper()])


def build_job(spec, rng, reverse=False, fold=None):
    """(target, contig, cigar, query as the job reads it) from a list of blocks: ('M', length, mismatch positions), ('I', length),
    ('D', length).  The query is upper-case ACGT; with `reverse` the contig handed over is its reverse complement.
    fold: True makes the tail `M (D|I) M` one the end check folds: the gap's bases repeat with the gap's length as period through
    the last block, and the last block's mismatch positions are where the period is broken (each breaks it once more one period
    later); False makes sure it does not fold."""
    target, query, cigar = [], [], ''
    for n, block in enumerate(spec):
        kind, length = block[0], block[1]
        cigar += '{}{}'.format(length, kind)
        if kind == 'M':
            bases = random_bases(rng, length)
            other = list(bases)
            for pos in block[2]:
                other[pos] = other_base(rng, bases[pos])
            target.append(bases)
            query.append(''.join(other))
        elif kind == 'I':
            target.append('')
            query.append(random_bases(rng, length))
        else:
            target.append(random_bases(rng, length))
            query.append('')
    if fold is not None:
        assert len(spec) >= 3 and spec[-1][0] == 'M' and spec[-3][0] == 'M' and spec[-2][0] in 'DI'
        gap_on_target = spec[-2][0] == 'D'
        gap = target[-2] if gap_on_target else query[-2]
        length = spec[-1][1]
        if fold:
            last = list((gap * (length // len(gap) + 1))[:length])
            for pos in spec[-1][2]:
                last[pos] = other_base(rng, last[pos])
            last = ''.join(last)
            end = (gap + last)[:length]
        else:
            last = target[-1] if gap_on_target else query[-1]
            end = other_base(rng, gap[0]) + (query[-1] if gap_on_target else target[-1])[1:]
        if gap_on_target:
            target[-1], query[-1] = last, end
        else:
            query[-1], target[-1] = last, end
    target, query = ''.join(target), ''.join(query)
    return target, (revcom(query) if reverse else query), cigar, query


def contig_coordinates(offset, ksize, qlen, reverse):
    """an (offset, ksize) in the coordinates of the query as the job reads it -> in the contig's"""
    return (qlen - offset - ksize if reverse else offset), ksize


def cigar_shapes(K=31):
    """[(spec, wanted class, fold argument of build_job, whether the end check folds)]: every shape a list of blocks can have for
    kevlar/varmap.py:49-54 and kevlar/cigar.py:46-71.  tests/test_gpu_call.py runs them through the device, tests/test_align_call_plan.py
    through the host plan alone."""
    shapes = []

    def add(spec, cls, fold=None, folded=0):
        shapes.append((spec, cls, fold, folded))

    for lead in (None, 'D', 'I'):
        for trail in (None, 'D', 'I'):
            head = [(lead, 9)] if lead else []
            tail = [(trail, 12)] if trail else []
            add(head + [('M', 120, [60])] + tail, 'snv')
            for gap in 'DI':
                unfold = False if not trail else None
                add(head + [('M', 80, [40]), (gap, 6), ('M', 90, [45])] + tail, 'indel', unfold)
    add([('M', 70, [30]), ('D', 5), ('M', 60, [20]), ('I', 4), ('M', 80, [40])], None, False)          # two indels
    add([('M', 70, [30]), ('D', 5), ('M', 60, [20]), ('I', 4), ('M', 80, [40]), ('D', 3)], None)
    add([('M', 40, [])], 'snv')
    add([('M', 40, []), ('D', 7)], 'snv')
    add([('I', 7), ('M', 40, [11])], 'snv')
    add([('D', 7), ('I', 9)], None)
    add([('I', 9), ('D', 7)], None)
    add([('M', 50, []), ('M', 50, [25])], None)                                                        # two runs are two blocks
    add([('M', 50, []), ('M', 50, [25]), ('M', 50, [])], None)
    add([('D', 3), ('M', 50, [5]), ('I', 2), ('M', 50, [25]), ('D', 2), ('M', 50, []), ('I', 1)], None)    # seven blocks
    # tails M (D|I) M: folded into snv / indel / none, and left alone
    for gap in 'DI':
        add([('M', 60, [30]), (gap, 3), ('M', 50, [])], 'snv', True, 1)
        add([('M', 60, [30]), (gap, 3), ('M', 50, [])], 'indel', False)
        add([('D', 4), ('M', 60, [30]), (gap, 3), ('M', 50, [20])], 'snv', True, 1)
        add([('M', 90, [40]), ('I', 5), ('M', 60, [30]), (gap, 7), ('M', 40, [])], 'indel', True, 1)
        add([('M', 90, [40]), ('D', 5), ('M', 60, [30]), (gap, 2), ('M', 140, [100])], 'indel', True, 1)
        add([('M', 90, [40]), ('D', 5), ('M', 60, [30]), (gap, 2), ('M', 140, [100])], None, False)
        add([('I', 2), ('M', 90, [40]), ('D', 5), ('M', 60, [30]), ('I', 5), ('M', 60, [30]), (gap, 7), ('M', 40, [])], None, True, 1)
        # a mismatch in each segment and at the seam (the last block's break of the period at 0 sits right behind it), windows
        # that straddle the seam, a gap longer than the last block, a last block of one base
        add([('M', 64, [10, 63]), (gap, 3), ('M', 70, [0, 40])], 'snv', True, 1)
        add([('M', 45, [44]), (gap, 5), ('M', 45, [])], 'snv', True, 1)
        add([('M', 45, [40]), (gap, 60), ('M', 45, [3])], 'snv', True, 1)
        add([('M', 45, [20]), (gap, 2), ('M', 1, [])], 'snv', True, 1)
        add([('M', 45, [20]), (gap, 2), ('M', 1, [])], 'indel', False)
        add([('M', 3, []), (gap, 2), ('M', 300, [150])], 'snv', True, 1)
    # flanks shorter than ksize - 1 on either side, an insertion longer than 2 * ksize, deletions
    for gap, size in (('D', 4), ('I', 4), ('I', 2 * K + 9), ('D', 200), ('I', 1), ('D', 1)):
        add([('M', 10, []), (gap, size), ('M', 200, [100])], 'indel', False)
        add([('M', 200, [100]), (gap, size), ('M', 10, [])], 'indel', False)
        add([('M', 10, [5]), (gap, size), ('M', 12, [6])], 'indel', False)
        add([('M', K - 2, []), (gap, size), ('M', K - 1, [])], 'indel', False)
        add([('M', 120, [30, 60, 90, 100]), (gap, size), ('M', 130, [20, 40, 60, 120])], 'indel', False)
        add([('I', 6), ('M', 120, [30, 60, 90, 100, 110]), (gap, size), ('M', 130, []), ('D', 9)], 'indel')
    return shapes


CIGAR_SHAPES = cigar_shapes()

FUZZ_JOBS = 300
FUZZ_KSIZE = 31
FUZZ_MINDIST = 5


def fuzz_jobs(seed=20261019, n=FUZZ_JOBS):
    """[(target, contig, reverse, cigar, annotations, wanted class, wanted fold)]: job k is of class k % 3 (none, snv, indel) and
    has a foldable tail when k % 4 == 0, by construction"""
    rng = random.Random(seed)
    jobs = []

    def match(lo=1, hi=300):
        length = rng.choice([rng.randint(lo, hi), rng.randint(lo, 70), 31, 64, 65])
        count = rng.choice([0, 0, 1, 1, 2, 3, 4, 5, 9])
        return ('M', length, sorted(rng.sample(range(length), min(count, length))))

    def gap(kind=None):
        return (kind or rng.choice('DI'), rng.choice([1, 2, 3, 7, 30, 70]))

    for k in range(n):
        wanted, fold = (None, 'snv', 'indel')[k % 3], k % 4 == 0
        lead = [gap()] if rng.random() < 0.4 else []
        if wanted == 'snv':
            spec = lead + [match()] + ([gap()] if fold or rng.random() < 0.4 else [])
        elif wanted == 'indel':
            spec = lead + [match(), gap(), match()] + ([gap()] if fold or rng.random() < 0.4 else [])
        else:
            spec = lead + [match(), gap(), match(), gap(), match()] + ([gap()] if fold or rng.random() < 0.3 else [])
        if fold:
            spec.append(match(1, 120))
        unfoldable = None
        if not fold and len(spec) >= 3 and spec[-1][0] == 'M' and spec[-3][0] == 'M' and spec[-2][0] in 'DI':
            unfoldable = False
        reverse = rng.random() < 0.4
        target, contig, cigar, query = build_job(spec, rng, reverse, True if fold else unfoldable)
        if rng.random() < 0.25 and not reverse and not fold:           # lower case and N compare as they are
            at = rng.randrange(len(contig))
            contig = contig[:at] + rng.choice([contig[at].lower(), 'N']) + contig[at + 1:]
        notes = []
        for _ in range(rng.choice([0, 1, 5, 20, 70])):
            ksize = rng.choice([13, 25, 31, 31, 31, 32, 33, 64, 65, 128])
            if ksize <= len(contig):
                notes.append((rng.randrange(len(contig) - ksize + 1), ksize))
        if notes and rng.random() < 0.5:
            notes.append(notes[0])
        jobs.append((target, contig, int(reverse), cigar, notes, wanted, fold))
    return jobs


# ---- the library call as it is, for the argument checks ------------------------------------------------------------------------

RECORD_WORDS = 32
UNTOUCHED = 0xAAAAAAAA


def raw_scan(lib, targets, queries, jobs, runlists, annotations, ksize, mindist, run_offsets=None, ik_offsets=None):
    """(return code, records) of kv_call_scan itself; records start out as UNTOUCHED words.  runlists: per job its
    `length << 4 | op` runs; annotations: per query its (offset, ksize) pairs; the two offset arrays can be overridden."""
    import numpy as np

    def text(sequences):
        offsets = np.zeros(len(sequences) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(s) for s in sequences])
        return np.frombuffer((''.join(sequences) or '\0').encode('latin-1'), dtype=np.uint8), offsets

    tbases, toff = text(targets)
    qbases, qoff = text(queries)
    jobs = np.array(jobs, dtype=np.uint32).reshape(-1, 3)
    counts = np.array([len(runs) for runs in runlists] + [0], dtype=np.uint32)
    if run_offsets is None:
        run_offsets = np.concatenate([[0], np.cumsum(counts[:-1])])
    run_offsets = np.array(run_offsets, dtype=np.uint64)
    runs = np.array([run for runs in runlists for run in runs] + [0], dtype=np.uint32)
    if ik_offsets is None:
        ik_offsets = np.concatenate([[0], np.cumsum([len(notes) for notes in annotations])])
    ik_offsets = np.array(ik_offsets, dtype=np.uint64)
    ikmers = np.array([value for notes in annotations for pair in notes for value in pair] + [0, 0], dtype=np.uint32)
    records = np.full((max(len(jobs), 1), RECORD_WORDS), UNTOUCHED, dtype=np.uint32)
    rc = lib.kv_call_scan(tbases.ctypes.data, toff.ctypes.data, len(targets), qbases.ctypes.data, qoff.ctypes.data, len(queries),
                          jobs.ctypes.data, len(jobs), run_offsets.ctypes.data, counts.ctypes.data, runs.ctypes.data, len(runs) - 1,
                          ik_offsets.ctypes.data, ikmers.ctypes.data, ksize, mindist, records.ctypes.data)
    return rc, records


def M(length):
    return length << 4


def I(length):  # noqa: E743
    return length << 4 | 1


def D(length):
    return length << 4 | 2


# (name, keyword arguments of raw_scan that differ from one good job): each is KV_ERR_ARG and nothing is launched
GOOD_CALL = dict(targets=['ACGTACGTAC'], queries=['ACGTTCGTAC'], jobs=[(0, 0, 0)], runlists=[[M(10)]], annotations=[[(2, 5)]], ksize=5,
                 mindist=2)
ARGUMENT_ERRORS = [
    ('ikmer-past-contig', dict(annotations=[[(6, 5)]])),
    ('ikmer-offset-past-contig', dict(annotations=[[(10, 1)]])),
    ('ikmer-without-bases', dict(annotations=[[(2, 0)]])),
    ('ikmer-offsets-decrease', dict(annotations=[[(2, 5)]], ik_offsets=[1, 0])),
    ('runs-short-of-both', dict(runlists=[[M(9)]])),
    ('runs-short-of-target', dict(runlists=[[M(9), I(1)]])),
    ('runs-short-of-query', dict(runlists=[[M(9), D(1)]])),
    ('runs-past-both', dict(runlists=[[M(11)]])),
    ('runs-past-target', dict(runlists=[[M(10), D(1)]])),
    ('runs-past-query', dict(runlists=[[I(1), M(10)]])),
    ('no-runs', dict(runlists=[[]])),
    ('run-of-length-0', dict(runlists=[[M(5), D(0), M(5)]])),
    ('run-of-another-op', dict(runlists=[[M(5), 5 << 4 | 3, M(5)]])),
    ('runs-outside-the-pool', dict(run_offsets=[5])),
    ('empty-target', dict(targets=[''], runlists=[[I(10)]])),
    ('empty-query', dict(queries=[''], runlists=[[D(10)]], annotations=[[]])),
    ('target-index', dict(jobs=[(1, 0, 0)])),
    ('query-index', dict(jobs=[(0, 1, 0)])),
    ('strand-flag', dict(jobs=[(0, 0, 2)])),
    ('ksize-0', dict(ksize=0)),
    ('negative-mindist', dict(mindist=-1)),
]
