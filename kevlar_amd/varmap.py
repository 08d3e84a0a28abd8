"""Variant calls from contig-to-cutout alignments (the reference's kevlar/varmap.py), the per-base work on the GPU.

The reference walks every aligned base of a mapping for mismatches and searches every call's window for every interesting k-mer
of the contig.  Here a batch of mappings is scanned on the device (`scan_batch`, kv_call_scan in kevlar_amd/csrc/kv_call.hip)
and every mapping gets one fixed record: whether the tokenizer's end check folded, the class of the CIGAR, the mismatches of the
scanned match blocks and the IKMERS number of every call.  `VariantMapping.call_variants` turns the record into `Variant`
objects: it cuts alleles and windows by slicing and walks no sequence.  A mapping built on its own is a batch of one; there is
no host path for the scan.

`kevlar_amd.call.call_partitions` scans all mappings of a run at once and hands each mapping its record."""
import re

import numpy as np

import kevlar_amd
from kevlar_amd import _lib
from kevlar_amd.alignment import _text, align_both_strands
from kevlar_amd.cigar import AlignmentTokenizer, cigar_blocks
from kevlar_amd.vcf import Variant
from kevlar_amd.vcf import VariantFilter as vf

RECORD_WORDS = 32                       # include/kvsketch.h KV_CALL_RECORD_WORDS
CLASSES = (None, 'snv', 'indel')        # KV_CALL_NONE / KV_CALL_SNV / KV_CALL_INDEL
NO_POSITION = 0xFFFFFFFF
_OPCODE = {'M': 0, 'I': 1, 'D': 2}
SNV_PATTERN = r'^((\d+)([DI]))?(\d+)M((\d+)[DI])?$'
INDEL_PATTERN = r'^((\d+)([DI]))?(\d+)M(\d+)([ID])(\d+)M((\d+)[DI])?$'


def cigar_runs(cigar):
    """the `length << 4 | op` runs of a CIGAR string, as kv_align_batch returns them"""
    return [length << 4 | _OPCODE[kind] for length, kind in cigar_blocks(cigar)]


class ScanRecord(object):
    """one job's record of kv_call_scan, by name"""
    __slots__ = ('words',)

    def __init__(self, words):
        self.words = words

    @property
    def folded(self):
        return bool(self.words[0])

    @property
    def vartype(self):
        return CLASSES[int(self.words[1])]

    def block(self, which):
        """(length, trimmed, kept, positions) of scanned block 0 or 1"""
        base = 2 + 7 * which
        length, trimmed, kept = (int(v) for v in self.words[base:base + 3])
        return length, trimmed, kept, [int(v) for v in self.words[base + 3:base + 3 + min(kept, 4)]]

    @property
    def indel_ikmers(self):
        return int(self.words[16])

    def snv_ikmers(self, which, n):
        return int(self.words[17 + 4 * which + n])

    def astuple(self):
        return tuple(int(v) for v in self.words[:25])


def scan_batch(targets, queries, jobs, cigars, annotations, ksize, mindist):
    """One ScanRecord per job.  targets / queries: str or bytes; jobs: (target index, query index, reverse flag); cigars: per
    job a CIGAR string or a list of runs; annotations: per query its (offset, ksize) pairs, in the contig's own coordinates;
    mindist None or 0: no trimming.  Wrong arguments raise KvArgError before anything is launched."""
    _lib.require_device()
    tbases, toff = _text(targets)
    qbases, qoff = _text(queries)
    jobs = np.ascontiguousarray(jobs, dtype=np.uint32).reshape(-1, 3)
    n = len(jobs)
    if len(cigars) != n or len(annotations) != len(queries):
        raise _lib.KvArgError('scan_batch: {} CIGARs for {} jobs, {} annotation lists for {} queries'.format(
            len(cigars), n, len(annotations), len(queries)))
    runlists = [cigar_runs(cigar) if isinstance(cigar, str) else list(cigar) for cigar in cigars]
    run_counts = np.array([len(runs) for runs in runlists], dtype=np.uint32)
    run_offsets = np.zeros(max(n, 1), dtype=np.uint64)
    if n > 1:
        run_offsets[1:n] = np.cumsum(run_counts[:-1], dtype=np.uint64)
    runs = np.array([run for runlist in runlists for run in runlist], dtype=np.uint32)
    ik_offsets = np.zeros(len(queries) + 1, dtype=np.uint64)
    ik_offsets[1:] = np.cumsum([len(notes) for notes in annotations], dtype=np.uint64)
    ikmers = np.array([pair for notes in annotations for pair in notes], dtype=np.int64).reshape(-1, 2)
    if len(ikmers) and (ikmers.min() < 0 or ikmers.max() > NO_POSITION):
        raise _lib.KvArgError('scan_batch: an interesting k-mer with a negative or oversized offset or size')
    ikmers = np.ascontiguousarray(ikmers, dtype=np.uint32)
    records = np.zeros((max(n, 1), RECORD_WORDS), dtype=np.uint32)
    run_counts = np.ascontiguousarray(run_counts) if n else np.zeros(1, dtype=np.uint32)
    rc = _lib.load().kv_call_scan(
        tbases.ctypes.data, toff.ctypes.data, len(targets), qbases.ctypes.data, qoff.ctypes.data, len(queries), jobs.ctypes.data, n,
        run_offsets.ctypes.data, run_counts.ctypes.data, runs.ctypes.data if len(runs) else None, len(runs), ik_offsets.ctypes.data,
        ikmers.ctypes.data if len(ikmers) else None, int(ksize), int(mindist or 0), records.ctypes.data)
    if rc != 0:
        _lib.check(rc)
    return [ScanRecord(records[k]) for k in range(n)]


def contig_annotations(contig):
    """the (offset, ksize) pairs of a record's interesting k-mers"""
    return [(ikmer.offset, ikmer.ksize) for ikmer in contig.annotations]


class VariantMapping(object):
    """One contig aligned to one cutout of the reference genome, and the calls read from that alignment."""

    def __init__(self, contig, cutout, score=None, cigar=None, strand=1, match=1, mismatch=2, gapopen=5, gapextend=0,
                 homopolyfilt=True, nocall=False, scan=None):
        """scan: (ScanRecord, ksize, mindist) when the mapping is one of a batch that has been scanned already"""
        if score is None and not nocall:
            score, cigar, strand = align_both_strands(cutout, contig, match, mismatch, gapopen, gapextend)
        self.contig = contig
        self.cutout = cutout
        self.nocall = nocall
        self.vartype = None
        if nocall:
            self.score = 0
            return
        self.score = score
        self.strand = strand
        self.do_homopolymer_filter = homopolyfilt
        self.trimmed = 0
        self._origcigar = cigar
        self._scan = scan if scan is not None else self._scan_alone(31, 5)
        record = self._scan[0]
        self.tok = AlignmentTokenizer(self.varseq, self.refrseq, cigar, folded=record.folded)
        self.cigar = self.tok._cigar
        self.vartype = record.vartype
        by_pattern = 'snv' if re.search(SNV_PATTERN, self.cigar) else 'indel' if re.search(INDEL_PATTERN, self.cigar) else None
        if by_pattern != self.vartype:
            raise _lib.KvError(_lib.KV_ERR_HIP, 'the scan classed {} as {}, its pattern says {}'.format(self.cigar, self.vartype, by_pattern))

    def _scan_alone(self, ksize, mindist):
        assert self.strand in (-1, 1)
        record = scan_batch([self.cutout.sequence], [self.contig.sequence], [(0, 0, int(self.strand == -1))], [self._origcigar],
                            [contig_annotations(self.contig)], ksize, mindist)[0]
        return record, ksize, mindist or 0

    def _record(self, ksize, mindist):
        if (self._scan[1], self._scan[2]) != (ksize, mindist or 0):
            self._scan = self._scan_alone(ksize, mindist)
        return self._scan[0]

    def __str__(self):
        target = ''.join(block.target if block.target else '-' * block.length for block in self.tok.blocks)
        query = ''.join(block.query if block.query else '-' * block.length for block in self.tok.blocks)
        same = np.frombuffer(target.encode('latin-1'), dtype=np.uint8) == np.frombuffer(query.encode('latin-1'), dtype=np.uint8)
        bars = np.where(same, ord('|'), ord(' ')).astype(np.uint8).tobytes().decode('latin-1')
        lines = []
        for at in range(0, len(target), 80):
            lines.extend([target[at:at + 80], bars[at:at + 80], query[at:at + 80], ''])
        return '\n'.join(lines).strip()

    @property
    def interval(self):
        return self.cutout.interval

    @property
    def ikmers(self):
        for ikmer in self.contig.annotations:
            seq = self.contig.ikmerseq(ikmer)
            yield seq
            yield kevlar_amd.revcom(seq)

    @property
    def varseq(self):
        assert self.strand in (-1, 1)
        return self.contig.sequence if self.strand == 1 else kevlar_amd.revcom(self.contig.sequence)

    @property
    def refrseq(self):
        return self.cutout.sequence

    @property
    def seqid(self):
        return self.cutout._seqid

    @property
    def pos(self):
        return self.cutout._startpos

    @property
    def _first_match(self):
        """index of the first M block of an interpretable mapping"""
        return 0 if self.tok.blocks[0].type == 'M' else 1

    @property
    def offset(self):
        if self.vartype is None:
            return None
        return 0 if self.tok.blocks[0].type == 'M' else self.tok.blocks[0].length

    @property
    def targetshort(self):
        if self.vartype is None:
            return None
        return self.tok.blocks[0].type == 'I'

    @property
    def match(self):
        return self.tok.blocks[self._first_match] if self.vartype == 'snv' else None

    @property
    def leftflank(self):
        return self.tok.blocks[self._first_match] if self.vartype == 'indel' else None

    @property
    def indel(self):
        return self.tok.blocks[self._first_match + 1] if self.vartype == 'indel' else None

    @property
    def indeltype(self):
        return self.indel.type if self.vartype == 'indel' else None

    @property
    def rightflank(self):
        if self.vartype != 'indel':
            return None
        return self.tok.blocks[-1 if self.tok.blocks[-1].type == 'M' else -2]

    def is_passenger(self, call):
        """no interesting k-mer of the contig, on either strand, lies in the call's window (kv_call_scan counted them)"""
        if call.window is None:
            return False
        return int(call.attribute('IKMERS')) == 0

    def homopolymer_filter(self):
        """an indel followed by a run of five equal bases within the first seven of the right flank"""
        if not self.do_homopolymer_filter:
            return False
        flank = self.rightflank
        if flank is None or len(flank.target) < 5:
            return False
        return flank.target[0] * 5 in flank.target[0:7]

    def call_variants(self, ksize, mindist=6):
        """The calls of this mapping: SNVs of a gapless alignment, or the indel of a one-gap alignment and the SNVs of its flanks,
        or a no-call.  SNVs within `mindist` bases of an end of their block are dropped (None or 0: kept); calls whose window
        holds none of the contig's interesting k-mers are marked as passengers."""
        if self.nocall:
            yield Variant('.', '.', '.', '.', CONTIG=self.contig.sequence, IKMERS=str(len(self.contig.annotations)))
            return
        if self.vartype is None:
            nocall = Variant(self.seqid, self.pos, '.', '.', CONTIG=self.varseq, CIGAR=self.cigar, KSW2=str(self.score))
            nocall.filter(vf.InscrutableCigar)
            yield nocall
            return
        record = self._record(ksize, mindist)
        offset = 0 if self.targetshort else self.offset
        if self.vartype == 'snv':
            calls = self._call_snv(record, 0, self.match, offset, ksize, mindist, True)
        else:
            indel = self._call_indel(record, ksize)
            if self.is_passenger(indel):
                indel.filter(vf.PassengerVariant)
            if self.homopolymer_filter():
                indel.filter(vf.Homopolymer)
            yield indel
            right_offset = offset + self.leftflank.length + (self.indel.length if self.indeltype == 'D' else 0)
            calls = self._call_snv(record, 0, self.leftflank, offset, ksize, mindist, False) + \
                self._call_snv(record, 1, self.rightflank, right_offset, ksize, mindist, False)
        for call in calls:
            if self.is_passenger(call):
                call.filter(vf.PassengerVariant)
            yield call

    def _call_snv(self, record, which, block, offset, ksize, mindist, donocall):
        """the SNVs of scanned block `which` (at most four), or the no-call that stands for none or too many"""
        qseq, tseq, length = block.query, block.target, block.length
        if length < ksize:
            return []
        scanned, trimmed, kept, positions = record.block(which)
        assert scanned == length, (scanned, length)
        if mindist:
            self.trimmed = trimmed
        if kept == 0 or kept > 4:
            if not donocall:
                return []
            nocall = Variant(self.seqid, self.cutout.local_to_global(offset), '.', '.', CONTIG=qseq, CIGAR=self.cigar,
                             KSW2=str(self.score), IKMERS=str(len(self.contig.annotations)))
            nocall.filter(vf.PerfectMatch if kept == 0 else vf.NumerousMismatches)
            return [nocall]
        calls = []
        for n, pos in enumerate(positions):
            lo, hi = max(pos - ksize + 1, 0), min(pos + ksize, length)
            calls.append(Variant(
                self.seqid, self.cutout.local_to_global(pos + offset), tseq[pos].upper(), qseq[pos].upper(), CONTIG=qseq,
                CIGAR=self.cigar, KSW2=str(self.score), IKMERS=str(record.snv_ikmers(which, n)), ALTWINDOW=qseq[lo:hi],
                REFRWINDOW=tseq[lo:hi]))
        return calls

    def _call_indel(self, record, ksize):
        left, gap, right = self.leftflank, self.indel, self.rightflank
        # (a slice from -(ksize - 1): the whole flank when ksize is 1, as in the reference)
        refrwindow = left.target[-(ksize - 1):] + (gap.target if gap.type == 'D' else '') + right.target[:ksize - 1]
        altwindow = left.query[-(ksize - 1):] + (gap.query if gap.type == 'I' else '') + right.query[:ksize - 1]
        refrallele = left.target[-1] + (gap.target if gap.type == 'D' else '')
        altallele = left.query[-1] + (gap.query if gap.type == 'I' else '')
        local = (0 if self.targetshort else self.offset) + left.length
        return Variant(self.seqid, self.cutout.local_to_global(local) - 1, refrallele, altallele, CONTIG=self.varseq, CIGAR=self.cigar,
                       KSW2=str(self.score), IKMERS=str(record.indel_ikmers), ALTWINDOW=altwindow, REFRWINDOW=refrwindow)


def n_ikmers_present(record, window):
    """How many of a record's interesting k-mers lie in `window`, as they are or reverse-complemented (whole-string searches of
    one window; the calls of a batch get this number from the device instead)."""
    n = 0
    for ikmer in record.annotations:
        seq = record.ikmerseq(ikmer)
        if seq in window or kevlar_amd.revcom(seq) in window:
            n += 1
    return n


def trim_terminal_snvs(mismatches, alnlength, mindist=5):
    """(number dropped, the rest) of mismatch positions: those closer than `mindist` to either end are dropped"""
    kept = [mm for mm in mismatches if not (mm < mindist or alnlength - mm < mindist)]
    return len(mismatches) - len(kept), kept
