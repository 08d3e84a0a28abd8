"""Contig-to-cutout alignment, the first half of `kevlar call` (the reference's kevlar/alignment.pyx over src/align.c and ksw2).

The reference aligns one contig against one reference cutout per call, on one host core, with ksw2's extension aligner run
unbanded and without z-drop: a global alignment with affine gaps whose tie-breaking decides the CIGAR.  Here whole batches of
such pairs go to the GPU (kv_align_batch, kevlar_amd/csrc/kv_align.hip) and come back with the reference's score and CIGAR,
character for character.  Public names follow the reference: `contig_align`, `align_both_strands` (and `kevlar_amd.align`);
`align_batch` is what they are built on, and `align_partitions` runs the alignments of `kevlar call` for whole partition files
in one batch, in the order of the reference's `prelim_call`.

Departures: an empty sequence is an error (the reference returns a degenerate answer), scores lie in 0..127 (the reference
narrows them to int8_t), and a CIGAR may have any length (the reference writes into 4096 characters)."""
import ctypes

import numpy as np

import kevlar_amd
from kevlar_amd import _lib

ALIGN_STRIP = 256                       # query columns per strip of the kernel (include/kvsketch.h KV_ALIGN_STRIP)
DEFAULT_Z_BUDGET = 32 << 30             # direction bytes alive at a time (one per cell of a launch's jobs); allocated only as far as needed
DEFAULT_RUN_CAPACITY = 1 << 16          # CIGAR runs a batch has room for before the call is repeated with more
_OPS = 'MID'


def cigar_string(runs):
    """'%d%c' per run of `length << 4 | op` values, op 0/1/2 = M/I/D (src/align.c:81-86)"""
    return ''.join('{:d}{}'.format(int(run) >> 4, _OPS[int(run) & 0xF]) for run in runs)


def _text(sequences):
    """(bytes as uint8 array, offsets) of a list of str / bytes"""
    raw = [s.encode('latin-1') if isinstance(s, str) else bytes(s) for s in sequences]
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        offsets[1:] = np.cumsum([len(s) for s in raw])
    return np.frombuffer(b''.join(raw) or b'\0', dtype=np.uint8), offsets


def check_scoring(match, mismatch, gapopen, gapextend):
    """The scores as the library takes them (mismatch as a penalty of either sign); raises on what it would refuse."""
    match, mismatch, gapopen, gapextend = int(match), abs(int(mismatch)), int(gapopen), int(gapextend)
    for name, value in (('match', match), ('mismatch', mismatch), ('gapopen', gapopen), ('gapextend', gapextend)):
        if not 0 <= value <= 127:
            raise _lib.KvArgError('alignment score {} = {} outside 0..127'.format(name, value))
    return match, mismatch, gapopen, gapextend


def plan_launches(tlens, qlens, z_budget):
    """(order, launch_ends) of kv_align_plan: the jobs by cell count, largest first (equal ones in the order given), cut where the
    direction bytes of a launch would exceed `z_budget`; launch l is order[launch_ends[l - 1] : launch_ends[l]].  Host code only.
    A job with an empty sequence raises KvArgError, one that alone exceeds the budget KvCapacityError."""
    tlens = np.ascontiguousarray(tlens, dtype=np.uint32)
    qlens = np.ascontiguousarray(qlens, dtype=np.uint32)
    n = len(tlens)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    ends = np.zeros(max(n, 1), dtype=np.uint64)
    n_launches = ctypes.c_uint64(0)
    _lib.check(_lib.load().kv_align_plan(tlens.ctypes.data, qlens.ctypes.data, n, int(z_budget), order.ctypes.data, ends.ctypes.data,
                                         ctypes.byref(n_launches)))
    return order[:n].tolist(), ends[:n_launches.value].tolist()


def z_bytes(tlen, qlen):
    """direction bytes one job keeps on the device"""
    out = ctypes.c_uint64(0)
    _lib.check(_lib.load().kv_align_z_bytes(int(tlen), int(qlen), ctypes.byref(out)))
    return int(out.value)


def last_stats():
    """(launches, ticks the waves spent filling, ticks they spent in traceback and copy, cells) of the last device batch; the
    ticks are those of the device's 100 MHz counter, summed over the jobs.  For measurements and tests."""
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.load().kv_align_stats(out.ctypes.data))
    return tuple(int(v) for v in out)


def _device_batch(targets, queries, jobs, scoring, z_budget, capacity):
    """[(score, cigar)] per (target index, query index, reverse flag) job: one upload, one library call (which launches once per
    budget chunk), repeated with a larger pool when the CIGARs did not fit"""
    _lib.require_device()
    lib = _lib.load()
    tbases, toff = _text(targets)
    qbases, qoff = _text(queries)
    jobs = np.ascontiguousarray(jobs, dtype=np.uint32).reshape(-1, 3)
    n = len(jobs)
    scores = np.zeros(max(n, 1), dtype=np.int32)
    offs = np.zeros(max(n, 1), dtype=np.uint64)
    counts = np.zeros(max(n, 1), dtype=np.uint32)
    need = ctypes.c_uint64(0)
    capacity = max(int(capacity), 1)
    while True:
        runs = np.zeros(capacity, dtype=np.uint32)
        rc = lib.kv_align_batch(tbases.ctypes.data, toff.ctypes.data, len(targets), qbases.ctypes.data, qoff.ctypes.data, len(queries),
                                jobs.ctypes.data, n, scoring[0], scoring[1], scoring[2], scoring[3], int(z_budget), scores.ctypes.data,
                                offs.ctypes.data, counts.ctypes.data, runs.ctypes.data, capacity, ctypes.byref(need))
        if rc != 0:
            _lib.check(rc)
        if need.value <= capacity:
            break
        capacity = int(need.value)
    return [(int(scores[k]), cigar_string(runs[int(offs[k]):int(offs[k]) + int(counts[k])])) for k in range(n)]


def align_batch(targets, queries, pairs, match=1, mismatch=2, gapopen=5, gapextend=0, both_strands=True, z_budget=None,
                run_capacity=DEFAULT_RUN_CAPACITY):
    """Align queries[q] against targets[t] for every (t, q) of `pairs`; sequences are str or bytes.

    both_strands=True: [(score, cigar, strand)], the reverse complement of the query winning only with a strictly greater score
    (strand -1), as in the reference's align_both_strands.  both_strands=False: [(score, cigar)] of the queries as given.
    z_budget: bytes of working memory (one per cell) alive on the device at a time; the batch is cut into launches to fit."""
    scoring = check_scoring(match, mismatch, gapopen, gapextend)
    targets, queries, pairs = list(targets), list(queries), [(int(t), int(q)) for t, q in pairs]
    for t, q in pairs:
        if not (0 <= t < len(targets) and 0 <= q < len(queries)):
            raise _lib.KvArgError('alignment pair ({}, {}) outside {} targets and {} queries'.format(t, q, len(targets), len(queries)))
        if len(targets[t]) == 0 or len(queries[q]) == 0:
            raise _lib.KvArgError('alignment pair ({}, {}) has an empty sequence'.format(t, q))
    if not pairs:
        return []
    strands = (0, 1) if both_strands else (0,)
    jobs = [(t, q, rev) for t, q in pairs for rev in strands]
    found = _device_batch(targets, queries, jobs, scoring, DEFAULT_Z_BUDGET if z_budget is None else z_budget, run_capacity)
    if not both_strands:
        return found
    out = []
    for k in range(len(pairs)):
        (score1, cigar1), (score2, cigar2) = found[2 * k], found[2 * k + 1]
        out.append((score2, cigar2, -1) if score2 > score1 else (score1, cigar1, 1))
    return out


def contig_align(target, query, match=1, mismatch=2, gapopen=5, gapextend=0):
    """(cigar, score) of one query against one target, as the reference's function of this name returns them"""
    score, cigar = align_batch([target], [query], [(0, 0)], match, mismatch, gapopen, gapextend, both_strands=False)[0]
    return cigar, score


def align_both_strands(target, query, match=1, mismatch=2, gapopen=5, gapextend=0):
    """(score, cigar, strand) of a query record against a target record (anything with a `.sequence`)"""
    return align_batch([target.sequence], [query.sequence], [(0, 0)], match, mismatch, gapopen, gapextend)[0]


def align_partitions(contigs_by_partition, cutouts_by_partition, match=1, mismatch=2, gapopen=5, gapextend=0, maxtargetlen=10000,
                     z_budget=None):
    """(partid, contig, cutout, score, cigar, strand) for every contig and every cutout of every partition both mappings know:
    the alignments `kevlar call` computes (kevlar/call.py:67-81), all partitions in one device batch.

    contigs_by_partition / cutouts_by_partition: {partid: [records]} (or (partid, records) pairs), as read by
    parse_partitioned_reads(parse_augmented_fastx(...)) and reference.load_refr_cutouts.  Partitions come in the order of the
    contigs' mapping; inside one, contigs longest first and cutouts by defline, as prelim_call walks them.  A cutout longer than
    `maxtargetlen` (by its defline's interval, as the reference measures it) is not aligned: score 0, cigar None, strand 1, the
    reference's `nocall`."""
    contig_items = contigs_by_partition.items() if hasattr(contigs_by_partition, 'items') else contigs_by_partition
    cutouts_by_partition = dict(cutouts_by_partition.items() if hasattr(cutouts_by_partition, 'items') else cutouts_by_partition)
    rows, targets, queries, pairs = [], [], [], []
    for partid, contigs in contig_items:
        if partid not in cutouts_by_partition:
            continue
        cutouts = sorted(cutouts_by_partition[partid], key=lambda cutout: cutout.defline)
        first_target = len(targets)
        targets.extend(cutout.sequence for cutout in cutouts)
        for contig in sorted(contigs, reverse=True, key=len):
            queries.append(contig.sequence)
            for n, cutout in enumerate(cutouts):
                if maxtargetlen and len(cutout) > maxtargetlen:
                    rows.append((partid, contig, cutout, None))
                else:
                    rows.append((partid, contig, cutout, len(pairs)))
                    pairs.append((first_target + n, len(queries) - 1))
    kevlar_amd.plog('[kevlar::alignment]', 'aligning {} contig/cutout pairs on both strands'.format(len(pairs)))
    found = align_batch(targets, queries, pairs, match, mismatch, gapopen, gapextend, z_budget=z_budget)
    for partid, contig, cutout, at in rows:
        if at is None:
            yield partid, contig, cutout, 0, None, 1
        else:
            score, cigar, strand = found[at]
            yield partid, contig, cutout, score, cigar, strand
