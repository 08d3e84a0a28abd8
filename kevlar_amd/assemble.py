"""`kevlar assemble`: the reads of every partition into contigs (kevlar/assemble.py), on the GPU.

The reference hands each partition to fermi-lite through a Cython binding.  Here a stated, order-independent rule is computed
for thousands of partitions in one device call (kevlar_amd/csrc/kv_assemble.hip): per partition, the
canonical K-mers seen at least `min_count` times are the nodes of a de Bruijn graph, every maximal chain of simple edges is a
unitig, reported once as the smaller of its two strands, and the contigs are the unitigs strictly longer than the partition's
longest read, longest first.  The device returns all unitigs; the filter, the order and the names are made here.  Names,
annotation, the skipped-partition warning and the closing log line are the reference's.

With `--clean` (tip_nodes, bubble_nodes above 0) the graph is cleaned on the device first, in rounds (section 13, rules 3a to 3c):
short dead ends beside a stronger branch are clipped and of the short paths between one pair of nodes the one of the highest mean
count stays.  Off by default: the answer is then what it was without the option."""
import argparse
import ctypes

import numpy as np

import kevlar_amd
from kevlar_amd import _lib
from kevlar_amd.sequence import Record

DEFAULT_KSIZE = 31
DEFAULT_MIN_COUNT = 2
BATCH_BASES = 256 << 20         # read bases handed to one device call
STAT_NAMES = ('windows', 'distinct', 'solid', 'heads', 'unitigs', 'cycle_keys', 'launches')
CLEAN_NAMES = ('tips', 'tip_keys', 'arms', 'arm_keys', 'rounds')
DEFAULT_CLEAN_ROUNDS = 8


def clean_limits(ksize):
    """(tip_nodes, bubble_nodes) that --clean selects: a read-end error leaves a tip of up to K - 1 nodes, a substitution an arm
    of K, an insertion of up to K bases one of up to 2K - 1"""
    return ksize, 2 * ksize


def unitigs_batch(partitions, ksize=DEFAULT_KSIZE, min_count=DEFAULT_MIN_COUNT, mem_budget=0, tip_nodes=0, bubble_nodes=0,
                  clean_rounds=DEFAULT_CLEAN_ROUNDS):
    """One device call: `partitions` is a list of lists of read sequences.  Returns (the list, per partition, of its unitigs
    as strings -- all of them, each once, in no particular order -- and the stats of the call by STAT_NAMES and CLEAN_NAMES:
    the latter are what the cleaning removed, all 0 at tip_nodes = bubble_nodes = 0)."""
    _lib.require_device()
    lib = _lib.load()
    partitions = [list(reads) for reads in partitions]
    reads = [seq for part in partitions for seq in part]
    read_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        read_off[1:] = np.cumsum(np.array([len(seq) for seq in reads], dtype=np.uint64))
    part_first = np.zeros(len(partitions) + 1, dtype=np.uint64)
    if partitions:
        part_first[1:] = np.cumsum(np.array([len(part) for part in partitions], dtype=np.uint64))
    bases = np.frombuffer(''.join(reads).encode('latin-1'), dtype=np.uint8)
    n_unitigs, n_bases, handle = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_void_p()
    if tip_nodes < 0 or bubble_nodes < 0 or clean_rounds < 0:
        raise _lib.KvArgError('unitigs_batch: tip_nodes, bubble_nodes and clean_rounds must not be negative')
    _lib.check(lib.kv_assemble_clean_batch(bases.ctypes.data if len(bases) else None, read_off.ctypes.data, len(reads),
                                           part_first.ctypes.data, len(partitions), int(ksize), int(min_count), int(mem_budget),
                                           int(tip_nodes), int(bubble_nodes), int(clean_rounds), ctypes.byref(n_unitigs),
                                           ctypes.byref(n_bases), ctypes.byref(handle)))
    try:
        text = np.empty(max(n_bases.value, 1), dtype=np.uint8)
        offsets = np.empty(n_unitigs.value + 1, dtype=np.uint64)
        part_of = np.empty(max(n_unitigs.value, 1), dtype=np.uint32)
        counts = np.empty(max(len(partitions), 1), dtype=np.uint32)
        _lib.check(lib.kv_assemble_fetch(handle, text.ctypes.data, offsets.ctypes.data, part_of.ctypes.data, counts.ctypes.data))
        stats = np.zeros(len(STAT_NAMES), dtype=np.uint64)
        _lib.check(lib.kv_assemble_stats(handle, stats.ctypes.data))
        clean = np.zeros(len(CLEAN_NAMES), dtype=np.uint64)
        _lib.check(lib.kv_assemble_clean_stats(handle, clean.ctypes.data))
    finally:
        lib.kv_assemble_destroy(handle)
    whole = text[:n_bases.value].tobytes().decode('latin-1')
    out = [[] for _ in partitions]
    bounds = offsets.tolist()
    for u, p in enumerate(part_of[:n_unitigs.value].tolist()):
        out[p].append(whole[bounds[u]:bounds[u + 1]])
    if [len(found) for found in out] != counts[:len(partitions)].tolist():
        raise _lib.KvError(_lib.KV_ERR_HIP, 'kv_assemble_fetch: the unitigs per partition do not add up')
    return out, dict(zip(STAT_NAMES + CLEAN_NAMES, (int(v) for v in stats.tolist() + clean.tolist())))


def contigs_of(unitigs, reads):
    """the unitigs strictly longer than the longest read (a contig no longer than a read says nothing a read did not), longest
    first, then by sequence"""
    longest = max([len(read) for read in reads] + [0])
    return sorted((u for u in unitigs if len(u) > longest), key=lambda u: (-len(u), u))


def _batches(partstream, maxreads):
    """lists of (partid, reads, too many reads?) holding at most BATCH_BASES bases of reads to assemble"""
    batch, size = [], 0
    for partid, partition in partstream:
        reads = list(partition)
        if len(reads) > maxreads:
            batch.append((partid, reads, True))
            continue
        nbases = sum(len(read.sequence) for read in reads)
        if size and size + nbases > BATCH_BASES:
            yield batch
            batch, size = [], 0
        batch.append((partid, reads, False))
        size += nbases
    if batch:
        yield batch


def assemble_partitions(partstream, ksize=DEFAULT_KSIZE, min_count=DEFAULT_MIN_COUNT, maxreads=10000, tip_nodes=0, bubble_nodes=0,
                        clean_rounds=DEFAULT_CLEAN_ROUNDS, removed=None):
    """(partid, reads, contig sequences) for every partition of (partid, reads) pairs, in their order; the sequences are None
    for a partition with more than `maxreads` reads.  Partitions go to the device in batches, each batch in one call.
    `removed`, a dictionary, is counted up by CLEAN_NAMES with what the cleaning removed."""
    for batch in _batches(partstream, maxreads):
        found, stats = unitigs_batch([[read.sequence for read in reads] for partid, reads, skip in batch if not skip], ksize, min_count,
                                     tip_nodes=tip_nodes, bubble_nodes=bubble_nodes, clean_rounds=clean_rounds)
        if removed is not None:
            for name in CLEAN_NAMES:
                removed[name] = removed.get(name, 0) + stats[name]
        found = iter(found)
        for partid, reads, skip in batch:
            yield partid, reads, None if skip else contigs_of(next(found), [read.sequence for read in reads])


def assemble(partstream, maxreads=10000, ksize=DEFAULT_KSIZE, min_count=DEFAULT_MIN_COUNT, tip_nodes=0, bubble_nodes=0,
             clean_rounds=DEFAULT_CLEAN_ROUNDS):
    """(partid, contig record) for every contig of every partition, as the reference's assemble(): contigs are named
    `contig{n} kvcc={partid}` with n running over the whole run and carry the partition's interesting k-mers."""
    n = 0
    pn = 0
    progress_indicator = kevlar_amd.ProgressIndicator('[kevlar::assemble] {counter} partitions assembled', interval=10,
                                                      breaks=[100, 1000, 10000], usetimer=True)
    removed = {}
    for partid, reads, sequences in assemble_partitions(partstream, ksize=ksize, min_count=min_count, maxreads=maxreads, tip_nodes=tip_nodes,
                                                        bubble_nodes=bubble_nodes, clean_rounds=clean_rounds, removed=removed):
        pn += 1
        progress_indicator.update()
        if sequences is None:
            kevlar_amd.plog('[kevlar::assemble] WARNING:', 'skipping partition with {:d} reads'.format(len(reads)))
            continue
        records = [Record(name='contig{:d}'.format(i), sequence=seq) for i, seq in enumerate(sequences, 1)]
        for contig in kevlar_amd.augment.augment(reads, records):
            n += 1
            newname = 'contig{}'.format(n)
            if partid is not None:
                newname += ' kvcc={}'.format(partid)
            contig.name = newname
            yield partid, contig
    message = 'processed {} partitions and assembled {} contigs'.format(pn, n)
    if tip_nodes or bubble_nodes:
        message += '; cleaning removed {} tips ({} k-mers) and {} bubble arms ({} k-mers)'.format(
            removed.get('tips', 0), removed.get('tip_keys', 0), removed.get('arms', 0), removed.get('arm_keys', 0))
    kevlar_amd.plog('[kevlar::assemble]', message)


def add_clean_arguments(group):
    """--clean and its three settings, for the parsers of `assemble` and `alac`"""
    group.add_argument('--clean', action='store_true',
                       help='clip tips of at most K nodes and pop bubbles with arms of at most 2K nodes before contigs are reported')
    group.add_argument('--tip-nodes', type=int, metavar='N', default=None, help='clip tips of at most N nodes; implies cleaning')
    group.add_argument('--bubble-nodes', type=int, metavar='N', default=None,
                       help='pop bubbles whose arms have at most N nodes; implies cleaning')
    group.add_argument('--clean-rounds', type=int, metavar='R', default=DEFAULT_CLEAN_ROUNDS,
                       help='at most R rounds of cleaning (default: 8)')


def clean_settings(args):
    """(tip_nodes, bubble_nodes, clean_rounds) of parsed arguments: --clean selects K and 2K, either limit given overrides its own
    and implies cleaning with the other at 0 unless --clean is there too"""
    tip_nodes, bubble_nodes = clean_limits(args.asm_k) if args.clean else (0, 0)
    if args.tip_nodes is not None:
        tip_nodes = args.tip_nodes
    if args.bubble_nodes is not None:
        bubble_nodes = args.bubble_nodes
    return tip_nodes, bubble_nodes, args.clean_rounds


def parser():
    """the reference's `kevlar assemble` flags and defaults (kevlar/cli/assemble.py), plus the two parameters of the rule and the
    cleaning options"""
    parser = argparse.ArgumentParser(prog='python -m kevlar_amd.assemble',
                                     description='Assemble reads into contigs representing putative variants')
    parser.add_argument('-p', '--part-id', type=str, metavar='ID', help='only assemble partition "ID" in the input')
    parser.add_argument('--max-reads', type=int, metavar='N', default=10000,
                        help='do not attempt to assemble any partitions with more than N reads (default: 10000)')
    parser.add_argument('--asm-k', type=int, metavar='K', default=DEFAULT_KSIZE,
                        help='K-mer size of the assembly graph, odd, 13..63 (default: 31)')
    parser.add_argument('--min-count', type=int, metavar='C', default=DEFAULT_MIN_COUNT,
                        help='a K-mer seen fewer than C times in its partition is left out of the graph (default: 2)')
    add_clean_arguments(parser)
    parser.add_argument('-o', '--out', metavar='FILE', help='output file; default is terminal (stdout)')
    parser.add_argument('augfastq', help='annotated reads in augmented Fastq/Fasta format')
    return parser


def main(args):
    readstream = kevlar_amd.parse_augmented_fastx(kevlar_amd.open(args.augfastq, 'r'))
    if args.part_id:
        pstream = kevlar_amd.parse_single_partition(readstream, args.part_id)
    else:
        pstream = kevlar_amd.parse_partitioned_reads(readstream)
    outstream = kevlar_amd.open(args.out, 'w')
    tip_nodes, bubble_nodes, clean_rounds = clean_settings(args)
    for partid, contig in assemble(pstream, maxreads=args.max_reads, ksize=args.asm_k, min_count=args.min_count, tip_nodes=tip_nodes,
                                   bubble_nodes=bubble_nodes, clean_rounds=clean_rounds):
        kevlar_amd.print_augmented_fastx(contig, outstream)
    if args.out not in ('-', None):
        outstream.close()


if __name__ == '__main__':
    main(parser().parse_args())
