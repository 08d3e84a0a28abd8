"""`kevlar call`: contigs and reference cutouts in, VCF out (the reference's kevlar/call.py and kevlar/cli/call.py).

Every contig of a partition is aligned to every cutout of that partition, the alignments worth reporting are read as variant
calls, the calls of a partition are de-duplicated and adjacent SNVs merged.  The reference does this one pair at a time on one
host core; here all pairs of a run are aligned in one device batch (kevlar_amd.alignment.align_partitions) and all alignments
scanned in one more (kevlar_amd.varmap.scan_batch), and the host only assembles `Variant` objects from the records.

The command line is this module's: `python -m kevlar_amd.call contigs.augfasta cutouts.fa -o calls.vcf`, with the reference's
flags; `python -m kevlar_amd call ...` takes the same ones (kevlar_amd.cli builds its subcommand from parser() below)."""
import argparse
from collections import defaultdict
import sys
import time

import kevlar_amd
from kevlar_amd import khmer
from kevlar_amd.alignment import align_partitions
from kevlar_amd.khmer import _buckets_per_byte
from kevlar_amd.varmap import VariantMapping, contig_annotations, scan_batch
from kevlar_amd.vcf import VCFWriter

last_timing = {}                # seconds of the last call_partitions run: 'align', 'scan', 'assemble' (for measurements)


def alignments_to_report(alignments):
    """Of several alignments of one contig: those that read as a variant if any does, and of these the best-scoring ones."""
    if len(alignments) <= 1:
        return alignments
    readable = [aln for aln in alignments if aln.vartype is not None] or alignments
    best = max(aln.score for aln in readable)
    return [aln for aln in readable if aln.score == best]


def dedup(callstream):
    """One call per (sequence, position), the one with the longest window (of equal ones the first made; the reference keeps
    them in a set and so takes any), sorted by sequence and position."""
    calls = defaultdict(lambda: defaultdict(list))
    for call in callstream:
        calls[call.seqid][call.position].append(call)
    for seqid in sorted(calls):
        for position in sorted(calls[seqid]):
            yield max(calls[seqid][position], key=lambda call: call.windowlength)


def merge_adjacent(callstream):
    """Neighbouring substitutions become one multi-nucleotide call (Variant.test_merge).  A merged call is not merged again
    with the call behind it unless that one follows it directly, as in the reference."""
    prev = None
    for call in callstream:
        if prev is not None:
            merged = prev.test_merge(call)
            if merged is not None:
                call, prev = merged, None
        if prev is not None:
            yield prev
        prev = call
    yield prev


def _mappings(contigs_by_partition, cutouts_by_partition, match, mismatch, gapopen, gapextend, ksize, mindist, homopolyfilt,
              maxtargetlen):
    """[(partid, [[VariantMapping of one contig per cutout] per contig])] in the order given: one alignment batch and one scan
    batch for everything"""
    clock = time.perf_counter()
    rows = list(align_partitions(contigs_by_partition, cutouts_by_partition, match, mismatch, gapopen, gapextend, maxtargetlen))
    last_timing['align'] = time.perf_counter() - clock
    clock = time.perf_counter()
    targets, queries, target_at, query_at = [], [], {}, {}
    jobs, cigars, annotations = [], [], []
    for partid, contig, cutout, score, cigar, strand in rows:
        if cigar is None:
            continue
        if id(cutout) not in target_at:
            target_at[id(cutout)] = len(targets)
            targets.append(cutout.sequence)
        if id(contig) not in query_at:
            query_at[id(contig)] = len(queries)
            queries.append(contig.sequence)
            annotations.append(contig_annotations(contig))
        jobs.append((target_at[id(cutout)], query_at[id(contig)], int(strand == -1)))
        cigars.append(cigar)
    records = iter(scan_batch(targets, queries, jobs, cigars, annotations, ksize, mindist) if jobs else [])
    last_timing['scan'] = time.perf_counter() - clock
    clock = time.perf_counter()
    out = []
    for partid, contig, cutout, score, cigar, strand in rows:
        if cigar is None:
            mapping = VariantMapping(contig, cutout, nocall=True)
        else:
            mapping = VariantMapping(contig, cutout, score, cigar, strand, homopolyfilt=homopolyfilt,
                                     scan=(next(records), ksize, mindist or 0))
        if not out or out[-1][0] != partid:
            out.append((partid, []))
        contigs = out[-1][1]
        if not contigs or contigs[-1][0].contig is not contig:
            contigs.append([])
        contigs[-1].append(mapping)
    last_timing['assemble'] = time.perf_counter() - clock
    return out


def _prelim_calls(partid, contigs, ksize, mindist, debug):
    for alignments in contigs:
        for alignment in alignments_to_report(alignments):
            if debug:
                kevlar_amd.plog('DEBUG ', alignment.cutout.defline, ' vs ', alignment.contig.name, '\n', str(alignment), sep='',
                                end='\n\n')
            for varcall in alignment.call_variants(ksize, mindist):
                if partid is not None:
                    varcall.annotate('PART', partid)
                yield varcall


def prelim_call(targetlist, querylist, partid=None, match=1, mismatch=2, gapopen=5, gapextend=0, ksize=31, refrfile=None,
                debug=False, mindist=5, homopolyfilt=True, maxtargetlen=10000):
    """The calls of one partition before de-duplication: contigs longest first, cutouts by defline."""
    clock = time.perf_counter()
    parts = _mappings([(partid, querylist)], {partid: targetlist}, match, mismatch, gapopen, gapextend, ksize, mindist, homopolyfilt,
                      maxtargetlen)
    for partid, contigs in parts:
        for varcall in _prelim_calls(partid, contigs, ksize, mindist, debug):
            yield varcall
    last_timing['assemble'] = time.perf_counter() - clock - last_timing['align'] - last_timing['scan']


def call(*args, **kwargs):
    """`prelim_call`, de-duplicated and with adjacent SNVs merged"""
    for varcall in merge_adjacent(dedup(prelim_call(*args, **kwargs))):
        yield varcall


def call_partitions(contigs_by_partition, cutouts_by_partition, match=1, mismatch=2, gapopen=5, gapextend=0, ksize=31, refrfile=None,
                    debug=False, mindist=5, homopolyfilt=True, maxtargetlen=10000):
    """(partid, call) for every partition of `cutouts_by_partition` (pairs of (partid, cutouts), in the cutout file's order) that
    `contigs_by_partition` ({partid: contigs}) knows: what the reference's main() writes, from one alignment batch and one scan
    batch for the whole run.  Within a partition the calls are merge_adjacent(dedup(...)) of its preliminary calls."""
    clock = time.perf_counter()
    cutout_items = list(cutouts_by_partition.items() if hasattr(cutouts_by_partition, 'items') else cutouts_by_partition)
    contigs_by_partition = dict(contigs_by_partition.items() if hasattr(contigs_by_partition, 'items') else contigs_by_partition)
    ordered = [(partid, contigs_by_partition[partid]) for partid, cutouts in cutout_items if partid in contigs_by_partition]
    parts = _mappings(ordered, cutout_items, match, mismatch, gapopen, gapextend, ksize, mindist, homopolyfilt, maxtargetlen)
    for partid, contigs in parts:
        for varcall in merge_adjacent(dedup(_prelim_calls(partid, contigs, ksize, mindist, debug))):
            yield partid, varcall
    last_timing['assemble'] = time.perf_counter() - clock - last_timing['align'] - last_timing['scan']


def load_contigs(contigstream):
    kevlar_amd.plog('[kevlar::call] Loading contigs into memory by partition')
    contigs_by_partition = {}
    ncontigs = 0
    for partid, contiglist in contigstream:
        ncontigs += len(contiglist)
        contigs_by_partition[partid] = contiglist
    kevlar_amd.plog('[kevlar::call]', 'Loaded {} contigs from {} partitions'.format(ncontigs, len(contigs_by_partition)))
    return contigs_by_partition


def parser():
    """the reference's `kevlar call` flags and defaults (kevlar/cli/call.py)"""
    parser = argparse.ArgumentParser(prog='python -m kevlar_amd.call', add_help=False, description='Align variant-related contigs '
                                     'to their cutouts of the reference genome and call the variants from the alignments.')
    parser._positionals.title = 'Required inputs'
    score_args = parser.add_argument_group('Alignment scoring')
    score_args.add_argument('-A', '--match', type=int, default=1, metavar='A', help='match score; default is 1')
    score_args.add_argument('-B', '--mismatch', type=int, default=2, metavar='B', help='mismatch penalty; default is 2')
    score_args.add_argument('-O', '--open', type=int, default=5, metavar='O', help='gap open penalty; default is 5')
    score_args.add_argument('-E', '--extend', type=int, default=0, metavar='E', help='gap extension penalty; default is 0')
    mask_args = parser.add_argument_group('Mask generation settings')
    mask_args.add_argument('--gen-mask', metavar='FILE', help='save a nodetable of all k-mers that span any variant call')
    mask_args.add_argument('--mask-mem', type=khmer.khmer_args.memory_setting, default=1e6, metavar='MEM',
                           help='memory of the node table')
    mask_args.add_argument('--mask-max-fpr', type=float, default=0.01, metavar='FPR',
                           help='warn if the estimated false positive rate of the mask exceeds FPR; default is 0.01')
    misc_args = parser.add_argument_group('Miscellaneous settings')
    misc_args.add_argument('-h', '--help', action='help', help='show this help message and exit')
    misc_args.add_argument('-d', '--debug', action='store_true', help='show debugging output')
    misc_args.add_argument('--no-homopoly-filter', action='store_true', help='do not filter short indels next to homopolymers')
    misc_args.add_argument('--max-target-length', type=int, default=10000, metavar='L',
                           help='make no call against a cutout of more than L bp; default is 10000')
    misc_args.add_argument('--refr', metavar='FILE', help='reference genome, named in the VCF header')
    misc_args.add_argument('-o', '--out', metavar='FILE', help='output file; default is terminal (stdout)')
    misc_args.add_argument('-k', '--ksize', type=int, default=31, metavar='K', help='k-mer size; default is 31')
    parser.add_argument('queryseq', help='contigs, as augmented FASTA / FASTQ with partition labels')
    parser.add_argument('targetseq', help='cutouts of the reference genome found by "kevlar localize"')
    return parser


def main(args):
    outstream = kevlar_amd.open(args.out, 'w')
    writer = VCFWriter(outstream, source='kevlar::call', refr=args.refr)
    writer.write_header()
    contigs_by_partition = load_contigs(kevlar_amd.parse_partitioned_reads(
        kevlar_amd.parse_augmented_fastx(kevlar_amd.open(args.queryseq, 'r'))))
    cutouts = list(kevlar_amd.parse_partitioned_reads(kevlar_amd.reference.load_refr_cutouts(kevlar_amd.open(args.targetseq, 'r'))))
    windows = []
    if args.gen_mask:
        kevlar_amd.plog('[kevlar::call]', 'generating mask of variant-spanning k-mers')
    caller = call_partitions(
        contigs_by_partition, cutouts, match=args.match, mismatch=args.mismatch, gapopen=args.open, gapextend=args.extend,
        ksize=args.ksize, refrfile=args.refr, debug=args.debug, mindist=5, homopolyfilt=not args.no_homopoly_filter,
        maxtargetlen=args.max_target_length)
    for partid, varcall in caller:
        window = varcall.attribute('ALTWINDOW')
        if args.gen_mask and window is not None and len(window) >= args.ksize:
            windows.append(window)
        writer.write(varcall)
    if outstream is not sys.stdout:
        outstream.close()
    if args.gen_mask:
        ntables = 4
        mask = khmer.Nodetable(args.ksize, args.mask_mem * _buckets_per_byte['nodegraph'] / ntables, ntables)
        if windows:
            mask.consume_batch(khmer.ReadBatch(windows))          # every window of the run in one device batch
        fpr = khmer.calc_expected_collisions(mask, max_false_pos=1.0)
        if fpr > args.mask_max_fpr:
            kevlar_amd.plog('[kevlar::call]', 'WARNING: mask FPR is {:.4f}; exceeds user-specified limit of {:.4f}'.format(
                fpr, args.mask_max_fpr))
        mask.save(args.gen_mask)


if __name__ == '__main__':
    main(parser().parse_args())
