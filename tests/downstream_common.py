"""What the tests of the stages behind the scan share (tests/test_downstream_reference.py on the host, tests/test_gpu_downstream.py
on the device): a seeded generator of annotated read streams with the irregularities real streams have, and LITERAL restatements
of `kevlar filter` (kevlar/filter.py:15-82) and `kevlar partition` (kevlar/readgraph.py:43-161 + kevlar/partition.py:15-55) in
plain Python -- dicts, sets and strings, one k-mer at a time.  The restatements import nothing of the product's filter, partition,
readgraph or annotated modules: only kevlar_amd.revcommin, the Record class and the text codec, which have their own tests against
the reference's files.  Not a test module and not a conftest: nothing here is collected.

The planted k-mers aim at the read graph's key arithmetic (kevlar_amd/csrc/kv_graph.hip): the canonical k-mer is held as a 256-bit
number, the k-mer RIGHT-aligned, in four 64-bit words, most significant first; base j of a k-mer lies in word (128 - k + j) // 32.
A k-mer and its reverse complement can agree in at most (k - 1) // 2 leading bases without being equal, so which word decides the
strand depends on k: the planted k-mers agree exactly up to every word boundary below that limit, through 32 bases where k allows
it, and through (k - 1) // 2 bases -- key_word_deciding() says which word that is, and the host test asserts that the case table
reaches the second, third and fourth word."""
import random
from collections import namedtuple

import kevlar_amd
from kevlar_amd.sequence import KmerOfInterest, Record, format_augmented_fastx

_COMP = str.maketrans('ACGT', 'TGCA')
PLANTED_MAX = 6          # the --max-abund the planted k-mers are cut for: one k-mer in exactly 6 reads, one in 8
PLANTED_MIN = 3          # the --min-abund under which the planted duplicate trio falls below the bound AFTER dedup
FAMILY = 150             # k-mers that differ only before their last 32 bases (k >= 36), each in two reads

Case = namedtuple('Case', 'name seed k nsamples flags')
Spec = namedtuple('Spec', 'name sequence quality notes mates')      # notes: [(offset, abundances)]


def rc(seq):
    return seq.translate(_COMP)[::-1]


def key_word_deciding(kmer):
    """index (0..3) of the 64-bit key word in which a k-mer and its reverse complement first differ; None for a palindrome"""
    k, other = len(kmer), rc(kmer)
    for j in range(k):
        if kmer[j] != other[j]:
            return (128 - k + j) // 32
    return None


# ---- the generator ---------------------------------------------------------------------------------------------------------
class Stream(object):
    """specs: the records as plain tuples (records() builds fresh Record objects: partition() renames the ones it is given);
    text: the same stream rendered by kevlar_amd.sequence.format_augmented_fastx (blank lines between records if the case asks);
    planted: what was planted, by read names; mask_seqs: the parts of the genome a mask is to consume"""

    def __init__(self, case, specs, text, planted, mask_seqs):
        self.case, self.specs, self.text, self.planted, self.mask_seqs = case, specs, text, planted, mask_seqs

    def records(self):
        return records_of(self.specs, self.case.k)


def records_of(specs, k):
    return [Record(s.name, s.sequence, s.quality, annotations=[KmerOfInterest(k, off, tuple(ab)) for off, ab in s.notes], mates=list(s.mates))
            for s in specs]


def render(specs, k, rng=None):
    pieces = []
    for rec in records_of(specs, k):
        pieces.append(format_augmented_fastx(rec))
        if rng is not None and rng.random() < 0.15:
            pieces.append('\n' * rng.randint(1, 2))
    return ''.join(pieces)


def _bases(rng, n):
    return ''.join(rng.choice('ACGT') for _ in range(n))


def _abund(rng, nsamples, controls):
    case = rng.choice([0, 1, 7, 12, 40, 255, 256, 300, 1000]) if rng.random() < 0.3 else rng.randint(6, 60)
    noisy = [c if rng.random() < 0.9 else rng.choice([0, 1, 2, 260]) for c in controls]
    return tuple([case] + noisy[:nsamples - 1])


def generate(case):
    """The stream of one case.  Flags: 'dupnames' (a name twice, with different annotation sets), 'dupseqs' (reads that repeat
    another's sequence or its reverse complement), 'fasta' (records without quality among the FASTQ ones), 'mates' (#mateseq=
    lines), 'blank' (blank lines between records), 'odd' (a read with an N outside every annotated k-mer at either end, and a
    lower-case read with annotations)."""
    rng = random.Random(case.seed * 1000003 + case.k)
    k, S, flags = case.k, case.nsamples, case.flags
    specs, planted, mask_seqs = [], {}, []
    serial = [0]

    def quality(n):
        return ''.join(chr(rng.randint(53, 73)) for _ in range(n))

    def add(name, seq, notes, fastq=True):
        if 'fasta' in flags and rng.random() < 0.3:
            fastq = False
        mates = []
        if 'mates' in flags and rng.random() < 0.25:
            mates = [_bases(rng, rng.randint(20, 120)) for _ in range(rng.randint(1, 2))]
        specs.append(Spec(name, seq, quality(len(seq)) if fastq else None, sorted(notes), mates))
        return name

    def fresh(prefix):
        serial[0] += 1
        name = '{}{}'.format(prefix, serial[0])
        return name + (' lane={}'.format(rng.randint(1, 8)) if rng.random() < 0.2 else '/{}'.format(rng.randint(1, 2)))

    # (1) loci of a small random genome: reads of either strand around a few interesting positions each
    nloci = 36
    for li in range(nloci + 1):
        long_one = li == nloci
        length = 3600 if long_one else rng.randint(2 * k + 150, 2 * k + 450)
        locus = _bases(rng, length)
        if li % 4 == 0:
            mask_seqs.append(locus[:length // 2 + k])             # (half a locus: reads across the middle keep some annotations)
        spots = sorted(rng.sample(range(0, length - k + 1), 6 if long_one else rng.randint(1, 3)))
        controls = {p: [rng.choice([0, 0, 0, 1, 1, 2, 9, 300]) if rng.random() < 0.25 else rng.choice([0, 1]) for _ in range(4)] for p in spots}
        nreads = 10 if long_one else rng.choice([2, 2, 2, 3, 3, 4, 4, 6, 8, 8, 12, 20])
        if li % 4 == 0:
            nreads = max(nreads, 14)                                     # (deep enough that the mask, not the depth, costs the annotations)
        for ri in range(nreads):
            p = rng.choice(spots)
            if long_one and ri == 0:
                rlen, start = 3300, 100                                  # the one read of several thousand bases
            else:
                rlen = k if rng.random() < 0.1 else rng.randint(k, min(length, k + rng.choice([1, 8, 60, 250])))
                start = rng.randint(max(0, p + k - rlen), min(p, length - rlen))
            seq = locus[start:start + rlen]
            here = [q for q in spots if start <= q and q + k <= start + rlen and rng.random() < 0.92]
            minus = rng.random() < 0.5
            notes = [((rlen - k - (q - start)) if minus else (q - start), _abund(rng, S, controls[q])) for q in here]
            add(fresh('g{}r'.format(li)), rc(seq) if minus else seq, notes)
    natural = list(specs)

    # (2) planted k-mers, each in reads of its own with random flanks (only the planted k-mer is annotated)
    def embed(prefix, kmer, minus):
        left, right = _bases(rng, rng.randint(3, 14)), _bases(rng, rng.randint(3, 14))
        seq, off = left + kmer + right, len(left)
        if minus:
            seq, off = rc(seq), len(right)
        return add(fresh(prefix), seq, [(off, _abund(rng, S, [0, 1, 0, 0]))])

    if k % 2 == 0:
        half = _bases(rng, k // 2)
        pal = half + rc(half)
        planted['palindrome'] = (pal, [embed('palf', pal, False) for _ in range(2)], [embed('palr', pal, True) for _ in range(2)])
    pairs = []
    for where in (k - 1, 0):                                     # equal except in the last / in the first base
        x = _bases(rng, k)
        y = x[:where] + rng.choice([b for b in 'ACGT' if b != x[where]]) + x[where + 1:]
        pairs.append(([embed('nx', x, False), embed('nx', x, True)], [embed('ny', y, False), embed('ny', y, True)]))
    planted['near'] = pairs
    limit = (k - 1) // 2
    agree = sorted({m for m in (k - 96, k - 64, k - 32, 32, limit) if 1 <= m <= limit})
    strands = []
    for m in agree:
        x = list(_bases(rng, k))
        for i in range(m):
            x[k - 1 - i] = x[i].translate(_COMP)
        if m != k - 1 - m:
            x[k - 1 - m] = x[m]                                   # base m and the complement of its mirror differ
        x = ''.join(x)
        assert x[:m] == rc(x)[:m] and x[m] != rc(x)[m]
        strands.append((x, m, [embed('sf', x, False), embed('sf', x, False)], [embed('sr', x, True)]))
    planted['strands'] = strands
    if k >= 36:
        tail = _bases(rng, 31) + 'A'                              # forward starts below T, reverse complement with T: forward is canonical
        heads = set()
        while len(heads) < FAMILY:
            heads.add(rng.choice('ACG') + _bases(rng, k - 33))
        planted['family'] = [[embed('fam', head + tail, False), embed('fam', head + tail, True)] for head in sorted(heads)]
    exact, over = _bases(rng, k), _bases(rng, k)
    planted['max_exact'] = [embed('mx', exact, i % 2 == 1) for i in range(PLANTED_MAX)]
    planted['max_over'] = [embed('mo', over, i % 2 == 1) for i in range(PLANTED_MAX + 2)]
    trio = _bases(rng, k)
    first = embed('tri', trio, False)
    src = specs[-1]
    mirrored = [(len(src.sequence) - k - off, ab) for off, ab in src.notes]
    planted['min_after_dedup'] = [first, add(fresh('tri'), rc(src.sequence), mirrored), embed('tri', trio, True)]

    # (3) irregularities over the natural reads
    if 'dupseqs' in flags:
        for src in rng.sample(natural, 25):
            if rng.random() < 0.5:
                add(fresh('dup'), src.sequence, list(src.notes))
            else:
                add(fresh('dup'), rc(src.sequence), [(len(src.sequence) - k - off, ab) for off, ab in src.notes])
    if 'dupnames' in flags:
        rich = [s for s in natural if len(s.notes) >= 2]
        for src in rng.sample(rich, min(12, len(rich))):
            at = specs.index(src)
            cut = rng.randint(1, len(src.notes) - 1)
            specs[at] = src._replace(notes=src.notes[:cut])
            specs.append(src._replace(notes=src.notes[cut:], mates=[]))
        planted['dupnames'] = True
    if 'odd' in flags:
        with_notes = [s for s in natural if s.notes and s.quality]
        a, b, c = rng.sample(with_notes, 3)
        odd = [add(fresh('nleft'), 'N' + a.sequence, [(off + 1, ab) for off, ab in a.notes]),
               add(fresh('nright'), b.sequence + 'N', list(b.notes)),
               add(fresh('lower'), c.sequence.lower(), list(c.notes))]
        planted['odd'] = odd
    rng.shuffle(specs)
    text = render(specs, k, rng if 'blank' in flags else None)
    return Stream(case, specs, text, planted, mask_seqs)


# ---- kevlar/filter.py:15-82 ---------------------------------------------------------------------------------------------------
FilterResult = namedtuple('FilterResult', 'records text processed validated stats')


def restate_filter(ok, records, memory=1e6, mask=None, casemin=6, ctrlmax=1):
    """first_pass + second_pass over an ORACLE Counttable(k, memory / 4, 4); `mask`: an oracle sketch or None.  The records are
    changed as the reference changes them (their annotations replaced by the validated ones)."""
    counts, n = None, 0
    unmasked = None          # what the recount would be with no mask at all: tells which annotations the MASK costs
    truth = {}
    for n, read in enumerate(records, 1):                                     # first_pass, filter.py:23-34
        if len(read.annotations) == 0:
            continue
        if counts is None:
            counts = ok.Counttable(read.annotations[0].ksize, memory / 4, 4)
            unmasked = ok.Counttable(read.annotations[0].ksize, memory / 4, 4)
        for ikmer in read.annotations:
            ikseq = read.ikmerseq(ikmer)
            unmasked.add(ikseq)
            if mask and mask.get(ikseq) > 0:
                continue
            counts.add(ikseq)
            truth[kevlar_amd.revcommin(ikseq.upper())] = truth.get(kevlar_amd.revcommin(ikseq.upper()), 0) + 1
    stats = dict(by_mask=0, by_recount=0, by_control=0, partial=0, vanished=0, inflated=0)
    kept = []
    for read in records:                                                      # second_pass, filter.py:59-78
        validated = []
        for ikmer in read.annotations:
            ikseq = read.ikmerseq(ikmer)
            if sum([1 for a in ikmer.abund[1:] if a > ctrlmax]) > 0:
                stats['by_control'] += 1
                continue
            newcount = counts.get(ikseq)
            if newcount > min(255, truth.get(kevlar_amd.revcommin(ikseq.upper()), 0)):
                stats['inflated'] += 1
            if newcount < casemin:
                # by the mask: kept in a run without the mask (same table geometry), dropped in this one
                stats['by_mask' if unmasked.get(ikseq) >= casemin else 'by_recount'] += 1
                continue
            validated.append(KmerOfInterest(ikmer.ksize, ikmer.offset, tuple([newcount] + list(ikmer.abund[1:]))))
        if len(validated) == 0:
            stats['vanished'] += 1
            continue
        if len(validated) < len(read.annotations):
            stats['partial'] += 1
        read.annotations = validated
        kept.append(read)
    text = ''.join(format_augmented_fastx(read) for read in kept)
    return FilterResult(kept, text, n, len(kept), stats)


# ---- kevlar/readgraph.py:43-161 + kevlar/partition.py:15-55 -------------------------------------------------------------------
PartitionResult = namedtuple('PartitionResult', 'partitions text nreads components nedges stats')


def restate_partition(records, minabund=None, maxabund=None, dedup=True):
    """partitions: [[name, ...], ...] in output order (numbered from 1); text: what `kevlar partition` prints for them; nreads:
    the reads written; components: every connected component of the graph, singletons included, as a set of frozensets of
    names; nedges: distinct pairs of nodes that share a retained k-mer."""
    node, temp = {}, {}
    for record in records:                                                    # ReadGraph.load, readgraph.py:62-73
        node[record.name] = record                                            # (add_node: the last record of a name is the node's)
        for kmer in record.annotations:
            temp.setdefault(kevlar_amd.revcommin(record.ikmerseq(kmer)), set()).add(record.name)
    stats = dict(by_max=0, by_min=0, dedup=0, dedup_rc=0, dropped_small=0, dupnames=len(records) - len(node))
    if minabund is None and maxabund is None:                                 # readgraph.py:75-84
        ikmers = temp
    else:
        ikmers = {}
        for kmer, readset in temp.items():
            minfail = minabund and len(readset) < minabund
            maxfail = maxabund and len(readset) > maxabund
            stats['by_min'] += bool(minfail)
            stats['by_max'] += bool(maxfail)
            if not minfail and not maxfail:
                ikmers[kmer] = readset
    edges, near = set(), {name: set() for name in node}                       # populate_edges, readgraph.py:111-125
    for readset in ikmers.values():
        names = sorted(readset)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                edges.add((a, b))
                near[a].add(b)
                near[b].add(a)
    seen, components = set(), []                                              # networkx.connected_components
    for name in node:
        if name in seen:
            continue
        cc, todo = {name}, [name]
        while todo:
            for other in near[todo.pop()]:
                if other not in cc:
                    cc.add(other)
                    todo.append(other)
        seen |= cc
        components.append(cc)
    partitions = []
    for cc in sorted(components, reverse=True, key=lambda c: (len(c), sorted(c))):      # partitions, readgraph.py:137-161
        if len(cc) == 1:
            continue
        members = sorted(cc)                                                  # (the deterministic order the product documents)
        if dedup:
            unique, kept = {}, []
            for name in members:
                minread = kevlar_amd.revcommin(node[name].sequence)
                if minread in unique:
                    stats['dedup'] += 1
                    stats['dedup_rc'] += unique[minread] != node[name].sequence
                    continue
                unique[minread] = node[name].sequence
                kept.append(name)
            members = kept
            if minabund and len(members) < minabund:
                stats['dropped_small'] += 1
                continue
        partitions.append(members)
    pieces = []
    for n, part in enumerate(partitions, 1):                                  # partition.py:44-48
        for name in part:
            rec = node[name]
            pieces.append(format_augmented_fastx(Record('{} kvcc={:d}'.format(rec.name, n), rec.sequence, rec.quality, rec.annotations, rec.mates)))
    return PartitionResult(partitions, ''.join(pieces), sum(len(p) for p in partitions), {frozenset(c) for c in components}, len(edges), stats)


def group_of(result, name):
    """the connected component (frozenset of names) that holds `name`"""
    return next(c for c in result.components if name in c)


# ---- the case tables ----------------------------------------------------------------------------------------------------------
ALL = frozenset(['dupnames', 'dupseqs', 'fasta', 'mates', 'blank'])


def _case(i, k, nsamples, *flags):
    return Case('k{}-s{}-{}'.format(k, nsamples, '+'.join(flags) or 'plain'), 100 + i, k, nsamples, frozenset(flags))


PARTITION_CASES = [
    _case(0, 13, 3, 'dupseqs', 'blank'),
    _case(1, 31, 1, 'dupnames', 'dupseqs', 'fasta', 'mates', 'blank'),
    _case(2, 32, 2, 'dupseqs', 'fasta'),
    _case(3, 33, 3, 'dupnames', 'dupseqs'),
    _case(4, 51, 4, 'dupnames', 'dupseqs', 'mates', 'blank'),
    _case(5, 63, 5, 'dupseqs'),
    _case(6, 64, 3, 'dupnames', 'dupseqs', 'fasta'),
    _case(7, 65, 2, 'dupseqs', 'mates'),
    _case(8, 95, 1, 'dupnames', 'dupseqs', 'blank'),
    _case(9, 96, 4, 'dupseqs', 'fasta', 'mates'),
    _case(10, 97, 3, 'dupnames', 'dupseqs'),
    _case(11, 100, 2, 'dupseqs'),
    _case(12, 127, 5, 'dupnames', 'dupseqs', 'fasta', 'mates', 'blank'),
    _case(13, 128, 3, 'dupnames', 'dupseqs', 'blank'),
]
# (min-abund, max-abund, dedup) of the runs of every partition case: the CLI's defaults, unbounded, and bounds that bite
PARTITION_OPTIONS = [(2, 200, True), (0, 0, True), (PLANTED_MIN, PLANTED_MAX, True), (2, PLANTED_MAX, False), (None, None, True)]

# (case, memory, kind of mask or None, case-min, ctrl-max)
FILTER_CASES = [
    (_case(20, 13, 3, 'fasta', 'blank'), 300, 'Nodegraph', 6, 1),
    (_case(41, 31, 1, 'dupnames', 'mates'), 1e6, 'Nodetable', 6, 1),
    (_case(22, 32, 2, 'dupseqs', 'fasta', 'odd'), 4000, 'Counttable', 5, 0),
    (_case(23, 33, 3, 'dupnames', 'dupseqs', 'fasta', 'mates', 'blank'), 500, None, 6, 1),
    (_case(24, 51, 4, 'dupseqs', 'mates', 'odd'), 3000, 'SmallCounttable', 4, 1),
    (_case(25, 63, 5, 'dupseqs'), 1e6, 'Nodetable', 6, 2),
    (_case(26, 64, 2, 'dupnames', 'blank'), 400, 'Counttable', 3, 1),
    (_case(27, 65, 3, 'dupseqs', 'fasta'), 5000, 'SmallCounttable', 6, 1),
    (_case(28, 96, 1, 'dupseqs', 'odd'), 1e6, None, 6, 1),
    (_case(29, 128, 4, 'dupnames', 'dupseqs', 'mates'), 600, 'Nodetable', 5, 1),
    (_case(30, 129, 3, 'dupseqs', 'blank'), 2500, 'Counttable', 6, 1),
    (_case(31, 200, 2, 'dupseqs', 'fasta', 'odd'), 1e6, 'Nodetable', 6, 0),
    (_case(32, 25, 3, 'dupseqs', 'mates'), 1e6, 'Nodegraph', 6, 1),
]
# partition on streams with an N outside every annotated k-mer and a lower-case read with annotations
ODD_CASES = [Case('odd-k{}'.format(k), 40 + k, k, 3, frozenset(['dupseqs', 'dupnames', 'odd'])) for k in (31, 64, 100)]
SMALL_MEMORY = 1000       # filter cases at or below this many bytes must show recounts inflated by collisions


def oracle_mask(ok, kind, stream):
    """a mask of the given kind that has consumed a part of the stream's genome (a quarter of its loci)"""
    if kind is None:
        return None
    mask = getattr(ok, kind)(stream.case.k, 20000, 4)
    for seq in stream.mask_seqs:
        mask.consume(seq)
    return mask
