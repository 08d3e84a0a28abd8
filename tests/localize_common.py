"""What the tests of `kevlar localize` share (tests/test_localize_reference.py on the host, tests/test_gpu_localize.py on the
device): a LITERAL restatement of the matching rule in plain Python -- strings, sets and dicts, one window at a time -- and of
the cutout procedure built on it (kevlar/localize.py:55-95,147-224), readers for the fixtures under tests/golden/localize, and
seeded generators of the synthetic cases.  Nothing of kevlar_amd.localize or kevlar_amd.reference is imported here.  Not a test
module and not a conftest: nothing here is collected.

The rule: a seed is the smaller (as a string) of a contig window of length Z and its reverse complement, upper-cased; a contig
window with any byte outside A/C/G/T (either case) yields no seed.  A genome window of length Z -- inside ONE sequence, all
bytes A/C/G/T in either case -- matches when the smaller of its upper-cased self and reverse complement is a seed; the match is
(seed, seqid, start of the window), seqid being the defline up to the first blank.  One window, one match: a palindromic seed
counts once per position.  A seed with more than max_occ matches in the whole genome has none."""
import gzip
import os
import random
import re
from collections import defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
LOCALIZE_DATA = os.path.join(HERE, 'golden', 'localize')
_COMP = str.maketrans('ACGT', 'TGCA')
_PLAIN = set('ACGT')
LANE_RUN = 64            # windows one lane of the scan kernel rolls over (kevlar_amd/csrc/kv_localize.hip LOC_RUN)


def fixture(name):
    return os.path.join(LOCALIZE_DATA, name)


def rc(seq):
    return seq.translate(_COMP)[::-1]


def minseq(seq):
    other = rc(seq)
    return seq if seq <= other else other


def _open(path):
    return gzip.open(path, 'rt') if path.endswith('.gz') else open(path, 'r')


def read_fasta(path):
    """[(seqid, sequence)] of a plain FASTA file; seqid is the defline up to the first blank"""
    records = []
    with _open(path) as stream:
        for line in stream:
            line = line.rstrip('\n')
            if line.startswith('>'):
                records.append([line[1:].split()[0] if line[1:].split() else '', []])
            elif records:
                records[-1][1].append(line.strip())
    return [(seqid, ''.join(parts)) for seqid, parts in records]


def read_contigs(path):
    """[(name, sequence)] of an augmented FASTA file (annotation lines end in '#')"""
    contigs = []
    with _open(path) as stream:
        lines = [line.rstrip('\n') for line in stream]
    for i, line in enumerate(lines):
        if line.startswith('>'):
            contigs.append((line[1:].strip(), lines[i + 1].strip()))
    return contigs


def partitions_of(contigs):
    """[(partition id or None, [(name, sequence)])]: runs of contigs with the same kvcc label"""
    parts = []
    for name, seq in contigs:
        found = re.search(r'kvcc=(\d+)', name)
        partid = found.group(1) if found else None
        if not parts or parts[-1][0] != partid:
            parts.append((partid, []))
        parts[-1][1].append((name, seq))
    return parts


def seeds_of(contig_seqs, z):
    seeds = set()
    for seq in contig_seqs:
        for i in range(len(seq) - z + 1):
            window = seq[i:i + z].upper()
            if set(window) <= _PLAIN:
                seeds.add(minseq(window))
    return seeds


def restated_hits(contig_seqs, records, z):
    """{seed: [(seqid, position)]} by the rule of the module's docstring, one genome window at a time, before any cap"""
    seeds = seeds_of(contig_seqs, z)
    either = seeds | {rc(seed) for seed in seeds}
    found = defaultdict(list)
    for seqid, seq in records:
        upper = seq.upper()
        run = 0                                   # bases A/C/G/T in a row ending here
        for end in range(len(upper)):
            run = run + 1 if upper[end] in _PLAIN else 0
            if run < z:
                continue
            window = upper[end - z + 1:end + 1]
            if window in either:
                found[minseq(window)].append((seqid, end - z + 1))
    return dict(found)


def capped(hits, max_occ=5000):
    """{(seed, seqid, position)}: a seed with more than max_occ positions has none (a false max_occ: no cap)"""
    return {(seed, seqid, pos) for seed, where in hits.items() if not max_occ or len(where) <= max_occ for seqid, pos in where}


def restated_matches(contig_seqs, records, z, max_occ=5000):
    return capped(restated_hits(contig_seqs, records, z), max_occ)


def restated_localize(partitions, records, z, delta=50, maxdiff=None, incl=None, excl=None, max_occ=5000, hits=None):
    """[(partition id, defline, sequence)] in the reference's order: partitions as given, sequences by id, clusters by
    position.  partitions: [(id, [(name, sequence)])]; hits: restated_hits() of all their contigs, if the caller has them."""
    if hits is None:
        hits = restated_hits([seq for pid, part in partitions for name, seq in part], records, z)
    triples = capped(hits, max_occ)
    where = defaultdict(list)
    for seed, seqid, pos in triples:
        where[seed].append((seqid, pos))
    genome = dict(records)
    out = []
    for partid, part in partitions:
        on = defaultdict(list)
        for seed in seeds_of([seq for name, seq in part], z):
            for seqid, pos in where.get(seed, ()):
                on[seqid].append(pos)
        dist = maxdiff if maxdiff is not None else 3 * max(len(seq) for name, seq in part)
        for seqid in sorted(on):
            if excl and re.search(excl, seqid) is not None:
                continue
            if incl and re.search(incl, seqid) is None:
                continue
            positions = sorted(on[seqid])
            clusters = [[positions[0]]]
            for pos in positions[1:]:
                if dist and pos - clusters[-1][-1] > dist:
                    clusters.append([])
                clusters[-1].append(pos)
            for cluster in clusters:
                start = max(cluster[0] - delta, 0)
                end = min(cluster[-1] + z + delta, len(genome[seqid]))
                out.append((partid, '{}_{}-{}'.format(seqid, start, end), genome[seqid][start:end]))
    return out


# ---- generators ---------------------------------------------------------------------------------------------------------
def random_dna(rng, n):
    return ''.join(rng.choice('ACGT') for _ in range(n))


def mutate(seq, at):
    return seq[:at] + 'ACGT'[('ACGT'.index(seq[at]) + 1) % 4] + seq[at + 1:]


def key_arithmetic_case(z, seed=0):
    """A 20 kb genome and 200 seeds of length z: 100 cut from the genome (every other one reverse-complemented), 100 random;
    then near misses of planted windows -- one base changed at position 0, z - 1 and at 31, 32, 33, 63, 64, 65 where z has
    them, the positions around the 64-bit word boundaries of the key -- and, for even z, a palindrome planted twice."""
    rng = random.Random(1000 + z + seed)
    genome = random_dna(rng, 20000)
    palindromes = []
    if z % 2 == 0:
        half = random_dna(rng, z // 2)
        palindromes.append(half + rc(half))
        genome = genome[:5000] + palindromes[0] + genome[5000 + z:12345] + palindromes[0] + genome[12345 + z:]
    seeds = list(palindromes)
    starts = rng.sample(range(0, 20000 - z), 100)
    for n, start in enumerate(starts):
        window = genome[start:start + z]
        seeds.append(rc(window) if n % 2 else window)
    seeds += [random_dna(rng, z) for _ in range(100)]
    for at in (0, z - 1, 31, 32, 33, 63, 64, 65):
        if at < z:
            for start in starts[:4]:
                window = mutate(genome[start:start + z], at)
                seeds.append(rc(window) if at % 2 else window)
    return [('chr', genome)], seeds, palindromes, [minseq(genome[start:start + z]) for start in starts]


def chunk_edge_case(z, chunk_sizes, seed=0):
    """A 64 kb genome and seeds cut from it: one at every residue of the position modulo 2 x LANE_RUN, and one at every offset
    within +-z of one interior chunk edge of every chunk size (chunks advance by size - (z - 1))."""
    rng = random.Random(77 + z + seed)
    genome = random_dna(rng, 65536)
    positions = {1000 + r * (2 * LANE_RUN + 1) for r in range(2 * LANE_RUN)}
    for size in chunk_sizes:
        step = size - (z - 1)
        edge = step * max(1, (30000 // step))
        for off in range(-z, z + 1):
            for at in (edge + off, edge + size + off):           # where the chunk starts and where it ends
                if 0 <= at <= len(genome) - z:
                    positions.add(at)
    return [('chr', genome)], [genome[at:at + z] for at in sorted(positions)], sorted(positions)


def partition_case(seed=0):
    """Three sequences (1 Mb in all) and 30 partitions of one to three contigs cut from them, each with a changed base in the
    middle; some contigs sit on the reverse strand, two partitions share a region (and so their seeds), one partition has a
    second contig far from its first, one region is duplicated on another sequence."""
    rng = random.Random(4242 + seed)
    records = [('chrA', random_dna(rng, 500000)), ('chrB desc text', random_dna(rng, 300000)), ('scaffold_7', random_dna(rng, 200000))]
    # a duplicated region: chrA[100000:100400] also on scaffold_7
    a = records[0][1]
    s7 = records[2][1]
    records[2] = ('scaffold_7', s7[:50000] + a[100000:100400] + s7[50400:])
    names = [seqid.split()[0] for seqid, seq in records]
    partitions = []
    for pid in range(1, 31):
        part = []
        for c in range(1 + pid % 3):
            which = rng.randrange(3)
            seq = records[which][1]
            length = rng.randrange(150, 400)
            if pid == 5 and c == 0:
                which, start = 0, 100050                         # inside the duplicated region
            elif pid == 6 and c == 0:
                which, start = 0, 100100                         # shares seeds with partition 5
            else:
                start = rng.randrange(0, len(records[which][1]) - length)
            seq = records[which][1]
            contig = mutate(seq[start:start + length], length // 2)
            if rng.random() < 0.5:
                contig = rc(contig)
            part.append(('contig{}_{} kvcc={}'.format(pid, c, pid), contig))
        if pid == 9:                                             # a second locus 3 kb further on the same sequence
            seq = records[0][1]
            part.append(('contig9_far kvcc=9', seq[403000:403250]))
            part.append(('contig9_near kvcc=9', seq[400000:400250]))
        partitions.append((str(pid), part))
    return [(name, seq) for name, (seqid, seq) in zip(names, records)], records, partitions
