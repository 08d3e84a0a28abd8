"""Plain-Python restatement of the assembly rule of `kevlar assemble`, literal and slow: strings,
dictionaries and sets, no packing, no table.  The GPU tests hold kv_assemble.hip to it and tests/test_assemble_reference.py holds
it to what the reference states about its own assembler and, through check_unitigs below (which takes an answer and checks rules 1
to 5 on it without a walk), to the rule itself on inputs made of repeats (structured_partition).

The rule, per partition, with K odd and min_count >= 1:
 1. windows: every window of K bases of every read, either letter case; one with a byte outside ACGT is skipped; its key is the
    smaller of the window and its reverse complement (plain string order: A < C < G < T);
 2. counts: c(x) = windows with key x, both strands together; x is solid when c(x) >= min_count;
 3. graph: an oriented node is a K-mer w whose key is solid; succ(w) = the solid w[1:] + b, pred(w) = the solid b + w[:-1]; the
    edge w -> v is simple when |succ(w)| = 1 and |pred(v)| = 1;
 4. unitigs: maximal chains of simple edges w1 -> ... -> wm (m = 1 allowed), S = w1 + the last base of each later node; a
    component of simple edges alone is a cycle, has no head and yields nothing;
 5. every unitig appears as S and as rc(S) and is reported once, as the smaller string;
 6. contigs: the unitigs strictly longer than the partition's longest read (N included), longest first, then by sequence.
"""
import gzip
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'assemble')
COMPLEMENT = str.maketrans('ACGT', 'TGCA')
STAT_NAMES = ('windows', 'distinct', 'solid', 'heads', 'unitigs', 'cycle_keys')


def rc(seq):
    return seq.translate(COMPLEMENT)[::-1]


def canonical(kmer):
    other = rc(kmer)
    return kmer if kmer < other else other


def key_counts(reads, K):
    """({key: windows}, valid windows) of one partition"""
    counts, windows = {}, 0
    for read in reads:
        text = read.upper()
        for i in range(len(text) - K + 1):
            window = text[i:i + K]
            if window.strip('ACGT'):
                continue
            windows += 1
            key = canonical(window)
            counts[key] = counts.get(key, 0) + 1
    return counts, windows


def unitigs(reads, K=31, min_count=2):
    """(sorted list of the unitigs of one partition, each once as the smaller strand; stats by STAT_NAMES)"""
    assert K % 2 == 1 and 13 <= K <= 63 and min_count >= 1
    counts, windows = key_counts(reads, K)
    solid = set(key for key, c in counts.items() if c >= min_count)

    def succ(w):
        return [w[1:] + b for b in 'ACGT' if canonical(w[1:] + b) in solid]

    def pred(w):
        return [b + w[:-1] for b in 'ACGT' if canonical(b + w[:-1]) in solid]

    def simple_in(w):
        """the node in front of w if the edge from it is simple"""
        before = pred(w)
        if len(before) == 1 and len(succ(before[0])) == 1:
            return before[0]
        return None

    found, heads, on_unitig = set(), 0, set()
    for key in solid:
        for w in (key, rc(key)):
            if simple_in(w) is not None:
                continue
            heads += 1
            seq, node, steps, nodes = w, w, 0, [w]
            while True:
                after = succ(node)
                if len(after) != 1 or len(pred(after[0])) != 1:
                    break
                node = after[0]
                steps += 1
                assert steps <= 2 * len(solid), 'a walk from a head cannot loop'
                seq += node[-1]
                nodes.append(node)
            found.add(min(seq, rc(seq)))
            on_unitig.update(canonical(n) for n in nodes)
    stats = dict(windows=windows, distinct=len(counts), solid=len(solid), heads=heads, unitigs=len(found),
                 cycle_keys=len(solid) - len(on_unitig))
    return sorted(found), stats


def contigs_of(unitig_list, reads):
    """rule 6: strictly longer than the longest read, longest first, then by sequence"""
    longest = max([len(r) for r in reads] + [0])
    return sorted((u for u in unitig_list if len(u) > longest), key=lambda u: (-len(u), u))


def contigs(reads, K=31, min_count=2):
    return contigs_of(unitigs(reads, K, min_count)[0], reads)


def add_stats(many):
    return {name: sum(s[name] for s in many) for name in STAT_NAMES}


def longest_common_substring(a, b):
    """length of the longest common substring, by rows of the classic table"""
    best, row = 0, [0] * (len(b) + 1)
    for ca in a:
        new = [0] * (len(b) + 1)
        for j, cb in enumerate(b, 1):
            if ca == cb:
                new[j] = row[j - 1] + 1
                if new[j] > best:
                    best = new[j]
        row = new
    return best


def common_either_strand(a, b):
    return max(longest_common_substring(a, b), longest_common_substring(a, rc(b)))


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
def _open(path):
    return gzip.open(path, 'rt') if path.endswith('.gz') else open(path, 'r')


def recorded():
    """what tests/golden/make_golden_assemble.py recorded of the reference's own tests"""
    import json
    with open(os.path.join(GOLDEN, 'recorded.json')) as fh:
        return json.load(fh)


def fixture_path(name):
    """where a data file of the reference's assemble / alac tests is kept under tests/golden"""
    return os.path.join(ROOT, 'tests', 'golden', recorded()['files'][name])


def read_partitions(name):
    """[(partition id or None, [sequences])] of an augmented FASTQ / FASTA fixture, partitions in file order (kvcc=N in the name)"""
    parts, index = [], {}
    with _open(fixture_path(name)) as fh:
        lines = [ln.rstrip('\n') for ln in fh]
    i = 0
    while i < len(lines):
        line = lines[i]
        if line.startswith('@') and i + 3 < len(lines) and lines[i + 2].startswith('+'):
            name_line, seq = line[1:], lines[i + 1]
            i += 4
        elif line.startswith('>'):
            name_line, seq = line[1:], lines[i + 1]
            i += 2
        else:
            i += 1                      # an annotation line (k-mer of interest) or a blank
            continue
        partid = None
        for field in name_line.split():
            if field.startswith('kvcc='):
                partid = field[5:]
        if partid not in index:
            index[partid] = len(parts)
            parts.append((partid, []))
        parts[index[partid]][1].append(seq)
    return parts


def all_reads(name):
    return [seq for partid, reads in read_partitions(name) for seq in reads]


# ---- seeded inputs for the device tests ----------------------------------------------------------------------------------------
def random_dna(rng, n):
    return ''.join(rng.choice('ACGT') for _ in range(n))


def tiled_reads(seq, length, step, copies=1):
    """reads of `length` bases every `step` bases over seq, the last one flush with its end, each `copies` times"""
    starts = list(range(0, max(len(seq) - length, 0) + 1, step))
    if starts[-1] != max(len(seq) - length, 0):
        starts.append(max(len(seq) - length, 0))
    return [seq[s:s + length] for s in starts for _ in range(copies)]


def seeded_partition(seed, n_reads=30, read_len=150, hap_len=400, error=0.01):
    """reads tiled at random over a random haplotype with substitutions, on either strand"""
    rng = random.Random(seed)
    hap = random_dna(rng, hap_len)
    reads = []
    for _ in range(n_reads):
        s = rng.randrange(0, hap_len - read_len + 1)
        read = list(hap[s:s + read_len])
        for j in range(read_len):
            if rng.random() < error:
                read[j] = rng.choice([b for b in 'ACGT' if b != read[j]])
        read = ''.join(read)
        reads.append(rc(read) if rng.random() < 0.5 else read)
    return reads


# ---- structured inputs: repeats, hairpins, rings ---------------------------------------------------------------------------------
# Random DNA has no repeated K-mer at K >= 13; these haplotypes are made of them.
KINDS = ('alpha2', 'alpha2rc', 'tandem', 'repeat', 'hairpin', 'ringtail')
TANDEM_UNITS = (1, 2, 3, 5, 7, 11, 14, 17)
FUZZ_SEEDS = range(600)


def letters(rng, alphabet, n):
    return ''.join(rng.choice(alphabet) for _ in range(n))


def structured_haplotype(rng, kind):
    """60 to 260 bases of the kind"""
    if kind == 'alpha2':                            # two letters: 2^13 possible 13-mers, forks and repeats everywhere
        hap = letters(rng, 'AC', rng.randrange(60, 261))
    elif kind == 'alpha2rc':                        # ... and every K-mer's reverse complement is of the same alphabet
        hap = letters(rng, 'AT', rng.randrange(60, 261))
    elif kind == 'tandem':                          # units shorter and longer than K = 13
        unit = random_dna(rng, rng.choice(TANDEM_UNITS))
        span = rng.randrange(20, 221)
        hap = random_dna(rng, 20) + (unit * (span // len(unit) + 1))[:span] + random_dna(rng, 20)
    elif kind == 'repeat':                          # one element several times, each copy on a random strand
        element = random_dna(rng, rng.randrange(13, 40))
        hap = random_dna(rng, rng.randrange(5, 40))
        for _ in range(rng.randrange(2, 6)):
            hap += (rc(element) if rng.random() < 0.5 else element) + random_dna(rng, rng.randrange(5, 40))
    elif kind == 'hairpin':                         # the node in the middle of the stem has its own reverse complement behind it
        stem = random_dna(rng, rng.randrange(10, 40))
        hap = random_dna(rng, rng.randrange(20, 90)) + stem + random_dna(rng, rng.randrange(0, 4)) + rc(stem) + random_dna(rng, rng.randrange(20, 90))
    else:                                           # a cycle with a way in and a way out
        assert kind == 'ringtail'
        hap = random_dna(rng, 25) + 3 * random_dna(rng, rng.randrange(13, 60)) + random_dna(rng, 25)
    hap = hap[:260]
    assert 60 <= len(hap) <= 260
    return hap


def structured_partition(seed):
    """(kind, reads): 4 to 29 reads of one length of 20 to 69 bases at random starts over a structured haplotype, about a third of
    them with one byte replaced by a letter of ACGTN, about half of the N-free ones reverse-complemented"""
    rng = random.Random(seed)
    kind = KINDS[seed % len(KINDS)]
    hap = structured_haplotype(rng, kind)
    length = rng.randrange(20, 70)
    reads = []
    for _ in range(rng.randrange(4, 30)):
        s = rng.randrange(0, len(hap) - length + 1)
        read = hap[s:s + length]
        if rng.random() < 1 / 3:
            at = rng.randrange(length)
            read = read[:at] + rng.choice('ACGTN') + read[at + 1:]
        if 'N' not in read and rng.random() < 0.5:
            read = rc(read)
        reads.append(read)
    return kind, reads


_structured = {}


def structured_answers(K, min_count, seeds=FUZZ_SEEDS):
    """[(kind, reads, unitigs, stats)] of the restatement over the seeds, each computed once and shared; nobody changes them"""
    rows = []
    for seed in seeds:
        if (K, min_count, seed) not in _structured:
            kind, reads = structured_partition(seed)
            _structured[K, min_count, seed] = (kind, reads) + unitigs(reads, K, min_count)
        rows.append(_structured[K, min_count, seed])
    return rows


# ---- an answer against rules 1 to 5, without a walk -------------------------------------------------------------------------------
def check_unitigs(reads, K, min_count, found, stats):
    """Asserts that `found` (a list of strings) and `stats` are the unitigs of the partition by rules 1 to 5 above.  Independent of
    unitigs(): it starts from the answer, not from heads, follows no chain and uses key_counts, canonical, rc and set membership
    only.  Every chain of the answer must be a chain of simple edges that cannot be extended, every solid key must lie on exactly
    one of them, and a solid key on none must have a simple edge coming in on both strands (so it is not on a chain with a head: the
    head of that chain would be a solid key on no unitig WITHOUT such an edge)."""
    counts, windows = key_counts(reads, K)
    solid = set(key for key, c in counts.items() if c >= min_count)

    def succ(w):
        return [w[1:] + b for b in 'ACGT' if canonical(w[1:] + b) in solid]

    def pred(w):
        return [b + w[:-1] for b in 'ACGT' if canonical(b + w[:-1]) in solid]

    def simple(w, v):
        return succ(w) == [v] and pred(v) == [w]

    def simple_edge_in(w):
        return len(pred(w)) == 1 and simple(pred(w)[0], w)

    def simple_edge_out(w):
        return len(succ(w)) == 1 and simple(w, succ(w)[0])

    where = {}                                      # key: the unitigs it lies on, once per node
    for i, u in enumerate(found):
        assert len(u) >= K and not u.strip('ACGT'), (i, u)
        assert u <= rc(u), 'unitig {} is the larger strand'.format(i)
        nodes = [u[j:j + K] for j in range(len(u) - K + 1)]
        for w in nodes:
            assert canonical(w) in solid, 'unitig {}: {} is not solid'.format(i, w)
            where.setdefault(canonical(w), []).append(i)
        for w, v in zip(nodes, nodes[1:]):
            assert simple(w, v), 'unitig {}: {} -> {} is not a simple edge'.format(i, w, v)
        assert not simple_edge_in(nodes[0]), 'unitig {} goes on in front'.format(i)
        assert not simple_edge_out(nodes[-1]), 'unitig {} goes on behind'.format(i)
    for key, on in where.items():
        assert len(set(on)) == 1, '{} lies on unitigs {}'.format(key, sorted(set(on)))
        assert len(on) == 1 or (len(on) == 2 and found[on[0]] == rc(found[on[0]])), '{} lies {} times on unitig {}'.format(key, len(on), on[0])
    off = solid - set(where)
    for key in off:
        assert simple_edge_in(key) and simple_edge_in(rc(key)), '{} is on no unitig and not on a cycle'.format(key)
    heads = sum(1 for key in solid for w in (key, rc(key)) if not simple_edge_in(w))
    assert stats['cycle_keys'] == len(off)
    assert stats['unitigs'] == len(found)
    assert stats['solid'] == len(solid)
    assert stats['distinct'] == len(counts)
    assert stats['windows'] == windows
    assert stats['heads'] == heads                  # (a unitig has two, or one when it is its own reverse complement)
    assert heads == sum(1 if u == rc(u) else 2 for u in found)


# ---- the device against the restatement ---------------------------------------------------------------------------------------------
def agree(partitions, K=31, min_count=2, mem_budget=0, launches=None, want=None):
    """the device's unitigs and stats equal the restatement's; returns (unitigs per partition, stats).  `want`: the restatement's
    (unitigs, stats) per partition where the caller has them already"""
    from kevlar_amd import assemble as asm
    got, stats = asm.unitigs_batch(partitions, K, min_count, mem_budget)
    if want is None:
        want = [unitigs(reads, K, min_count) for reads in partitions]
    assert len(got) == len(partitions) == len(want)
    for p, (mine, (theirs, _)) in enumerate(zip(got, want)):
        assert len(set(mine)) == len(mine), 'partition {}: a unitig reported twice'.format(p)
        assert sorted(mine) == theirs, 'partition {}'.format(p)
    assert {name: stats[name] for name in STAT_NAMES} == add_stats([s for _, s in want])
    if launches is not None:
        assert stats['launches'] == launches
    return [u for u, _ in want], stats


def device_plan(parts, K, budget):
    """(return code, one past the last partition of every launch) of kv_assemble_plan"""
    import ctypes
    import numpy as np
    from kevlar_amd import _lib
    lib = _lib.load()
    lengths = [len(r) for reads in parts for r in reads]
    read_off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    read_off[1:] = np.cumsum(np.array(lengths, dtype=np.uint64))
    part_first = np.zeros(len(parts) + 1, dtype=np.uint64)
    part_first[1:] = np.cumsum(np.array([len(reads) for reads in parts], dtype=np.uint64))
    ends = np.zeros(max(len(parts), 1), dtype=np.uint64)
    n = ctypes.c_uint64(0)
    rc_ = lib.kv_assemble_plan(read_off.ctypes.data, len(lengths), part_first.ctypes.data, len(parts), K, budget, ends.ctypes.data, ctypes.byref(n))
    return rc_, ends[:n.value].tolist()


# ---- the planner of kv_asm_plan.h, restated -------------------------------------------------------------------------------------
RUN = 32
THREADS = 256
MAX_WINDOWS = 0x3FFFFFF0


def table_cap(n_windows):
    cap = 1024
    while cap < 2 * n_windows + 16:
        cap *= 2
    return cap


def launch_bytes(n_windows, n_bases, n_reads, K):
    words = 1 if K <= 31 else 2
    chunks = (n_windows + THREADS - 1) // THREADS
    return n_windows * (8 * words + 16) + (chunks + 1) * 12 + 8 * table_cap(n_windows) + n_bases + 32 * (n_reads + 1)


def partition_size(read_lengths, K):
    """(windows, bases, reads) of one partition"""
    return sum(max(n - K + 1, 0) for n in read_lengths), sum(read_lengths), len(read_lengths)


def plan(partition_read_lengths, K, budget):
    """one past the last partition of every launch, or None when one partition alone passes the budget: a launch takes
    partitions in order until the next one would pass it"""
    ends, cur, open_ = [], (0, 0, 0), False
    for p, lengths in enumerate(partition_read_lengths):
        size = partition_size(lengths, K)
        if launch_bytes(size[0], size[1], size[2], K) > budget or size[0] > MAX_WINDOWS:
            return None
        joined = tuple(a + b for a, b in zip(cur, size))
        if open_ and (launch_bytes(joined[0], joined[1], joined[2], K) > budget or joined[0] > MAX_WINDOWS):
            ends.append(p)
            joined = size
        cur, open_ = joined, True
    if open_:
        ends.append(len(partition_read_lengths))
    return ends
