"""Plain-Python restatement of the cleaning rule of `kevlar assemble --clean` (rules 3a to 3c), literal and
slow, on top of tests/assemble_common.py: strings, dictionaries and sets.  The GPU tests hold kv_assemble.hip to it, and
tests/test_asmclean_reference.py holds it to assemble_common.unitigs at limits 0, 0, to hand-built cases with the answer written
out, and to what tests/golden/assemble/recorded.json states about pico-var/cc2.

Let G0 be the solid keys of a partition.  Round t = 0, 1, ... (at most clean_rounds) works on the live keys Gt:
 every oriented unitig U = w1 ... wm of Gt (rules 3 and 4) has m nodes, S = the sum of its nodes' counts, P = pred(w1),
 Q = succ(wm) and id(U) = the smaller canonical key of w1 and wm;
 3a tip: m <= tip_nodes, Q empty, P = {j}, and some s in succ(j) other than w1 has c(s) > c(w1), or c(s) = c(w1) and a smaller key;
 3b arm: m <= bubble_nodes, P = {a}, Q = {b}, and another unitig V (other keys) starts in succ(a) with m_V <= bubble_nodes,
    P_V = {a}, Q_V = {b} and beats U: S_V * m > S * m_V; on equality m_V > m; on equality again id(V) < id(U);
 3c all removals of a round are decided on Gt; G(t+1) = Gt minus the keys of the removed unitigs; a round that removes nothing
    ends the cleaning.
Rules 4 to 6 then run on the last live set."""
import random

import assemble_common as ac
from assemble_common import canonical, key_counts, rc

CLEAN_NAMES = ('tips', 'tip_keys', 'arms', 'arm_keys', 'rounds')
EVENT_NAMES = ('mean_tie', 'three_arms', 'hairpin_self')


def _graph(live):
    def succ(w):
        return [w[1:] + b for b in 'ACGT' if canonical(w[1:] + b) in live]

    def pred(w):
        return [b + w[:-1] for b in 'ACGT' if canonical(b + w[:-1]) in live]
    return succ, pred


def oriented_unitigs(live):
    """{first node: [nodes]} of every oriented unitig of the graph of the live keys: a unitig and its reverse complement are two
    entries (one when they are equal)"""
    succ, pred = _graph(live)
    out = {}
    for key in live:
        for w in (key, rc(key)):
            before = pred(w)
            if len(before) == 1 and len(succ(before[0])) == 1:
                continue                            # the edge coming in is simple: not a head
            nodes, node = [w], w
            while True:
                after = succ(node)
                if len(after) != 1 or len(pred(after[0])) != 1:
                    break
                node = after[0]
                nodes.append(node)
                assert len(nodes) <= 2 * len(live) + 2, 'a walk from a head cannot loop'
            out[w] = nodes
    return out


def beats(v, u):
    """V beats U: records are (S, m, id)"""
    if v[0] * u[1] != u[0] * v[1]:
        return v[0] * u[1] > u[0] * v[1]
    if v[1] != u[1]:
        return v[1] > u[1]
    return v[2] < u[2]


def clean_round(live, counts, tip_nodes, bubble_nodes, events=None):
    """(keys of the unitigs removed as tips, as arms: two lists of frozensets, one per unitig) of one round on `live`"""
    succ, pred = _graph(live)
    units = oriented_unitigs(live)
    record = {}
    for first, nodes in units.items():
        record[first] = (sum(counts[canonical(w)] for w in nodes), len(nodes), min(canonical(nodes[0]), canonical(nodes[-1])))
    tips, arms = {}, {}
    for first, nodes in units.items():
        S, m, ident = record[first]
        P, Q = pred(first), succ(nodes[-1])
        keys = frozenset(canonical(w) for w in nodes)
        if m <= tip_nodes and not Q and len(P) == 1:
            mine = (counts[canonical(first)], canonical(first))
            for s in succ(P[0]):
                if s != first and (counts[canonical(s)] > mine[0] or (counts[canonical(s)] == mine[0] and canonical(s) < mine[1])):
                    tips[ident] = keys
        if m <= bubble_nodes and len(P) == 1 and len(Q) == 1:
            rivals, own = [], False
            for s in succ(P[0]):
                other = units.get(s)
                if other is None:
                    continue                        # (cannot be: the edge from a node with two successors is not simple)
                if len(other) > bubble_nodes or pred(s) != P or succ(other[-1]) != Q:
                    continue
                if frozenset(canonical(w) for w in other) == keys:
                    own = own or s != first         # U's own reverse complement runs between the same two nodes
                    continue
                rivals.append(record[s])
            lost = [v for v in rivals if beats(v, record[first])]
            if lost:
                arms[ident] = keys
            if events is not None:
                if any(v[0] * m == S * v[1] for v in rivals):
                    events['mean_tie'] += 1
                if len(rivals) >= 2:
                    events['three_arms'] += 1
                if not lost and (own or (first == rc(nodes[-1]) and Q[0] == rc(P[0]))):
                    events['hairpin_self'] += 1
    assert not set(tips) & set(arms)                # a tip needs Q empty, an arm |Q| = 1
    return list(tips.values()), list(arms.values())


def clean_unitigs(reads, K=31, min_count=2, tip_nodes=0, bubble_nodes=0, clean_rounds=8, events=None):
    """(sorted unitigs of one partition after cleaning, each once as the smaller strand; the six stats by ac.STAT_NAMES over the
    final graph, `solid` before cleaning; the five clean stats by CLEAN_NAMES).  `events`, if given, is a dictionary by EVENT_NAMES
    that is counted up: arms that met a rival of equal mean, arms with two rivals or more, hairpin arms left alone."""
    assert K % 2 == 1 and 13 <= K <= 63 and min_count >= 1 and tip_nodes >= 0 and bubble_nodes >= 0 and clean_rounds >= 1
    counts, windows = key_counts(reads, K)
    solid = set(key for key, c in counts.items() if c >= min_count)
    live = set(solid)
    clean = dict.fromkeys(CLEAN_NAMES, 0)
    if events is not None:
        for name in EVENT_NAMES:
            events.setdefault(name, 0)
    if tip_nodes or bubble_nodes:
        for _ in range(clean_rounds):
            tips, arms = clean_round(live, counts, tip_nodes, bubble_nodes, events)
            if not tips and not arms:
                break
            clean['tips'] += len(tips)
            clean['tip_keys'] += sum(len(keys) for keys in tips)
            clean['arms'] += len(arms)
            clean['arm_keys'] += sum(len(keys) for keys in arms)
            clean['rounds'] += 1
            for keys in tips + arms:
                live -= keys
    units = oriented_unitigs(live)
    found, on_unitig = set(), set()
    for first, nodes in units.items():
        seq = first + ''.join(w[-1] for w in nodes[1:])
        found.add(min(seq, rc(seq)))
        on_unitig.update(canonical(w) for w in nodes)
    stats = dict(windows=windows, distinct=len(counts), solid=len(solid), heads=len(units), unitigs=len(found),
                 cycle_keys=len(live) - len(on_unitig))
    return sorted(found), stats, clean


def clean_limits(K):
    """what --clean selects"""
    return K, 2 * K


def add_clean(many, launch_ends=None):
    """the clean stats of a call: sums, but `rounds` is summed over launches and a launch runs as many removing rounds as the
    partition of it that needs the most (a partition that removes nothing in a round never removes again)"""
    many = list(many)
    total = {name: sum(c[name] for c in many) for name in CLEAN_NAMES[:4]}
    ends = [len(many)] if launch_ends is None else list(launch_ends)
    total['rounds'] = sum(max([c['rounds'] for c in many[a:b]] + [0]) for a, b in zip([0] + ends, ends))
    return total


# ---- planted inputs ------------------------------------------------------------------------------------------------------------------
PLANTED = ('snp', 'two_on_one', 'two_on_two', 'indel', 'tie_id', 'tie_length', 'three', 'tip', 'tip_on_arm', 'hairpin', 'at_limits',
           'fork_tips')
PLANTED_SEEDS = range(600)


def other_base(rng, b):
    return rng.choice([c for c in 'ACGT' if c != b])


def substituted(rng, seq, at):
    return seq[:at] + other_base(rng, seq[at]) + seq[at + 1:]


def insertion(rng, hap, at, length):
    """`length` random bases to put in front of hap[at]: the first is not hap[at] and the last not hap[at - 1], so every K-mer over
    an inserted base is new -- length + K - 1 nodes between the flanks, `length` nodes where the sequence ends with them"""
    while True:
        ins = ac.random_dna(rng, length)
        if ins[0] != hap[at] and ins[-1] != hap[at - 1]:
            return ins


def pieces(rng, seq, K):
    """seq cut into reads that overlap by K - 1 bases: every window of seq is a window of exactly one read"""
    out, at = [], 0
    while len(seq) - at >= 2 * K + 2 and rng.random() < 0.7:
        cut = rng.randrange(at + K, len(seq) - K)
        out.append(seq[at:cut + K - 1])
        at = cut
    out.append(seq[at:])
    return out


def planted_partition(seed, K=31):
    """(kind, reads): haplotypes over one random sequence of 4K to 6K bases, each seen a stated number of times (so every K-mer's
    count is known), cut into reads that share no window, shuffled, about half reverse-complemented.  Sizes follow K: arms of a
    substitution have K nodes whatever K is."""
    rng = random.Random(1000003 * K + seed)
    kind = PLANTED[seed % len(PLANTED)]
    n = rng.randrange(4 * K, 6 * K + 1)
    hap = ac.random_dna(rng, n)
    at = rng.randrange(K + 2, n - 2 * K - 4)        # the planted site: K + 2 bases in front, 2K + 4 behind at least
    cover = rng.randrange(3, 7)
    lower = rng.randrange(2, cover)                 # 2 .. cover - 1: solid at min_count 1 and 2
    haps = [(hap, cover)]                           # (sequence, times seen)
    if kind == 'snp':                               # a second haplotype with one substitution: arms of K nodes
        haps.append((substituted(rng, hap, at), lower))
    elif kind == 'two_on_one':                      # two substitutions closer than K on one haplotype: one arm of K + d nodes
        d = rng.randrange(1, K)
        haps.append((substituted(rng, substituted(rng, hap, at), at + d), lower))
    elif kind == 'two_on_two':                      # ... and on two haplotypes: the arms share nodes with neither or both
        d = rng.randrange(1, K)
        haps.append((substituted(rng, hap, at), lower))
        haps.append((substituted(rng, hap, at + d), rng.randrange(2, cover + 1)))
    elif kind == 'indel':                           # arms of unequal m: K - 1 nodes against K - 1 + length
        length = rng.randrange(1, K + 3)
        if rng.random() < 0.5:
            haps.append((hap[:at] + insertion(rng, hap, at, length) + hap[at:], rng.randrange(2, cover + 2)))
        else:
            haps.append((hap[:at] + hap[at + min(length, K):], rng.randrange(2, cover + 2)))
    elif kind == 'tie_id':                          # equal mean, equal m: the smaller id stays
        haps.append((substituted(rng, hap, at), cover))
    elif kind == 'tie_length':                      # equal mean, unequal m: the longer arm stays
        haps.append((hap[:at] + insertion(rng, hap, at, rng.randrange(1, K // 2)) + hap[at:], cover))
    elif kind == 'three':                           # three haplotypes between one pair of anchors
        first = substituted(rng, hap, at)
        third = rng.choice([c for c in 'ACGT' if c not in (hap[at], first[at])])
        haps.append((first, rng.randrange(2, cover + 1)))
        haps.append((hap[:at] + third + hap[at + 1:], rng.randrange(2, cover + 1)))
    elif kind == 'tip':                             # a read-end error seen twice: r bases behind it, r + 1 nodes
        r = rng.randrange(0, K - 1)
        haps.append((substituted(rng, hap, at)[:at + r + 1], 2))
    elif kind == 'tip_on_arm':                      # a tip hanging on an arm: the tip goes first, then the arm
        arm = substituted(rng, hap, at)
        haps.append((arm, lower + 1))
        r = rng.randrange(1, K // 2)
        haps.append((substituted(rng, arm, at + rng.randrange(2, K // 2))[:at + K // 2 + r], 2))
    elif kind == 'hairpin':                         # an arm from a to rc(a): its only partner is its own reverse complement
        x = hap[:at]
        if rng.random() < 0.5:
            half = ac.random_dna(rng, rng.randrange(1, (K + 1) // 2 + 1))
            middle = half + rc(half)                # the arm is its own reverse complement: one head
        else:
            middle = ac.random_dna(rng, rng.randrange(1, K + 2))    # it is not: two heads, one key set
        haps = [(x + middle + rc(x), cover), (hap, lower)]
    elif kind == 'at_limits':                       # arms of 2K and 2K + 1 nodes, tips of K and K + 1: at and one beyond --clean's limits
        which = rng.randrange(4)
        if which < 2:
            haps.append((hap[:at] + insertion(rng, hap, at, K + 1 + which) + hap[at:], lower))
        else:
            haps.append((hap[:at] + insertion(rng, hap, at, K + which - 2), 2))
    else:                                           # a fork with two tips, the stronger stays; or tips of equal count
        assert kind == 'fork_tips'
        stem = hap[:at]
        haps = [(stem + ac.random_dna(rng, rng.randrange(1, K)), cover), (stem + ac.random_dna(rng, rng.randrange(1, K)), rng.choice([lower, cover]))]
        if rng.random() < 0.5:
            haps.append((stem + ac.random_dna(rng, rng.randrange(K + 2, 2 * K)), rng.randrange(2, cover + 2)))
    reads = []
    for seq, times in haps:
        for _ in range(times):
            reads.extend(pieces(rng, seq, K))
    rng.shuffle(reads)
    reads = [rc(read) if rng.random() < 0.5 else read for read in reads]
    return kind, reads


_planted = {}
planted_events = {}                                 # (K, min_count, seed): what clean_unitigs counted at --clean's limits and 8 rounds


def planted_answers(K, min_count, seeds=PLANTED_SEEDS, tip_nodes=None, bubble_nodes=None, clean_rounds=8):
    """[(kind, reads, unitigs, stats, clean)] of the restatement over the seeds at --clean's limits (or the given ones), each
    computed once and shared; nobody changes them"""
    tip_nodes = K if tip_nodes is None else tip_nodes
    bubble_nodes = 2 * K if bubble_nodes is None else bubble_nodes
    rows = []
    for seed in seeds:
        at = (K, min_count, tip_nodes, bubble_nodes, clean_rounds, seed)
        if at not in _planted:
            kind, reads = planted_partition(seed, K)
            events = {}
            _planted[at] = (kind, reads) + clean_unitigs(reads, K, min_count, tip_nodes, bubble_nodes, clean_rounds, events)
            planted_events[at[:2] + at[5:]] = events if at[2:5] == (K, 2 * K, 8) else None
        rows.append(_planted[at])
    return rows


# ---- hand-built cases with the answer written out ------------------------------------------------------------------------------------
def smaller(seq):
    return min(seq, rc(seq))


def hand_cases(K=13):
    """{name: (reads, unitigs after cleaning or None for "what assemble_common.unitigs gives", (tips, tip keys, arms, arm keys,
    rounds))} at min_count 2 and --clean's limits K and 2K: small graphs over one random haplotype of 5K bases with the planted
    site 2K + 3 bases in, the answer stated from how each was built, not computed"""
    rng = random.Random(77 + K)
    hap = ac.random_dna(rng, 5 * K)
    at = 2 * K + 3
    snp = substituted(rng, hap, at)
    whole, nothing = [smaller(hap)], (0, 0, 0, 0, 0)
    cases = {}
    cases['snp'] = ([hap] * 4 + [snp] * 2, whole, (0, 0, 1, K, 1))                   # the arm of the lower mean goes: K nodes
    # equal mean, equal m: the arm whose id -- the smaller canonical key of its first and last node -- is smaller stays
    ids = {seq: min(canonical(seq[at - K + 1:at + 1]), canonical(seq[at:at + K])) for seq in (hap, snp)}
    cases['tie_id'] = ([hap] * 3 + [snp] * 3, [smaller(min(ids, key=ids.get))], (0, 0, 1, K, 1))
    ins = hap[:at] + insertion(rng, hap, at, 4) + hap[at:]
    cases['indel'] = ([hap] * 2 + [ins] * 5, [smaller(ins)], (0, 0, 1, K - 1, 1))      # the K - 1 nodes across the site go
    cases['tie_length'] = ([hap] * 3 + [ins] * 3, [smaller(ins)], (0, 0, 1, K - 1, 1))  # equal mean: the arm of more nodes stays
    third = hap[:at] + [c for c in 'ACGT' if c not in (hap[at], snp[at])][0] + hap[at + 1:]
    cases['three'] = ([hap] * 4 + [snp] * 3 + [third] * 2, whole, (0, 0, 2, 2 * K, 1))  # three arms lose two in one round
    two = substituted(rng, snp, at + 5)
    cases['two_on_one'] = ([hap] * 4 + [two] * 2, whole, (0, 0, 1, K + 5, 1))
    # two substitutions 5 apart on two haplotypes: the three paths share nodes in pairs, no unitig runs from fork to join
    cases['two_on_two'] = ([hap] * 4 + [snp] * 2 + [substituted(rng, hap, at + 5)] * 3, None, nothing)
    cases['tip'] = ([hap] * 3 + [snp[:at + 4]] * 2, whole, (1, 4, 0, 0, 1))            # 3 bases behind the error: 4 nodes
    # the tip splits the arm in two, so round 1 sees no arm and clips the tip; round 2 pops the arm
    cases['tip_on_arm'] = ([hap] * 5 + [snp] * 3 + [substituted(rng, snp, at + 4)[:at + 8]] * 2, whole, (1, 4, 1, K, 2))
    x, half = hap[:at], ac.random_dna(rng, 4)
    cases['hairpin'] = ([x + half + rc(half) + rc(x)] * 3 + [hap] * 2, None, nothing)  # an arm from a to rc(a): its own partner
    cases['arm_at_limit'] = ([hap] * 3 + [hap[:at] + insertion(rng, hap, at, K + 1) + hap[at:]] * 2, whole, (0, 0, 1, 2 * K, 1))
    # 2K + 1 nodes: not an arm, so no rival of the K - 1 nodes beside it either
    cases['arm_beyond_limit'] = ([hap] * 3 + [hap[:at] + insertion(rng, hap, at, K + 2) + hap[at:]] * 2, None, nothing)
    cases['tip_at_limit'] = ([hap] * 3 + [hap[:at] + insertion(rng, hap, at, K)] * 2, whole, (1, K, 0, 0, 1))
    cases['tip_beyond_limit'] = ([hap] * 3 + [hap[:at] + insertion(rng, hap, at, K + 1)] * 2, None, nothing)
    left = insertion(rng, hap, at, 6)
    right = other_base(rng, left[0]) + ac.random_dna(rng, 6)
    cases['fork_two_tips'] = ([x + left] * 4 + [x + right] * 2, [smaller(x + left)], (1, 7, 0, 0, 1))   # the stronger tip stays
    cases['edge_beside_arm'] = (direct_edge_case(rng, K), None, nothing)
    # a ring three times round and a read that leaves it with an error two bases before its end: 3 nodes; the ring has no head left
    ring = ac.random_dna(rng, K + 7)
    cases['ring_with_tip'] = ([ring * 3] * 2 + [ring[3:3 + K - 1] + other_base(rng, ring[3 + K - 1]) + ac.random_dna(rng, 2)] * 2,
                              [], (1, 3, 0, 0, 1))
    return cases


def direct_edge_case(rng, K):
    """reads in which a -> b is an edge and a path a -> u1 .. u5 -> b lies beside it.  b = a[1:] + c and the path's last node must
    end with a[1:] too, so the K - 1 bases T = a[1:] occur twice on the path and T + (the base behind the first T) = u1 follows u5
    as well: the path closes a ring, u5 has two successors and is no arm by 3b.  Made by a unit of 5 bases: a run of K - 1 bases
    of it in one haplotype, of K + 4 in the other."""
    while True:
        unit = ac.random_dna(rng, 5)
        if len(set(unit)) < 3:
            continue
        left, right = ac.random_dna(rng, 2 * K), ac.random_dna(rng, 2 * K)
        if left[-1] == unit[-1] or right[0] == unit[(K - 1) % 5]:
            continue
        short = (unit * K)[:K - 1]
        long_ = (unit * K)[:K - 1 + 5]
        return [left + short + right] * 3 + [left + long_ + right] * 2


# ---- the device against the restatement -----------------------------------------------------------------------------------------------
def agree_clean(partitions, K=31, min_count=2, tip_nodes=None, bubble_nodes=None, clean_rounds=8, mem_budget=0, launches=None, want=None,
                launch_ends=None):
    """the device's unitigs, seven stats and five clean stats equal the restatement's; returns (unitigs per partition, stats,
    clean stats).  `want`: the restatement's (unitigs, stats, clean) per partition where the caller has them already"""
    from kevlar_amd import assemble as asm
    tip_nodes = K if tip_nodes is None else tip_nodes
    bubble_nodes = 2 * K if bubble_nodes is None else bubble_nodes
    got, stats = asm.unitigs_batch(partitions, K, min_count, mem_budget, tip_nodes=tip_nodes, bubble_nodes=bubble_nodes,
                                   clean_rounds=clean_rounds)
    clean = {name: stats[name] for name in CLEAN_NAMES}
    if want is None:
        want = [clean_unitigs(reads, K, min_count, tip_nodes, bubble_nodes, clean_rounds) for reads in partitions]
    assert len(got) == len(partitions) == len(want)
    for p, (mine, theirs) in enumerate(zip(got, want)):
        assert len(set(mine)) == len(mine), 'partition {}: a unitig reported twice'.format(p)
        assert sorted(mine) == theirs[0], 'partition {}'.format(p)
    assert {name: stats[name] for name in ac.STAT_NAMES} == ac.add_stats([w[1] for w in want])
    if launches is not None:
        assert stats['launches'] == launches
    assert clean == add_clean([w[2] for w in want], launch_ends)
    return [w[0] for w in want], stats, clean


# ---- the cleaning-aware planner of kv_asm_plan.h, restated ---------------------------------------------------------------------------
CLEAN_BYTES_PER_WINDOW = 12                         # the inverse map (two head indices) and the liveness word


def clean_launch_bytes(n_windows, n_bases, n_reads, K, cleaning):
    return ac.launch_bytes(n_windows, n_bases, n_reads, K) + (CLEAN_BYTES_PER_WINDOW * n_windows if cleaning else 0)


def clean_plan(partition_read_lengths, K, budget, tip_nodes, bubble_nodes):
    """ac.plan with the bytes of a cleaning launch: one past the last partition of every launch, or None"""
    cleaning = bool(tip_nodes or bubble_nodes)
    ends, cur, open_ = [], (0, 0, 0), False
    for p, lengths in enumerate(partition_read_lengths):
        size = ac.partition_size(lengths, K)
        if clean_launch_bytes(size[0], size[1], size[2], K, cleaning) > budget or size[0] > ac.MAX_WINDOWS:
            return None
        joined = tuple(a + b for a, b in zip(cur, size))
        if open_ and (clean_launch_bytes(joined[0], joined[1], joined[2], K, cleaning) > budget or joined[0] > ac.MAX_WINDOWS):
            ends.append(p)
            joined = size
        cur, open_ = joined, True
    if open_:
        ends.append(len(partition_read_lengths))
    return ends
