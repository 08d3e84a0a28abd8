"""The restatements of tests/downstream_common.py against the reference's RECORDED outputs (tests/golden/expected), which is what
entitles them to judge the product in tests/test_gpu_downstream.py, and the generated inputs of that file against the conditions
that make them worth running: every irregularity a case claims is really there, judged by the restatement alone.  Needs the
oracle library (the restated filter counts into an oracle Counttable) but no GPU."""
import json

import pytest

from conftest import data_file, expected_file
import downstream_common as dc


def load(path):
    import kevlar_amd
    with kevlar_amd.open(path, 'r') as fh:
        return [rec for rec in kevlar_amd.parse_augmented_fastx(fh) if rec is not None]


# ---- the restatements reproduce the reference's recorded results ------------------------------------------------------------
@pytest.mark.parametrize('name,infile,kw', [
    ('filter-trio1-nomask.augfastq', 'trio1/novel_3_1,2.txt', dict(memory=1e7)),
    ('filter-alpha.augfastq', 'collect.alpha.txt', dict(memory=500)),
    ('filter-worm.augfasta', 'worm.augfasta', dict(memory=1000, casemin=5, ctrlmax=0)),
])
def test_restated_filter_reproduces_the_recorded_outputs(ok, name, infile, kw):
    got = dc.restate_filter(ok, load(data_file(infile)), **kw)
    assert got.text == open(expected_file(name)).read()
    assert got.validated == len(got.records) > 0


def test_restated_filter_with_the_recorded_mask(ok):
    """kevlar/tests/test_filter.py:27-57: the genome mask leaves 18 of 178 reads"""
    mask = ok.Nodetable.load(data_file('bogus-genome/mask.nt'))
    got = dc.restate_filter(ok, load(data_file('trio1/novel_3_1,2.txt')), memory=1e7, mask=mask, casemin=6)
    assert got.text == open(expected_file('filter-trio1-masked.augfastq')).read()
    assert (got.processed, got.validated) == (178, 18)


@pytest.mark.parametrize('name,infile,kw', [
    ('partition-dup', 'dup.augfastq', dict(minabund=2, maxabund=200)),
    ('partition-dup-nodedup', 'dup.augfastq', dict(minabund=2, maxabund=200, dedup=False)),
    ('partition-pico-minabund5', 'pico-filtered.fq.gz', dict(minabund=5, maxabund=200)),
    ('partition-pico-default', 'pico-filtered.fq.gz', dict(minabund=2, maxabund=200)),
    ('partition-conn1311', 'connectivity-1311.augfastq', dict(minabund=2, maxabund=200)),
    ('partition-conn1541-nodedup', 'connectivity-1541.augfastq', dict(minabund=2, maxabund=200, dedup=False)),
])
def test_restated_partition_reproduces_the_recorded_outputs(name, infile, kw):
    """the relation of test_partition_golden: same numbering; per partition the same canonical sequences and
    the same number of reads, and without dedup the same names"""
    import kevlar_amd
    records = load(data_file(infile))
    got = dc.restate_partition(records, **kw)
    want = json.load(open(expected_file(name + '.json')))
    seq_of = {rec.name: kevlar_amd.revcommin(rec.sequence) for rec in records}
    assert [str(n) for n in range(1, len(got.partitions) + 1)] == sorted(want['partitions'], key=int)
    for n, members in enumerate(got.partitions, 1):
        recorded = want['partitions'][str(n)]
        assert sorted({seq_of[m] for m in members}) == sorted({s for _, s in recorded})
        assert len(members) == len(recorded)
        if not kw.get('dedup', True):
            assert sorted([m, seq_of[m]] for m in members) == sorted(recorded)
    assert 'grouped {:d} reads into {:d} connected components'.format(got.nreads, len(got.partitions)) in want['log'][0]


# ---- the generated cases are not vacuous ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def streams():
    return {case.name: dc.generate(case) for case in dc.PARTITION_CASES}


def test_generated_text_is_the_records(streams):
    """what the file path parses is what the record path is handed: the text read back by the record parser gives the specs"""
    import io
    import kevlar_amd
    for stream in streams.values():
        back = [rec for rec in kevlar_amd.parse_augmented_fastx(io.StringIO(stream.text)) if rec is not None]
        want = stream.records()
        assert [(r.name, r.sequence, r.quality, list(r.annotations), r.mates) for r in back] == \
               [(r.name, r.sequence, r.quality, list(r.annotations), r.mates) for r in want]
        lengths = [len(r.sequence) for r in want]
        assert min(lengths) == stream.case.k and max(lengths) > 3000
        assert dc.generate(stream.case).text == stream.text, 'the generator is a function of its seed'
        if 'blank' in stream.case.flags:
            assert '\n\n' in stream.text
        if 'fasta' in stream.case.flags:
            assert any(r.quality is None for r in want) and any(r.quality is not None for r in want)
        if 'mates' in stream.case.flags:
            assert '#mateseq=' in stream.text
        values = [a for r in want for note in r.annotations for a in note.abund]
        assert min(values) == 0 and max(values) > 255
        assert all(len(note.abund) == stream.case.nsamples for r in want for note in r.annotations)


def test_case_table_spans_what_the_issue_names():
    ks = {case.k for case in dc.PARTITION_CASES}
    assert ks >= {13, 31, 32, 33, 51, 63, 64, 65, 95, 96, 97, 127, 128}
    assert {case.nsamples for case in dc.PARTITION_CASES} == {1, 2, 3, 4, 5}
    assert {case.k for case, *_ in dc.FILTER_CASES} >= {129, 200}
    assert {case.nsamples for case, *_ in dc.FILTER_CASES} == {1, 2, 3, 4, 5}
    kinds = {kind for _c, _m, kind, *_ in dc.FILTER_CASES}
    assert kinds >= {'Nodetable', 'Counttable', 'SmallCounttable', 'Nodegraph', None}
    assert all(case.k <= 32 for case, _m, kind, *_ in dc.FILTER_CASES if kind == 'Nodegraph')


@pytest.mark.parametrize('case', dc.PARTITION_CASES, ids=lambda c: c.name)
def test_partition_cases_hold_what_they_claim(streams, case):
    stream = streams[case.name]
    planted = stream.planted
    default = dc.restate_partition(stream.records(), 2, 200)
    assert len(default.partitions) >= 20
    sizes = [len(p) for p in default.partitions]
    assert len(sizes) > len(set(sizes)), 'no two partitions of one size: the tie-break is not exercised'
    assert max(sizes) > 4 and min(sizes) == 2
    if 'dupseqs' in case.flags:
        assert default.stats['dedup'] > 0 and default.stats['dedup_rc'] > 0
        assert dc.restate_partition(stream.records(), 2, 200, dedup=False).nreads >= default.nreads + default.stats['dedup']
    if 'dupnames' in case.flags:
        assert default.stats['dupnames'] > 0
    # the planted k-mers, with no bound on abundance
    free = dc.restate_partition(stream.records(), None, None)
    if case.k % 2 == 0:
        pal, forward, backward = planted['palindrome']
        assert dc.rc(pal) == pal and dc.key_word_deciding(pal) is None
        assert len({dc.group_of(free, name) for name in forward + backward}) == 1
    for side_a, side_b in planted['near']:
        assert len({dc.group_of(free, name) for name in side_a}) == 1 and len({dc.group_of(free, name) for name in side_b}) == 1
        assert dc.group_of(free, side_a[0]) != dc.group_of(free, side_b[0])
    for kmer, agree, forward, backward in planted['strands']:
        assert len({dc.group_of(free, name) for name in forward + backward}) == 1
        assert dc.group_of(free, forward[0]) == frozenset(forward + backward)
    if case.k >= 36:
        groups = {dc.group_of(free, pair[0]) for pair in planted['family']}
        assert len(groups) == dc.FAMILY and all(g == frozenset(pair) for pair, g in zip(planted['family'], [dc.group_of(free, p[0]) for p in planted['family']]))
    # bounds that bite
    tight = dc.restate_partition(stream.records(), dc.PLANTED_MIN, dc.PLANTED_MAX)
    assert tight.stats['by_max'] > 0 and tight.stats['by_min'] > 0 and tight.stats['dropped_small'] > 0
    assert dc.group_of(tight, planted['max_exact'][0]) == frozenset(planted['max_exact'])       # exactly the bound: kept
    assert all(dc.group_of(tight, name) == frozenset([name]) for name in planted['max_over'])   # above it: dropped
    trio = planted['min_after_dedup']
    assert dc.group_of(tight, trio[0]) == frozenset(trio)
    assert not any(name in part for part in tight.partitions for name in trio), 'dedup leaves two of three: below min-abund'
    assert any(trio[0] in part for part in dc.restate_partition(stream.records(), dc.PLANTED_MIN, dc.PLANTED_MAX, dedup=False).partitions)
    assert tight.nedges > 0 and free.nedges > tight.nedges


def test_strand_choice_is_decided_in_every_key_word_but_the_first(streams):
    """which 64-bit word of the read graph's key decides between a k-mer and its reverse complement, over all planted k-mers: the
    second, third and fourth word are all reached (the first would need k-mers that differ within their first k - 96 bases, which
    every random k-mer of k > 96 does: those are counted too)"""
    words = {}
    for stream in streams.values():
        for kmer, agree, _f, _b in stream.planted['strands']:
            words.setdefault(dc.key_word_deciding(kmer), set()).add((stream.case.k, agree))
        for rec in stream.records()[:50]:
            for note in rec.annotations:
                words.setdefault(dc.key_word_deciding(rec.ikmerseq(note)), set()).add((stream.case.k, 0))
    assert set(words) >= {0, 1, 2, 3}, words
    for word in (1, 2, 3):
        assert any(agree > 0 for _k, agree in words[word]), (word, words[word])
    # the agreement reaches past a word boundary of the key somewhere: equal first word(s), decision in a later one
    assert any(agree >= 32 for _k, agree in words[1] | words[2] | words[3])


@pytest.mark.parametrize('entry', dc.FILTER_CASES, ids=lambda e: e[0].name)
def test_filter_cases_hold_what_they_claim(ok, entry):
    case, memory, kind, casemin, ctrlmax = entry
    stream = dc.generate(case)
    mask = dc.oracle_mask(ok, kind, stream)
    got = dc.restate_filter(ok, stream.records(), memory=memory, mask=mask, casemin=casemin, ctrlmax=ctrlmax)
    stats = got.stats
    assert got.processed == len(stream.specs) and 0 < got.validated < got.processed
    assert stats['by_recount'] > 0 and stats['partial'] > 0 and stats['vanished'] > 0, stats
    if case.nsamples > 1:
        assert stats['by_control'] > 0, stats
    if kind is not None:
        # the mask is the CAUSE: annotations that a run without the mask keeps and this one drops, and another output text
        assert stats['by_mask'] > 0, stats
        bare = dc.restate_filter(ok, stream.records(), memory=memory, mask=None, casemin=casemin, ctrlmax=ctrlmax)
        assert bare.stats['by_mask'] == 0 and bare.text != got.text and bare.validated > got.validated
    if memory <= dc.SMALL_MEMORY:
        assert stats['inflated'] > 0, stats
    if 'odd' in case.flags:
        assert len(stream.planted['odd']) == 3


def kept_notes(result):
    return [(r.name, [(n.offset, tuple(n.abund)) for n in r.annotations]) for r in result.records]


def test_filter_output_depends_on_the_lower_case_read_being_hashed_from_text(ok):
    """a lower-case k-mer hashes differently from its upper-case form (the hash goes over the text's bytes), so the lower-case read's
    k-mers are counted apart from the same k-mers of the reads beside it: in at least one filter case with such a read the validated
    annotations differ from those of the same stream with the read in upper case -- a product that packed the read and hashed it
    as upper case would be caught"""
    depends = []
    for case, memory, kind, casemin, ctrlmax in dc.FILTER_CASES:
        if 'odd' not in case.flags:
            continue
        stream = dc.generate(case)
        lower = stream.planted['odd'][2]
        upper = [s._replace(sequence=s.sequence.upper()) if s.name == lower else s for s in stream.specs]
        mask = dc.oracle_mask(ok, kind, stream)
        as_is = dc.restate_filter(ok, stream.records(), memory=memory, mask=mask, casemin=casemin, ctrlmax=ctrlmax)
        as_upper = dc.restate_filter(ok, dc.records_of(upper, case.k), memory=memory, mask=mask, casemin=casemin, ctrlmax=ctrlmax)
        depends.append(kept_notes(as_is) != kept_notes(as_upper))
    assert len(depends) >= 3 and sum(depends) >= 1, depends


def test_host_bound_on_k_is_the_device_key_width():
    """the host path of the read graph refuses the k the device's key cannot hold: 32 bases per word of KEY_WORDS (kv_graph.hip)"""
    import os
    import re
    from kevlar_amd import khmer
    source = open(os.path.join(os.path.dirname(khmer.__file__), 'csrc', 'kv_graph.hip')).read()
    assert khmer.READGRAPH_MAX_K == 32 * int(re.search(r'#define KEY_WORDS (\d+)', source).group(1))


@pytest.mark.parametrize('k', [21, 64, 128])
def test_host_components_from_text_are_the_restatement(k):
    """kevlar_amd.readgraph.text_components -- where `partition` builds the graph when an annotated k-mer holds a character the
    packed reads cannot (an N, lower case) -- against the restated loop: labels (smallest node of the component) and edge count"""
    import numpy as np
    from kevlar_amd import readgraph
    stream = dc.generate(dc.Case('odd', 60 + k, k, 2, frozenset(['dupseqs', 'dupnames', 'odd'])))
    records = stream.records()
    names = list(dict.fromkeys(r.name for r in records))
    node_id = {name: i for i, name in enumerate(names)}
    kmers = [r.ikmerseq(note) for r in records for note in r.annotations]
    nodes = np.array([node_id[r.name] for r in records for _ in r.annotations], dtype=np.uint32)
    assert any(kmer != kmer.upper() for kmer in kmers)
    for minabund, maxabund in [(0, 0), (2, 200), (dc.PLANTED_MIN, dc.PLANTED_MAX)]:
        want = dc.restate_partition(stream.records(), minabund, maxabund)
        labels, nedges = readgraph.text_components(kmers, nodes, len(names), minabund, maxabund, want_edges=True)
        groups = {}
        for name, label in zip(names, labels.tolist()):
            groups.setdefault(label, set()).add(name)
        assert {frozenset(g) for g in groups.values()} == want.components and nedges == want.nedges
        assert all(label == min(node_id[name] for name in g) for label, g in groups.items())
        assert np.array_equal(readgraph.text_components(kmers, nodes, len(names), minabund, maxabund), labels)


def test_a_lower_case_read_links_differently_from_its_upper_case_form():
    """the streams of the device test's odd cases, by the restatement: the lower-case read's k-mers are keyed by their upper-case
    reverse complement whichever strand is the smaller, so it joins only the reads whose canonical k-mer that is -- in two of the
    three streams that is not the component its upper-case form would join"""
    differs = 0
    for case in dc.ODD_CASES:
        stream = dc.generate(case)
        lower = stream.planted['odd'][2]
        assert [s for s in stream.specs if s.name == lower][0].notes
        upper = [s._replace(sequence=s.sequence.upper()) if s.name == lower else s for s in stream.specs]
        as_is = dc.restate_partition(stream.records(), 2, 200)
        as_upper = dc.restate_partition(dc.records_of(upper, case.k), 2, 200)
        assert len(dc.group_of(as_upper, lower)) > 1
        differs += dc.group_of(as_is, lower) != dc.group_of(as_upper, lower)
    assert differs >= 2
