"""`kevlar filter` and `kevlar partition` on the device against the literal restatements of tests/downstream_common.py (which
tests/test_downstream_reference.py holds to the reference's recorded outputs), over generated streams with ragged reads, both
strands, duplicate names and sequences, FASTA among FASTQ, mates, blank lines, 1 to 5 abundance columns, and k-mers planted for the
read graph's multi-word key: k from 13 to 128 for partition (129 is refused), to 200 for filter.  Each command runs three ways --
the CLI on a file (parsed natively, computed on arrays, formatted natively), the API on a file name or on records, and the device
call itself -- and everything is compared exactly: the output bytes with the restatement's text, the counts of the log lines,
component labels and edge counts."""
import gzip
import os

import numpy as np
import pytest

import downstream_common as dc

pytestmark = pytest.mark.gpu

NO_FPR_BOUND = 1e9      # the estimate of a table of a few hundred bytes exceeds 1: the runs that are not about it lift the bound
EXT = {'Nodetable': '.nt', 'Counttable': '.ct', 'SmallCounttable': '.sct', 'Nodegraph': '.ng'}


def run(argv, log):
    """one subcommand through the CLI's parser and main; returns what it logged"""
    import kevlar_amd
    log.seek(0)
    log.truncate()
    args = kevlar_amd.cli.parser().parse_args(argv)
    kevlar_amd.cli.mains[args.cmd](args)
    return log.getvalue()


def host_note():
    """the log line of a read graph built from k-mer text on the host"""
    from kevlar_amd import readgraph
    return readgraph.HOST_NOTE


def rendered(reads):
    from kevlar_amd.sequence import format_augmented_fastx
    return ''.join(format_augmented_fastx(read) for read in reads)


def fields(records):
    return [(r.name, r.sequence, r.quality, list(r.mates), [(n.offset, tuple(n.abund)) for n in r.annotations]) for r in records]


def parsed(text):
    import io
    import kevlar_amd
    return [rec for rec in kevlar_amd.parse_augmented_fastx(io.StringIO(text)) if rec is not None] if text.strip() else []


def numbered(text):
    """[(name, partition number)] of a partitioned stream, in order"""
    out = []
    for rec in parsed(text):
        name, number = rec.name.rsplit(' kvcc=', 1)
        out.append((name, int(number)))
    return out


def partition_args(minabund, maxabund, dedup):
    return ['--min-abund', str(minabund or 0), '--max-abund', str(maxabund or 0)] + ([] if dedup else ['--no-dedup'])


def grouped_line(want):
    return 'grouped {:d} reads into {:d} connected components'.format(want.nreads, len(want.partitions))


def device_components(hk, records, k, minabund, maxabund):
    """hk.readgraph_components on the records' own arrays: (components as a set of frozensets of names, labels, node names, edges)"""
    names = list(dict.fromkeys(r.name for r in records))
    node_id = {name: i for i, name in enumerate(names)}
    node_of_read = np.array([node_id[r.name] for r in records], dtype=np.uint32)
    ann_read = np.array([i for i, r in enumerate(records) for _ in r.annotations], dtype=np.uint32)
    ann_off = np.array([n.offset for r in records for n in r.annotations], dtype=np.uint32)
    batch = hk.ReadBatch([r.sequence for r in records])
    labels, nedges = hk.readgraph_components(batch, k, ann_read, ann_off, node_of_read, len(names), minabund or 0, maxabund or 0, want_edges=True)
    batch.close()
    groups = {}
    for name, label in zip(names, labels.tolist()):
        groups.setdefault(label, set()).add(name)
    return {frozenset(g) for g in groups.values()}, labels, names, nedges


# ---- partition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', dc.PARTITION_CASES, ids=lambda c: c.name)
def test_partition_three_ways_equal_the_reference_loop(hk, kevlar_log, tmp_path, case):
    import kevlar_amd
    stream = dc.generate(case)
    infile = str(tmp_path / 'in.augfastq')
    with open(infile, 'w') as fh:
        fh.write(stream.text)
    for minabund, maxabund, dedup in dc.PARTITION_OPTIONS:
        tag = (case.name, minabund, maxabund, dedup)
        want = dc.restate_partition(stream.records(), minabund, maxabund, dedup)
        # the device call itself: labels and edge count
        comps, labels, names, nedges = device_components(hk, stream.records(), case.k, minabund, maxabund)
        print(tag, 'partitions', len(want.partitions), 'reads', want.nreads, 'components', len(want.components), len(comps), 'edges', want.nedges, nedges)
        assert comps == want.components, tag
        assert nedges == want.nedges, tag
        first = {}
        for i, label in enumerate(labels.tolist()):
            first.setdefault(label, i)
        assert all(label == at for label, at in first.items()), 'a label is the smallest node id of its component'
        # the ReadGraph path, on records
        kevlar_log.seek(0)
        kevlar_log.truncate()
        by_records = rendered(read for _n, reads in kevlar_amd.partition.partition(stream.records(), minabund=minabund, maxabund=maxabund, dedup=dedup)
                              for read in reads)
        assert numbered(by_records) == [(name, n) for n, part in enumerate(want.partitions, 1) for name in part], tag
        assert by_records == want.text, tag
        assert host_note() not in kevlar_log.getvalue()
        # the array path: the CLI on a file
        if minabund is None:
            continue                       # (the CLI has no way to say None: 0 is the same bound)
        out = str(tmp_path / 'out.augfastq')
        log = run(['partition'] + partition_args(minabund, maxabund, dedup) + ['-o', out, infile], kevlar_log)
        got = open(out).read()
        assert numbered(got) == numbered(want.text), tag
        assert got == want.text, tag
        assert got == by_records, tag
        assert grouped_line(want) in log, tag


def test_partition_split_and_gzip_input(hk, kevlar_log, tmp_path):
    import kevlar_amd
    case = dc.PARTITION_CASES[4]                      # k = 51: the k of the benchmark's config 5
    assert case.k == 51
    stream = dc.generate(case)
    infile = str(tmp_path / 'in.augfastq.gz')
    with gzip.open(infile, 'wt') as fh:
        fh.write(stream.text)
    want = dc.restate_partition(stream.records(), 2, 200)
    out = str(tmp_path / 'out.augfastq')
    log = run(['partition', '-o', out, infile], kevlar_log)
    assert open(out).read() == want.text and grouped_line(want) in log
    prefix = str(tmp_path / 'split' / 'part')
    log = run(['partition', '--split', prefix, infile], kevlar_log)
    assert grouped_line(want) in log
    files = sorted(os.listdir(str(tmp_path / 'split')))
    assert files == sorted('part.cc{:d}.augfastq.gz'.format(n) for n in range(1, len(want.partitions) + 1))
    whole = []
    for n, part in enumerate(want.partitions, 1):
        with kevlar_amd.open('{}.cc{:d}.augfastq.gz'.format(prefix, n), 'r') as fh:
            text = fh.read()
        assert numbered(text) == [(name, n) for name in part]
        whole.append(text)
    assert ''.join(whole) == want.text
    # through split's own reader: the partitions come back under their numbers
    back = list(kevlar_amd.parse_partitioned_reads(parsed(open(out).read())))
    assert [(pid, [r.name.rsplit(' kvcc=', 1)[0] for r in reads]) for pid, reads in back] == [(str(n), part) for n, part in enumerate(want.partitions, 1)]


def test_partition_refuses_k_129_and_takes_a_stream_without_annotations(hk, kevlar_log, tmp_path):
    import kevlar_amd
    stream = dc.generate(dc.Case('k129', 7, 129, 2, frozenset(['dupseqs'])))
    infile, out = str(tmp_path / 'in.augfastq'), str(tmp_path / 'out.augfastq')
    with open(infile, 'w') as fh:
        fh.write(stream.text)
    with pytest.raises(ValueError, match='partition supports k <= 128'):
        run(['partition', '-o', out, infile], kevlar_log)
    assert not os.path.exists(out) or os.path.getsize(out) == 0
    seen = []
    with pytest.raises(ValueError, match='partition supports k <= 128'):
        for item in kevlar_amd.partition.partition(stream.records()):
            seen.append(item)
    assert seen == []
    # no annotation anywhere: every read on its own, nothing to write (at any k)
    bare = [spec._replace(notes=[]) for spec in stream.specs]
    with open(infile, 'w') as fh:
        fh.write(dc.render(bare, 129))
    want = dc.restate_partition(dc.records_of(bare, 129), 2, 200)
    assert want.partitions == [] and len(want.components) == len({s.name for s in bare})
    log = run(['partition', '-o', out, infile], kevlar_log)
    assert open(out).read() == '' and 'grouped 0 reads into 0 connected components' in log
    assert list(kevlar_amd.partition.partition(dc.records_of(bare, 129))) == []


# ---- reads outside upper-case ACGT in partition ----------------------------------------------------------------------------
def both_paths(kevlar_log, tmp_path, specs, k, minabund=2, maxabund=200):
    """(text of the CLI on a file, its log, text of partition() on records, its log)"""
    import kevlar_amd
    infile, out = str(tmp_path / 'odd.augfastq'), str(tmp_path / 'odd.out.augfastq')
    with open(infile, 'w') as fh:
        fh.write(dc.render(specs, k))
    log_file = run(['partition'] + partition_args(minabund, maxabund, True) + ['-o', out, infile], kevlar_log)
    kevlar_log.seek(0)
    kevlar_log.truncate()
    by_records = rendered(read for _n, reads in kevlar_amd.partition.partition(dc.records_of(specs, k), minabund=minabund, maxabund=maxabund)
                          for read in reads)
    return open(out).read(), log_file, by_records, kevlar_log.getvalue()


def test_partition_keys_an_annotated_N_by_its_text(hk, kevlar_log, tmp_path):
    """The reference keys the graph by revcommin() of the k-mer TEXT (kevlar/readgraph.py:71-73): a k-mer with an N is not the
    k-mer with an A in its place.  Packed into two bits the N becomes an A, so the device's key would link the two; streams with
    such annotations are keyed from text on the host instead (kevlar_amd.readgraph.text_components)."""
    k = 21
    with_a = 'GATTACAGGCATCAGCTAAGT'
    with_n = with_a[:10] + 'N' + with_a[11:]
    assert with_a[10] == 'A' and len(with_a) == k

    def spec(name, left, kmer, right, minus=False):
        seq, off = left + kmer + right, len(left)
        if minus:
            seq, off = dc.rc(seq), len(right)             # (the N stays an N, as in the reference's complement table)
        return dc.Spec(name, seq, 'I' * len(seq), [(off, (12, 0, 1))], [])
    specs = [spec('n1', 'CCGT', with_n, 'TTGAC'), spec('a1', 'GGA', with_a, 'CATG'), spec('a2', 'TCT', with_a, 'AAGC', minus=True),
             spec('n2', 'ACAC', with_n, 'GTC', minus=True)]
    want = dc.restate_partition(dc.records_of(specs, k), 2, 200)
    assert sorted(map(sorted, want.partitions)) == [['a1', 'a2'], ['n1', 'n2']], 'by the reference\'s arithmetic: no link between N and A'
    by_file, log_file, by_records, log_records = both_paths(kevlar_log, tmp_path, specs, k)
    assert by_file == want.text and by_records == want.text
    assert grouped_line(want) in log_file
    assert host_note() in log_file and host_note() in log_records


@pytest.mark.parametrize('case', dc.ODD_CASES, ids=lambda c: c.name)
def test_partition_with_odd_reads_equals_the_reference_loop(hk, kevlar_log, tmp_path, case):
    """a lower-case read with annotations (its k-mers' keys are always their upper-case reverse complements in the reference: it
    links to the reads whose canonical k-mer that is, and to no others) and reads with an N outside every annotated k-mer (which
    changes nothing, and leaves the stream on the device)"""
    stream, k = dc.generate(case), case.k
    lower = stream.planted['odd'][2]
    want = dc.restate_partition(stream.records(), 2, 200)
    by_file, log_file, by_records, log_records = both_paths(kevlar_log, tmp_path, stream.specs, k)
    assert by_file == want.text and by_records == want.text
    assert grouped_line(want) in log_file
    assert host_note() in log_file and host_note() in log_records
    # without the lower-case read only the Ns outside the annotated k-mers are left: the device path, the same partitions as the
    # reference's, and the same as with the Ns cut off again
    rest = [s for s in stream.specs if s.name != lower]
    want = dc.restate_partition(dc.records_of(rest, k), 2, 200)
    by_file, log_file, by_records, log_records = both_paths(kevlar_log, tmp_path, rest, k)
    assert by_file == want.text and by_records == want.text
    assert host_note() not in log_file and host_note() not in log_records
    left, right = stream.planted['odd'][:2]
    cut = [s._replace(sequence=s.sequence[1:], quality=s.quality and s.quality[1:], notes=[(o - 1, a) for o, a in s.notes]) if s.name == left else
           s._replace(sequence=s.sequence[:-1], quality=s.quality and s.quality[:-1]) if s.name == right else s for s in rest]
    assert 'N' not in ''.join(s.sequence for s in cut) and 'N' in ''.join(s.sequence for s in rest)
    assert dc.restate_partition(dc.records_of(cut, k), 2, 200).components == want.components
    comps, _labels, _names, nedges = device_components(hk, dc.records_of(rest, k), k, 2, 200)
    assert comps == want.components and nedges == want.nedges


# ---- filter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', dc.FILTER_CASES, ids=lambda e: e[0].name)
def test_filter_three_ways_equal_the_reference_loop(hk, ok, kevlar_log, tmp_path, entry):
    import kevlar_amd
    case, memory, kind, casemin, ctrlmax = entry
    stream = dc.generate(case)
    infile, out = str(tmp_path / 'in.augfastq'), str(tmp_path / 'out.augfastq')
    with open(infile, 'w') as fh:
        fh.write(stream.text)
    mask_file, ref_mask = None, dc.oracle_mask(ok, kind, stream)
    if ref_mask is not None:
        mask_file = str(tmp_path / ('mask' + EXT[kind]))
        ref_mask.save(mask_file)
    want = dc.restate_filter(ok, stream.records(), memory=memory, mask=ref_mask, casemin=casemin, ctrlmax=ctrlmax)
    print(case.name, memory, kind, 'processed', want.processed, 'validated', want.validated, want.stats)
    counts = ['Processed {:d} reads'.format(want.processed), 'Validated {:d} reads'.format(want.validated)]
    # the CLI on a file, written to a plain file (the native formatter writes the file itself)
    argv = ['filter', '--memory', str(int(memory)), '--max-fpr', str(NO_FPR_BOUND), '--case-min', str(casemin), '--ctrl-max', str(ctrlmax), '-o', out]
    log = run(argv + (['--mask', mask_file] if mask_file else []) + [infile], kevlar_log)
    by_cli = open(out).read()
    assert fields(parsed(by_cli)) == fields(want.records)
    assert by_cli == want.text
    assert all(line in log for line in counts), log
    # filter() on a file name and on records
    for source in (infile, iter(stream.records())):
        kevlar_log.seek(0)
        kevlar_log.truncate()
        mask = kevlar_amd.sketch.load(mask_file) if mask_file else None
        got = list(kevlar_amd.filter.filter(source, mask=mask, memory=memory, maxfpr=NO_FPR_BOUND, casemin=casemin, ctrlmax=ctrlmax))
        assert fields(got) == fields(want.records)
        assert rendered(got) == by_cli
        assert all(line in kevlar_log.getvalue() for line in counts)


def test_filter_bails_out_above_max_fpr(hk, kevlar_log, tmp_path):
    import kevlar_amd
    stream = dc.generate(dc.FILTER_CASES[0][0])
    infile, out = str(tmp_path / 'in.augfastq'), str(tmp_path / 'out.augfastq')
    with open(infile, 'w') as fh:
        fh.write(stream.text)
    with pytest.raises(kevlar_amd.sketch.KevlarUnsuitableFPRError, match='FPR too high, bailing out'):
        run(['filter', '--memory', '300', '--max-fpr', '0.01', '-o', out, infile], kevlar_log)
    assert 'First pass complete! Processed {:d} reads'.format(len(stream.specs)) in kevlar_log.getvalue()
    assert 'Second pass' not in kevlar_log.getvalue()
    assert not os.path.exists(out) or os.path.getsize(out) == 0
