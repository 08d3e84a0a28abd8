"""`kevlar localize`: where in the reference genome do the contigs of each partition sit (the reference's kevlar/localize.py).

Every window of length Z of every contig is a seed.  The reference writes the seeds to a temporary FASTA and runs
`bwa mem -k Z -T Z -a -c 5000` on them, which reports nothing but the perfect, full-length matches of each seed
(kevlar/localize.py:131-144).  That is an exact join between the canonical seeds and the windows of the genome, and here it is
one: the seeds become a table in GPU memory (kv_localize_create) and the genome text is streamed past it chunk by chunk
(kv_localize_scan).  No aligner, no index files, no temporary files.

Public names and behaviour follow the reference: `Localizer`, `decompose_seeds`, `contigs_2_seeds`, `get_seed_matches`,
`cutout`, `localize`, `main`.  `localize()` keeps the matches as arrays in CSR form (seed -> positions) and walks Python objects
only for the per-partition clustering.

One deliberate departure: `max_occ`.  With `-c 5000` bwa keeps a sample of 5000 occurrences of a seed that has more, picked in
suffix-array order, which cannot be reproduced without its index.  Here a seed with more than `max_occ` positions in the genome
(both strands counted, the position of a palindromic seed once) contributes none."""
import ctypes
import re
from collections import defaultdict

import numpy as np

import kevlar_amd
from kevlar_amd import _lib
from kevlar_amd.reference import ReferenceCutout

DEFAULT_MAX_OCC = 5000
DEFAULT_CHUNK_BYTES = 64 << 20          # genome text per scan call
DEFAULT_MATCH_CAPACITY = 1 << 20        # (seed, position) pairs a scan call has room for before it is repeated with more
SEPARATOR = b'>'                        # one byte between the sequences of the genome text: no window spans two sequences
NO_SEED = 0xFFFFFFFF


class KevlarRefrSeqNotFoundError(ValueError):
    """Raised if the reference sequence cannot be found."""
    pass


class Localizer(object):
    """Seed match positions per reference sequence, and the cutouts that span them."""

    def __init__(self, seedsize, incl=None, excl=None):
        self._positions = defaultdict(list)
        self._seedsize = seedsize
        self.inclpattern = incl
        self.exclpattern = excl

    def __len__(self):
        return sum(len(hits) for seqid, hits in self._positions.items() if not self.ignore_seqid(seqid))

    def ignore_seqid(self, seqid):
        """Is this sequence left out (alternate or decoy sequences, organelles...)?"""
        if self.exclpattern and re.search(self.exclpattern, seqid) is not None:
            return True
        return bool(self.inclpattern) and re.search(self.inclpattern, seqid) is None

    def add_seed_match(self, seqid, pos):
        self._positions[seqid].append(pos)

    def _cutout(self, seqid, cluster, refrseqs, delta):
        start = max(cluster[0] - delta, 0)
        end = cluster[-1] + self._seedsize + delta
        subseq = None
        if refrseqs:
            end = min(end, len(refrseqs[seqid]))
            subseq = refrseqs[seqid][start:end]
        return ReferenceCutout('{:s}_{:d}-{:d}'.format(seqid, start, end), subseq)

    def get_cutouts(self, refrseqs=None, delta=0, clusterdist=1000):
        """One cutout per cluster of matches: their span plus `delta` on either side.  Neighbouring matches further apart than
        `clusterdist` start a new cluster; a false `clusterdist` gives one cutout per sequence."""
        for seqid in sorted(self._positions):
            if self.ignore_seqid(seqid):
                continue
            hits = sorted(self._positions[seqid])
            assert len(hits) > 0
            if refrseqs and seqid not in refrseqs:
                raise KevlarRefrSeqNotFoundError(seqid)
            first = 0
            if clusterdist:
                for i in range(1, len(hits)):
                    if hits[i] - hits[i - 1] > clusterdist:
                        yield self._cutout(seqid, hits[first:i], refrseqs, delta)
                        first = i
            yield self._cutout(seqid, hits[first:], refrseqs, delta)


def decompose_seeds(seq, seedsize):
    """The windows of length `seedsize` of a sequence: k-mers by another name, because the seed size of this step need not
    be the k of k-mer counting."""
    return (seq[i:i + seedsize] for i in range(len(seq) - seedsize + 1))


def contigs_2_seeds(partstream, seedstream, seedsize=51):
    """The canonical seeds of all contigs of all partitions, sorted, as FASTA (what the reference feeds to bwa)."""
    kevlar_amd.plog('[kevlar::localize]', 'decomposing contigs into seeds of length {}'.format(seedsize))
    seeds = sorted({kevlar_amd.revcommin(seed) for partition in partstream for contig in partition
                    for seed in decompose_seeds(contig.sequence, seedsize)})
    for n, seed in enumerate(seeds):
        print('>seed{}\n{}'.format(n, seed), file=seedstream)
    seedstream.flush()
    # the reference reports the index of the last seed, one less than their number (0 when there is none)
    kevlar_amd.plog('[kevlar::localize]', 'contigs decomposed into {} seeds'.format(max(len(seeds) - 1, 0)))


# ---- the device scan ------------------------------------------------------------------------------------------------------
class Genome(object):
    """The sequences of a reference as one text: sequence i is text[starts[i] : starts[i] + len(seqs[i])], with one SEPARATOR
    byte between neighbours, so a global position maps back to (sequence, local position) by a search over `starts`."""
    on_device = False

    def __init__(self, records):
        self.ids = [seqid for seqid, seq in records]
        self.seqs = [seq for seqid, seq in records]
        lengths = np.array([len(seq) for seq in self.seqs], dtype=np.int64)
        self.starts = np.zeros(len(self.seqs), dtype=np.int64)
        if len(self.seqs) > 1:
            self.starts[1:] = np.cumsum(lengths[:-1] + 1)
        self.text = np.frombuffer(SEPARATOR.join(seq.encode('latin-1') for seq in self.seqs), dtype=np.uint8)

    @classmethod
    def from_file(cls, refrfile):
        """seqid = the defline up to the first blank; `refrfile`: a path, '-' or an open text stream (left open)"""
        if not (refrfile is None or isinstance(refrfile, str)):
            return cls(list(kevlar_amd.seqio.parse_seq_dict(refrfile).items()))
        stream = kevlar_amd.open(refrfile, 'r')
        try:
            return cls(list(kevlar_amd.seqio.parse_seq_dict(stream).items()))
        finally:
            if refrfile not in ('-', None):
                stream.close()

    def seqdict(self):
        return dict(zip(self.ids, self.seqs))

    def locate(self, positions):
        """(sequence index, local position) of global positions"""
        positions = np.asarray(positions, dtype=np.int64)
        which = np.searchsorted(self.starts, positions, side='right') - 1
        return which, positions - self.starts[which]


class GenomeDeclined(ValueError):
    """The device FASTA splitter does not take this file (KV_ERR_TYPE): the host parser reads it."""


class _PendingSlice(object):
    """A slice of a device-resident sequence that has been asked for and not fetched yet: it knows its length, and `value` once
    DeviceGenome.fetch_many has filled the collector it sits in."""

    def __init__(self, index, start, stop):
        self.index, self.start, self.stop = index, start, stop
        self.value = None

    def __len__(self):
        return self.stop - self.start

    def __str__(self):
        return self.value


class _LazySequence(object):
    """Sequence i of a DeviceGenome as far as localize needs a string: len() and slicing with Python's clipping.  A slice is
    fetched from the device at once, or, with a collector, noted there and fetched with all the others."""

    def __init__(self, genome, index, collector=None):
        self._genome, self._index, self._collector = genome, index, collector

    def __len__(self):
        return int(self._genome.lengths[self._index])

    def __getitem__(self, key):
        if not isinstance(key, slice):
            key = range(len(self))[key]
            key = slice(key, key + 1)
        start, stop, step = key.indices(len(self))
        if step != 1:
            return str(self)[key]
        stop = max(stop, start)
        if self._collector is not None:
            pending = _PendingSlice(self._index, start, stop)
            self._collector.append(pending)
            return pending
        return self._genome.fetch_many([(self._index, start, stop)])[0]

    def __str__(self):
        return self._genome.fetch_many([(self._index, 0, len(self))])[0]


class DeviceGenome(object):
    """Genome whose text was parsed on the device (kv_genome_open) and stays there: `ids`, `starts`, `lengths` and `locate` as
    Genome has them, the sequences as lazy slices (`seqdict`, `fetch_many`), and SeedSet.scan_genome scans the text where it is.
    Raises GenomeDeclined for a file the device does not take; duplicate ids are the AssertionError of seqio.parse_seq_dict."""
    on_device = True

    def __init__(self, path, segment_text=0):
        self._handle = None
        _lib.require_device()
        self._lib = _lib.load()
        handle = ctypes.c_void_p()
        rc = self._lib.kv_genome_open(str(path).encode(), int(segment_text), ctypes.byref(handle))
        if rc == _lib.KV_ERR_TYPE:
            raise GenomeDeclined(_lib.last_error())
        _lib.check(rc)
        self._handle = handle
        nseq, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
        stats = np.zeros(4, dtype=np.uint64)
        ids, id_offs, starts, lengths = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self._lib.kv_genome_info(handle, ctypes.byref(nseq), ctypes.byref(nbytes), stats.ctypes.data, ctypes.byref(ids),
                                            ctypes.byref(id_offs), ctypes.byref(starts), ctypes.byref(lengths)))
        n = int(nseq.value)
        self.n_text = int(nbytes.value)
        self.container, self.n_segments = ('plain', 'bgzf', 'gzip')[int(stats[0])], int(stats[1])

        def column(pointer, count):
            if count == 0:
                return np.zeros(0, dtype=np.int64)
            return np.ctypeslib.as_array(ctypes.cast(pointer, ctypes.POINTER(ctypes.c_uint64)), shape=(count,)).astype(np.int64)
        offs = column(id_offs, n + 1)
        blob = ctypes.string_at(ids, int(offs[-1])) if n and offs[-1] else b''
        self.ids = [blob[offs[i]:offs[i + 1]].decode('ascii') for i in range(n)]
        self.starts, self.lengths = column(starts, n), column(lengths, n)
        seen = set()
        for seqid in self.ids:
            assert seqid not in seen, seqid
            seen.add(seqid)

    def close(self):
        if self._handle is not None:
            self._lib.kv_genome_close(self._handle)
            self._handle = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def seqdict(self, collector=None):
        """{id: lazy sequence}; with a list as `collector` the slices taken are noted in it and filled by resolve()"""
        return {seqid: _LazySequence(self, i, collector) for i, seqid in enumerate(self.ids)}

    def locate(self, positions):
        """(sequence index, local position) of global positions"""
        positions = np.asarray(positions, dtype=np.int64)
        which = np.searchsorted(self.starts, positions, side='right') - 1
        return which, positions - self.starts[which]

    def fetch_text(self, start, length):
        """bytes [start, start + length) of the genome text, clipped at its end"""
        starts, lens = np.array([start], dtype=np.uint64), np.array([length], dtype=np.uint64)
        out = ctypes.create_string_buffer(max(int(length), 1))
        offs = np.zeros(2, dtype=np.uint64)
        _lib.check(self._lib.kv_genome_fetch(self._handle, starts.ctypes.data, lens.ctypes.data, 1, out, offs.ctypes.data))
        return out.raw[:int(offs[1])]

    def fetch_many(self, requests):
        """[sequence[start:stop] as str for (sequence index, start, stop) in requests], clipped as Python clips slices, all of
        them in one gather launch"""
        requests = list(requests)
        if not requests:
            return []
        index = np.array([r[0] for r in requests], dtype=np.int64)
        length = self.lengths[index]
        start = np.clip(np.array([r[1] for r in requests], dtype=np.int64), 0, length)
        stop = np.clip(np.array([r[2] for r in requests], dtype=np.int64), start, length)
        starts = (self.starts[index] + start).astype(np.uint64)
        lens = (stop - start).astype(np.uint64)
        out = ctypes.create_string_buffer(max(int(lens.sum()), 1))
        offs = np.zeros(len(requests) + 1, dtype=np.uint64)
        _lib.check(self._lib.kv_genome_fetch(self._handle, starts.ctypes.data, lens.ctypes.data, len(requests), out, offs.ctypes.data))
        blob = out.raw[:int(offs[-1])].decode('latin-1')
        offs = offs.astype(np.int64).tolist()
        return [blob[offs[i]:offs[i + 1]] for i in range(len(requests))]

    def resolve(self, collector):
        """fetch every slice noted in `collector` (one fetch_many) and fill its value"""
        for pending, value in zip(collector, self.fetch_many([(p.index, p.start, p.stop) for p in collector])):
            pending.value = value


last_load = {}          # how the last load_genome went: on_device, container, declined (the reason, or None); for tests and tools


def load_genome(refrfile, segment_text=0):
    """The reference for localize: parsed and kept on the device when `refrfile` is a file on disk that the device splitter
    takes (`on_device` is then true), else today's host Genome -- for '-', an open stream, a file whose name and content disagree
    about gzip (the host goes by the name), and a file the device declines."""
    import os
    last_load.clear()
    last_load.update(on_device=False, declined=None)
    if isinstance(refrfile, str) and refrfile != '-' and os.path.isfile(refrfile):
        with open(refrfile, 'rb') as fh:
            gzipped = fh.read(2) == b'\x1f\x8b'
        if gzipped == refrfile.endswith('.gz'):
            try:
                genome = DeviceGenome(refrfile, segment_text=segment_text)
                last_load.update(on_device=True, container=genome.container)
                return genome
            except GenomeDeclined as why:
                last_load.update(declined=str(why))           # (why the device did not take it; nothing is printed)
    return Genome.from_file(refrfile)


class SeedSet(object):
    """The canonical seeds of a list of contig sequences on the device.  `seed_of_window[w]`: seed id of window w (windows
    counted contig after contig; contig c owns windows wpre[c] .. wpre[c + 1]), NO_SEED for a window with a byte outside ACGT.
    The id of a seed is the index of one of its windows, so `sequence(id)` reads it back from the contigs."""

    def __init__(self, sequences, seedsize):
        self._handle = None
        _lib.require_device()
        self._lib = _lib.load()
        self.seedsize = int(seedsize)
        self.sequences = list(sequences)
        lengths = np.array([len(s) for s in self.sequences], dtype=np.int64)
        offsets = np.zeros(len(lengths) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(lengths)
        self.wpre = np.zeros(len(lengths) + 1, dtype=np.int64)
        self.wpre[1:] = np.cumsum(np.maximum(lengths - self.seedsize + 1, 0))
        self.n_windows = int(self.wpre[-1])
        bases = np.frombuffer(''.join(self.sequences).encode('latin-1'), dtype=np.uint8)
        self.seed_of_window = np.empty(self.n_windows, dtype=np.uint32)
        distinct = ctypes.c_uint64(0)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.kv_localize_create(bases.ctypes.data, offsets.ctypes.data, len(lengths), self.seedsize,
                                                self.seed_of_window.ctypes.data, self.n_windows, ctypes.byref(distinct),
                                                ctypes.byref(handle)))
        self._handle = handle
        self.n_distinct = int(distinct.value)

    def close(self):
        if self._handle is not None:
            self._lib.kv_localize_destroy(self._handle)
            self._handle = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sequence(self, seed_id):
        """the seed as the reference spells it: the smaller of the window and its reverse complement"""
        contig = int(np.searchsorted(self.wpre, seed_id, side='right')) - 1
        start = int(seed_id) - int(self.wpre[contig])
        return kevlar_amd.revcommin(self.sequences[contig][start:start + self.seedsize].upper())

    def counts(self):
        """occurrences per seed id over everything scanned so far"""
        out = np.zeros(self.n_windows, dtype=np.uint32)
        _lib.check(self._lib.kv_localize_counts(self._handle, out.ctypes.data, self.n_windows))
        return out

    def stats(self):
        """(windows of valid bases scanned, windows that passed the prefilter, matches, distinct seeds)"""
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(self._lib.kv_localize_stats(self._handle, out.ctypes.data))
        return tuple(int(v) for v in out)

    def scan(self, text, chunk_bytes=DEFAULT_CHUNK_BYTES, capacity=DEFAULT_MATCH_CAPACITY):
        """(seed ids, global positions) of every window of `text` (uint8 array) that equals a seed or its reverse complement.
        The text goes to the device in chunks of `chunk_bytes` that overlap by seedsize - 1, so every window lies in exactly
        one of them; a chunk with more matches than `capacity` is scanned again with room for all of them."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        z, n = self.seedsize, len(text)
        chunk_bytes = max(int(chunk_bytes), z)
        step = chunk_bytes - (z - 1)
        capacity = max(int(capacity), 1)
        ids = np.empty(capacity, dtype=np.uint32)
        pos = np.empty(capacity, dtype=np.uint64)
        found = ctypes.c_uint64(0)
        found_ref = ctypes.byref(found)
        scan, handle, base = self._lib.kv_localize_scan, self._handle, text.ctypes.data
        got_ids, got_pos = [], []
        start = 0
        while start + z <= n:
            size = min(chunk_bytes, n - start)
            while True:
                rc = scan(handle, base + start, size, start, ids.ctypes.data, pos.ctypes.data, capacity, found_ref)
                if rc != 0:
                    _lib.check(rc)
                if found.value <= capacity:
                    break
                capacity = max(int(found.value), 2 * capacity)
                ids = np.empty(capacity, dtype=np.uint32)
                pos = np.empty(capacity, dtype=np.uint64)
            if found.value:
                got_ids.append(ids[:found.value].copy())
                got_pos.append(pos[:found.value].copy())
            start += step
        if not got_ids:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64)
        return np.concatenate(got_ids), np.concatenate(got_pos)

    def scan_genome(self, genome, chunk_bytes=0, capacity=DEFAULT_MATCH_CAPACITY):
        """scan() over the text of a DeviceGenome where it lies: one call, nothing uploaded.  chunk_bytes: the most text one
        chunk holds (0: the whole text in one); more matches than `capacity`: the call is repeated with room for all of them."""
        capacity = max(int(capacity), 1)
        found = ctypes.c_uint64(0)
        while True:
            ids = np.empty(capacity, dtype=np.uint32)
            pos = np.empty(capacity, dtype=np.uint64)
            _lib.check(self._lib.kv_localize_scan_genome(self._handle, genome._handle, int(chunk_bytes), ids.ctypes.data, pos.ctypes.data,
                                                         capacity, ctypes.byref(found)))
            if found.value <= capacity:
                return ids[:found.value].copy(), pos[:found.value].copy()
            capacity = max(int(found.value), 2 * capacity)


class SeedMatches(object):
    """Matches of a seed set in a genome, sorted by seed id, in CSR form: seed ids `seeds` (ascending), the matches of
    seeds[r] are rows indptr[r] .. indptr[r + 1] of (`seqidx`, `local`); `row_of` maps a seed id to r (-1: no match kept)."""

    def __init__(self, seedset, genome, max_occ=DEFAULT_MAX_OCC, chunk_bytes=None,
                 capacity=DEFAULT_MATCH_CAPACITY):
        # chunk_bytes None: DEFAULT_CHUNK_BYTES of an uploaded text at a time; a resident text (no upload buffer to bound) in one
        if genome.on_device:
            ids, pos = seedset.scan_genome(genome, chunk_bytes=chunk_bytes or 0, capacity=capacity)
        else:
            ids, pos = seedset.scan(genome.text, chunk_bytes=chunk_bytes or DEFAULT_CHUNK_BYTES, capacity=capacity)
        self.counts = seedset.counts()
        if max_occ:
            keep = self.counts[ids] <= max_occ
            ids, pos = ids[keep], pos[keep]
        order = np.lexsort((pos, ids))
        ids, pos = ids[order], pos[order]
        self.seeds, first = np.unique(ids, return_index=True)
        self.indptr = np.append(first, len(ids)).astype(np.int64)
        self.seqidx, self.local = genome.locate(pos)
        self.row_of = np.full(seedset.n_windows + 1, -1, dtype=np.int64)      # (+1: NO_SEED is looked up as the last entry)
        self.row_of[self.seeds] = np.arange(len(self.seeds))
        self.seedset, self.genome = seedset, genome

    def __len__(self):
        return len(self.seeds)

    def of_windows(self, window_ids):
        """rows of the matches of the given contig windows, window after window (a seed two windows share comes twice, as it
        does when the reference looks every window up in its dictionary)"""
        seed = self.seedset.seed_of_window[window_ids].astype(np.int64)
        seed[seed == NO_SEED] = self.seedset.n_windows
        rows = self.row_of[seed]
        rows = rows[rows >= 0]
        lo, count = self.indptr[rows], self.indptr[rows + 1] - self.indptr[rows]
        total = int(count.sum())
        if total == 0:
            return np.zeros(0, dtype=np.int64)
        ends = np.cumsum(count)
        return np.repeat(lo - (ends - count), count) + np.arange(total)

    def triples(self):
        """{(seed sequence, seqid, local position)}"""
        out = set()
        for r, seed_id in enumerate(self.seeds):
            seq = self.seedset.sequence(seed_id)
            for i in range(self.indptr[r], self.indptr[r + 1]):
                out.add((seq, self.genome.ids[self.seqidx[i]], int(self.local[i])))
        return out


def get_seed_matches(seedfile, refrfile, seedsize=51, max_occ=DEFAULT_MAX_OCC, chunk_bytes=None):
    """{canonical seed: {(seqid, position)}} for the seeds of a FASTA file: the reference's dictionary, computed by the device
    scan.  A seed with more than `max_occ` positions is left out (see the module's docstring)."""
    kevlar_amd.plog('[kevlar::localize] computing seed matches')
    stream = kevlar_amd.open(seedfile, 'r')
    try:
        seqs = [seq for defline, seq in kevlar_amd.seqio.parse_fasta(stream)]
    finally:
        if seedfile not in ('-', None):
            stream.close()
    genome = load_genome(refrfile)
    with SeedSet(seqs, seedsize) as seedset:
        matches = SeedMatches(seedset, genome, max_occ=max_occ, chunk_bytes=chunk_bytes)
        seed_index = defaultdict(set)
        for seq, seqid, pos in matches.triples():
            seed_index[seq].add((seqid, pos))
    kevlar_amd.plog('[kevlar::localize]', 'found positions for {} seeds'.format(len(seed_index)))
    return dict(seed_index)


def cutout(contigs, refrseqs, seed_matches, seedsize=51, delta=50, maxdiff=None, inclpattern=None, exclpattern=None,
           debug=False):
    """Reference target sequences of one partition's contigs from a {seed: {(seqid, position)}} dictionary: the span of the
    positions of all their seeds, clustered by `maxdiff` (None: three times the longest contig), widened by `delta`."""
    localizer = Localizer(seedsize, incl=inclpattern, excl=exclpattern)
    for contig in contigs:
        for seed in decompose_seeds(contig.sequence, seedsize):
            hits = seed_matches.get(kevlar_amd.revcommin(seed))
            if hits is None:
                if debug:  # pragma: no cover
                    kevlar_amd.plog('[kevlar::localize]', 'WARNING: no position for seed {}'.format(kevlar_amd.revcommin(seed)))
                continue
            for seqid, position in hits:
                localizer.add_seed_match(seqid, position)
    if maxdiff is None:
        maxdiff = 3 * max(len(c.sequence) for c in contigs)
    yield from localizer.get_cutouts(refrseqs=refrseqs, delta=delta, clusterdist=maxdiff)


def localize(partstream, refrfile, seedsize=51, delta=50, maxdiff=None, inclpattern=None, exclpattern=None, debug=False,
             max_occ=DEFAULT_MAX_OCC, chunk_bytes=None):
    """(partition id, ReferenceCutout) for every reference target of every partition of (partition id, contigs) pairs.

    refrfile: a path (the genome is then parsed and kept on the device where the file allows it: load_genome), '-' or an open
    text stream (parsed on the host).  maxdiff=None clusters by three times the partition's longest contig; a false maxdiff (0)
    gives one cutout per sequence.  max_occ: a seed with more genome positions than this contributes none (the reference's bwa
    keeps an irreproducible sample of 5000 of them instead).  chunk_bytes: genome text per scan chunk (None: 64 MiB of a text
    that is uploaded, all of a resident one)."""
    partdata = [(partid, list(part)) for partid, part in partstream]
    kevlar_amd.plog('[kevlar::localize]', 'loaded {} read partitions into memory'.format(len(partdata)))
    contigs = [contig for partid, part in partdata for contig in part]
    kevlar_amd.plog('[kevlar::localize]', 'decomposing contigs into seeds of length {}'.format(seedsize))
    with SeedSet([contig.sequence for contig in contigs], seedsize) as seedset:
        # the reference reports the index of the last seed, one less than their number (0 when there is none)
        kevlar_amd.plog('[kevlar::localize]', 'contigs decomposed into {} seeds'.format(max(seedset.n_distinct - 1, 0)))
        kevlar_amd.plog('[kevlar::localize] computing seed matches')
        genome = load_genome(refrfile)
        matches = SeedMatches(seedset, genome, max_occ=max_occ, chunk_bytes=chunk_bytes)
    kevlar_amd.plog('[kevlar::localize]', 'found positions for {} seeds'.format(len(matches)))
    if len(matches) == 0:
        kevlar_amd.plog('[kevlar::localize]', 'WARNING: no reference matches')
        return
    kevlar_amd.plog('[kevlar::localize]', 'loading reference sequences into memory')
    # a resident genome hands out slices that are fetched later, all cutouts of the call in one gather (DeviceGenome.resolve)
    pending = [] if genome.on_device else None
    refrseqs = genome.seqdict(pending) if genome.on_device else genome.seqdict()          # (the scan read them already)
    kevlar_amd.plog('[kevlar::localize]', 'computing the reference target sequence for each partition')
    progress = kevlar_amd.ProgressIndicator('[kevlar::localize]     computed targets for {counter} partitions',
                                            interval=100, breaks=[1000, 10000, 100000])

    def targets():
        contig_at = 0
        for partid, part in partdata:
            progress.update()
            windows = np.arange(seedset.wpre[contig_at], seedset.wpre[contig_at + len(part)])
            contig_at += len(part)
            rows = matches.of_windows(windows)
            localizer = Localizer(seedsize, incl=inclpattern, excl=exclpattern)
            for which, position in zip(matches.seqidx[rows].tolist(), matches.local[rows].tolist()):
                localizer.add_seed_match(genome.ids[which], position)
            clusterdist = maxdiff
            if clusterdist is None:
                clusterdist = 3 * max(len(contig.sequence) for contig in part)
            for gdna in localizer.get_cutouts(refrseqs=refrseqs, delta=delta, clusterdist=clusterdist):
                yield partid, gdna

    ncutouts = 0
    if genome.on_device:
        found = list(targets())
        genome.resolve(pending)
        genome.close()
        for partid, gdna in found:
            if isinstance(gdna.sequence, _PendingSlice):
                gdna.sequence = gdna.sequence.value
        found = iter(found)
    else:
        found = targets()
    for partid, gdna in found:
        ncutouts += 1
        yield partid, gdna
    if ncutouts == 0:
        kevlar_amd.plog('[kevlar::localize]', 'WARNING: no reference matches')


def main(args):
    contigstream = kevlar_amd.seqio.afxstream(args.contigs)
    if args.part_id:
        pstream = kevlar_amd.parse_single_partition(contigstream, args.part_id)
    else:
        pstream = kevlar_amd.parse_partitioned_reads(contigstream)
    outstream = kevlar_amd.open(args.out, 'w')
    targets = localize(pstream, args.refr, seedsize=args.seed_size, delta=args.delta, maxdiff=args.max_diff,
                       inclpattern=args.include, exclpattern=args.exclude,
                       max_occ=getattr(args, 'max_occ', DEFAULT_MAX_OCC))
    for partid, gdna in targets:
        seqname = gdna.defline
        if partid is not None:
            seqname += ' kvcc={}'.format(partid)
        kevlar_amd.sequence.write_record(kevlar_amd.sequence.Record(name=seqname, sequence=gdna.sequence), outstream)
    if args.out not in ('-', None):
        outstream.close()
