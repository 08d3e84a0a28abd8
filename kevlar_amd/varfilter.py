"""`kevlar varfilter` (the reference's kevlar/varfilter.py and kevlar/cli/varfilter.py): calls that overlap a region of a BED file
get the `UserFilter`.

The reference keeps the calls in an interval tree per chromosome and looks every BED line up in it, one Python iteration per line.
Here the calls become an index on the device (sorted by chromosome and start, kv_varfilter.hip) and the BED text is scanned against
it: varfilter_files() hands the text itself to the device, chunk by chunk, where the lines are parsed and joined in one kernel;
varfilter() takes regions that are already parsed, as the reference's function of that name does, packs them into arrays and runs
the same join.  The grammar of a BED line, the overlap rule and the differences to Python's text-mode reading: DESIGN.md section 14.

Order of the output.  The reference yields the calls in the order of a Python set, which is arbitrary.  Here: chromosomes in the
order of their first appearance among the calls, the calls of a chromosome in input order.  A call whose position is `.` cannot
be indexed (the reference raises TypeError on it): it is passed through unflagged, after all others.

`load_predictions` is not ported: it returns the reference's IntervalForest, which does not exist here.

Also a command of its own, `python -m kevlar_amd.varfilter` (the flags of the reference's `kevlar varfilter`)."""
import argparse
import ctypes
import gzip
import sys

import numpy as np

import kevlar_amd
from kevlar_amd import _lib
from kevlar_amd.vcf import VariantFilter, VCFWriter, vcfstream

DEFAULT_CHUNK_BYTES = 256 << 20
REGION_BATCH = 1 << 20
NO_CHROM = 0xFFFFFFFF
NO_OFFSET = 0xFFFFFFFFFFFFFFFF
STATS = ('lines', 'skipped', 'regions', 'known', 'overlaps', 'flagged')


def _ptr(array):
    return ctypes.c_void_p(array.ctypes.data)


def _name_bytes(name):
    return name.encode('utf-8', 'surrogateescape') if isinstance(name, str) else bytes(name)


class CallIndex(object):
    """The calls on the device: regions (chromosome, start, end), 0-based half-open, as `Variant.region` gives them; a chromosome
    name is a str or bytes."""

    def __init__(self, regions):
        self._handle = None
        _lib.require_device()
        self._lib = _lib.load()
        self._ids = {}                                      # chromosome name, as bytes -> id, in order of first appearance
        for chrom, _, _ in regions:
            self._ids.setdefault(_name_bytes(chrom), len(self._ids))
        encoded = list(self._ids)
        blob = np.frombuffer(b''.join(encoded) or b'\0', dtype=np.uint8)
        offsets = np.zeros(len(encoded) + 1, dtype=np.uint64)
        np.cumsum([len(name) for name in encoded], out=offsets[1:])
        self.n_calls = len(regions)
        chrom = np.array([self._ids[_name_bytes(region[0])] for region in regions], dtype=np.uint32)
        start = np.array([region[1] for region in regions], dtype=np.int64)
        end = np.array([region[2] for region in regions], dtype=np.int64)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.kv_varfilter_create(_ptr(blob), _ptr(offsets), len(encoded), _ptr(chrom), _ptr(start), _ptr(end), self.n_calls,
                                                 ctypes.byref(handle)))
        self._handle = handle

    def chrom_id(self, name):
        """the id the join knows a chromosome by (str or bytes), NO_CHROM when no call is on it"""
        return self._ids.get(_name_bytes(name), NO_CHROM)

    def scan(self, text, text_offset=0):
        """One chunk of BED text (bytes, or a uint8 array) that ends at a line end or with the file.  A line outside the grammar
        raises ValueError; bad_line() then says where it begins."""
        view = text if isinstance(text, np.ndarray) else np.frombuffer(text, dtype=np.uint8)
        rc = self._lib.kv_varfilter_scan(self._handle, _ptr(view) if len(view) else None, len(view), text_offset)
        _lib.check(rc)

    def bad_line(self):
        """file offset of the first line of the last scan that is outside the grammar, None when there was none"""
        offset = ctypes.c_uint64()
        _lib.check(self._lib.kv_varfilter_bad_line(self._handle, ctypes.byref(offset)))
        return None if offset.value == NO_OFFSET else offset.value

    def regions(self, chrom_ids, starts, ends):
        chrom_ids = np.ascontiguousarray(chrom_ids, dtype=np.uint32)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        ends = np.ascontiguousarray(ends, dtype=np.int64)
        if not len(chrom_ids) == len(starts) == len(ends):
            raise ValueError('regions: {} chromosome ids, {} starts, {} ends'.format(len(chrom_ids), len(starts), len(ends)))
        _lib.check(self._lib.kv_varfilter_regions(self._handle, _ptr(chrom_ids), _ptr(starts), _ptr(ends), len(chrom_ids)))

    def hits(self):
        """one flag per call, in the order the calls were given"""
        flags = np.zeros(self.n_calls, dtype=np.uint8)
        _lib.check(self._lib.kv_varfilter_hits(self._handle, _ptr(flags), self.n_calls))
        return flags

    def stats(self):
        values = np.zeros(len(STATS), dtype=np.uint64)
        _lib.check(self._lib.kv_varfilter_stats(self._handle, _ptr(values)))
        return dict(zip(STATS, (int(value) for value in values)))

    def close(self):
        if self._handle is not None:
            self._lib.kv_varfilter_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def _load_calls(callstream):
    """(indexed calls grouped by chromosome in order of first appearance, calls without a position)"""
    kevlar_amd.plog('[kevlar::varfilter] Loading predictions to filter')
    by_chrom, unplaced = {}, []
    for call in callstream:
        if isinstance(call.position, int):
            by_chrom.setdefault(call.seqid, []).append(call)
        else:
            unplaced.append(call)
    return [call for calls in by_chrom.values() for call in calls], unplaced


def _filtered(calls, unplaced, index):
    for call, hit in zip(calls, index.hits()):
        if hit:
            call.filter(VariantFilter.UserFilter)
        yield call
    for call in unplaced:
        yield call


def varfilter(callstream, maskstream):
    """Every call of `callstream`, those that overlap a region of `maskstream` carrying the UserFilter.  `maskstream` yields
    (chromosome, start, end, data) as parse_bed does.  Order of the output: see the module's text."""
    calls, unplaced = _load_calls(callstream)
    with CallIndex([call.region for call in calls]) as index:
        kevlar_amd.plog('[kevlar::varfilter]', 'Filtering preliminary variant calls')
        chroms, starts, ends = [], [], []
        for chrom, start, end, _ in maskstream:
            chroms.append(index.chrom_id(chrom))
            starts.append(start)
            ends.append(end)
            if len(chroms) == REGION_BATCH:
                index.regions(chroms, starts, ends)
                chroms, starts, ends = [], [], []
        index.regions(chroms, starts, ends)
        for call in _filtered(calls, unplaced, index):
            yield call


def _inflate(image):
    """the text of a gzip file image: the device inflaters (blocked gzip, then one deflate stream), Python's gzip for what they
    leave to the host"""
    lib = _lib.load()
    total, members = ctypes.c_uint64(), ctypes.c_uint64()
    if lib.kv_bgzf_text_size(image, len(image), ctypes.byref(total), ctypes.byref(members)) == _lib.KV_OK:
        out = np.empty(total.value + 1, dtype=np.uint8)
        ms = ctypes.c_double()
        _lib.check(lib.kv_bgzf_inflate_host(image, len(image), _ptr(out), total.value, ctypes.byref(ms)))
        return out[:total.value]
    size = int.from_bytes(image[-4:], 'little') if len(image) >= 18 else 0      # ISIZE: the text's length mod 2^32, of the last member
    out = np.empty(size + 64, dtype=np.uint8)
    n, ms, stats = ctypes.c_uint64(), ctypes.c_double(), (ctypes.c_uint64 * 4)()
    rc = lib.kv_gunzip_host(image, len(image), _ptr(out), size + 64, 0, ctypes.byref(n), stats, ctypes.byref(ms))
    if rc in (_lib.KV_ERR_TYPE, _lib.KV_ERR_CAPACITY):          # not for the device; or several members, or more than 4 GiB of text
        return np.frombuffer(gzip.decompress(image), dtype=np.uint8)
    _lib.check(rc)
    return out[:n.value]


def _chunks(path, chunk_bytes):
    """the chunks of a BED file (plain or gzip; `-`: standard input): arrays of bytes that end at a line end, or with the file"""
    lib = _lib.load()
    cut = ctypes.c_uint64()

    def cut_of(buffer, at_eof):
        _lib.check(lib.kv_varfilter_chunk_cut(_ptr(buffer) if len(buffer) else None, len(buffer), int(at_eof), ctypes.byref(cut)))
        return cut.value

    if path in ('-', None) or path.endswith('.gz'):
        image = sys.stdin.buffer.read() if path in ('-', None) else open(path, 'rb').read()
        text = _inflate(image) if path not in ('-', None) else np.frombuffer(image, dtype=np.uint8)
        at = 0
        while at < len(text):
            want = chunk_bytes
            while True:                                     # a line longer than a chunk grows the chunk
                piece = text[at:at + want]
                at_eof = at + len(piece) == len(text)
                n = cut_of(piece, at_eof)
                if n:
                    break
                want *= 2
            yield piece[:n]
            at += n
        return
    with open(path, 'rb') as stream:
        held = b''
        while True:
            data = stream.read(chunk_bytes)
            buffer = np.frombuffer(held + data, dtype=np.uint8)
            n = cut_of(buffer, not data)
            if n:
                yield buffer[:n]
            held = buffer[n:].tobytes()
            if not data:
                return


def _raise_bad_line(path, index, chunk, chunk_offset, lines_before):
    offset = index.bad_line()
    if offset is None:
        return
    at = offset - chunk_offset
    raw = chunk.tobytes()
    number = lines_before + raw.count(b'\n', 0, at) + 1
    end = raw.find(b'\n', at)
    line = raw[at:end if end >= 0 else len(raw)]
    raise ValueError('{}, line {}: not "chromosome start end" with integer coordinates: {!r}'.format(
        path, number, line[:200].decode('utf-8', 'replace')))


def varfilter_files(callstream, bedfiles, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """varfilter() for BED files (plain or gzip), the fast path: the device parses the text.  Plain files are read `chunk_bytes`
    at a time, cut behind the last line end; a line longer than a chunk grows the chunk.  A line outside the grammar raises
    ValueError with its 1-based number."""
    if chunk_bytes < 1:
        raise ValueError('chunk_bytes must be positive')
    calls, unplaced = _load_calls(callstream)
    with CallIndex([call.region for call in calls]) as index:
        kevlar_amd.plog('[kevlar::varfilter]', 'Filtering preliminary variant calls')
        for path in bedfiles:
            offset = lines = 0
            for chunk in _chunks(path, chunk_bytes):
                try:
                    index.scan(chunk, offset)
                except _lib.KvArgError:
                    _raise_bad_line(path, index, chunk, offset, lines)
                    raise
                offset += len(chunk)
                lines += int(np.count_nonzero(chunk == 10))
        for call in _filtered(calls, unplaced, index):
            yield call


def parser():
    """the reference's `kevlar varfilter` flags (kevlar/cli/varfilter.py)"""
    parser = argparse.ArgumentParser(
        prog='python -m kevlar_amd.varfilter', description='Filter out variants falling in the genomic regions specified by the BED '
        'file(s). This can be used to exclude putative variant calls corresponding to common variants, segmental duplications, or '
        'other problematic loci.')
    parser.add_argument('-o', '--out', metavar='FILE', help='file to which filtered variants will be written; default is terminal '
                        '(standard output)')
    parser.add_argument('filt', help='BED file containing regions to filter out')
    parser.add_argument('vcf', nargs='+', help='VCF file(s) with calls to filter')
    return parser


def main(args):
    reader = vcfstream(args.vcf)
    outstream = kevlar_amd.open(args.out, 'w')
    writer = VCFWriter(outstream, source='kevlar::varfilter')
    writer.write_header()
    for call in varfilter_files(reader, [args.filt]):
        writer.write(call)
    if outstream is not sys.stdout:
        outstream.close()


if __name__ == '__main__':
    main(parser().parse_args())
