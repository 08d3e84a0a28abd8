"""What the tests of the two device inflaters share (tests/test_deflate_streams.py on the host, tests/test_gpu_deflate.py on
the device): an assembler for DEFLATE streams (RFC 1951) that writes what zlib's compressor never does -- any code lengths,
any spelling of them, any length / distance symbol with any extra bits, empty blocks, codes zlib's inflate refuses -- the
text a list of tokens means (computed here, without zlib), gzip and BGZF framing, and the catalogue of named streams the
tests run.  Not a test module and not a conftest: nothing here is collected.  Nothing of kevlar_amd is imported.

A token is a literal byte (int), a match (length, distance) -- the helper picks the symbols and the extra bits --, or the raw
form (length symbol, its extra bits, distance symbol, its extra bits), which reaches the encodings the helper would not choose
(258 as symbol 284 with extra 31) and the symbols that do not exist (286, 287; distance 30, 31).

CASES: (name, raw deflate bytes, expected) with expected the text (bytes) or, for a stream zlib's inflate refuses, its
message (str).  The name starts with the catalogue group ('tables', 'deep', 'headers', 'runs', 'distsets', 'empty', 'stored',
'refill', 'copies', 'far', 'chains', 'false', 'rejected').  IMAGES: the same for whole gzip files (several members, header
fields), expected the text or None for a file that must be an error.  zlib_space(): (name, raw, text) of the part of zlib's own
space gzip.compress() does not reach.  LENIENT[name]: for a refused stream, the text a decoder that missed the fault would
produce -- the trailers the tests put behind such a stream announce THAT text, so neither CRC-32 nor ISIZE catches what the
decoder itself has to."""
import functools
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """bits go out LSB first; a Huffman code is sent from its most significant bit (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        assert 0 <= value < (1 << count)
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def tell(self):
        return len(self.out) * 8 + self.n

    def copy(self):
        other = BitWriter()
        other.out, other.acc, other.n = bytearray(self.out), self.acc, self.n
        return other

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b'')


def canonical(lengths):
    """{symbol: (code with its bits already reversed for BitWriter.bits, length)} of RFC 1951 3.2.2; no check of the lengths:
    the refused cases need over-subscribed and incomplete sets spelled out too"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, first = 0, [0] * 17
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        first[l] = code
    codes = {}
    for sym, l in enumerate(lengths):
        if l:
            c = first[l] & ((1 << l) - 1)          # (an over-subscribed set runs out of codes: wrap, the stream is refused anyway)
            first[l] += 1
            codes[sym] = (int(format(c, '0{}b'.format(l))[::-1], 2), l)
    return codes


def complete(size, used):
    """`size` code lengths, zero except for the symbols `used`, which share a complete code of near-equal lengths (the first
    ones get the shorter codes); a single symbol gets length 1"""
    used = list(used)
    n = len(used)
    out = [0] * size
    if n == 1:
        out[used[0]] = 1
        return out
    k = n.bit_length() - 1
    r = n - (1 << k)
    for i, sym in enumerate(used):
        out[sym] = k if i < n - 2 * r else k + 1
    return out


def staircase(size, used):
    """lengths 1, 2, ..., 14, 15, 15 for the 16 symbols `used`, in that order: the deepest complete code there is"""
    used = list(used)
    assert len(used) == 16
    out = [0] * size
    for i, sym in enumerate(used):
        out[sym] = min(i + 1, 15)
    return out


def split(token):
    """a token -> None for a literal, else (length symbol, extra bits, distance symbol, extra bits)"""
    if isinstance(token, int):
        return None
    if len(token) == 4:
        return token
    length, dist = token
    assert 3 <= length <= 258 and 1 <= dist <= 32768
    ls = 28 if length == 258 else max(s for s in range(28) if LEN_BASE[s] <= length)
    ds = max(s for s in range(30) if DIST_BASE[s] <= dist)
    return (257 + ls, length - LEN_BASE[ls], ds, dist - DIST_BASE[ds])


def expand(tokens, text=b''):
    """the text a list of tokens means, behind `text`"""
    out = bytearray(text)
    for token in tokens:
        m = split(token)
        if m is None:
            out.append(token)
            continue
        length = LEN_BASE[m[0] - 257] + m[1]
        dist = DIST_BASE[m[2]] + m[3]
        assert dist <= len(out), 'a match in front of the text'
        at = len(out) - dist
        if dist >= length:
            out += out[at:at + length]
        else:
            for j in range(length):
                out.append(out[at + j])
    return bytes(out[len(text):]) if text else bytes(out)


def _symbols(w, tokens, ll, dist, eob=True):
    for token in tokens:
        m = split(token)
        if m is None:
            w.bits(*ll[token])
            continue
        w.bits(*ll[m[0]])
        if m[0] - 257 < 29:
            w.bits(m[1], LEN_EXTRA[m[0] - 257])
        w.bits(*dist[m[2]])
        if m[2] < 30:
            w.bits(m[3], DIST_EXTRA[m[2]])
    if eob:
        w.bits(*ll[256])


def stored(w, data, final, nlen=None):
    assert len(data) <= 65535
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack('<HH', len(data), (len(data) ^ 0xffff) if nlen is None else nlen))
    w.raw(data)


def fixed(w, tokens, final, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    _symbols(w, tokens, canonical(FIXED_LL), canonical(FIXED_DIST), eob)


def plain_spelling(lengths):
    return [(l,) for l in lengths]


def run_spelling(lengths):
    """the code-length sequence with the longest runs 16 / 17 / 18 can carry, greedily"""
    out, i = [], 0
    while i < len(lengths):
        v = lengths[i]
        run = 1
        while i + run < len(lengths) and lengths[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            take = min(run, 138)
            out.append((18, take - 11))
        elif v == 0 and run >= 3:
            take = run
            out.append((17, take - 3))
        elif v != 0 and run >= 4:
            take = min(run - 1, 6) + 1
            out += [(v,), (16, take - 1 - 3)]
        else:
            take = 1
            out.append((v,))
        i += take
    return out


def dynamic(w, tokens, ll_lengths, dist_lengths, final, precode_lengths=None, clen_symbols=None, eob=True, hlit=None, hdist=None):
    """a dynamic-Huffman block.  HLIT / HDIST are the lengths of the two lists (hlit / hdist: announce other counts than that);
    clen_symbols spells the code-length sequence itself: (length,), (16, extra), (17, extra), (18, extra); the default sends
    each length plainly.  precode_lengths: the 19 lengths of the code-length code (default: a complete code over the symbols
    the spelling uses); HCLEN is what they need, from 4 to 19."""
    spelling = clen_symbols if clen_symbols is not None else plain_spelling(list(ll_lengths) + list(dist_lengths))
    if precode_lengths is None:
        used = sorted({s[0] for s in spelling})
        if len(used) == 1:
            used.append(0 if used[0] != 0 else 1)      # the code-length code must be complete: a second symbol nobody sends
        precode_lengths = complete(19, used)
    assert len(precode_lengths) == 19
    hclen = max([4] + [i + 1 for i, s in enumerate(CLEN_ORDER) if precode_lengths[s]])
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits((len(ll_lengths) if hlit is None else hlit) - 257, 5)
    w.bits((len(dist_lengths) if hdist is None else hdist) - 1, 5)
    w.bits(hclen - 4, 4)
    for s in CLEN_ORDER[:hclen]:
        w.bits(precode_lengths[s], 3)
    pre = canonical(precode_lengths)
    for s in spelling:
        w.bits(*pre[s[0]])
        if s[0] >= 16:
            w.bits(s[1], {16: 2, 17: 3, 18: 7}[s[0]])
    _symbols(w, tokens, canonical(ll_lengths), canonical(dist_lengths), eob)


def gzip_member(raw, text, flags=0):
    """a gzip member around raw deflate data: header (FEXTRA 4, FNAME 8, FCOMMENT 16, FHCRC 2 as `flags` asks), CRC-32 and
    ISIZE of `text`"""
    head = b'\x1f\x8b\x08' + bytes([flags]) + b'\x00\x00\x00\x00\x00\x03'
    if flags & 4:
        head += b'\x05\x00hello'
    if flags & 8:
        head += b'a name\x00'
    if flags & 16:
        head += b'a comment\x00'
    if flags & 2:
        head += struct.pack('<H', zlib.crc32(head) & 0xffff)
    return head + raw + struct.pack('<II', zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff)


BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def fits_bgzf(raw, text):
    return len(raw) + 26 <= 65536 and len(text) <= 65536


def bgzf_member(raw, text):
    """a BGZF member: the 'BC' extra field holds the member's size - 1"""
    assert fits_bgzf(raw, text)
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', len(raw) + 25) + raw +
            struct.pack('<II', zlib.crc32(text) & 0xffffffff, len(text)))


def reference(raw):
    """zlib's inflate on raw deflate data: the text, which must end exactly with the data; raises zlib.error"""
    z = zlib.decompressobj(-15)
    text = z.decompress(raw)
    assert z.eof and not z.unused_data, 'the stream does not end with its data'
    return text


# ---------------------------------------------------------------- the catalogue
def _noise(seed, n, lo=0, hi=256):
    return bytes(np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8))


def fastq_like(seed, n_reads, read_len=100):
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, (n_reads, read_len))]
    quals = rng.integers(33, 74, (n_reads, read_len), dtype=np.uint8)
    out = []
    for i in range(n_reads):
        out.append(b'@read%d/1 sample=proband\n%s\n+\n%s\n' % (i, bases[i].tobytes(), quals[i].tobytes()))
    return b''.join(out)


ALL_LL = complete(286, range(286))             # every literal / length symbol, 8 and 9 bits
ALL_DIST = complete(30, range(30))             # every distance symbol, 4 and 5 bits


def _tables():
    """group 1: every length symbol with every distance symbol, extra bits all 0 and all 1, behind 32 768 random literals;
    one stream with all 1 740 matches, and one per length symbol that fits a BGZF member"""
    prefix = _noise(101, 32768)
    head = BitWriter()
    # (the block of every case begins alike: written once)
    dynamic(head, list(prefix), ALL_LL, ALL_DIST, False, clen_symbols=run_spelling(ALL_LL + ALL_DIST), eob=False)
    ll, dist = canonical(ALL_LL), canonical(ALL_DIST)

    def matches(ls):
        return [(257 + ls, x * ((1 << LEN_EXTRA[ls]) - 1), ds, x * ((1 << DIST_EXTRA[ds]) - 1)) for ds in range(30) for x in (0, 1)]

    cases = []
    for ls in [None] + list(range(29)):
        tokens = [m for s in range(29) for m in matches(s)] if ls is None else matches(ls)
        w = head.copy()
        _symbols(w, tokens, ll, dist)
        fixed(w, [], True)
        cases.append(('tables: ' + ('all 1740 matches' if ls is None else 'length symbol {}'.format(257 + ls)), w.getvalue(),
                      expand(list(prefix) + tokens)))
    w = BitWriter()
    tokens = list(b'abc') + [(285, 0, 0, 0), ord('d'), (284, 31, 0, 0), ord('e'), (284, 30, 1, 0), (258, 3)]
    dynamic(w, tokens, ALL_LL, ALL_DIST, True)
    cases.append(('tables: 258 as symbol 285 and as symbol 284 + 31', w.getvalue(), expand(tokens)))
    return cases


def _deep():
    """group 3: the staircase 1, 2, ..., 14, 15, 15 over the literal/length symbols (end-of-block and the length symbol among
    the 15s, then among the short ones), over 16 distance symbols, and 1 ... 6, 7, 7 over the code-length code"""
    cases = []
    rng = np.random.default_rng(103)
    lits = list(range(65, 79))                                      # 14 literals
    for name, order in (('end-of-block and the length symbol deepest', lits + [256, 264]), ('literals deepest', [256, 264] + lits)):
        ll = staircase(265, order)
        tokens = []
        for _ in range(6):
            tokens += lits + [int(x) for x in rng.choice(lits, 20)] + [(264, 0, int(rng.integers(0, 4)), 0)]
        w = BitWriter()
        for last in (False, True):                                   # twice: the end-of-block code is decoded and another block follows
            dynamic(w, tokens, ll, [2, 2, 2, 2], last)
        cases.append(('deep: literal/length staircase, ' + name, w.getvalue(), expand(tokens + tokens)))
    dsyms = [int(x) for x in rng.permutation(16)]                  # distance symbols 0 .. 15 (distances 1 .. 256), any of them deepest
    prefix = list(_noise(104, 300, 97, 123))
    tokens = prefix[:]
    for rep in range(3):
        for ds in dsyms:
            tokens += [(int(rng.integers(3, 40)), DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds]))), int(rng.integers(97, 123))]
    w = BitWriter()
    dynamic(w, tokens, complete(286, list(range(97, 123)) + list(range(256, 286))), staircase(16, dsyms), True)
    cases.append(('deep: distance staircase', w.getvalue(), expand(tokens)))
    # the code-length code: 8 of its symbols, lengths 1 .. 6, 7, 7; the lengths it spells are 0, 1, 7, 8, 9 and the three runs
    ll = [0] * 286
    unused = {3, 4, 5, 100} | set(range(200, 212))                 # zeros for 17, a plain 0 and 18 to carry
    for i, sym in enumerate(s for s in range(286) if s not in unused):
        ll[sym] = 7 if i < 60 else 8 if i < 122 else 9             # 60 / 2^7 + 62 / 2^8 + 148 / 2^9 = 1
    pre = [0] * 19
    for l, sym in zip((1, 2, 3, 4, 5, 6, 7, 7), (9, 8, 7, 16, 18, 17, 0, 1)):
        pre[sym] = l
    text = [b for b in _noise(105, 600) if ll[b]]
    tokens = text + [(258, 1), (100, 2)] + text[:50]
    w = BitWriter()
    dynamic(w, tokens, ll, [1, 1], True, precode_lengths=pre, clen_symbols=run_spelling(ll + [1, 1]))
    cases.append(('deep: code-length code 1 2 3 4 5 6 7 7', w.getvalue(), expand(tokens)))
    return cases


def _headers():
    """group 4: HLIT 286 / HDIST 30 / HCLEN 19 with every symbol of all three codes in use; HLIT 257 / HDIST 1 with the fewest
    code-length codes that can spell an end-of-block code at all (HCLEN 5; with HCLEN 4 only zeros can be sent: refused)"""
    cases = []
    text = list(_noise(106, 700))
    tokens = text + [(3, 1), (258, 700), (17, 33)]
    w = BitWriter()
    dynamic(w, tokens, ALL_LL, ALL_DIST, True, precode_lengths=complete(19, range(19)))
    cases.append(('headers: widest, 286 / 30 / 19', w.getvalue(), expand(tokens)))
    ll = [8] * 255 + [0, 8]                                        # 256 codes of 8 bits: bytes 0 .. 254 and end-of-block
    pre = [0] * 19
    pre[0] = pre[8] = 1
    text = [b for b in _noise(107, 500) if b != 255]
    w = BitWriter()
    dynamic(w, text, ll, [0], True, precode_lengths=pre)
    cases.append(('headers: narrowest, 257 / 1 / 5', w.getvalue(), bytes(text)))
    return cases


def _runs():
    """group 5: the code-length runs.  Behind a block that leaves every length non-zero: 18 of 65, five chained 16s, 18 of 138,
    18 of 11, 17 of 10, 17 of 3, and a 16 that starts in the literal/length lengths and ends in the distance lengths"""
    ll = [0] * 259
    for sym in list(range(65, 94)) + [256, 257, 258]:
        ll[sym] = 5                                                # 32 codes of 5 bits
    dist = [5] * 28 + [4, 4]
    spelling = [(18, 65 - 11), (5,), (16, 3), (16, 3), (16, 3), (16, 3), (16, 1),          # 65 zeros, 1 + 6 + 6 + 6 + 6 + 4 = 29 fives
                (18, 138 - 11), (18, 0), (17, 7), (17, 0),                                  # 138 + 11 + 10 + 3 = 162 zeros
                (5,), (16, 3),                                                              # 256, then 257, 258 and distance symbols 0 .. 3
                (16, 3), (16, 3), (16, 3), (16, 3), (4,), (4,)]                             # distance symbols 4 .. 27, 28, 29
    text = list(_noise(108, 400, 65, 94))
    tokens = text + [(4, 1), (3, 300), (4, 400)]
    first = list(_noise(109, 100))
    w = BitWriter()
    dynamic(w, first, ALL_LL, ALL_DIST, False)
    dynamic(w, tokens, ll, dist, True, clen_symbols=spelling)
    return [('runs: 16 across the two sets, 18 of 138 and 11, 17 of 10 and 3, chained 16s', w.getvalue(), expand(first + tokens))]


def _distsets():
    """group 6, accepted: one distance code of length 1 on symbol 0 and on another symbol; no distance code at all"""
    cases = []
    lits = list(range(97, 123))
    ll = complete(286, lits + [256] + list(range(257, 286)))
    text = list(_noise(110, 200, 97, 123))
    for name, dist, tokens in (('symbol 0', [1], text + [(5, 1), 97, (258, 1)]), ('symbol 9', [0] * 9 + [1], text + [(5, 25), 97, (258, 32), 98, (9, 28)]),
                               ('none, literals only', [0], text)):
        w = BitWriter()
        dynamic(w, tokens, ll, dist, True)
        cases.append(('distsets: ' + ('one code of length 1 on ' if dist != [0] else '') + name, w.getvalue(), expand(tokens)))
    return cases


EOB_ONLY = [0] * 256 + [1]                     # the one code of an empty dynamic block: end-of-block, length 1


def _empty():
    """group 7: empty stored, fixed and dynamic blocks between blocks of text and as the last block"""
    cases = []
    text = _noise(111, 64, 97, 123)
    two = complete(257, [97, 256])
    for name, last in (('a stored block of length 0', 'stored'), ('an empty fixed block', 'fixed'), ('an empty dynamic block', 'dynamic')):
        w = BitWriter()
        fixed(w, list(text[:7]), False)
        stored(w, b'', False)
        dynamic(w, list(text[7:20]), ALL_LL, ALL_DIST, False)
        for _ in range(3):
            stored(w, b'', False)
        fixed(w, list(text[20:33]), False)
        fixed(w, [], False)                                          # 10 bits
        stored(w, text[33:40], False)
        for i in range(5):
            dynamic(w, [], EOB_ONLY if i % 2 == 0 else two, [0], False)
        dynamic(w, list(text[40:]) + [(30, 64)], ALL_LL, ALL_DIST, False)
        if last == 'stored':
            stored(w, b'', True)
        elif last == 'fixed':
            fixed(w, [], True)
        else:
            dynamic(w, [], EOB_ONLY, [0], True)
        cases.append(('empty: blocks without text of all three kinds, the last one ' + name, w.getvalue(), text + text[:30]))
    return cases


def _stored():
    """group 8: stored blocks of 1 byte, of 65 535, the longest a BGZF member holds, and one behind a fixed-Huffman block that
    ends on each of the 8 bit positions of a byte (a 9-bit literal moves the end by one)"""
    cases = []
    w = BitWriter()
    stored(w, b'x', True)
    cases.append(('stored: 1 byte', w.getvalue(), b'x'))
    for name, n in (('65535 bytes', 65535), ('65505 bytes, the longest in a BGZF member', 65505)):
        data = _noise(112, n)
        w = BitWriter()
        stored(w, data, True)
        cases.append(('stored: ' + name, w.getvalue(), data))
    w = BitWriter()
    text = bytearray()
    phases = set()
    for nine in range(8):
        lits = [65 + nine] * 3 + [200 + nine] * nine
        fixed(w, lits, False)
        phases.add(w.tell() % 8)
        data = _noise(113 + nine, 5 + nine, 97, 123)
        stored(w, data, nine == 7)
        text += bytes(lits) + data
    assert len(phases) == 8
    cases.append(('stored: behind Huffman blocks that end on each bit of a byte', w.getvalue(), bytes(text)))
    return cases


def _refill():
    """group 9: a Huffman block whose end-of-block code ends on each of the 32 bits of a word, another block behind it (where
    the words lie depends on the bytes in front of the stream: all 32, so that every framing meets bit 0, 1, 15, 16, 30, 31)"""
    w = BitWriter()
    text = bytearray()
    for r in range(32):
        n = 0
        while (w.tell() + 10 + 8 * 4 + 9 * n) % 32 != r:
            n += 1
        lits = [66 + r % 20] * 4 + [180 + r] * n
        fixed(w, lits, False)
        assert w.tell() % 32 == r
        text += bytes(lits)
    tokens = [ord('z')] * 3 + [(40, 3)]
    dynamic(w, tokens, ALL_LL, ALL_DIST, True)
    return [('refill: end-of-block on every bit of a 32-bit word', w.getvalue(), bytes(text) + expand(tokens))]


def _copies():
    """group 10: matches on either side of the decoders' 1 K LDS ring (a source nearer than 1024 - 258 comes from the ring, a
    farther one from the text in HBM), overlapping matches of every small period, distance = length and length - 1"""
    rng = np.random.default_rng(121)
    tokens = list(_noise(122, 1100))
    pairs = [(l, d) for d in (766, 767, 768, 1023, 1024) for l in (3, 63, 64, 65, 258)]
    pairs += [(258, d) for d in (1, 2, 3, 63, 64, 65)]
    pairs += [(l, l) for l in (3, 64, 65, 258)] + [(l, l - 1) for l in (3, 64, 65, 258)]
    for l, d in pairs:
        tokens += [(l, d)] + [int(x) for x in rng.integers(0, 256, int(rng.integers(1, 4)))]
    w = BitWriter()
    dynamic(w, tokens, ALL_LL, ALL_DIST, True)
    return [('copies: either side of the ring, overlaps, distance = length', w.getvalue(), expand(tokens))]


def _far():
    """group 11: distance 32 768 at the first position where it is legal"""
    tokens = list(_noise(123, 32768)) + [(3, 32768), (258, 32768), 7, (258, 32768)]
    w = BitWriter()
    dynamic(w, tokens, ALL_LL, ALL_DIST, True)
    return [('far: distance 32768 at position 32768', w.getvalue(), expand(tokens))]


def _chains():
    """group 12: 32 768 random bytes in blocks of about 1 KB, then 64 blocks of nothing but matches of length 258 at distance
    32 768 (128 of them: a stretch that starts at such a block ends with a tail of 32 768 markers), then 64 more with distances
    drawn from 16 385 .. 32 768 (markers that name markers)"""
    rng = np.random.default_rng(124)
    data = _noise(125, 32768)
    w = BitWriter()
    tokens = []
    for at in range(0, 32768, 1000):
        dynamic(w, list(data[at:at + 1000]), ALL_LL, ALL_DIST, False)
    tokens += list(data)
    ll = [0] * 286
    ll[256] = ll[285] = 1
    for _ in range(64):
        block = [(285, 0, 29, 8191)] * 128
        dynamic(w, block, ll, [0] * 29 + [1], False, clen_symbols=run_spelling(ll + [0] * 29 + [1]))
        tokens += block
    for _ in range(64):
        block = [(258, int(d)) for d in rng.integers(16385, 32769, 128)]
        dynamic(w, block, ll, [0] * 28 + [1, 1], False, clen_symbols=run_spelling(ll + [0] * 28 + [1, 1]))
        tokens += block
    fixed(w, list(b'end'), True)
    return [('chains: tails of nothing but markers', w.getvalue(), expand(tokens) + b'end')]


def _false():
    """group 13: stored blocks full of genuine block headers that are not blocks of this stream"""
    inner_text = fastq_like(126, 2500)
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    inner = z.compress(inner_text) + z.flush()
    z = zlib.compressobj(0, zlib.DEFLATED, -15)
    cases = [('false: a deflate stream inside stored blocks', z.compress(inner) + z.flush(), inner)]
    # six copies of a real (non-final) dynamic block inside one stored block, then real blocks: more false starts than a chunk
    # keeps, in front of a true one
    block = BitWriter()
    dynamic(block, list(_noise(127, 300)), ALL_LL, ALL_DIST, False)
    block.align()
    payload = block.getvalue() * 6
    w = BitWriter()
    stored(w, payload, False)
    text = bytearray(payload)
    for i in range(3):
        part = _noise(128 + i, 800)
        dynamic(w, list(part), ALL_LL, ALL_DIST, i == 2)
        text += part
    cases.append(('false: six false starts in front of a true one', w.getvalue(), bytes(text)))
    return cases


def _rejected():
    """groups 5 and 6, refused: (name, raw, zlib's message); LENIENT[name] is filled as they are made"""
    cases = []
    lits = list(range(97, 123))
    text = list(_noise(131, 60, 97, 123))
    good_ll = complete(286, lits + [256] + list(range(257, 286)))

    def add(name, w, message, lenient=b''):
        cases.append(('rejected: ' + name, w.getvalue(), message))
        LENIENT['rejected: ' + name] = bytes(lenient)

    def block(name, message, tokens, ll, dist, lenient=None, **how):
        w = BitWriter()
        dynamic(w, tokens, ll, dist, True, **how)
        add(name, w, message, expand(tokens) if lenient is None else lenient)

    # -- the code-length sequence
    spelling = run_spelling(good_ll + [1])
    block('16 as the first code-length symbol', 'invalid bit length repeat', text, good_ll, [1], precode_lengths=complete(19, [0, 1, 5, 6, 16, 17, 18]),
          clen_symbols=[(16, 0)] + spelling[1:])
    block('a run past HLIT + HDIST', 'invalid bit length repeat', text, good_ll, [1], precode_lengths=complete(19, [0, 1, 5, 6, 16, 17, 18]),
          clen_symbols=run_spelling(good_ll) + [(17, 0)])
    # -- the sets
    block('a single distance code of length 2', 'invalid distances set', text + [(5, 1)], good_ll, [2])
    ll = complete(286, lits + [256] + list(range(257, 286)))
    ll[285] = 0                                                    # one code taken away: incomplete
    block('an incomplete literal/length set', 'invalid literal/lengths set', text, ll, [1])
    ll = [0] * 257
    ll[97] = ll[256] = 2
    block('two literal/length codes of length 2', 'invalid literal/lengths set', [97] * 9, ll, [0])
    block('distance codes of lengths 2 2 2', 'invalid distances set', text + [(5, 1)], good_ll, [2, 2, 2])
    ll = list(good_ll)
    ll[0] = 1
    block('an over-subscribed literal/length set', 'invalid literal/lengths set', text, ll, [1], lenient=b'')
    block('an over-subscribed distance set', 'invalid distances set', text, good_ll, [1, 1, 1], lenient=b'')
    pre = complete(19, [0, 1, 5, 6, 7])
    pre[7] = 0                                                     # nobody sends a 7: the rest still decodes
    block('an incomplete code-length code', 'invalid code lengths set', text, good_ll, [1], precode_lengths=pre)
    pre = complete(19, [0, 1, 5, 6])
    pre[7] = 1
    block('an over-subscribed code-length code', 'invalid code lengths set', text, good_ll, [1], precode_lengths=pre, lenient=b'')
    pre = [0] * 19
    pre[5] = 1
    block('a code-length code of one code', 'invalid code lengths set', [], [5] * 257, [5], precode_lengths=pre, lenient=b'')
    ll = complete(256, range(256))
    block('no end-of-block code', 'invalid code -- missing end-of-block', text, ll + [0], [1], eob=False, lenient=b'')
    pre = [0] * 19
    pre[0] = pre[18] = 1
    block('HCLEN 4: only zeros can be spelled', 'invalid code -- missing end-of-block', [], [0] * 257, [0], precode_lengths=pre, eob=False,
          clen_symbols=[(18, 127), (18, 120 - 11)], lenient=b'')
    w = BitWriter()
    dynamic(w, text, good_ll, [0], True, eob=False)
    w.bits(*canonical(good_ll)[260])                               # a length symbol, and no code a distance could have
    w.bits(0, 16)
    add('a match in a block without distance codes', w, 'invalid distance code', bytes(text))
    w = BitWriter()
    dynamic(w, text, good_ll, [1], True, eob=False)
    w.bits(*canonical(good_ll)[260])
    w.bits(1, 1)                                                   # the unused half of a one-code distance set
    w.bits(0, 16)
    add('the unused code of a one-code distance set', w, 'invalid distance code', bytes(text))
    for name, hlit, hdist in (('HLIT 287', 287, 1), ('HDIST 31', 257, 31)):
        w = BitWriter()
        dynamic(w, [], [0] * 257, [0], True, eob=False, hlit=hlit, hdist=hdist)
        add(name, w, 'too many length or distance symbols')
    # -- symbols that do not exist, in a fixed block
    for ds in (30, 31):
        w = BitWriter()
        fixed(w, text + [(260, 0, ds, 0)] + [0, 0], True)
        add('distance symbol {} in a fixed block'.format(ds), w, 'invalid distance code', bytes(text))
    for sym in (286, 287):
        w = BitWriter()
        fixed(w, text + [(sym, 0, 0, 0)] + [0, 0], True)
        add('length symbol {} in a fixed block'.format(sym), w, 'invalid literal/length code', bytes(text))
    # -- blocks
    w = BitWriter()
    fixed(w, text, False)
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 32)
    add('BTYPE 3', w, 'invalid block type', bytes(text))
    w = BitWriter()
    fixed(w, text, False)
    stored(w, b'stored text', True, nlen=len(b'stored text') ^ 0xfffe)
    add('a stored block whose LEN and NLEN disagree', w, 'invalid stored block lengths', bytes(text) + b'stored text')
    # -- distances in front of the text: a lenient decoder reads zeros there
    # (the largest distance DEFLATE can say is 32 768 -- symbol 29, extra bits all 1 --, so the case at the far end is that
    # distance one byte too early)
    data = _noise(132, 32767)
    w = BitWriter()
    dynamic(w, list(data) + [(10, 32768), 65], ALL_LL, ALL_DIST, True)
    add('distance 32768 at position 32767', w, 'invalid distance too far back', data + b'\x00' + data[:9] + b'A')
    w = BitWriter()
    fixed(w, [66, (5, 2), 67], True)
    add('distance 2 at position 1', w, 'invalid distance too far back', b'B\x00B\x00B\x00C')
    return cases


LENIENT = {}


def _build_cases():
    out = []
    for make in (_tables, _deep, _headers, _runs, _distsets, _empty, _stored, _refill, _copies, _far, _chains, _false, _rejected):
        out += make()
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _build_cases()
GROUPS = ['tables', 'deep', 'headers', 'runs', 'distsets', 'empty', 'stored', 'refill', 'copies', 'far', 'chains', 'false']


def group(name):
    return [c for c in CASES if c[0].startswith(name + ':')]


def _build_images():
    """group 14 and the rest of 13: whole gzip files"""
    images = []
    parts = [_noise(140 + i % 7, 100, 65, 91) for i in range(300)]
    members = []
    for i, part in enumerate(parts):
        w = BitWriter()
        if i % 3 == 0:
            fixed(w, list(part), True)
        elif i % 3 == 1:
            dynamic(w, list(part), ALL_LL, ALL_DIST, True)
        else:
            stored(w, part, True)
        members.append(gzip_member(w.getvalue(), part))
    text = b''.join(parts)
    images.append(('members: 300 of 100 bytes', b''.join(members), text))
    bad = list(members)
    bad[150] = bad[150][:-4] + struct.pack('<I', 101)
    images.append(('members: 300 of 100 bytes, one ISIZE altered', b''.join(bad), None))
    flagged = list(members[:40])
    flagged[20] = gzip_member(members[20][10:-8], parts[20], flags=4 | 8 | 16 | 2)
    images.append(('members: FEXTRA + FNAME + FCOMMENT + FHCRC in the middle of the file', b''.join(flagged), b''.join(parts[:40])))
    name, raw, inner = group('false')[0]
    more = _noise(150, 3000)
    w = BitWriter()
    dynamic(w, list(more), ALL_LL, ALL_DIST, True)
    images.append(('false: a deflate stream inside stored blocks, then a member of one dynamic block', gzip_member(raw, inner) + gzip_member(w.getvalue(), more),
                   inner + more))
    return images


IMAGES = _build_images()

STRATEGIES = {'default': zlib.Z_DEFAULT_STRATEGY, 'filtered': zlib.Z_FILTERED, 'huffman': zlib.Z_HUFFMAN_ONLY, 'rle': zlib.Z_RLE, 'fixed': zlib.Z_FIXED}


@functools.lru_cache(maxsize=None)
def zlib_space(strategy):
    """group 15: one strategy of zlib's compressor x memLevel {1, 9} x flushes {none, Z_SYNC_FLUSH every 1 000 bytes, Z_FULL_FLUSH
    every 65 536} x three inputs of about 300 KB (FASTQ-like, runs, periodic with period 40 000)"""
    rng = np.random.default_rng(160)
    runs = np.repeat(rng.integers(65, 70, 3000, dtype=np.uint8), rng.integers(1, 200, 3000))[:300000].tobytes()
    inputs = {'fastq': fastq_like(161, 1200), 'runs': runs, 'periodic': (_noise(162, 40000, 97, 123) * 8)[:300000]}
    out = []
    for kind, data in inputs.items():
        for mem in (1, 9):
            for flush, step in (('none', len(data)), ('sync', 1000), ('full', 65536)):
                z = zlib.compressobj(6, zlib.DEFLATED, -15, mem, STRATEGIES[strategy])
                raw = []
                for at in range(0, len(data), step):
                    raw.append(z.compress(data[at:at + step]))
                    if at + step < len(data):
                        raw.append(z.flush(zlib.Z_SYNC_FLUSH if flush == 'sync' else zlib.Z_FULL_FLUSH))
                raw.append(z.flush())
                out.append(('zlib: {} {} memLevel {} flush {}'.format(strategy, kind, mem, flush), b''.join(raw), data))
    return out
