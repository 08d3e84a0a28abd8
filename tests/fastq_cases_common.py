"""A byte-level statement of four-line FASTQ and the table of files that hold the device parser (kevlar_amd/csrc/kv_fastq.hip) and
the host parser (kv_fastx.hip) to it at their edges: a newline on either side of every boundary of the two line kernels, dense and
sparse lines, every way for a file to end, the bytes the vectorised newline test could mistake, and the cut between two stretches
moved across every byte of a record.  No GPU, no HIP: tests/test_fastq_cases_reference.py checks the reference and the table here,
tests/test_gpu_fastq_cases.py runs the table on the device."""
import functools
import gzip
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_fastq.hip')
KINDS = ('name', 'sequence', 'plus', 'quality')
MAX_FILE = 256 << 10
ONE_BATCH = 100000


def constants():
    """what the edges are computed from, read out of kv_fastq.hip: the chunk and workgroup of the line kernels, the first guess of
    a record's size and the budget rule of a stretch (FqBatch), and the smallest file the device opens"""
    text = open(SRC).read()
    out = {}
    for name in ('FQ_CHUNK', 'FQ_THREADS'):
        out[name] = int(re.search(r'#define\s+{}\s+(\d+)u?\b'.format(name), text).group(1))
    out['per_read'] = float(re.search(r'd->bytes_per_read\s*:\s*([0-9.]+)\s*;', text).group(1))
    margin, slack = re.search(r'max_reads\s*\*\s*per_read\s*\*\s*([0-9.]+)\)\s*\+\s*(\d+)\s*,\s*text_cap', text).groups()
    out['margin'], out['slack'] = float(margin), int(slack)
    out['min_file'] = int(re.search(r'sb\.st_size\s*<\s*(\d+)', text).group(1))
    out['min_fresh'] = int(re.search(r'b\.want\s*-\s*d->carry_len\s*:\s*(\d+)\s*\)', text).group(1))     # of an uncompressed file, behind a carry
    return out


C = constants()


def first_stretch(max_reads):
    """bytes of an uncompressed file that the device takes for its first batch (fq_select with nothing carried)"""
    return int(max_reads * C['per_read'] * C['margin']) + C['slack']


# ---- the reference
def parse_fastx(data):
    """[(name, sequence, quality)] of four-line FASTQ, all bytes: lines end in \\n (the last may lack it) and lose one trailing \\r;
    lines of blanks, tabs and \\r between records are skipped; '@' opens a record of four lines, of which those the file ends
    before are empty"""
    lines = data.split(b'\n')
    if lines[-1] == b'':
        lines.pop()                                     # nothing stands behind the last newline
    lines = [line[:-1] if line.endswith(b'\r') else line for line in lines]
    out, at = [], 0
    while at < len(lines):
        if not lines[at].strip(b' \t\r'):
            at += 1
            continue
        if lines[at][:1] != b'@':
            raise ValueError('line {} opens no record'.format(at))
        rest = lines[at + 1:at + 4] + [b''] * 3
        out.append((lines[at][1:], rest[0], rest[2]))
        at += 4
    return out


_CODE = np.zeros(256, dtype=np.uint32)
for _i, (_u, _l) in enumerate(zip(b'ACGT', b'acgt')):
    _CODE[_u] = _CODE[_l] = _i
_SHIFT = 2 * np.arange(16, dtype=np.uint32)


def pack_words(seqs):
    """the words of a batch: every read starts on a word, base j in bits 2 (j mod 16), ACGT and acgt as 0..3, any other byte as 0;
    a read without bases takes no word"""
    out = []
    for s in seqs:
        codes = np.zeros((len(s) + 15) // 16 * 16, dtype=np.uint32)
        codes[:len(s)] = _CODE[np.frombuffer(s, dtype=np.uint8)]
        out.append((codes.reshape(-1, 16) << _SHIFT).sum(axis=1, dtype=np.uint32))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)


def flagged(seqs):
    """indices of the reads that hold a byte which is not an upper-case A, C, G or T"""
    return [i for i, s in enumerate(seqs) if s.strip(b'ACGT')]


def num_kmers(seqs, k):
    return sum(max(0, len(s) - k + 1) for s in seqs)


# ---- building files
def text_of(recs, eol=b'\n'):
    """records (name, sequence, what follows '+', quality) as a file"""
    return b''.join(b'@' + n + eol + s + eol + b'+' + p + eol + q + eol for n, s, p, q in recs)


def _bases(rng, n):
    return np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def _quals(rng, n):
    return rng.integers(33, 74, size=n, dtype=np.uint8).tobytes()


def short_records(total, seed, lo=1, hi=60):
    """seeded records of `lo` to `hi` bases and short names until they fill `total` bytes; the first eight are tiny (eleven bytes),
    so that every kind of line ends within the first sixteen bytes"""
    rng = np.random.default_rng(seed)
    recs, size = [], 0
    while size < total:
        i = len(recs)
        n = 2 if i < 8 else int(rng.integers(lo, hi + 1))
        name = b'abcdefgh'[i:i + 1] if i < 8 else 'r{:x}'.format(i).encode()
        recs.append((name, _bases(rng, n), b'', _quals(rng, n)))
        size += len(name) + 2 * n + 6
    return recs


def line_ends(recs, eol=b'\n'):
    """offset of the \\n that ends each line: [record][kind]"""
    out, at = [], 0
    for n, s, p, q in recs:
        row = []
        for size in (1 + len(n), len(s), 1 + len(p), len(q)):
            at += size + len(eol)
            row.append(at - 1)
        out.append(row)
    return out


def with_newline_at(offset, line_kind, total=None, seed=0):
    """a file of short records in which the \\n that ends a line of that kind sits at byte `offset`: the last record whose line of
    the kind ends at or before it has its name padded by the difference"""
    total = total or 4 * C['FQ_CHUNK'] + 4500
    recs = short_records(total, seed)
    col = KINDS.index(line_kind)
    ends = [row[col] for row in line_ends(recs)]
    r = max(i for i, e in enumerate(ends) if e <= offset)
    n, s, p, q = recs[r]
    recs[r] = (n + b'x' * (offset - ends[r]), s, p, q)
    return text_of(recs)


def sized(total, final_newline, seed):
    """short records that make a file of exactly `total` bytes, with or without the \\n behind its last line"""
    body = total + (0 if final_newline else 1)
    recs = short_records(body - 200, seed)
    while len(text_of(recs)) > body:
        recs.pop()
    n, s, p, q = recs[-1]
    recs[-1] = (n + b'y' * (body - len(text_of(recs))), s, p, q)
    data = text_of(recs)
    return data if final_newline else data[:-1]


def write_as(data, container, path):
    """write `data` as the container says: as it is, as blocked gzip (BGZF), or as one gzip stream"""
    if container == 'plain':
        with open(path, 'wb') as fh:
            fh.write(data)
    elif container == 'bgzf':
        from kevlar_amd import bgzf
        bgzf.write_file(path, data)
    else:
        with open(path, 'wb') as fh:
            fh.write(gzip.compress(data, compresslevel=6, mtime=0))
    return path


def write_case(folder, data, container):
    return write_as(data, container, os.path.join(str(folder), 'reads.fq' if container == 'plain' else 'reads.fq.gz'))


# ---- the table
ALL3 = ('plain', 'bgzf', 'gzip')
PLAIN = ('plain',)

# (a case's route holds for each of its containers: on the MI355X the device gunzip takes every one of these streams, small as they are)


def boundaries():
    return [16, 16 * 64, 16 * C['FQ_THREADS'], C['FQ_CHUNK'], 2 * C['FQ_CHUNK'], 3 * C['FQ_CHUNK']]


@functools.lru_cache(maxsize=None)
def group_a():
    """a line end two and one bytes in front of, on and one byte behind every boundary of the line kernels; the kind of line cycles
    so that every boundary meets all four"""
    out = []
    for bi, b in enumerate(boundaries()):
        for di, delta in enumerate((-2, -1, 0, 1)):
            kind = KINDS[(bi + di) % 4]
            data = with_newline_at(b + delta, kind, seed=100 + 4 * bi + di)
            containers = ALL3 if b % C['FQ_CHUNK'] == 0 else PLAIN
            out.append(('A_at{}{:+d}_{}'.format(b, delta, kind), data, ONE_BATCH, containers, 'device'))
    return out


DENSE_BASES = (1, 15, 16, 17, 31, 32, 33)


def dense(n, eol, some_bases):
    """n records without bases, @a / empty / + / empty; eight in every hundred have no name either, which puts ten newlines into
    sixteen bytes.  some_bases: every 50th record carries 1, 15, 16, 17, 31, 32 or 33 of them"""
    rng = np.random.default_rng(7)
    recs = []
    for i in range(n):
        m = DENSE_BASES[(i // 50) % len(DENSE_BASES)] if some_bases and i % 50 == 25 else 0
        recs.append((b'' if 50 <= i % 100 < 58 else b'a', _bases(rng, m), b'', _quals(rng, m)))
    return text_of(recs, eol)


def one_long(n_bases, n_qual, at, seed, n_records):
    """short records with one long read as record `at`"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n_records):
        n = int(rng.integers(20, 61))
        recs.append(('s{}'.format(i).encode(), _bases(rng, n), b'', _quals(rng, n)))
    recs[at] = (b'long', _bases(rng, n_bases), b'', _quals(rng, n_qual))
    return text_of(recs)


def group_b():
    out = [('B_dense', dense(10000, b'\n', False), ONE_BATCH, ALL3, 'device'),
           ('B_dense_crlf', dense(10000, b'\r\n', False), ONE_BATCH, ALL3, 'device'),
           ('B_dense_some_bases', dense(10000, b'\n', True), ONE_BATCH, ALL3, 'device'),
           # (chunks of the long lines hold no newline)
           ('B_long40k', one_long(40000, 40000, 150, 11, 300), ONE_BATCH, ('plain', 'bgzf'), 'device'),
           # the first stretch of a batch of one read holds no whole record: the reader asks again with twice the budget.  (The long
           # read's quality line is short: the file stays within MAX_FILE)
           ('B_long150k_first', one_long(150000, 64, 0, 12, 40), 1, ('plain', 'bgzf'), 'device'),
           # behind one short record the read is cut by the first stretch and still not whole with the next: asked again with a carry
           ('B_long150k_second', one_long(150000, 64, 1, 14, 40), 1, ('plain', 'bgzf'), 'device'),
           # (further back it is whole by the time its batch comes: every batch of one short read takes min_fresh bytes more)
           ('B_long150k_20th', one_long(150000, 64, 19, 13, 40), 1, ('plain', 'bgzf'), 'device')]
    return out


def tails():
    """(label, what follows the last quality line, batch size or None for one batch, route)"""
    rng = np.random.default_rng(5)
    blanks = b''.join((b'\n', b' \n', b'\t\n', b'\r\n', b' \t \r\n', b'  \n')[i] for i in rng.integers(0, 6, size=4000))[:4999] + b'\n'
    assert len(blanks) == 5000
    return [('nl', b'\n', None, 'device'), ('nlnl', b'\n\n', None, 'device'), ('crlf_blank', b'\n\r\n \n', None, 'device'),
            # four blank lines look like a fifth record to the device: it serves the batches in front of them, then the host
            ('four_blank', b'\n' + 4 * b'\n', 'most', 'handover'),
            ('blanks5000', b'\n' + blanks, None, 'any')]


def group_c():
    out = []
    m = 4
    for delta in (-1, 0, 1):
        for final_newline in (True, False):
            total = m * C['FQ_CHUNK'] + delta
            out.append(('C_size{}{:+d}_{}'.format(m * C['FQ_CHUNK'], delta, 'nl' if final_newline else 'cut'),
                        sized(total, final_newline, 200 + delta + 3 * final_newline), ONE_BATCH, PLAIN, 'device'))
    for rest in (0, 1, 15):                       # the last vector of the text: whole, one byte, fifteen bytes
        total = m * C['FQ_CHUNK'] + 16 * (C['FQ_THREADS'] // 2 + 3) + rest
        out.append(('C_size_mod16_{}'.format(rest), sized(total, True, 210 + rest), ONE_BATCH, PLAIN, 'device'))
    body = text_of(short_records(4 * C['FQ_CHUNK'], 220))
    n_body = len(parse_fastx(body))
    for label, tail, batch, route in tails():
        out.append(('C_tail_' + label, body[:-1] + tail, n_body - 100 if batch == 'most' else ONE_BATCH, ALL3, route))
    # a file that stops inside its last record: the device serves the whole records, the host the cut one
    last = (b'last', b'ACGTACGTAC', b'', b'IIIIIIIIII')
    for label, keep in (('name', 1), ('sequence', 2), ('plus', 3)):
        cut = b'\n'.join((b'@' + last[0], last[1], b'+' + last[2])[:keep]) + b'\n'
        out.append(('C_stops_after_' + label, body + cut, ONE_BATCH, PLAIN, 'handover'))
    one = b'@read1\nACGTACGT\n+\nIIIIIIII\n'
    assert len(one) == C['min_file'] - 1
    out.append(('C_one_record_{}'.format(len(one)), one, ONE_BATCH, PLAIN, 'any'))                # below what the device opens
    out.append(('C_one_record_{}'.format(len(one) + 1), one.replace(b'read1', b'read12'), ONE_BATCH, PLAIN, 'device'))
    return out


def group_d():
    out = []
    base = short_records(4 * C['FQ_CHUNK'], 300, lo=5)

    def edited(fn, eol=b'\n', every=3):
        rng = np.random.default_rng(301)
        return text_of([fn(rng, *rec) if i % every == 0 else rec for i, rec in enumerate(base)], eol)

    def names_of(alphabet):
        letters = np.frombuffer(alphabet, dtype=np.uint8)
        return lambda rng, n, s, p, q: (letters[rng.integers(0, len(letters), size=int(rng.integers(1, 24)))].tobytes(), s, p, q)
    # bytes one bit, or the high bit, away from \n: what a vectorised comparison with 0x0a could take for one
    out.append(('D_names_near_newline', edited(names_of(b'\x0b\x1a\x2aAz'), every=2), ONE_BATCH, PLAIN, 'device'))
    out.append(('D_names_high_bytes', edited(names_of(b'\x8a\xff\x0b\x1a\x2a'), every=2), ONE_BATCH, PLAIN, 'device'))
    out.append(('D_quality_starts_at_or_plus', edited(lambda rng, n, s, p, q: (n, s, p, (b'@', b'+')[int(rng.integers(0, 2))] + q[1:])),
                ONE_BATCH, PLAIN, 'device'))
    out.append(('D_plus_repeats_name', edited(lambda rng, n, s, p, q: (n, s, n, q), every=1), ONE_BATCH, PLAIN, 'device'))
    letters = np.frombuffer(b'ACGTacgtnNRYKMSWBDHV.-', dtype=np.uint8)
    out.append(('D_sequence_alphabet', edited(lambda rng, n, s, p, q: (n, letters[rng.integers(0, len(letters), size=len(s))].tobytes(), p, q)),
                ONE_BATCH, PLAIN, 'device'))
    out.append(('D_crlf', text_of(base, b'\r\n'), ONE_BATCH, PLAIN, 'device'))
    out.append(('D_cr_on_sequence_only', edited(lambda rng, n, s, p, q: (n, s + b'\r', p, q), every=1), ONE_BATCH, PLAIN, 'device'))
    out.append(('D_sequence_just_cr', edited(lambda rng, n, s, p, q: (n, b'\r', p, b'')), ONE_BATCH, PLAIN, 'device'))
    for _, data, _, _, _ in out:
        assert b'\0' not in data
    return out


E_BATCH = 512
E_NAME, E_BASES = 5, 21
E_L = (1 + E_NAME + 1) + (E_BASES + 1) + 2 + (E_BASES + 1)           # bytes of a record: 53


@functools.lru_cache(maxsize=None)
def _e_records(length=E_L):
    """records of one length that fill the first stretch of a batch of E_BATCH and 36 KB more (at `length` bytes a record with its
    line ends): the file takes two stretches"""
    rng = np.random.default_rng(400)
    n = (first_stretch(E_BATCH) + 36000) // length + 1
    return tuple(('{:05d}'.format(i).encode(), _bases(rng, E_BASES), b'', _quals(rng, E_BASES)) for i in range(n))


def e_file(p, eol=b'\n'):
    """the first record's name padded by p bytes: the cut behind the first stretch falls p bytes earlier in its record"""
    recs = list(_e_records(E_L + 4 * (len(eol) - 1)))
    n, s, q_plus, q = recs[0]
    recs[0] = (n + b'p' * p, s, q_plus, q)
    return text_of(recs, eol)


def e_crlf_pads():
    """(label, p) of eight CRLF files: the cut between \\r and \\n of each of the four lines, right in front of the \\r and right
    behind the \\n of the name line and of the quality line"""
    cut = first_stretch(E_BATCH)
    length = E_L + 4
    newline = line_ends([_e_records()[0]], b'\r\n')[0]             # offset of each line's \n in an unpadded record
    out = []
    for col, kind in enumerate(KINDS):
        out.append(('between_' + kind, (cut - newline[col]) % length))                  # the \n is the first byte behind the cut
    for col in (0, 3):
        out.append(('before_cr_' + KINDS[col], (cut - (newline[col] - 1)) % length))    # the \r is
        out.append(('behind_nl_' + KINDS[col], (cut - (newline[col] + 1)) % length))    # the \n is the last byte in front of it
    return out


def group_e():
    out = []
    for p in range(E_L):
        containers = ALL3 if p == 0 else ('plain', 'bgzf') if p in (E_L // 2, E_L - 1) else PLAIN
        out.append(('E_cut_p{:02d}'.format(p), e_file(p), E_BATCH, containers, 'device'))
    for label, p in e_crlf_pads():
        out.append(('E_crlf_' + label, e_file(p, b'\r\n'), E_BATCH, PLAIN, 'device'))
    rng = np.random.default_rng(401)
    recs = [('carry{}'.format(i).encode(), _bases(rng, 118 + i % 5), b'', _quals(rng, 118 + i % 5)) for i in range(300)]
    out.append(('E_300_batches_of_one', text_of(recs), 1, PLAIN, 'device'))
    name, data = group_a()[13][:2]                  # (a line end right in front of the chunk boundary)
    for batch in (4, 5, 64):                         # the last line a batch may take ends inside a vector, more newlines behind it
        out.append(('E_batch{}_{}'.format(batch, name), data, batch, PLAIN, 'device'))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, data, max_reads, containers, route)] in a fixed order"""
    return tuple(group_a() + group_b() + group_c() + group_d() + group_e())


def e_sweep():
    """names of the p-sweep of group E: one test runs fifteen or so of them"""
    return [case[0] for case in cases() if case[0].startswith('E_cut_p')]


def e_crlf():
    return [case[0] for case in cases() if case[0].startswith('E_crlf_')]


def single_file_params():
    """(case name, container) of everything that is one file per test"""
    grouped = set(e_sweep()) | set(e_crlf())
    return [(case[0], container) for case in cases() for container in case[3] if not (case[0] in grouped and container == 'plain')]


@functools.lru_cache(maxsize=None)
def by_name():
    return {case[0]: case for case in cases()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case's records by the reference"""
    return tuple(parse_fastx(by_name()[name][1]))
