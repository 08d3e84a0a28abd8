"""What `kevlar varfilter` must compute, in plain Python and numpy, for tests/test_varfilter_reference.py and
tests/test_gpu_varfilter.py: the grammar of a BED line restated on bytes (the reference's kevlar.parse_bed: kevlar/__init__.py:131-140),
the overlap of every region with every call (intervaltree >= 3.0.2, which the reference pins), the counters the device keeps, and
the generators of the inputs.  Nothing here imports the product."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
BED_SINGLE = os.path.join(GOLDEN, 'assemble', 'fiveparts-ignore-single.bed')
BED_TWO = os.path.join(GOLDEN, 'assemble', 'fiveparts-ignore.bed')
BED_INTERVALS = os.path.join(GOLDEN, 'varfilter', 'intervals.bed')
BED_SEGDUPS = os.path.join(GOLDEN, 'varfilter', 'hg38.segdups.sample.bed.gz')
VCF_FIVE = os.path.join(GOLDEN, 'call', 'five-snvs-with-likelihood.vcf.gz')
VCF_LOW_ABUND = os.path.join(GOLDEN, 'simlike', 'case-low-abund', 'calls.vcf.gz')

SEPARATORS = bytes(range(0x09, 0x0e)) + bytes(range(0x1c, 0x21))
_SPLIT = re.compile(b'[' + re.escape(SEPARATORS) + b']+')
_NUMBER = re.compile(b'[+-]?[0-9]+')
NO_CHROM = 0xFFFFFFFF
STATS = ('lines', 'skipped', 'regions', 'known', 'overlaps', 'flagged')


class BadLine(ValueError):
    """a line outside the grammar: its 1-based number and its byte offset in the text"""

    def __init__(self, number, offset, line):
        super(BadLine, self).__init__('line {} (byte {}): {!r}'.format(number, offset, line[:80]))
        self.number, self.offset, self.line = number, offset, line


def number(token):
    """[+-]?[0-9]+ within int64, or None"""
    if _NUMBER.fullmatch(token) is None:
        return None
    value = int(token)
    return value if -2 ** 63 <= value < 2 ** 63 else None


def lines_of(text):
    """(offset, line) of every line: lines end at b'\\n' alone, a last line needs none"""
    at = 0
    for line in text.split(b'\n'):
        if at < len(text):
            yield at, line
        at += len(line) + 1


def parse_text(text):
    """(regions, counters) of a BED text: regions = [(chromosome bytes, start, end)] in file order, counters = lines seen and
    lines skipped.  Raises BadLine for the FIRST line in file order that has fewer than three tokens or a token that is no number."""
    regions, n_lines, n_skipped = [], 0, 0
    for number_of_line, (offset, line) in enumerate(lines_of(text), 1):
        n_lines += 1
        if line.startswith(b'#'):           # before stripping: b' #x' is no comment
            n_skipped += 1
            continue
        line_stripped = line.strip(SEPARATORS)
        if line_stripped == b'':
            n_skipped += 1
            continue
        tokens = _SPLIT.split(line_stripped)
        if len(tokens) < 3:
            raise BadLine(number_of_line, offset, line)
        start, end = number(tokens[1]), number(tokens[2])
        if start is None or end is None:
            raise BadLine(number_of_line, offset, line)
        regions.append((tokens[0], start, end))
    return regions, {'lines': n_lines, 'skipped': n_skipped}


def overlaps(region, call):
    """a region (s, e) hits a call (a, b): an empty or inverted region hits nothing"""
    (s, e), (a, b) = region, call
    return s < e and a < e and b > s


def brute_force(calls, regions):
    """calls: [(chromosome bytes, start, end)], regions likewise (or chromosome None: not among the calls' names).
    Every region against every call of its chromosome, as integer arrays.  -> (flags per call, the device's counters but the two
    of the text)."""
    flags = np.zeros(len(calls), dtype=np.uint8)
    by_chrom = {}
    for number_of_call, (chrom, _, _) in enumerate(calls):
        by_chrom.setdefault(chrom, []).append(number_of_call)
    n_known = n_overlaps = 0
    regions_by_chrom = {}
    for chrom, start, end in regions:
        if chrom in by_chrom:
            n_known += 1
            regions_by_chrom.setdefault(chrom, []).append((start, end))
    for chrom, found in regions_by_chrom.items():
        members = np.array(by_chrom[chrom])
        a = np.array([calls[i][1] for i in members], dtype=np.int64)
        b = np.array([calls[i][2] for i in members], dtype=a.dtype)
        for first in range(0, len(found), 4096):
            s = np.array([r[0] for r in found[first:first + 4096]], dtype=a.dtype)[:, None]
            e = np.array([r[1] for r in found[first:first + 4096]], dtype=a.dtype)[:, None]
            hit = (s < e) & (a[None, :] < e) & (b[None, :] > s)
            n_overlaps += int(hit.sum())
            flags[members[hit.any(axis=0)]] = 1
    return flags, {'regions': len(regions), 'known': n_known, 'overlaps': n_overlaps, 'flagged': int(flags.sum())}


def expected(calls, text):
    """(flags, all six counters) of a text against calls, or raises BadLine"""
    regions, counters = parse_text(text)
    flags, more = brute_force(calls, regions)
    counters.update(more)
    return flags, counters


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def chrom_names(rng, n):
    """n distinct names, some of them prefixes of others"""
    pool = ['chr{}'.format(i) for i in range(1, 23)] + ['chrX', 'chrY', 'chrM', '1', '2', '10', '11', 'X', 'chr1_KI270706v1_random', 'scaffold_{}'.format(10 ** 6)]
    names = list(rng.choice(pool, size=min(n, len(pool)), replace=False))
    while len(names) < n:
        names.append('ctg{}'.format(len(names)))
    return [name.encode() for name in names]


def fuzz_case(seed):
    """(calls, regions, text): 1-2000 calls on 1-40 chromosomes with lengths 1-10000, 0-20000 BED lines drawn around the calls --
    just in front of one, just behind one, across one, far away, on a chromosome without calls, empty and inverted -- and the
    text that spells them, with the separators, comments, blank lines and extra columns a BED file may have."""
    rng = np.random.default_rng(seed)
    n_chroms = int(rng.integers(1, 41))
    names = chrom_names(rng, n_chroms)
    n_calls = int(rng.integers(1, 2001)) if seed % 7 else int(rng.integers(1, 20))
    span = int(rng.choice([2000, 100000, 10 ** 7, 2 ** 33]))
    call_chrom = rng.integers(0, n_chroms, size=n_calls)
    call_start = rng.integers(0, span, size=n_calls)
    call_len = np.where(rng.random(n_calls) < 0.9, rng.integers(1, 40, size=n_calls), rng.integers(1, 10001, size=n_calls))
    calls = [(names[c], int(s), int(s + l)) for c, s, l in zip(call_chrom, call_start, call_len)]
    n_lines = int(rng.integers(0, 20001)) if seed % 5 else int(rng.integers(0, 50))
    kinds = rng.integers(0, 8, size=n_lines)
    picks = rng.integers(0, n_calls, size=n_lines)
    jitter = rng.integers(-3, 4, size=(n_lines, 2))
    lengths = rng.integers(0, 3000, size=n_lines)
    far = rng.integers(-span // 10, span + span // 10 + 1, size=n_lines)
    others = [b'chrUn', names[0] + b'x', names[0][:-1] or b'c', names[0].upper() if names[0].upper() != names[0] else names[0].lower()]
    others = [name for name in others if name not in names]
    regions = []
    for kind, pick, (j0, j1), length, where in zip(kinds.tolist(), picks.tolist(), jitter.tolist(), lengths.tolist(), far.tolist()):
        chrom, a, b = calls[pick]
        if kind == 0:
            region = (chrom, a - length, a + j1)            # ends around the call's start
        elif kind == 1:
            region = (chrom, b + j0, b + length)            # starts around the call's end
        elif kind == 2:
            region = (chrom, a + j0, b + j1)                # the call itself, a base more or less
        elif kind == 3:
            region = (chrom, where, where + length)         # anywhere
        elif kind == 4:
            region = (others[pick % len(others)] if others else chrom, a, b)
        elif kind == 5:
            region = (chrom, a + j0, a + j0 + min(length, 2) - 1)      # empty, inverted or a base or two
        elif kind == 6:
            region = (names[pick % n_chroms], a - length, b + length)  # maybe another chromosome, same coordinates
        else:
            region = (chrom, b - 1, b + j1)                 # the call's last base
        regions.append(region)
    return calls, regions, spell(rng, regions)


def spell(rng, regions, final_newline=None):
    """a BED text of the regions: tabs mostly, sometimes spaces, mixtures, surrounding separators, CRLF, signs, leading zeros,
    extra columns; comments and blank lines in between"""
    style = rng.integers(0, 16, size=len(regions)).tolist()
    extras = rng.integers(0, 40, size=len(regions)).tolist()
    out = []
    for (chrom, start, end), how, extra in zip(regions, style, extras):
        s, e = b'%d' % start, b'%d' % end
        if how == 0:
            line = chrom + b' ' + s + b' ' + e
        elif how == 1:
            line = b' \t' + chrom + b'\t \t' + s + b' ' + e + b'\t '
        elif how == 2:
            line = chrom + b'\t' + s + b'\t' + e + b'\r'
        elif how == 3:
            line = chrom + b'\t' + (b'+' + s if start >= 0 else s) + b'\t' + (b'00' + e if end >= 0 else e)
        elif how == 4:
            line = chrom + b'\t' + s + b'\t' + e + b'\tname%d\t0\t+' % extra
        elif how == 5:
            line = chrom + b'\x1c' + s + b'\x0b\x0c' + e + b'\x1f#not a comment'
        else:
            line = chrom + b'\t' + s + b'\t' + e
        out.append(line)
        if extra == 0:
            out.append(b'# a comment\tchr1\t1\t2')
        elif extra == 1:
            out.append(b'')
        elif extra == 2:
            out.append(b' \t \r')
    text = b'\n'.join(out)
    if final_newline is None:
        final_newline = bool(rng.integers(0, 2))
    return text + b'\n' if out and final_newline else text


def region_arrays(names, regions):
    """(chromosome ids, starts, ends) of regions for kv_varfilter_regions; names: the distinct chromosomes of the calls, in id order"""
    ids = {name: number_of_name for number_of_name, name in enumerate(names)}
    return (np.array([ids.get(r[0], NO_CHROM) for r in regions], dtype=np.uint32), np.array([r[1] for r in regions], dtype=np.int64),
            np.array([r[2] for r in regions], dtype=np.int64))


def distinct(calls):
    """the calls' chromosomes in order of first appearance"""
    return list(dict.fromkeys(call[0] for call in calls))


def cut_lines(text, lines_per_chunk):
    """the text cut into chunks of so many lines (the last one shorter): each ends at a line end, or with the text"""
    pieces, at, count = [], 0, 0
    for offset, line in lines_of(text):
        count += 1
        if count == lines_per_chunk:
            end = min(offset + len(line) + 1, len(text))
            pieces.append(text[at:end])
            at, count = end, 0
    if at < len(text):
        pieces.append(text[at:])
    return pieces


def chunk_cut(buffer, at_eof):
    """vf_chunk_cut of kevlar_amd/csrc/kv_varfilter_plan.h"""
    return len(buffer) if at_eof else buffer.rfind(b'\n') + 1
