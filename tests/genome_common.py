"""What the tests of the device FASTA splitter share (tests/test_genome_reference.py on the host, tests/test_gpu_genome.py on the
device): a byte-level restatement of the rule the splitter must reproduce, the predicate that says which
files it may take, today's host path as the oracle, and the files -- hand-built ones for every edge the rule and the kernels
have, files whose edges sit where a pass over the text ends, and seeded ones.  Not a test module and not a conftest: nothing here
is collected.  Nothing of the device path is imported here.

The rule: lines end at LF; a line is taken without its trailing run of space, TAB, VT, FF and CR; a line whose first byte is '>'
is a defline, its id the bytes behind the '>' up to the first space or TAB; a record's sequence is the concatenation of the
stripped lines up to the next defline; text in front of the first defline is nothing.  Declined: any byte >= 0x80, 0x1c-0x1f,
NUL, a CR that no LF follows, and (the splitter's own bounds) more than MAX_TRAIL strippable bytes on end or an id of more than
MAX_ID bytes."""
import gzip
import io
import os
import random
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_genome_plan.h')
SEPARATOR = b'>'
STRIP = b' \t\x0b\x0c\r'


def constants():
    text = open(PLAN).read()
    return {name: int(re.search(r'#define\s+{}\s+(\d+)u?\b'.format(name), text).group(1)) for name in ('GN_CHUNK', 'GN_THREADS', 'GN_MAX_TRAIL', 'GN_MAX_ID')}


C = constants()
CHUNK, MAX_TRAIL, MAX_ID = C['GN_CHUNK'], C['GN_MAX_TRAIL'], C['GN_MAX_ID']


# ---- the rule, the predicate, the oracle
def split_rule(data):
    """([id], [sequence]) of FASTA bytes, both as bytes"""
    ids, seqs = [], []
    for raw in data.split(b'\n'):
        line = raw.rstrip(STRIP)
        if raw[:1] == b'>':
            ids.append(re.match(rb'>([^ \t]*)', line).group(1))
            seqs.append([])
        elif ids:
            seqs[-1].append(line)
    return ids, [b''.join(parts) for parts in seqs]


def joined(seqs):
    """(genome text, starts, lengths) as Genome.__init__ computes them"""
    lengths = [len(s) for s in seqs]
    starts, at = [], 0
    for n in lengths:
        starts.append(at)
        at += n + 1
    return SEPARATOR.join(seqs), starts, lengths


def device_eligible(data):
    """may the device splitter take these bytes?"""
    if any(b >= 0x80 or b == 0 or 0x1c <= b <= 0x1f for b in data):
        return False
    if re.search(rb'\r(?!\n)', data):
        return False
    for raw in data.split(b'\n'):
        if len(raw) - len(raw.rstrip(STRIP)) > MAX_TRAIL:
            return False
        if raw[:1] == b'>' and len(re.match(rb'>([^ \t]*)', raw.rstrip(STRIP)).group(1)) > MAX_ID:
            return False
    return True


def host_genome(data):
    """today's host path on the bytes: a text stream as kevlar_amd.open(path, 'r') makes it, parse_seq_dict, Genome"""
    from kevlar_amd.localize import Genome
    return Genome.from_file(io.TextIOWrapper(io.BytesIO(data)))


def rule_equals_host(data):
    """the restatement against the host path; returns what they agree on"""
    ids, seqs = split_rule(data)
    text, starts, lengths = joined(seqs)
    genome = host_genome(data)
    assert genome.ids == [i.decode('ascii') for i in ids]
    assert [s.encode('latin-1') for s in genome.seqs] == seqs
    assert genome.starts.tolist() == starts and genome.text.tobytes() == text
    return ids, seqs


# ---- ingredients
def bases(rng, n, alphabet='ACGT'):
    return ''.join(rng.choice(alphabet) for _ in range(n)).encode()


def wrap(seq, width, eol=b'\n'):
    return b''.join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def filler(n, rng=None):
    """exactly n bytes (n >= 8) of one record in lines of at most 60 bases, the last byte an LF"""
    rng = rng or random.Random(n)
    out = b'>f%d\n' % (n % 7)
    assert n >= len(out) + 2
    while len(out) < n:
        room = n - len(out)
        take = min(60, room - 1)
        if room - take - 1 == 1:          # never leave room for an LF alone... a blank line is fine, but keep lines of bases
            take -= 1
        out += bases(rng, take) + b'\n'
    assert len(out) == n
    return out


# ---- hand-built files
def hand_built():
    rng = random.Random(20261021)
    dna = lambda n: bases(rng, n)                                     # noqa: E731
    cases = {
        'empty_file': b'',
        'no_defline': b'ACGTACGT\nGGCC\n',
        'only_blank_lines': b'\n\n \n',
        'text_in_front': b'junk in front\nACGT\n>s1\nAC\nGT\n',
        'no_trailing_newline': b'>s1\nACGT\n>s2\nGGCC',
        'no_trailing_newline_blanks': b'>s1\nACGT  \t',
        'crlf_throughout': b'>s1 d\r\nACGT\r\nGG\r\n>s2\r\nTT\r\n',
        'crlf_mixed': b'>s1\r\nACGT\nGG\r\n>s2\nTT\r\n\r\nAA\n',
        'trailing_blanks': b'>s1 \t\nACGT  \nGG\t\t \n>s2\x0b\x0c\nTT \x0b\x0c\n',
        'interior_blanks': b'>s1\nAC GT\n G\tG \n\x0bTT\n',
        'blank_lines': b'>s1\n\nAC\n\n\nGT\n\n>s2\n   \nTT\n\t\n',
        'defline_runs': b'>a\n>b\n>c\nACGT\n>d\n>e\n',
        'defline_at_eof': b'>a\nACGT\n>b',
        'defline_at_eof_newline': b'>a\nACGT\n>b\n',
        'gt_alone': b'>\nACGT\n>x\nGG\n',
        'gt_alone_blanks': b'>  \nACGT\n',
        'gt_mid_line': b'>s1\nAC>GT\nGG>\n >not_a_defline\n',
        'id_space_vs_tab': b'>id1 rest of it\nAC\n>id2\trest\tof it\nGT\n>id3\x0bstill id\x0c more\nTT\n',
        'id_only_blanks_behind': b'>s1   \nAC\n',
        'lower_n_iupac': b'>s1\nacgtNNNNnnnnRYKMSWBDHV\nacgu*-.\n',
        'empty_records_beside': b'>e1\n>s1\nACGTACGTACGTACGT\n>e2\n\n>e3\n>s2\nGGGGCCCCGGGGCCCC\n>e4\n',
    }
    for width in (1, 59, 60, 61, CHUNK - 1, CHUNK, CHUNK + 1):
        cases['width_%d' % width] = b'>w\n' + wrap(dna(3 * width + min(width, 7)), width) + b'>x\n' + wrap(dna(2 * width), width)
    cases['one_line_100000'] = b'>chr\n' + dna(100000) + b'\n>next\nACGT\n'
    cases['one_line_100000_cut'] = b'>chr\n' + dna(100000)
    # an LF as the first byte of a 16-KB chunk, and as the last
    for name, lf_at in (('lf_first_of_chunk', CHUNK), ('lf_last_of_chunk', CHUNK - 1)):
        data = filler(lf_at - 30, rng) + dna(30) + b'\n' + wrap(dna(500), 60)
        assert data[lf_at] == 0x0a and data[lf_at - 1] != 0x0a
        cases[name] = data
    data = filler(2 * CHUNK - 6, rng) + b'>across_the_edge and its description\n' + wrap(dna(200), 60)
    assert data[2 * CHUNK - 6] == ord('>')
    cases['defline_across_chunk'] = data
    data = filler(CHUNK - 3, rng)[:-1] + b'  \t \t \n' + wrap(dna(100), 60)
    cases['blanks_across_chunk'] = data
    cases['records_3000'] = b''.join(b'>r%d some text\n' % i + wrap(dna(rng.randint(1, 100)), rng.choice((7, 60, 100))) for i in range(3000))
    cases['empty_records_3000'] = b''.join(b'>e%d\n' % i for i in range(3000))
    return cases


# ---- files whose edges sit where a segment ends: an uncompressed file's segment k is its bytes [k S, (k + 1) S)
def segment_cases(S):
    rng = random.Random(S)
    dna = lambda n: bases(rng, n)                                     # noqa: E731
    cases = {
        'long_line': filler(100, rng) + b'>long\n' + dna(3 * S + 500) + b'\n>after\nACGT\n',
        'long_line_to_eof': b'>long\n' + dna(3 * S + 17),
        'long_defline': b'>id ' + dna(3 * S + 5) + b'\nACGT\n>z\nGG\n',
        'in_defline': filler(S - 10, rng) + b'>chr_cut some description here\n' + dna(50) + b'\n',
        'in_defline_id': filler(S - 4, rng) + b'>abcdefgh tail\nAC\n',
        'in_defline_behind_blank': filler(S - 12, rng) + b'>abcdefgh tail of it\nAC\n',
        'in_defline_vt_then_id': filler(S - 4, rng) + b'>abc\x0bdef ghi\nAC\n',
        'blanks_then_lf': filler(S - 40, rng) + dna(37) + b' \t \t  \n' + b'ACGT\n',
        'blanks_then_bases': filler(S - 40, rng) + dna(37) + b' \t \t  GGCC\n' + b'ACGT\n',
        'blanks_then_eof': filler(S - 40, rng) + dna(37) + b' \t \t  ',
        'blanks_in_front_of_first_defline': b'x' * (S - 3) + b' \t \t  \n>s\nACGT\n',
        'on_lf': filler(S, rng) + b'ACGT\n>next\nAC\n',
        'on_lf_then_defline': filler(S, rng) + b'>next\nAC\n',
        'gt_last_byte': filler(S - 1, rng) + b'>next_id x\nACGT\n',
        'gt_first_byte': filler(S, rng) + b'>next_id\nACGT\n',
        'crlf_cut': filler(S - 21, rng) + dna(20) + b'\r\nACGT\r\n',
        'exactly_one_segment': filler(S, rng),
        'one_byte_more': filler(S, rng) + b'A',
    }
    if S + 6 <= MAX_TRAIL:            # (a run of blanks that two segments end in; a longer one is held back no further: over_bound())
        cases['two_cuts_in_blanks'] = filler(S - 40, rng) + dna(37) + b' ' * (S + 6) + b'TT\n'
    assert cases['in_defline'][S - 10] == ord('>') and cases['gt_last_byte'][S - 1] == ord('>') and cases['gt_first_byte'][S] == ord('>')
    assert cases['on_lf'][S - 1] == 0x0a and cases['crlf_cut'][S - 1] == 0x0d and cases['crlf_cut'][S] == 0x0a
    assert cases['blanks_then_lf'][S - 3:S + 4] == b' \t \t  \n'
    return cases


def over_bound(S):
    """an INTERIOR run of blanks longer than MAX_TRAIL: nothing the rule minds, and taken when one segment holds the line; where
    segments of S bytes end inside it the splitter would have to hold more than MAX_TRAIL bytes back, and declines"""
    return b'>s1\nACGT' + b' ' * (MAX_TRAIL + S) + b'TT\nGG\n'


# ---- files the device declines
def declines():
    return {
        'high_byte': b'>s1\nACGT\xc3\xa9\n',
        'high_byte_in_defline': b'>s\xff1\nACGT\n',
        'sep_1c': b'>s1\nAC\x1cGT\n',
        'sep_1f_trailing': b'>s1\nACGT\x1f\n',
        'nul': b'>s1\nAC\x00GT\n',
        'lone_cr': b'>s1\nAC\rGT\n',
        'lone_cr_at_eof': b'>s1\nACGT\r',
        'cr_cr_lf': b'>s1\nACGT\r\r\n',
        'long_trail': b'>s1\nACGT' + b' ' * (MAX_TRAIL + 1) + b'\nGG\n',
        'long_id': b'>' + b'i' * (MAX_ID + 1) + b' x\nACGT\n',
    }


# ---- seeded files
def seeded(seed):
    """one FASTA file made of everything above, a few hundred bytes to a few KB (now and then beyond a 16-KB chunk)"""
    rng = random.Random(seed)
    eol = rng.choice((b'\n', b'\n', b'\r\n', None))                   # None: mixed
    out = []
    if rng.random() < 0.2:
        out.append(rng.choice((b'leading text', b'', b'  ', b'ACGT', b' >no')) + b'\n')
    alphabet = rng.choice(('ACGT', 'ACGT', 'ACGTNacgtn', 'ACGTRYKMSWBDHVN'))
    n_records = rng.choice((0, 1, 2, 3, 5, 8, 40))
    big = rng.random() < 0.1
    for r in range(n_records):
        le = eol or rng.choice((b'\n', b'\r\n'))
        name = b'' if r == 0 and rng.random() < 0.05 else b'seq%d_%d' % (seed, r)
        tail = rng.choice((b'', b'', b' desc', b'\tdesc two', b' ', b'\t', b'  a>b', b'\x0bvt'))
        trail = rng.choice((b'', b'', b' ', b'\t ', b'\x0c'))
        out.append(b'>' + name + tail + trail + le)
        shape = rng.random()
        if shape < 0.15:
            continue                                                  # an empty record
        length = rng.choice((1, 2, 59, 60, 61, 130, 700)) if not big else rng.choice((700, 9000, 20000))
        width = rng.choice((1, 7, 59, 60, 61, 10 ** 6)) if length < 2000 else rng.choice((60, 61, 10 ** 6))
        seq = bases(rng, length, alphabet)
        for i in range(0, len(seq), width):
            le = eol or rng.choice((b'\n', b'\r\n'))
            line = seq[i:i + width]
            roll = rng.random()
            if roll < 0.05:
                line += rng.choice((b' ', b'\t', b'  \t', b'\x0b', b' \x0c '))          # trailing blanks
            elif roll < 0.08 and len(line) > 2:
                line = line[:1] + rng.choice((b' ', b'\t', b'>')) + line[1:]           # an interior blank, a '>' in mid-line
            elif roll < 0.10:
                line = b' ' + line                                                     # a leading blank stays
            out.append(line + le)
            if rng.random() < 0.04:
                out.append(rng.choice((b'', b' ', b'\t\t')) + le)                      # a blank line
    data = b''.join(out)
    if data and rng.random() < 0.3:
        data = data.rstrip(b'\r\n')                                                    # no trailing newline
    return data


N_SEEDED = 300


def gzip_of(data):
    """one gzip stream"""
    return gzip.compress(data, compresslevel=6, mtime=0)


def bgzf_of(data, path):
    """re-blocked as BGZF by the package's own writer; returns the path"""
    from kevlar_amd.bgzf import BgzfWriter
    writer = BgzfWriter(path)
    writer.write(data)
    writer.close()
    return path


def golden_references():
    """the reference FASTA fixtures under tests/golden that the end-to-end tests read"""
    import assemble_common as ac
    import localize_common as lc
    return [lc.fixture('fiveparts-refr.fa.gz'), lc.fixture('maxdiff-refr.fa.gz'), lc.fixture('localize-refr.fa'),
            ac.fixture_path('fiveparts-refr.fa.gz'), ac.fixture_path('human-random-pico.fa.gz')]


def file_text(path):
    """the bytes of text of a fixture, whatever its container"""
    raw = open(path, 'rb').read()
    return gzip.decompress(raw) if raw[:2] == b'\x1f\x8b' else raw


def as_arrays(values):
    return np.array(values, dtype=np.int64)
