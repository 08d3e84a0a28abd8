"""The host rules of the parallel gzip decoder (kevlar_amd/csrc/kv_gunzip_plan.h) restated in plain Python -- segment extent,
starts, cuts, jobs, the chain walk, the CRC ranges -- and a simulated DEFLATE stream whose decoder answers a job as k_gz_decode's
contract says.  tests/test_gunzip_plan.py holds the header to both, without a GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_gunzip_plan.h')
INTERNAL = os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_internal.h')
NONE = 2 ** 64 - 1
LANDED, END, BAD, FULL, SHORT = range(5)
WALK_OK, WALK_REPAIRS, WALK_BAD, WALK_SHORT, WALK_DEVICE = range(5)


def constants():
    """the #defines the rules are made of, read from the headers"""
    text = open(HDR).read() + open(INTERNAL).read()
    out = {}
    for name in ('GZ_FIND_KEEP', 'GZ_MARGIN', 'GZ_MAX_REPAIRS', 'GZ_MAX_CAP', 'KV_CRC_SLICE'):
        value = re.search(r'#define\s+{}\s+(\([^)]*\)|\S+)'.format(name), text).group(1)
        out[name] = eval(re.sub(r'(?<=[0-9a-fA-F])(ull|u)\b', '', value))
    return out


C = constants()


def round_up(v, m):
    return (v + m - 1) // m * m


def extent(pos_bit, file_size, want_text, ratio, chunk):
    first_byte = (pos_bit >> 3) & ~255
    seg = max(int(want_text / ratio), 4 * chunk)
    seg_end = min(round_up(first_byte + seg, chunk), file_size)
    upto = min(seg_end + C['GZ_MARGIN'], file_size)
    n_bytes = upto - first_byte
    return {'first_byte': first_byte, 'seg_end': seg_end, 'upto': upto, 'n_bytes': n_bytes, 'n_chunks': (n_bytes + chunk - 1) // chunk,
            'to_file_end': int(seg_end == file_size), 'is_file_end': int(upto == file_size), 'start_rel': pos_bit - first_byte * 8,
            'seg_end_rel': (seg_end - first_byte) * 8}


EXTENT_FIELDS = ('first_byte', 'seg_end', 'upto', 'n_bytes', 'n_chunks', 'to_file_end', 'is_file_end', 'start_rel', 'seg_end_rel')


def starts_of(x, cand):
    """(found a start in the margin or need none, starts, have_terminal, stop_rel)"""
    starts, have_terminal = [x['start_rel']], False
    for c in cand:
        if have_terminal:
            break
        if c == NONE or c <= x['start_rel']:
            continue
        starts.append(c)
        if not x['to_file_end'] and c >= x['seg_end_rel']:
            have_terminal = True
    ok = bool(x['to_file_end'] or have_terminal or x['is_file_end'])
    return ok, starts, have_terminal, (starts[-1] if have_terminal else NONE)


def cut_guesses(x, starts, have_terminal, wanted, max_guesses):
    piece = 0 if len(starts) * 4 >= wanted * 3 else max(4096 * 8, (x['seg_end_rel'] - x['start_rel']) // wanted)
    guesses = []
    n_blocks = len(starts) - 1 if have_terminal else len(starts)
    for j in range(n_blocks if piece else 0):
        nxt = starts[j + 1] if j + 1 < len(starts) else x['n_bytes'] * 8
        span = nxt - starts[j]
        cuts = min(8, span // piece)
        for i in range(1, cuts):
            if len(guesses) < max_guesses:
                guesses.append((starts[j], starts[j] + i * (span // cuts)))
    return guesses


def merge_cuts(starts, have_terminal, guesses, found):
    stop_rel = starts[-1] if have_terminal else NONE
    both, taken = [(s, s) for s in starts], 0
    for (header, _), f in zip(guesses, found):
        if f == NONE or f <= header or f >= stop_rel:
            continue
        later = [s for s in starts if s > header]
        if later and f >= later[0]:
            continue
        both.append((f, header))
        taken += 1
    both.sort()
    out = []
    for pair in both:
        if not out or pair[0] != out[-1][0]:
            out.append(pair)
    return [p[0] for p in out], [p[1] for p in out], taken


def room(ratio, bits):
    factor = min(max(2.5 * ratio, 8.0), 64.0)
    return min(int((bits // 8 + 1) * factor) + 16384, C['GZ_MAX_CAP'])


def plan_jobs(starts, headers, have_terminal, n_bytes, ratio):
    n_first = len(starts) - 1 if have_terminal else len(starts)
    jobs, total_cap = [], 0
    for j in range(n_first):
        nb = j + 1
        while nb < len(starts) and headers[nb] != starts[nb]:
            nb += 1
        nxt = starts[nb] if nb < len(starts) else n_bytes * 8
        cap = room(ratio, nxt - starts[j])
        jobs.append({'start_bit': starts[j], 'header_bit': headers[j], 'target_idx': j + 1, 'out_off': total_cap, 'out_cap': cap})
        total_cap += round_up(cap, 64)
    return {'jobs': jobs, 'total_cap': total_cap, 'repair_room': max(256 << 20, total_cap // 4),
            'exact': int(any(h != s for h, s in zip(headers, starts)))}


def walk_chain(starts, headers, have_terminal, n_bytes, ratio, decode):
    """decode(job) -> result dict; the chain as a dict of the fields of GzChain"""
    plan = plan_jobs(starts, headers, have_terminal, n_bytes, ratio)
    stop_rel = starts[-1] if have_terminal else NONE
    results = [decode(dict(job)) for job in plan['jobs']]
    c = {'v': [], 'ends': [], 'text': 0, 'end_rel': 0, 'isize_seg': 0, 'repairs': 0, 'ended': 0, 'crc_lost': 0, 'fail': WALK_OK, 'fail_bit': 0}
    later = starts[1:]
    used, job, cur = 0, plan['jobs'][0], results[0]

    def accept():
        c['v'].append((job['out_off'], cur['n_out'], c['text']))
        if cur['members'] >= 1:
            c['ends'].append((c['text'] + cur['trailer_at'], cur['trailer_crc']))
        if cur['members'] > 1:
            c['crc_lost'] = 1
        c['text'] += cur['n_out']
        c['isize_seg'] = (c['isize_seg'] + cur['isize_sum']) & 0xffffffff

    while True:
        if cur['status'] == FULL or (cur['status'] == LANDED and cur['end_bit'] < stop_rel and cur['end_bit'] not in later):
            if cur['status'] == FULL:
                if job['out_off'] >= plan['total_cap']:
                    used = job['out_off'] - plan['total_cap']
                again = dict(job, out_cap=min(job['out_cap'] * 32, C['GZ_MAX_CAP']))
            else:
                accept()
                behind = [i + 1 for i, s in enumerate(later) if s > cur['end_bit']]
                nxt = starts[behind[0]] if behind else n_bytes * 8
                again = {'start_bit': cur['end_bit'], 'header_bit': cur['end_bit'], 'target_idx': behind[0] if behind else len(starts),
                         'out_cap': room(ratio, nxt - cur['end_bit'])}
            again['out_off'] = plan['total_cap'] + used
            used += round_up(again['out_cap'], 64)
            c['repairs'] += 1
            if c['repairs'] > C['GZ_MAX_REPAIRS'] or used > plan['repair_room'] or (cur['status'] == FULL and job['out_cap'] >= C['GZ_MAX_CAP']):
                c['fail'], c['fail_bit'] = WALK_REPAIRS, job['start_bit']
                return c
            cur, job = decode(dict(again)), again
            continue
        if cur['status'] in (BAD, SHORT):
            c['fail'], c['fail_bit'] = (WALK_BAD if cur['status'] == BAD else WALK_SHORT), cur['end_bit']
            return c
        accept()
        c['end_rel'] = cur['end_bit']
        if cur['status'] == END:
            c['ended'] = 1
            return c
        if cur['end_bit'] >= stop_rel:
            return c
        k = 1 + later.index(cur['end_bit'])
        job, cur = plan['jobs'][k], results[k]


def crc_ranges(text, ends, piece):
    """[(start, len, closes)]: closes = 1 + the index of the member end the range closes, or 0"""
    out, at, e = [], 0, 0
    while at < text or e < len(ends):
        stop = ends[e] if e < len(ends) else text
        if at == stop:
            if e >= len(ends):
                break
            e += 1
            out.append((at, 0, e))
            continue
        n = min(stop - at, piece)
        at += n
        closes = 0
        if at == stop and e < len(ends):
            e += 1
            closes = e
        out.append((at - n, n, closes))
    return out


class SimStream:
    """A DEFLATE stream as the decoders see it.  true: {bit: header} of every true boundary that matters -- a block start (header
    == bit) or a symbol boundary inside the block that begins at `header`; text_at: a monotone map from bit to text offset;
    end_bit: where the stream ends; member_ends: [(bit, crc, isize)] of the member trailers; poison: (bit, status) a decoder
    that gets there reports.  decode() answers a job over starts / headers (false starts among them) as k_gz_decode does: it
    stops ON the first later start of its kind that is true -- a block start at a block boundary, a start inside a block between
    two symbols of that block -- or on the first block boundary at or behind stop_rel, runs over every other start, and reports
    GZ_FULL when the text in between does not fit out_cap and GZ_END at the end of the stream.  Every job is logged."""

    def __init__(self, true, text_at, end_bit, member_ends=(), poison=None):
        self.true, self.text_at, self.end_bit, self.member_ends, self.poison = dict(true), text_at, end_bit, list(member_ends), poison
        self.order = sorted(self.true)
        self.log = []

    def decoder(self, starts, headers, stop_rel):
        kind = dict(zip(starts, headers))

        def decode(job):
            start, end, status = job['start_bit'], self.end_bit, END
            for bit in self.order:
                if bit <= start:
                    continue
                header = self.true[bit]
                if (bit in kind and kind[bit] == header and starts.index(bit) >= job['target_idx']) or (header == bit and bit >= stop_rel):
                    end, status = bit, LANDED
                    break
            if self.poison and start < self.poison[0] <= end:
                end, status = self.poison
            passed = [m for m in self.member_ends if start < m[0] <= end]
            n_out = self.text_at(end) - self.text_at(start)
            result = {'end_bit': end, 'n_out': n_out, 'status': status, 'members': len(passed), 'isize_sum': sum(m[2] for m in passed) & 0xffffffff,
                      'trailer_at': self.text_at(passed[0][0]) - self.text_at(start) if passed else 0, 'trailer_crc': passed[0][1] if passed else 0}
            if status in (LANDED, END) and n_out > job['out_cap']:
                result = dict(result, status=FULL, n_out=job['out_cap'], members=0, isize_sum=0, trailer_at=0, trailer_crc=0)
            self.log.append((dict(job), result))
            return result
        return decode
