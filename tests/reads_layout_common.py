"""The layout rule of a read batch (kevlar_amd/csrc/kv_reads_layout.h) restated in plain Python, and the length vectors
tests/test_reads_layout.py and tests/test_gpu_reads_build.py run it on.  The boundary cases follow the header's constants."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_reads_layout.h')
API = os.path.join(ROOT, 'include', 'kvsketch.h')


def constants():
    """the #defines the rule is made of, read from the headers"""
    text = open(HDR).read() + open(API).read()
    out = {}
    for name in ('KV_TILE_LDS_BYTES', 'KV_TILE_MAX_READS', 'KV_READ_PAD', 'KV_SEG_BASES', 'KV_MAX_K'):
        out[name] = int(re.search(r'#define\s+{}\s+(\d+)'.format(name), text).group(1))
    return out


def need(c, length):
    """bytes of LDS one read takes: both strands, padded"""
    return 2 * ((length + c['KV_READ_PAD'] + 3) & ~3)


def budget(c):
    return c['KV_TILE_LDS_BYTES'] - 64


def plan(c, lens):
    """the rule, read by read: scalars, word offsets and tile table as (first, count, seg_start, seg)"""
    woff, tiles, run = [], [], []
    n_words = tile_max_bases = used = 0

    def close_run():
        nonlocal used, tile_max_bases
        if run:
            tiles.append((run[0], len(run), 0, 0))
            tile_max_bases = max(tile_max_bases, sum(lens[i] for i in run))
        del run[:]
        used = 0

    for i, length in enumerate(lens):
        woff.append(n_words)
        n_words += (length + 15) // 16
        if need(c, length) > budget(c):
            close_run()
            tiles.extend((i, 1, start, 1) for start in range(0, length, c['KV_SEG_BASES']))
            tile_max_bases = max(tile_max_bases, min(length, c['KV_SEG_BASES'] + c['KV_MAX_K']))
            continue
        if run and (len(run) == c['KV_TILE_MAX_READS'] or used + need(c, length) > budget(c)):
            close_run()
        run.append(i)
        used += need(c, length)
    close_run()
    woff.append(n_words)
    uniform = len(lens) > 0 and lens[0] > 0 and all(x == lens[0] for x in lens) and need(c, lens[0]) <= budget(c)
    return {'n_words': n_words, 'n_bases': sum(lens), 'max_len': max(lens, default=0), 'tile_max_bases': tile_max_bases,
            'n_tiles': len(tiles), 'uni_len': lens[0] if uniform else 0,
            'uni_per_tile': min(c['KV_TILE_MAX_READS'], budget(c) // need(c, lens[0])) if uniform else 0,
            'woff': woff, 'tiles': tiles or [(0, 0, 0, 0)]}


def closed_form(c, length, n):
    """word offsets and tile table of n reads of one length, by arithmetic"""
    wpr = (length + 15) // 16
    per_tile = min(c['KV_TILE_MAX_READS'], budget(c) // need(c, length))
    tiles = [(t * per_tile, min(per_tile, n - t * per_tile), 0, 0) for t in range((n + per_tile - 1) // per_tile)]
    return [i * wpr for i in range(n + 1)], tiles, per_tile


def cases(c):
    """name -> lengths.  With the constants as they stand: a tile holds 64 reads of 100 bases but 63 of 102; a read of 8136 bases
    is the longest that fits one tile; a segment has 7680 k-mer starts."""
    full = c['KV_TILE_MAX_READS']
    std = max(x for x in range(1, budget(c)) if budget(c) // need(c, x) >= full)           # 100: the longest read a tile holds `full` of
    fit = max(x for x in range(1, budget(c)) if need(c, x) <= budget(c))                    # 8136
    seg = c['KV_SEG_BASES']
    rng = random.Random(20)
    mixed = [0 if rng.random() < 0.1 else rng.randint(0, 300) for _ in range(300)]
    assert 0 in mixed
    out = {'empty': []}
    for n in (1, full, full + 1, 2 * full + 1):
        out['std_x{}'.format(n)] = [std] * n
    out['budget_limited'] = [std + 2] * full                 # 63 to a tile
    assert budget(c) // need(c, std + 2) < full
    out['short_x200'] = [37] * 200
    out['short_x5'] = [20] * 5
    out['one_empty_read'] = [0]
    out['three_empty_reads'] = [0] * 3                       # not uniform
    out['mixed'] = mixed
    out['longest_one_tile'] = [fit]
    out['two_segments_just'] = [fit + 1]
    out['two_segments_full'] = [2 * seg]
    out['three_segments'] = [2 * seg + 1]
    out['long_between_short'] = [std, 2 * seg + 1, std]
    out['equal_but_segmented'] = [max(9000, fit + 1)] * 3    # equal lengths but not uniform
    return out
