"""The case table of the super-k-mer kernel instances (kv_skm.hip, kv_skm_emit_device.h, kv_skm_bucket_device.h): one row per case, each
with the exact list of template instances kv_skm_last_instances must report for every library call the case makes.  Shared by
tests/test_gpu_skm_instances.py (runs every row on the GPU, holds it to the oracle) and tests/test_skm_instances_ledger.py (no GPU:
the instances named here are exactly the ones the launch sites of kv_skm.hip can launch).  Not collected itself.

The boundary lengths are derived from the host planners and written down as literals; the report then shows whether a planner still
agrees with them.  For equal-length reads of L bases, wpr = ceil(L / 16) packed words per read:

  skm_lane_fits_len   m == 12 and w == 20 (k = 31) or 40 (k = 51), and two workgroups' LDS per CU (skm_lane_wgs_per_cu):
                      4 * 8 * skm_lane_slice_words(wpr) + 1200 = 4096 wpr + 22000 <= 80000, i.e. wpr <= 14: L <= 224.  (The `L > 256`
                      of the same condition is never the one that decides.)  Three workgroups per CU up to wpr = 7: L <= 112.
                      The instance changes from NW = 8 to NW = 16 between wpr = 8 and 9: L = 128 | 129.
                      npos = L - 11 m-mers in blocks of SKM_LANE_B = 20: whole blocks at L = 31, 51, 71.
  skm_wave_plan       w > 8; R = min(64 / wpr, 64 / ceil(nk / c), 58 / runs) >= 2 with runs = 1 + 2 (nk - 1) / (w + 1) + nk / (2 ncap);
                      the chunk c is 16 unless c = 8 gives as many reads per wave (and never 16 when w <= 16).  The longest L with
                      R >= 2:  k = 25: 216   k = 31: 285   k = 32: 295   k = 40: 411   k = 51: 512 (there 64 / wpr decides).
                      (skm_wave_slice_words stays inside the 54000 bytes of three workgroups per CU at every one of these.)
  tile kernel         everything else: ragged batches, and equal lengths beyond the wave plan; CH = 16 for w > 16, else 8."""

import re

# ---- the instances, by the names the launch sites give them (blanks removed) ----------------------------------------------------
LANE_1_8, LANE_1_16 = 'k_skm_emit_lane<1,8>', 'k_skm_emit_lane<1,16>'
LANE_2_8, LANE_2_16 = 'k_skm_emit_lane<2,8>', 'k_skm_emit_lane<2,16>'
WAVE_16, WAVE_8 = 'k_skm_emit_wave<16,512>', 'k_skm_emit_wave<8,512>'
WAVE_16_1024, WAVE_8_1024 = 'k_skm_emit_wave<16,1024>', 'k_skm_emit_wave<8,1024>'
TILE_16, TILE_8 = 'k_skm_emit<16>', 'k_skm_emit<8>'
SORT_2, SORT_3, SORT_4 = 'k_skm_split_sorted<2>', 'k_skm_split_sorted<3>', 'k_skm_split_sorted<4>'
PLAIN_C, PLAIN = 'k_skm_split<true>', 'k_skm_split<false>'
COUNT_1, COUNT_1_LOOSE = 'k_skm_count<1,4096,false,0>', 'k_skm_count<1,4096,true,0>'
COUNT_2, COUNT_2_LOOSE = 'k_skm_count<2,2048,false,0>', 'k_skm_count<2,2048,true,0>'
COUNT_31, COUNT_51 = 'k_skm_count<1,SKM_TS31,false,31>', 'k_skm_count<2,SKM_TS51,false,51>'
COUNT_C, COUNT_C_LOOSE, COUNT_C_31 = 'k_skm_count<1,4096,false,0,true>', 'k_skm_count<1,4096,true,0,true>', 'k_skm_count<1,SKM_TS31,false,31,true>'
LOOSE_COUNT_1, LOOSE_COUNT_2 = 'k_skm_loose_count<1>', 'k_skm_loose_count<2>'
NOVEL_1, NOVEL_2 = 'k_skm_novel<1,4096>', 'k_skm_novel<2,2048>'
LIST_1, LIST_2 = 'k_skm_novel_list<1,2048>', 'k_skm_novel_list<2,1024>'
LOOSE_NOVEL_1, LOOSE_NOVEL_2 = 'k_skm_loose_novel<1>', 'k_skm_loose_novel<2>'
ROUTE_1, ROUTE_2, ROUTE_C = 'k_skm_route<1,4096>', 'k_skm_route<2,2048>', 'k_skm_route<1,4096,true>'
LOOSE_ROUTE_1, LOOSE_ROUTE_2 = 'k_skm_loose_route<1>', 'k_skm_loose_route<2>'
SET_1, SET_2 = 'k_skm_set_hits<1,2048>', 'k_skm_set_hits<2,1024>'
LOOSE_SET_1, LOOSE_SET_2 = 'k_skm_loose_set_hits<1>', 'k_skm_loose_set_hits<2>'

# every knob a row may set (the test removes them all after each row)
KNOBS = ('KV_COUNT_PATH', 'KV_NOVEL_PATH', 'KV_ROUTE_PATH', 'KV_SKM_BUCKET_KMERS', 'KV_SKM_CAP_PCT', 'KV_SKM_FORCE_LOOSE', 'KV_SKM_DL', 'KV_SKM_ANY_K',
         'KV_SKM_S2')

ONE_BUCKET = '100000000'        # KV_SKM_BUCKET_KMERS: one coarse x one fine bucket (tests/test_gpu_skm.py, test_skm_single_bucket_and_default_geometry)

CASES = []


def split_report(text):
    """kv_skm_last_instances' list into names: it is comma separated, and a name's own commas stand between its angle brackets"""
    return re.split(r',(?![^<]*>)', text) if text else []


def case(id, entry, k, shape, n, expect, make='packed', buckets='512', hint=False, short=False, why='', **knobs):
    """entry   'count_scan'  one sample: consume_batch (expect['count']), then the scan of that batch with no control and case-min 1 --
                             every k-mer position of every scanned read is a hit (expect['scan'])
               'trio'        mother, father, proband counted (expect['count'] for the controls, expect['case'] for the case sample), then
                             the scan with thresholds (expect['scan'])
               'route'       kv_route_distinct to two band owners (expect['route']), each owner's weighted count against the banded oracle
               'exchange'    kv_mex_emit (expect['emit']), kv_mex_route (expect['route']), the owner's sketch against the oracle; with
                             expect['set_scan']: kept for the scan, and kv_mex_scan_set's hits against the oracle's
       shape   a read length (n reads sampled from the proband of synth.make_trio(60000, ...)) or the name of a batch in
               tests/test_gpu_skm_instances.py (SHAPES)
       make    'packed': ReadBatch.from_packed; 'strings': ReadBatch of strings
       hint    Counttable.expect_scan() on the case sample and KV_SKM_DL=1: records keep positions, the count leaves its distinct list
       short   (exchange) hk.mex_plan(short=True): 16-byte records, nothing kept for a scan
       buckets KV_SKM_BUCKET_KMERS
       why     the planner condition the row stands on (shown when the row fails)"""
    knobs = dict(knobs, KV_SKM_BUCKET_KMERS=buckets)
    if hint:
        knobs['KV_SKM_DL'] = '1'
    assert all(name in KNOBS for name in knobs), knobs
    assert all(isinstance(v, list) and v for v in expect.values())
    CASES.append(dict(id=id, entry=entry, k=k, shape=shape, n=n, make=make, hint=hint, short=short, why=why, knobs=knobs, expect=expect))


# what a count and the scan behind it launch, given S1's instance.  k = 31, equal-length reads the lane kernel cuts, nobody said a
# scan would follow: 16-byte records (S2 <2>, the compact fixed-k count), which the scan cannot answer from -- it cuts again, 24-byte
def k31_compact(s1):
    return {'count': [s1, SORT_2, COUNT_C_31, LOOSE_COUNT_1], 'scan': [s1, SORT_3, NOVEL_1, LOOSE_NOVEL_1]}


# k = 31 with positions (reads the lane kernel does not cut): 24-byte records, the scan reuses the count's buckets
def k31_wide(s1):
    return {'count': [s1, SORT_3, COUNT_31, LOOSE_COUNT_1], 'scan': [NOVEL_1, LOOSE_NOVEL_1]}


def k51(s1):
    return {'count': [s1, SORT_4, COUNT_51, LOOSE_COUNT_2], 'scan': [NOVEL_2, LOOSE_NOVEL_2]}


def one_word(s1):       # k <= 32, not 31
    return {'count': [s1, SORT_3, COUNT_1, LOOSE_COUNT_1], 'scan': [NOVEL_1, LOOSE_NOVEL_1]}


def two_words(s1):      # k > 32, not 51
    return {'count': [s1, SORT_4, COUNT_2, LOOSE_COUNT_2], 'scan': [NOVEL_2, LOOSE_NOVEL_2]}


# ---- S1, the lane-per-read cut: k = 31 (C = 1) and k = 51 (C = 2) --------------------------------------------------------------------
for L, s1, why in [(31, LANE_1_8, 'L == k: one k-mer a read; npos = 20, one whole block'), (32, LANE_1_8, 'L == k + 1; npos = 21: a block and one m-mer'),
                   (51, LANE_1_8, 'npos = 40: two whole blocks'), (52, LANE_1_8, 'npos = 41'),
                   (112, LANE_1_8, 'wpr = 7, no padding in the last word; the longest with three workgroups per CU'), (113, LANE_1_8, 'wpr = 8: two workgroups per CU'),
                   (127, LANE_1_8, 'one base of padding'), (128, LANE_1_8, 'wpr = 8: the last NW = 8 length, wl[rbase + w0 + 2] behind the last word'),
                   (129, LANE_1_16, 'wpr = 9: NW = 16'), (224, LANE_1_16, 'wpr = 14: the longest the lane cut takes')]:
    case('lane-k31-L%d' % L, 'count_scan', 31, L, 3000, k31_compact(s1), buckets='64' if L < 60 else '512', why=why)
for L, s1, why in [(225, WAVE_8, 'wpr = 15: two workgroups of the lane cut no longer fit a CU'), (256, WAVE_8, 'the `L > 256` of skm_lane_fits_len, this side'),
                   (257, WAVE_8, '... and that side'), (285, WAVE_8, 'nk = 255: the longest with R >= 2'), (286, TILE_16, 'R = 1: the tile kernel')]:
    case('lane-k31-L%d' % L, 'count_scan', 31, L, 2000, k31_wide(s1), buckets='2048', why=why)
for L, s1, why in [(51, LANE_2_8, 'L == k; npos = 40: two whole blocks, one pair'), (52, LANE_2_8, 'L == k + 1; npos = 41: a third block without its pair'),
                   (71, LANE_2_8, 'npos = 60: three whole blocks'), (72, LANE_2_8, 'npos = 61'),
                   (112, LANE_2_8, 'wpr = 7'), (113, LANE_2_8, 'wpr = 8'), (127, LANE_2_8, 'one base of padding'), (128, LANE_2_8, 'the last NW = 8 length'),
                   (129, LANE_2_16, 'wpr = 9: NW = 16'), (224, LANE_2_16, 'the longest the lane cut takes'),
                   (225, WAVE_16, 'the wave kernel: R = 4 by 64 / wpr, which c = 8 does not reach'), (256, WAVE_16, 'L == 256'), (257, WAVE_16, 'L > 256'),
                   (512, WAVE_16, 'wpr = 32: the longest with R >= 2'), (513, TILE_16, 'wpr = 33: R = 1, the tile kernel')]:
    case('lane-k51-L%d' % L, 'count_scan', 51, L, 3000 if L < 225 else 1500, k51(s1), buckets='64' if L < 80 else '512' if L < 225 else '2048', why=why)
# the last group of a batch: 1, 63, 64, 65 reads, and 64 n + 1
for n in (1, 63, 64, 65, 513):
    case('lane-k31-n%d' % n, 'count_scan', 31, 100, n, k31_compact(LANE_1_8), buckets='64')
    case('lane-k51-n%d' % n, 'count_scan', 51, 150, n, k51(LANE_2_16), buckets='64')
# A wave of the lane cut takes a second group (the loop that prefetches the next group's words behind the current one) only when the
# batch has more groups of 64 than the grid has waves: 8 x min(768, 3 x CUs) for k = 31 up to 112 bases, 8 x 2 x CUs for k = 51.  Short
# reads make that cheap: two k-mers a read.  (The two rows with more than 4 000 reads: this edge shows at no smaller size.)
case('lane-k31-groups-beyond-the-grid', 'count_scan', 31, 32, 64 * 6150 + 1, k31_compact(LANE_1_8), buckets='128', why='6151 groups for at most 6144 waves')
case('lane-k51-groups-beyond-the-grid', 'count_scan', 51, 52, 64 * 4100 + 1, k51(LANE_2_8), buckets='128', why='4101 groups for at most 4096 waves')
# one minimizer from end to end and ties at every position
case('lane-k31-polyA-AC', 'count_scan', 31, 'polyA_AC', 600, k31_compact(LANE_1_8), make='strings')
case('lane-k51-polyA-AC', 'count_scan', 51, 'polyA_AC', 600, k51(LANE_2_8), make='strings')
# strings of one length with N at base 0, at the last base, at bases 15 and 16, and a lower-case read
case('lane-k31-N', 'count_scan', 31, 'with_N', 2005, k31_compact(LANE_1_8), make='strings')
case('lane-k51-N', 'count_scan', 51, 'with_N', 2005, k51(LANE_2_8), make='strings')
# the same cut with 24-byte records (a scan was announced): the fixed-k count of 24-byte records, the scan from the distinct list
case('lane-k31-hint-L100', 'count_scan', 31, 100, 3000, {'count': [LANE_1_8, SORT_3, COUNT_31, LOOSE_COUNT_1], 'scan': [LIST_1, LOOSE_NOVEL_1]}, hint=True)
case('lane-k31-hint-L129', 'count_scan', 31, 129, 3000, {'count': [LANE_1_16, SORT_3, COUNT_31, LOOSE_COUNT_1], 'scan': [LIST_1, LOOSE_NOVEL_1]}, hint=True)
case('lane-k51-hint-L150', 'count_scan', 51, 150, 3000, {'count': [LANE_2_16, SORT_4, COUNT_51, LOOSE_COUNT_2], 'scan': [LIST_2, LOOSE_NOVEL_2]}, hint=True)

# ---- S1, the wave kernel ------------------------------------------------------------------------------------------------------------
for L, s1, why in [(25, WAVE_8, 'L == k'), (26, WAVE_8, 'L == k + 1'), (48, WAVE_8, 'wpr = 3, no padding'), (63, WAVE_8, 'one base of padding'), (64, WAVE_8, 'wpr = 4'), (65, WAVE_8, 'wpr = 5'),
                   (216, WAVE_8, 'nk = 192: the longest with R >= 2'), (217, TILE_8, 'R = 1: the tile kernel')]:
    case('wave-k25-L%d' % L, 'count_scan', 25, L, 3000 if L < 200 else 2000, one_word(s1), buckets='64' if L < 40 else '512' if L < 200 else '2048', why=why)      # w = 14: chunks of 8 only
for L, s1, why in [(32, WAVE_8, 'L == k'), (48, WAVE_8, 'R = 16 either way: the smaller chunk'), (63, WAVE_8, ''), (64, WAVE_16, 'c = 8 brings 12 reads a wave, c = 16 13'), (65, WAVE_8, ''),
                   (295, WAVE_16, 'the longest with R >= 2'), (296, TILE_16, 'R = 1')]:
    case('wave-k32-L%d' % L, 'count_scan', 32, L, 3000 if L < 200 else 2000, one_word(s1), buckets='64' if L < 40 else '512' if L < 200 else '2048', why=why)       # w = 21: either chunk
for L, s1, why in [(40, WAVE_8, 'L == k'), (48, WAVE_8, ''), (63, WAVE_8, ''), (64, WAVE_8, ''), (65, WAVE_8, ''), (100, WAVE_16, 'c = 8 brings 8 reads a wave, c = 16 9'),
                   (411, WAVE_16, 'the longest with R >= 2'), (412, TILE_16, 'R = 1')]:
    case('wave-k40-L%d' % L, 'count_scan', 40, L, 3000 if L < 200 else 1500, two_words(s1), buckets='64' if L < 50 else '512' if L < 200 else '2048', why=why)     # w = 29, two-word keys

# ---- S1, the tile kernel on ragged batches ------------------------------------------------------------------------------------------
case('tile-k31-ragged', 'count_scan', 31, 'ragged', 1517, k31_wide(TILE_16), make='strings')
case('tile-k45-ragged', 'count_scan', 45, 'ragged', 1517, two_words(TILE_16), make='strings')
case('tile-k19-ragged', 'count_scan', 19, 'ragged', 1517, one_word(TILE_8), make='strings')           # m = 9, w = 11

# ---- S2 -------------------------------------------------------------------------------------------------------------------------------
# (<2>, <3> and <4> of the sorted split are in every row above)  KV_SKM_S2=plain: the plain split, and no 16-byte records
case('split-plain-k31', 'count_scan', 31, 100, 3000, {'count': [LANE_1_8, PLAIN, COUNT_31, LOOSE_COUNT_1], 'scan': [NOVEL_1, LOOSE_NOVEL_1]}, KV_SKM_S2='plain')
case('split-plain-k51', 'count_scan', 51, 150, 3000, {'count': [LANE_2_16, PLAIN, COUNT_51, LOOSE_COUNT_2], 'scan': [NOVEL_2, LOOSE_NOVEL_2]}, KV_SKM_S2='plain')

# ---- S3 -------------------------------------------------------------------------------------------------------------------------------
# (COUNT_C_31, COUNT_31, COUNT_51, COUNT_1 and COUNT_2 are in the rows above)
case('count-k31-any-k-compact', 'count_scan', 31, 100, 3000, {'count': [LANE_1_8, SORT_2, COUNT_C, LOOSE_COUNT_1], 'scan': [LANE_1_8, SORT_3, NOVEL_1, LOOSE_NOVEL_1]}, KV_SKM_ANY_K='1')
case('count-k31-any-k', 'count_scan', 31, 100, 3000, {'count': [LANE_1_8, SORT_3, COUNT_1, LOOSE_COUNT_1], 'scan': [LIST_1, LOOSE_NOVEL_1]}, hint=True, KV_SKM_ANY_K='1')
case('count-k51-any-k', 'count_scan', 51, 150, 3000, {'count': [LANE_2_16, SORT_4, COUNT_2, LOOSE_COUNT_2], 'scan': [NOVEL_2, LOOSE_NOVEL_2]}, KV_SKM_ANY_K='1')
# one key in 64 refused by the LDS tables: those occurrences travel through the loose list, one at a time
case('count-k31-force-loose-compact', 'count_scan', 31, 100, 3000, {'count': [LANE_1_8, SORT_2, COUNT_C_LOOSE, LOOSE_COUNT_1], 'scan': [LANE_1_8, SORT_3, NOVEL_1, LOOSE_NOVEL_1]},
     KV_SKM_FORCE_LOOSE='1')
case('count-k31-force-loose', 'count_scan', 31, 100, 3000, {'count': [LANE_1_8, SORT_3, COUNT_1_LOOSE, LOOSE_COUNT_1], 'scan': [LIST_1, LOOSE_NOVEL_1]}, hint=True, KV_SKM_FORCE_LOOSE='1')
case('count-k25-force-loose', 'count_scan', 25, 100, 3000, {'count': [WAVE_8, SORT_3, COUNT_1_LOOSE, LOOSE_COUNT_1], 'scan': [NOVEL_1, LOOSE_NOVEL_1]}, KV_SKM_FORCE_LOOSE='1')
case('count-k51-force-loose', 'count_scan', 51, 150, 3000, {'count': [LANE_2_16, SORT_4, COUNT_2_LOOSE, LOOSE_COUNT_2], 'scan': [LIST_2, LOOSE_NOVEL_2]}, hint=True, KV_SKM_FORCE_LOOSE='1')
# undersized segments: whole records through the loose list in S1 and S2
case('count-k31-cap30', 'count_scan', 31, 100, 3000, k31_compact(LANE_1_8), KV_SKM_CAP_PCT='30')
case('count-k51-cap30', 'count_scan', 51, 150, 3000, k51(LANE_2_16), KV_SKM_CAP_PCT='30')
# The fixed-k instances count a key's occurrences in 16 bits.  547 poly-A reads of 150 bases hold 547 x 120 = 65640 = 65536 + 104 occurrences
# of one 31-mer; 656 hold 656 x 100 = 65600 = 65536 + 64 of one 51-mer: a count that wrapped would leave 104 / 64 in a counter that must
# saturate at 255.  With buckets whose segments hold fewer than 65536 k-mers (nwg2 x cap2 x ncap: a few thousand here) the fixed-k instance
# runs and the surplus of that one bucket travels through the loose list; with one bucket for everything (nwg2 x cap2 x ncap is two
# million) the guard in kv_consume_skm must choose the generic instance.
case('count-k31-65640-compact', 'count_scan', 31, 'polyA_547', 3547, k31_compact(LANE_1_16), buckets='4096')
case('count-k31-65640', 'count_scan', 31, 'polyA_547', 3547, {'count': [LANE_1_16, SORT_3, COUNT_31, LOOSE_COUNT_1], 'scan': [LIST_1, LOOSE_NOVEL_1]}, buckets='4096', hint=True)
case('count-k31-65640-one-bucket-compact', 'count_scan', 31, 'polyA_547', 3547,
     {'count': [LANE_1_16, SORT_2, COUNT_C, LOOSE_COUNT_1], 'scan': [LANE_1_16, SORT_3, NOVEL_1, LOOSE_NOVEL_1]}, buckets=ONE_BUCKET)
case('count-k31-65640-one-bucket', 'count_scan', 31, 'polyA_547', 3547, {'count': [LANE_1_16, SORT_3, COUNT_1, LOOSE_COUNT_1], 'scan': [LIST_1, LOOSE_NOVEL_1]}, buckets=ONE_BUCKET, hint=True)
case('count-k51-65600', 'count_scan', 51, 'polyA_656', 3656, k51(LANE_2_16), buckets='4096')
case('count-k51-65600-one-bucket', 'count_scan', 51, 'polyA_656', 3656, {'count': [LANE_2_16, SORT_4, COUNT_2, LOOSE_COUNT_2], 'scan': [NOVEL_2, LOOSE_NOVEL_2]}, buckets=ONE_BUCKET)

# ---- scans with thresholds and controls -----------------------------------------------------------------------------------------------
case('trio-walk-k31', 'trio', 31, 100, 4000, {'count': [LANE_1_8, SORT_2, COUNT_C_31, LOOSE_COUNT_1], 'case': [LANE_1_8, SORT_2, COUNT_C_31, LOOSE_COUNT_1],
                                              'scan': [LANE_1_8, SORT_3, NOVEL_1, LOOSE_NOVEL_1]})
case('trio-walk-k25', 'trio', 25, 100, 4000, {'count': [WAVE_8, SORT_3, COUNT_1, LOOSE_COUNT_1], 'case': [WAVE_8, SORT_3, COUNT_1, LOOSE_COUNT_1], 'scan': [NOVEL_1, LOOSE_NOVEL_1]})
case('trio-walk-k51', 'trio', 51, 150, 4000, {'count': [LANE_2_16, SORT_4, COUNT_51, LOOSE_COUNT_2], 'case': [LANE_2_16, SORT_4, COUNT_51, LOOSE_COUNT_2], 'scan': [NOVEL_2, LOOSE_NOVEL_2]})
case('trio-list-k31', 'trio', 31, 100, 4000, {'count': [LANE_1_8, SORT_2, COUNT_C_31, LOOSE_COUNT_1], 'case': [LANE_1_8, SORT_3, COUNT_31, LOOSE_COUNT_1], 'scan': [LIST_1, LOOSE_NOVEL_1]},
     hint=True)
case('trio-list-k51', 'trio', 51, 150, 4000, {'count': [LANE_2_16, SORT_4, COUNT_51, LOOSE_COUNT_2], 'case': [LANE_2_16, SORT_4, COUNT_51, LOOSE_COUNT_2], 'scan': [LIST_2, LOOSE_NOVEL_2]},
     hint=True)
# (k-mers the count's tables refused are not in the distinct list: k_skm_loose_novel evaluates them)
case('trio-list-k31-force-loose', 'trio', 31, 100, 4000, {'count': [LANE_1_8, SORT_2, COUNT_C_LOOSE, LOOSE_COUNT_1], 'case': [LANE_1_8, SORT_3, COUNT_1_LOOSE, LOOSE_COUNT_1],
                                                          'scan': [LIST_1, LOOSE_NOVEL_1]}, hint=True, KV_SKM_FORCE_LOOSE='1')
case('trio-list-k51-force-loose', 'trio', 51, 150, 4000, {'count': [LANE_2_16, SORT_4, COUNT_2_LOOSE, LOOSE_COUNT_2], 'case': [LANE_2_16, SORT_4, COUNT_2_LOOSE, LOOSE_COUNT_2],
                                                          'scan': [LIST_2, LOOSE_NOVEL_2]}, hint=True, KV_SKM_FORCE_LOOSE='1')
case('trio-walk-k31-cap30', 'trio', 31, 100, 4000, {'count': [LANE_1_8, SORT_2, COUNT_C_31, LOOSE_COUNT_1], 'case': [LANE_1_8, SORT_2, COUNT_C_31, LOOSE_COUNT_1],
                                                    'scan': [LANE_1_8, SORT_3, NOVEL_1, LOOSE_NOVEL_1]}, KV_SKM_CAP_PCT='30')
case('trio-walk-k51-cap30', 'trio', 51, 150, 4000, {'count': [LANE_2_16, SORT_4, COUNT_51, LOOSE_COUNT_2], 'case': [LANE_2_16, SORT_4, COUNT_51, LOOSE_COUNT_2],
                                                    'scan': [NOVEL_2, LOOSE_NOVEL_2]}, KV_SKM_CAP_PCT='30')

# ---- the deduplicated route and the minimizer exchange -------------------------------------------------------------------------------
case('route-k31', 'route', 31, 100, 3000, {'route': [LANE_1_8, SORT_3, ROUTE_1, LOOSE_ROUTE_1]}, KV_ROUTE_PATH='skm')
case('route-k51', 'route', 51, 150, 3000, {'route': [LANE_2_16, SORT_4, ROUTE_2, LOOSE_ROUTE_2]}, KV_ROUTE_PATH='skm')
case('route-k31-cap30', 'route', 31, 100, 3000, {'route': [LANE_1_8, SORT_3, ROUTE_1, LOOSE_ROUTE_1]}, KV_ROUTE_PATH='skm', KV_SKM_CAP_PCT='30')
# kv_mex_emit cuts with the 1024-thread wave kernel where the lane cut does not apply; the owner splits, combines and answers the scan
case('exchange-k31', 'exchange', 31, 100, 3000, {'emit': [LANE_1_8], 'route': [SORT_3, ROUTE_1, LOOSE_ROUTE_1], 'set_scan': [SET_1, LOOSE_SET_1]})
case('exchange-k51', 'exchange', 51, 150, 3000, {'emit': [LANE_2_16], 'route': [SORT_4, ROUTE_2, LOOSE_ROUTE_2], 'set_scan': [SET_2, LOOSE_SET_2]})
case('exchange-k25', 'exchange', 25, 100, 3000, {'emit': [WAVE_8_1024], 'route': [SORT_3, ROUTE_1, LOOSE_ROUTE_1], 'set_scan': [SET_1, LOOSE_SET_1]})
case('exchange-k40', 'exchange', 40, 100, 3000, {'emit': [WAVE_16_1024], 'route': [SORT_4, ROUTE_2, LOOSE_ROUTE_2], 'set_scan': [SET_2, LOOSE_SET_2]})
case('exchange-k31-L250', 'exchange', 31, 250, 1500, {'emit': [WAVE_8_1024], 'route': [SORT_3, ROUTE_1, LOOSE_ROUTE_1], 'set_scan': [SET_1, LOOSE_SET_1]})
# hk.mex_plan(short=True): 16-byte records through the exchange, either split
case('exchange-short-k31', 'exchange', 31, 100, 3000, {'emit': [LANE_1_8], 'route': [SORT_2, ROUTE_C, LOOSE_ROUTE_1]}, short=True)
case('exchange-short-k31-plain', 'exchange', 31, 100, 3000, {'emit': [LANE_1_8], 'route': [PLAIN_C, ROUTE_C, LOOSE_ROUTE_1]}, short=True, KV_SKM_S2='plain')
case('exchange-k51-plain', 'exchange', 51, 150, 3000, {'emit': [LANE_2_16], 'route': [PLAIN, ROUTE_2, LOOSE_ROUTE_2], 'set_scan': [SET_2, LOOSE_SET_2]}, KV_SKM_S2='plain')

assert len({c['id'] for c in CASES}) == len(CASES)


def declared_instances():
    """every instance some row expects"""
    return {name for c in CASES for names in c['expect'].values() for name in names}


def rows_by_instance():
    """instance -> ids of the rows that expect it"""
    out = {}
    for c in CASES:
        for names in c['expect'].values():
            for name in names:
                if c['id'] not in out.setdefault(name, []):
                    out[name].append(c['id'])
    return out


if __name__ == '__main__':              # python tests/instances_common.py: every instance with the rows that reach it
    for name, ids in sorted(rows_by_instance().items()):
        print('{:45s} {:3d}  {}'.format(name, len(ids), ' '.join(ids[:6]) + (' ...' if len(ids) > 6 else '')))
