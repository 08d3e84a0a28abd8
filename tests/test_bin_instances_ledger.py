"""No GPU: the template instances the launch sites of kv_binned.hip can launch are exactly the instances the case table of
tests/bin_instances_common.py declares -- none without a row, none that no launch site names.  There are no exceptions: whoever adds
an instance adds a row (tests/test_gpu_bin_instances.py then runs it against the oracle), whoever removes one removes its rows."""
import os
import re

from bin_instances_common import BOUNDARY_PRIMES, CASES, GEOMETRIES, N_HASHES, N_READS, SMALL, WIDE, declared_instances
from conftest import ROOT

CSRC = os.path.join(ROOT, 'kevlar_amd', 'csrc')
SOURCE = os.path.join(CSRC, 'kv_binned.hip')


def launch_sites(path=SOURCE):
    """(instances named through BIN_INST, bin-stage kernels launched without it)"""
    text = open(path).read()
    named = {re.sub(r'\s+', '', m) for m in re.findall(r'\bBIN_INST\(\s*(k_bin_[^()]*?)\s*\)', text)}
    direct = set(re.findall(r'hipLaunchKernelGGL\(\s*\(*\s*(k_bin_\w+)', text))
    return named, direct


def test_every_instance_a_launch_site_names_has_a_row_and_no_row_names_another():
    named, direct = launch_sites()
    assert len(named) >= 25, sorted(named)
    declared = declared_instances()
    assert named - declared == set(), 'instances without a row in tests/bin_instances_common.py: {}'.format(sorted(named - declared))
    assert declared - named == set(), 'rows name instances no launch site has: {}'.format(sorted(declared - named))
    # a bin-stage kernel launched by its bare name would not be reported
    assert direct == set(), sorted(direct)


def test_no_other_source_launches_a_bin_stage_kernel():
    """the super-k-mer count reaches stages B and C through kv_bin_finish alone: the kernels live in kv_binned.hip's unnamed namespace"""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')) and name != 'kv_binned.hip':
            text = open(os.path.join(CSRC, name)).read()
            assert not re.search(r'hipLaunchKernelGGL\([^;]*\bk_bin_\w+', text), name
            assert 'BIN_INST(' not in text, name


def test_the_pointer_and_its_name_are_one_expression():
    """BIN_INST stringifies the very expression it hands on, and every launch takes its pointer from bin_launching, which notes that
    name: the report cannot name another kernel than the one launched"""
    text = open(SOURCE).read()
    assert re.search(r'#define BIN_INST\(\.\.\.\) bin_inst\(__VA_ARGS__, #__VA_ARGS__\)', text)
    assert re.search(r'bin_inst\(F \*fn, const char \*name\) \{ return kv_inst\(fn, name\); \}', text)
    header = open(os.path.join(CSRC, 'kv_binned.h')).read()
    assert re.search(r'kv_inst\(F \*fn, const char \*name\) \{ return KvInst<F>\{fn, name\}; \}', header)
    named, _ = launch_sites()
    families = {name.split('<')[0] for name in named}
    assert families == {'k_bin_hash_2bit', 'k_bin_hash_direct', 'k_bin_list', 'k_bin_split', 'k_bin_apply', 'k_bin_spill'}
    launches = re.findall(r'hipLaunchKernelGGL\(([^;]*);', text)
    for args in launches:
        assert args.startswith('bin_launching('), 'launched without bin_launching: ' + args[:120]
    # stage A from reads' 2-bit form, from their text and from a list; stages B and C; the spill list
    assert len(launches) == 6
    # the name is noted where the pointer is handed out, nowhere else
    assert len(re.findall(r'\.note\(', text)) == 1 and re.search(r'list\.note\(k\.name\);\s*return k\.fn;', text)


def test_the_list_is_emptied_where_every_partitioned_count_begins():
    """kv_bin_plan is the first step of kv_consume_binned and of the super-k-mer count's bin stages, and begins the list before it can fail"""
    text = open(SOURCE).read()
    plan = text[text.index('int kv_bin_plan('):text.index('int kv_bin_finish(')]
    assert plan.index('launched.list.begin();') < plan.index('return KV_ERR_CAPACITY;')
    consume = text[text.index('int kv_consume_binned('):]
    assert consume.index('kv_bin_plan(') < consume.index('bin_launching(')
    skm = open(os.path.join(CSRC, 'kv_skm.hip')).read()
    count = skm[skm.index('int kv_consume_skm('):]
    assert count.index('kv_bin_plan(') < count.index('kv_bin_finish(')


def test_the_primes_are_what_the_table_says(ok):
    """lo(S), lo2(S): what both prime searches give below S x 2^16; hi(S): the smallest prime beyond it, by trial division"""
    from kevlar_amd import khmer as hk

    def divisor(n):
        return next((d for d in range(3, int(n ** 0.5) + 2, 2) if n % d == 0), None)
    for s, (lo, lo2, hi) in BOUNDARY_PRIMES.items():
        assert hk.primes_below(s << 16, 2) == ok.primes_below(s << 16, 2) == [lo, lo2], s
        assert (lo + 65535) >> 16 == (lo2 + 65535) >> 16 == s and (hi + 65535) >> 16 == s + 1
        assert hi % 2 == 1 and divisor(hi) is None, hi
        assert all(divisor(n) is not None for n in range((s << 16) + 1, hi, 2)), s
    assert hk.primes_below(14 << 16, 2) == ok.primes_below(14 << 16, 2) == SMALL['primes']


def test_every_row_is_well_formed():
    ids = [row['id'] for row in CASES]
    for row in CASES:
        limit = N_HASHES if row['entry'] == 'list' else N_READS
        assert 1 <= row['n'] <= limit or row['big'], row['id']
        maxsl, cmax, F, C, ringB, threadsA = row['plan']
        assert maxsl == max((p + 65535) >> 16 for p in row['primes']), row['id']
        assert (threadsA, cmax <= 32) in ((512, True), (1024, False)) and C <= cmax and (C - 1) * F < maxsl <= C * F, row['id']
        assert ringB & (ringB - 1) == 0 and (32 if row['weighted'] or row['path'] == 'skm' else 64) <= ringB <= 4096, row['id']
        # stage A runs with the plan's workgroup size, and a row that says 'weighted' expects the weighted stages
        stage_a = [name for name in row['expect'] if name.startswith(('k_bin_hash', 'k_bin_list'))]
        assert len(stage_a) == (0 if row['path'] == 'skm' else 1), row['id']
        assert all('<{},'.format(threadsA) in name for name in stage_a), row['id']
        w = 'true' if row['weighted'] or row['path'] == 'skm' else 'false'
        assert row['expect'][-3] == 'k_bin_split<{}>'.format(w) and row['expect'][-2].endswith(',{}>'.format(w)) and row['expect'][-1] == 'k_bin_spill', row['id']
    # every geometry through its four entries, from both sides of every boundary
    for gid, cls, primes, plan, ring_w, why in GEOMETRIES:
        assert all(gid + tail in ids for tail in ('-packed', '-skm', '-list', '-listw')), gid
    assert sorted(BOUNDARY_PRIMES) == [1, 4, 16, 32, 64, 128, 256, 512, 1024, 1536, 12288, 16384]
    assert all(lo2 < lo <= (s << 16) < hi for s, (lo, lo2, hi) in BOUNDARY_PRIMES.items())
    assert WIDE['primes'] == [BOUNDARY_PRIMES[16384][2], BOUNDARY_PRIMES[16384][0]] and SMALL['plan'][0] == 14
