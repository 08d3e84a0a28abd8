"""No GPU: the template instances the launch sites of kv_skm.hip can launch are exactly the instances the case table of
tests/instances_common.py declares -- none without a row, none that no launch site names.  There are no exceptions: whoever adds an
instance adds a row (tests/test_gpu_skm_instances.py then runs it against the oracle), whoever removes one removes its rows."""
import os
import re

from conftest import ROOT
from instances_common import CASES, declared_instances

SOURCE = os.path.join(ROOT, 'kevlar_amd', 'csrc', 'kv_skm.hip')


def launch_sites():
    """(instances named through SKM_INST, super-k-mer kernels launched without it)"""
    text = open(SOURCE).read()
    named = {re.sub(r'\s+', '', m) for m in re.findall(r'\bSKM_INST\(\s*(k_skm_[^()]*?)\s*\)', text)}
    direct = set(re.findall(r'hipLaunchKernelGGL\(\s*\(*\s*(k_skm_\w+)', text))
    return named, direct


def test_every_instance_a_launch_site_names_has_a_row_and_no_row_names_another():
    named, direct = launch_sites()
    assert len(named) >= 41, sorted(named)
    declared = declared_instances()
    assert named - declared == set(), 'instances without a row in tests/instances_common.py: {}'.format(sorted(named - declared))
    assert declared - named == set(), 'rows name instances no launch site has: {}'.format(sorted(declared - named))
    # a super-k-mer kernel launched by its bare name would not be reported: only the one-thread flag forwarder is (it has no instances)
    assert direct == {'k_skm_forward_flag'}, sorted(direct)


def test_the_pointer_and_its_name_are_one_expression():
    """SKM_INST stringifies the very expression it hands to skm_inst, and every launch takes its pointer from skm_launching, which
    notes that name: the report cannot name another kernel than the one launched"""
    text = open(SOURCE).read()
    assert re.search(r'#define SKM_INST\(\.\.\.\) skm_inst\(__VA_ARGS__, #__VA_ARGS__\)', text)
    named, _ = launch_sites()
    families = {name.split('<')[0] for name in named}
    # every launch of one of these families goes through skm_launching (the loose kernels inside skm_launch_loose, the route inside skm_launch_route)
    for m in re.finditer(r'hipLaunchKernelGGL\(([^;]*);', text):
        if any(re.search(r'\b' + f + r'\b', m.group(1)) for f in families):
            raise AssertionError('launched without skm_launching: ' + m.group(0)[:120])
    assert len(re.findall(r'hipLaunchKernelGGL\(skm_launching\(', text)) >= 10


def test_every_row_is_well_formed():
    entries = {'count_scan': {'count', 'scan'}, 'trio': {'count', 'case', 'scan'}, 'route': {'route'}}
    for row in CASES:
        if row['entry'] == 'exchange':
            assert set(row['expect']) in ({'emit', 'route'}, {'emit', 'route', 'set_scan'}), row['id']
            assert row['short'] == ('set_scan' not in row['expect']), row['id']
        else:
            assert set(row['expect']) == entries[row['entry']], row['id']
        assert 1 <= row['n'] <= 4000 or row['id'].endswith('-groups-beyond-the-grid'), row['id']
