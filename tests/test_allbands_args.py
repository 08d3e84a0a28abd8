"""`kevlar novel --all-bands`: the command line, and what it refuses before anything touches a device (no GPU needed)."""
import pytest


BASE = ['novel', '--case', 'case1.fq', '--control', 'ctrl1.fq', '--control', 'ctrl2.fq']


def parse(extra):
    import kevlar_amd
    return kevlar_amd.cli.parser().parse_args(BASE + extra)


def test_parser_takes_the_new_flags():
    args = parse(['--num-bands', '4', '--all-bands', '--distributed', '--dist-backend', 'gloo'])
    assert args.all_bands is True and args.distributed is True and args.dist_backend == 'gloo' and args.num_bands == 4
    args = parse(['--num-bands', '4', '--all-bands', '--dist-backend', 'nccl'])
    assert args.all_bands is True and args.distributed is False and args.dist_backend == 'nccl'
    args = parse([])
    assert args.all_bands is False and args.distributed is False and args.dist_backend is None
    with pytest.raises(SystemExit):
        parse(['--num-bands', '4', '--all-bands', '--dist-backend', 'mpi'])


@pytest.mark.parametrize('extra,match', [
    (['--all-bands'], '--all-bands needs --num-bands'),
    (['--all-bands', '--num-bands', '4', '--band', '2'], '--band cannot be given'),
    (['--all-bands', '--num-bands', '4', '--case-counts', 'kid.ct'], 'out of scope'),
    (['--all-bands', '--num-bands', '4', '--control-counts', 'mom.ct', 'dad.ct'], 'out of scope'),
    (['--all-bands', '--num-bands', '4', '--save-case-counts', 'kid.ct'], 'out of scope'),
    (['--all-bands', '--num-bands', '4', '--save-ctrl-counts', 'mom.ct', 'dad.ct'], 'out of scope'),
    (['--all-bands', '--num-bands', '4', '--ref-band-quirk'], '--ref-band-quirk'),
    (['--distributed', '--num-bands', '4', '--band', '1'], '--distributed shares the bands of an --all-bands run'),
])
def test_refused_combinations_raise_before_any_device_call(monkeypatch, extra, match):
    """every refusal is a ValueError from novel.main, raised before a sketch, a batch or a process group exists: the input
    files do not exist, no device is asked for, torch.distributed is not imported"""
    import sys
    import kevlar_amd
    from kevlar_amd import _lib

    def no_device(*_):
        raise AssertionError('a refused combination reached the device')
    monkeypatch.setattr(_lib, 'require_device', no_device)
    had_dist = 'torch.distributed' in sys.modules
    with pytest.raises(ValueError, match=match):
        kevlar_amd.novel.main(parse(extra))
    assert had_dist or 'torch.distributed' not in sys.modules


def test_band_flags_without_all_bands_raise_as_before(monkeypatch):
    import kevlar_amd
    from kevlar_amd import _lib
    monkeypatch.setattr(_lib, 'require_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    for extra in (['--band', '1'], ['--num-bands', '4']):
        with pytest.raises(ValueError, match='Must specify --num-bands and --band together'):
            kevlar_amd.novel.main(parse(extra))


def test_band_plan_deals_the_bands_round_robin():
    from kevlar_amd.allbands import band_plan
    assert band_plan(4) == [0, 1, 2, 3]
    assert [band_plan(4, 2, r) for r in range(2)] == [[0, 2], [1, 3]]
    assert [band_plan(4, 3, r) for r in range(3)] == [[0, 3], [1], [2]]
    assert [band_plan(2, 3, r) for r in range(3)] == [[0], [1], []]
    assert sorted(b for r in range(5) for b in band_plan(8, 5, r)) == list(range(8))


def test_rows_carry_read_and_offset_at_full_width():
    """the travelling form of a batch's runs: four bytes of read, four of offset, the abundances -- nothing packed into 16 bits"""
    import numpy as np
    from kevlar_amd.allbands import _rows
    runs = [(np.array([0, 4294967295], dtype=np.uint32), np.array([65536, 4000000000], dtype=np.uint32), np.array([[7, 0, 0], [9, 1, 0]], dtype=np.uint8)),
            (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.uint8)),
            (np.array([5], dtype=np.uint32), np.array([3], dtype=np.uint32), np.array([[8, 0, 1]], dtype=np.uint8))]
    rows = _rows(runs, 3)
    assert rows.shape == (3, 11) and rows.dtype == np.uint8
    assert np.ascontiguousarray(rows[:, 0:4]).view('<u4').reshape(-1).tolist() == [0, 4294967295, 5]
    assert np.ascontiguousarray(rows[:, 4:8]).view('<u4').reshape(-1).tolist() == [65536, 4000000000, 3]
    assert rows[:, 8:].tolist() == [[7, 0, 0], [9, 1, 0], [8, 0, 1]]
    assert _rows([], 3).shape == (0, 11)
