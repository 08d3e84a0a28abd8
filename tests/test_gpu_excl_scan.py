"""kv_excl_scan_u32 (kv_scan.hip): the one counts-to-bases kernel -- exclusive scan of n uint32 counts into n + 1 uint64
bases, the total last.  The novel scan places its hits per tile with it and the FASTQ reader its lines per 16-KB chunk
(more than 1024 chunks is a text no ingest test reaches).  One workgroup of 16 waves takes 8192 counts a round, a wave
512 of them 64 at a time, and asks for the next round's counts ahead: the sizes sit at those edges."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16385, 3 * 8192 + 700]
CASES = [('random', n) for n in SIZES] + [('zeros', 8193), ('ones', 8193)]


def make_counts(fill, n):
    if fill == 'random':         # the full uint32 range: from 64 counts on the totals pass 2^32
        return np.random.default_rng(1000 + n).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return np.full(n, 0 if fill == 'zeros' else 0xffffffff, dtype=np.uint32)


@pytest.mark.parametrize('fill,n', CASES)
def test_bases_equal_cumsum(hk, fill, n):
    import torch
    from kevlar_amd import _lib
    counts = make_counts(fill, n)
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_base = torch.full((n + 1,), -1, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.load().kv_excl_scan_u32(d_counts.data_ptr() if n else None, n, d_base.data_ptr()))
    got = d_base.cpu().numpy().view(np.uint64)
    want = np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(counts, dtype=np.uint64)))
    assert got.dtype == want.dtype and got.shape == want.shape == (n + 1,)
    assert np.array_equal(got, want)
    if fill == 'random' and n >= 64:
        assert int(want[-1]) > 2 ** 32
