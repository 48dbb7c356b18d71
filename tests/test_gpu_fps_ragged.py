"""``ws3d_furthest_point_sampling_ragged`` (csrc/fps_ragged.hip): clouds of different sizes in ONE call, every row bit-equal to the
C oracle and to the per-cloud kernel on that cloud alone -- on both sides of every block-size step, of the 1024 cap and of the
kernel's on-chip limit, with exact ties (tests/ragged_clouds.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ragged_clouds as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def limit():
    from ws3d_amd import pn2_ops
    value = pn2_ops.fps_ragged_limit()
    assert 1024 < value <= 16384
    return value


def _run(cs, m):
    from ws3d_amd import pn2_ops
    xyz, offsets = rc.packed(cs)
    idx = pn2_ops.furthest_point_sample_ragged(torch.from_numpy(xyz).cuda(), torch.from_numpy(offsets).cuda(), m)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (len(cs), m)
    return idx.cpu().numpy()


def _differing(got, want, cs):
    bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i], want[i])]
    return ["cloud %d (%d points)" % (i, cs[i].shape[0]) for i in bad]


@pytest.mark.parametrize("m", rc.MS)
def test_rows_match_oracle_and_the_per_cloud_kernel(limit, m):
    from ws3d_amd import pn2_ops
    cs = rc.clouds(limit)
    got = _run(cs, m)
    assert not _differing(got, rc.expected(limit, m), cs)
    alone = np.stack([pn2_ops.furthest_point_sample(torch.from_numpy(c[None].copy()).cuda(), m)[0].cpu().numpy() for c in cs])
    assert not _differing(got, alone, cs)


def test_cloud_order_does_not_matter(limit):
    cs = rc.clouds(limit)
    got = _run(cs[::-1], 100)
    assert not _differing(got[::-1], rc.expected(limit, 100), cs)


def test_forwarded_clouds_up_to_16384_points(oracle):
    """clouds above the on-chip limit take the per-cloud kernels (8192: the pruned kernel's range, 16384: its upper end) between
    clouds the ragged kernel samples itself, in one call"""
    from ws3d_amd import synth
    cs = [synth.roi_clouds(1, n, 70 + j)[0] for j, n in enumerate((700, 16384, 333, 8192, 4000))]
    got = _run(cs, 100)
    want = np.stack([oracle.furthest_point_sample(c[None], 100)[0] for c in cs])
    assert not _differing(got, want, cs)


def test_no_clouds_and_bad_sizes_launch_nothing(limit):
    """clouds == 0 succeeds; a cloud without points or with fewer than m is refused by the entry before any launch: idx keeps its
    sentinel, also for the valid clouds of the same call"""
    from ws3d_amd import _lib, pn2_ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    empty = pn2_ops.furthest_point_sample_ragged(torch.zeros((0, 3), device=dev), torch.zeros(1, dtype=torch.int32, device=dev), 8)
    assert tuple(empty.shape) == (0, 8)
    assert lib.ws3d_furthest_point_sampling_ragged(0, None, None, 8, None, None, None) == 0
    xyz = torch.from_numpy(rc.clouds(limit)[0][:60].copy()).to(dev)
    for sizes, m in (([40, 0, 20], 4), ([50, 10], 16)):
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
        idx = torch.full((len(sizes), m), -7, dtype=torch.int32, device=dev)
        host = (ctypes.c_int32 * len(sizes))(*sizes)
        rc_ = lib.ws3d_furthest_point_sampling_ragged(len(sizes), offsets.data_ptr(), ctypes.cast(host, ctypes.c_void_p), m, xyz.data_ptr(),
                                                      idx.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc_ == _lib.E_INVALID and b"invalid" in lib.ws3d_last_error()
        assert bool((idx == -7).all())
    with pytest.raises(ValueError):
        pn2_ops.furthest_point_sample_ragged(xyz, torch.tensor([0, 50, 60], dtype=torch.int32, device=dev), 16)
