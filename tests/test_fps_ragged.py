"""``pn2_ops.furthest_point_sample_ragged`` on CPU tensors (the numpy route ``ws3d_amd.fps_host``, what the loader processes and a
device-less database build use) against the C oracle, cloud by cloud, bit for bit."""
import numpy as np
import pytest
import torch

from tests import ragged_clouds as rc


@pytest.fixture(scope="module")
def limit():
    from ws3d_amd import _lib
    value = int(_lib.load().ws3d_fps_ragged_limit())     # a host function: no device needed
    assert 1024 < value <= 16384
    return value


@pytest.mark.parametrize("m", rc.MS)
def test_numpy_route_matches_oracle(limit, m):
    from ws3d_amd import pn2_ops
    xyz, offsets = rc.packed(rc.clouds(limit))
    got = pn2_ops.furthest_point_sample_ragged(torch.from_numpy(xyz), torch.from_numpy(offsets), m)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(rc.clouds(limit)), m)
    want = rc.expected(limit, m)
    bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i].numpy(), want[i])]
    assert not bad, "clouds %s (sizes %s) differ from the oracle" % (bad, [rc.clouds(limit)[i].shape[0] for i in bad])


def test_entry_validates_before_any_hip_call():
    """like the other entries (tests/test_abi.py): bad sizes and the empty call are decided on the host, so they are testable here"""
    import ctypes
    from ws3d_amd import _lib
    lib = _lib.load()
    assert lib.ws3d_furthest_point_sampling_ragged(0, None, None, 8, None, None, None) == 0
    buf = (ctypes.c_float * 64)()
    for sizes, m in (([4, 0, 2], 2), ([5, 1], 3)):
        host = (ctypes.c_int32 * len(sizes))(*sizes)
        args = [ctypes.cast(p, ctypes.c_void_p) for p in (buf, host, buf, buf)]
        assert lib.ws3d_furthest_point_sampling_ragged(len(sizes), args[0], args[1], m, args[2], args[3], None) == _lib.E_INVALID
        assert b"invalid" in lib.ws3d_last_error()


def test_numpy_route_arguments():
    from ws3d_amd import pn2_ops
    xyz = torch.zeros((10, 3))
    assert tuple(pn2_ops.furthest_point_sample_ragged(torch.zeros((0, 3)), torch.zeros(1, dtype=torch.int32), 4).shape) == (0, 4)
    with pytest.raises(ValueError):
        pn2_ops.furthest_point_sample_ragged(xyz, torch.tensor([0, 3, 10], dtype=torch.int32), 4)       # a cloud smaller than m
    with pytest.raises(ValueError):
        pn2_ops.furthest_point_sample_ragged(xyz, torch.tensor([0, 10, 10], dtype=torch.int32), 1)      # an empty cloud

