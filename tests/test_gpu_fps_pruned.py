"""GPU parity of the pruned furthest point sampling for 16385 .. 65536 points (csrc/fps_pruned.hip, ws3d_furthest_point_sampling_ws):
indices, the min-distance buffer and the gathered centres against the oracle and against the plain entry, bit for bit -- ragged
sizes, pure ties, degenerate boxes, a caller's initial temp, the forwarding rules, the Python route, the other distance conventions.
Small m keeps the oracle cheap; every case is a few seconds at the most."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ws3d_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from ws3d_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def oracle():
    import oracle as o
    o.set_threads(max(1, min(o.max_threads(), 64)))
    yield o
    o.set_threads(1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_ws(lib, pcs, m, temp="1e10", ws="full", gather=True):
    """ws3d_furthest_point_sampling_ws on pcs (B, N, 3) -> (rc, idx, temp or None, new_xyz or None, workspace was written).
    temp: "1e10" (filled), None (NULL) or an array (B, N); ws: "full", None (NULL) or a number of bytes to hand over"""
    B, N, _ = pcs.shape
    x = dev(pcs.astype(np.float32))
    t = None if temp is None else (torch.full((B, N), 1e10, device="cuda") if isinstance(temp, str) else dev(temp))
    idx = torch.full((B, m), -7, dtype=torch.int32, device="cuda")
    nx = torch.full((B, m, 3), -7.0, device="cuda") if gather else None
    full = int(lib.ws3d_fps_workspace_bytes(B, N))
    nbytes = full if ws == "full" else (0 if ws is None else int(ws))
    buf = None if ws is None else torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device="cuda")
    p = lambda a: None if a is None else a.data_ptr()
    rc = lib.ws3d_furthest_point_sampling_ws(B, N, m, p(x), p(t), p(idx), p(nx), p(buf), nbytes, _stream())
    torch.cuda.synchronize()
    written = buf is not None and bool((buf != 0xA5).any().item())
    return rc, host(idx), None if t is None else host(t), None if nx is None else host(nx), written


def run_plain(lib, pcs, m, temp="1e10"):
    """the plain entry (the parent's kernels) on the same inputs -> (rc, idx, temp or None, new_xyz)"""
    B, N, _ = pcs.shape
    x = dev(pcs.astype(np.float32))
    t = None if temp is None else (torch.full((B, N), 1e10, device="cuda") if isinstance(temp, str) else dev(temp))
    idx = torch.full((B, m), -7, dtype=torch.int32, device="cuda")
    nx = torch.full((B, m, 3), -7.0, device="cuda")
    rc = lib.ws3d_furthest_point_sampling_gather(B, N, m, x.data_ptr(), None if t is None else t.data_ptr(), idx.data_ptr(), nx.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, host(idx), None if t is None else host(t), host(nx)


def check_against_oracle(lib, oracle, pcs, m):
    pcs = np.ascontiguousarray(pcs, dtype=np.float32)
    ref, ref_temp = oracle.furthest_point_sample(pcs, m, return_temp=True)
    rc, idx, temp, nx, written = run_ws(lib, pcs, m)
    assert rc == 0 and written, "the pruned kernels did not run"
    np.testing.assert_array_equal(idx, ref)
    np.testing.assert_array_equal(temp, ref_temp)
    np.testing.assert_array_equal(nx, np.stack([pcs[b][ref[b]] for b in range(pcs.shape[0])]))


def two_scenes(n, seed):
    return np.stack([synth.lidar_cloud(n, seed)[:, :3], synth.make_batch("lidar", 1, n, seed + 1, dup_frac=0.05)[0, :, :3]]).astype(np.float32)


# (16385: one point in the last bucket; 16448 = 257 * 64; 20000: deep in the pruned regime; 32769, 50001: ragged; 65536: the largest)
@pytest.mark.parametrize("N,M", [(16385, 2048), (16448, 1024), (20000, 4096), (32769, 512), (50001, 300), (65536, 1024)])
def test_against_the_oracle(lib, oracle, N, M):
    check_against_oracle(lib, oracle, two_scenes(N, 7100 + N % 89), M)


def test_every_point_gets_selected(lib, oracle):
    """m = n = 16385: the sweep runs down to zero distances, where duplicates tie"""
    pcs = synth.make_batch("lidar", 1, 16385, 7201, dup_frac=0.05)[:, :, :3]
    check_against_oracle(lib, oracle, pcs, 16385)


def test_pure_ties_repeated_points(lib, oracle):
    """260 distinct points, each 64 times, shuffled: from step 260 on every running distance is 0 and the rank alone decides"""
    r = np.random.Generator(np.random.PCG64(7301))
    base = r.uniform(-20.0, 20.0, (260, 3)).astype(np.float32)
    assert len(np.unique(base, axis=0)) == 260
    pts = np.repeat(base, 64, axis=0)[r.permutation(260 * 64)]
    check_against_oracle(lib, oracle, pts[None], 520)


def test_pure_ties_one_point(lib, oracle):
    pts = np.tile(np.array([[1.5, -0.25, 20.0]], dtype=np.float32), (16385, 1))
    check_against_oracle(lib, oracle, pts[None], 200)


def test_ties_integer_lattice(lib, oracle):
    """26^3 = 17576 lattice points, shuffled: many equal distances at every step"""
    r = np.random.Generator(np.random.PCG64(7303))
    g = np.stack(np.meshgrid(np.arange(26), np.arange(26), np.arange(26), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    check_against_oracle(lib, oracle, g[r.permutation(len(g))][None], 700)


def test_degenerate_boxes(lib, oracle):
    """a line along y (one (x, z) cell holds the scene) and a plane of constant x (one row of cells)"""
    r = np.random.Generator(np.random.PCG64(7401))
    n = 17000
    line = np.stack([np.full(n, 3.0), r.uniform(-3.0, 1.0, n), np.full(n, 30.0)], -1).astype(np.float32)
    plane = np.stack([np.full(n, -2.0), r.uniform(-3.0, 1.0, n), r.uniform(0.0, 70.0, n)], -1).astype(np.float32)
    check_against_oracle(lib, oracle, np.stack([line, plane]), 400)


def test_initial_temp(lib):
    """a caller's temp in [0, 1]: everything equals the plain entry (the parent's kernel) given the same buffer; NULL == 1e10"""
    r = np.random.Generator(np.random.PCG64(7501))
    pcs = two_scenes(20000, 7502)
    t0 = r.uniform(0.0, 1.0, (2, 20000)).astype(np.float32)
    rc, idx, temp, nx, written = run_ws(lib, pcs, 600, temp=t0)
    rc0, idx0, temp0, nx0 = run_plain(lib, pcs, 600, temp=t0)
    assert rc == 0 and rc0 == 0 and written
    np.testing.assert_array_equal(idx, idx0)
    np.testing.assert_array_equal(temp, temp0)
    np.testing.assert_array_equal(nx, nx0)
    assert not np.array_equal(temp0, t0)

    rc1, idx1, temp1, nx1, w1 = run_ws(lib, pcs, 600, temp=None)
    rc2, idx2, temp2, nx2, w2 = run_ws(lib, pcs, 600, temp="1e10")
    assert rc1 == 0 and rc2 == 0 and w1 and w2 and temp1 is None
    np.testing.assert_array_equal(idx1, idx2)
    np.testing.assert_array_equal(nx1, nx2)
    # and without the gathered centres
    rc3, idx3, _, nx3, w3 = run_ws(lib, pcs, 600, temp=None, gather=False)
    assert rc3 == 0 and w3 and nx3 is None
    np.testing.assert_array_equal(idx3, idx2)


@pytest.mark.parametrize("case", ["null", "short", "n16384", "n70000"])
def test_forwarding(lib, case):
    """no usable workspace, or n outside (16384, 65536]: the entry IS the plain one (same outputs, WS3D_OK, workspace untouched)"""
    N = {"n16384": 16384, "n70000": 70000}.get(case, 20000)
    pcs = two_scenes(N, 7600 + N % 89)
    full = int(lib.ws3d_fps_workspace_bytes(2, N))
    assert (full == 0) == (case in ("n16384", "n70000"))
    ws = {"null": None, "short": full - 1}.get(case, 1 << 20)
    rc, idx, temp, nx, written = run_ws(lib, pcs, 300, ws=ws)
    rc0, idx0, temp0, nx0 = run_plain(lib, pcs, 300)
    assert rc == 0 and rc0 == 0 and not written
    np.testing.assert_array_equal(idx, idx0)
    np.testing.assert_array_equal(temp, temp0)
    np.testing.assert_array_equal(nx, nx0)


def test_python_route_and_the_switch(lib, tmp_path):
    """compat.furthest_point_sampling_gather at n = 20000 equals the _ws entry; a fresh process with WS3D_FPS_PRUNED=0 (the parent's
    kernel through the same wrapper) returns the same indices"""
    from ws3d_amd import compat
    pcs = two_scenes(20000, 7700)
    M = 500
    rc, idx, temp, nx, written = run_ws(lib, pcs, M)
    assert rc == 0 and written
    x = dev(pcs)
    t = torch.full((2, 20000), 1e10, device="cuda")
    gi = torch.empty((2, M), dtype=torch.int32, device="cuda")
    gx = torch.empty((2, M, 3), device="cuda")
    compat.furthest_point_sampling_gather(2, 20000, M, x, t, gi, gx)
    np.testing.assert_array_equal(host(gi), idx)
    np.testing.assert_array_equal(host(t), temp)
    np.testing.assert_array_equal(host(gx), nx)
    wi = torch.empty((2, M), dtype=torch.int32, device="cuda")
    compat.furthest_point_sampling_wrapper(2, 20000, M, x, None, wi)
    np.testing.assert_array_equal(host(wi), idx)

    np.save(tmp_path / "pcs.npy", pcs)
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {ROOT!r})
        from ws3d_amd import compat
        pcs = np.load({str(tmp_path / "pcs.npy")!r})
        idx = torch.empty((2, {M}), dtype=torch.int32, device="cuda"); nx = torch.empty((2, {M}, 3), device="cuda")
        compat.furthest_point_sampling_gather(2, 20000, {M}, torch.from_numpy(pcs).cuda(), None, idx, nx)
        np.save({str(tmp_path / "idx.npy")!r}, idx.cpu().numpy())
        print("PLAIN_OK")
    """)
    r = subprocess.run([sys.executable, "-B", "-c", code], env=dict(os.environ, WS3D_FPS_PRUNED="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLAIN_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
    np.testing.assert_array_equal(np.load(tmp_path / "idx.npy"), idx)


@pytest.mark.parametrize("mode", [1, 2])
def test_alternative_distance_conventions_subprocess(mode):
    """libws3d_hip_dm<N>.so against the oracle built under the SAME convention, (20000, 1024), through the _ws entry"""
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {ROOT!r})
        import oracle
        from ws3d_amd import synth, _lib
        lib = _lib.load()
        assert lib.ws3d_dist_mode() == {mode} and oracle.dist_mode() == {mode}
        oracle.set_threads(max(1, min(oracle.max_threads(), 64)))
        N, M = 20000, 1024
        pcs = np.stack([synth.lidar_cloud(N, 7800)[:, :3], synth.make_batch("lidar", 1, N, 7801, dup_frac=0.05)[0, :, :3]]).astype(np.float32)
        ref, ref_temp = oracle.furthest_point_sample(pcs, M, return_temp=True)
        x = torch.from_numpy(pcs).cuda()
        t = torch.full((2, N), 1e10, device="cuda")
        idx = torch.empty((2, M), dtype=torch.int32, device="cuda"); nx = torch.empty((2, M, 3), device="cuda")
        nbytes = int(lib.ws3d_fps_workspace_bytes(2, N))
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = lib.ws3d_furthest_point_sampling_ws(2, N, M, x.data_ptr(), t.data_ptr(), idx.data_ptr(), nx.data_ptr(), ws.data_ptr(), nbytes,
                                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and nbytes > 0 and bool((ws != 0xA5).any().item())
        assert np.array_equal(idx.cpu().numpy(), ref), "idx"
        assert np.array_equal(t.cpu().numpy(), ref_temp), "temp"
        assert np.array_equal(nx.cpu().numpy(), np.stack([pcs[b][ref[b]] for b in range(2)])), "new_xyz"
        print("DIST_MODE_OK")
    """)
    r = subprocess.run([sys.executable, "-B", "-c", code], env=dict(os.environ, WS3D_DIST_MODE=str(mode)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIST_MODE_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
