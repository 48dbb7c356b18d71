"""GPU parity: the HIP kernels (through the C ABI of libws3d_hip.so) against the CPU
oracle on the same seeded inputs.  Bit-exact for every index/mask output and for the
pure-copy float outputs; 1e-5 for interpolated features (BASELINE.json north_star)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import helpers as H  # noqa: E402
from ws3d_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from ws3d_amd import compat, iou3d_ops, pn2_modules, pn2_ops, roipool3d_ops
    import types
    return types.SimpleNamespace(pn=pn2_ops, mod=pn2_modules, iou=iou3d_ops, roi=roipool3d_ops, c=compat)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------- FPS
FPS_CASES = [
    # (B, N, M, kind, dup_frac)
    (2, 64, 64, "uniform", 0.0), (3, 100, 37, "uniform", 0.0), (2, 256, 64, "lidar", 0.0),
    (2, 512, 128, "lidar", 0.0), (2, 1000, 250, "lidar", 0.1), (2, 1024, 256, "uniform", 0.0),
    (2, 1025, 100, "uniform", 0.0), (2, 2048, 256, "lidar", 0.05), (2, 3000, 100, "lidar", 0.0),
    (2, 4096, 1024, "lidar", 0.02), (1, 5000, 64, "uniform", 0.0), (1, 8192, 128, "lidar", 0.0),
    (2, 16384, 4096, "lidar", 0.02), (1, 16384, 4096, "uniform", 0.0), (1, 12345, 777, "lidar", 0.3),
    (1, 20000, 64, "lidar", 0.0), (1, 65536, 48, "uniform", 0.0),
    (2, 16384, 4096, "hdl64", 0.0), (1, 4096, 1024, "hdl64", 0.0),      # KITTI's density (ray-cast scan): near-range rings, long empty stretches
]


@pytest.mark.parametrize("B,N,M,kind,dup", FPS_CASES)
def test_fps_bit_exact(ops, oracle, B, N, M, kind, dup):
    pcs = synth.make_batch(kind, B, N, 7, dup_frac=dup)[:, :, :3].copy()
    ref = oracle.furthest_point_sample(pcs, M)
    got = ops.pn.furthest_point_sample(dev(pcs), M)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, M)
    np.testing.assert_array_equal(host(got), ref)
    if N <= 16384:
        idx2, new_xyz = ops.pn.furthest_point_sample_gather(dev(pcs), M)
        np.testing.assert_array_equal(host(idx2), ref)
        np.testing.assert_array_equal(host(new_xyz), np.stack([pcs[b][ref[b]] for b in range(B)]))


@pytest.mark.parametrize("case", ["dups", "lattice", "all_same", "two_points", "one_point"])
def test_fps_ties(ops, oracle, case):
    rng = np.random.default_rng(5)
    if case == "dups":
        base = synth.lidar_cloud(300, 9)[:, :3]
        xyz, m = base[rng.integers(0, 300, 1500)], 400
    elif case == "lattice":
        g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1)
        xyz, m = g.reshape(-1, 3).astype(np.float32)[rng.permutation(4096)], 600
    elif case == "all_same":
        xyz, m = np.ones((130, 3), dtype=np.float32), 20
    elif case == "two_points":
        xyz, m = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float32), 2
    else:
        xyz, m = np.array([[3, 2, 1]], dtype=np.float32), 1
    xyz = np.ascontiguousarray(xyz[None])
    np.testing.assert_array_equal(host(ops.pn.furthest_point_sample(dev(xyz), m)),
                                  oracle.furthest_point_sample(xyz, m))


def test_fps_bucket_kernel_subprocess(oracle, tmp_path):
    """the pruned (bucket) FPS kernel forced for every cloud of 4097..16384 points (env var read once per
    process): run it in a child and compare with the oracle, incl. heavy duplication (tie rounds)"""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [(2, 16384, 1024, "lidar", 0.02), (1, 5000, 300, "uniform", 0.0), (1, 12345, 777, "lidar", 0.3)]
    refs = []
    for i, (B, N, M, kind, dup) in enumerate(cases):
        pcs = synth.make_batch(kind, B, N, 7, dup_frac=dup)[:, :, :3].copy()
        np.save(tmp_path / f"in{i}.npy", pcs)
        refs.append(oracle.furthest_point_sample(pcs, M))
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {root!r})
        from ws3d_amd import pn2_ops
        for i, M in enumerate({[c[2] for c in cases]!r}):
            x = torch.from_numpy(np.load({str(tmp_path)!r} + f"/in{{i}}.npy")).cuda()
            idx, new_xyz = pn2_ops.furthest_point_sample_gather(x, M)
            np.save({str(tmp_path)!r} + f"/out{{i}}.npy", idx.cpu().numpy())
            np.save({str(tmp_path)!r} + f"/xyz{{i}}.npy", new_xyz.cpu().numpy())
    """)
    r = subprocess.run([sys.executable, "-B", "-c", code], env=dict(os.environ, WS3D_FPS_BUCKET="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(np.load(tmp_path / f"out{i}.npy"), ref)
        pcs = np.load(tmp_path / f"in{i}.npy")
        np.testing.assert_array_equal(np.load(tmp_path / f"xyz{i}.npy"),
                                      np.stack([pcs[b][ref[b]] for b in range(pcs.shape[0])]))


def test_fps_two_scenes_per_cu_kernel_subprocess(ops, oracle, tmp_path):
    """fps_zlds_kernel (z in LDS, two workgroups per CU; chosen when the batch exceeds the CU count)
    forced with WS3D_FPS_PAIR=1 in a child process: indices, gathered centres and the final
    min-distance buffer against the oracle, incl. duplicated points and a ragged size"""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [(3, 16384, 4096, "lidar", 0.02), (1, 12345, 777, "lidar", 0.3), (2, 9000, 300, "uniform", 0.0)]
    refs = []
    for i, (B, N, M, kind, dup) in enumerate(cases):
        pcs = synth.make_batch(kind, B, N, 11, dup_frac=dup)[:, :, :3].copy()
        np.save(tmp_path / f"in{i}.npy", pcs)
        refs.append(oracle.furthest_point_sample(pcs, M, return_temp=True))
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {root!r})
        from ws3d_amd import compat
        for i, M in enumerate({[c[2] for c in cases]!r}):
            x = torch.from_numpy(np.load({str(tmp_path)!r} + f"/in{{i}}.npy")).cuda()
            B, N = x.shape[0], x.shape[1]
            idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); nx = torch.empty((B, M, 3), device="cuda")
            temp = torch.full((B, N), 1e10, device="cuda")
            compat.furthest_point_sampling_gather(B, N, M, x, temp, idx, nx)
            np.save({str(tmp_path)!r} + f"/out{{i}}.npy", idx.cpu().numpy())
            np.save({str(tmp_path)!r} + f"/xyz{{i}}.npy", nx.cpu().numpy())
            np.save({str(tmp_path)!r} + f"/tmp{{i}}.npy", temp.cpu().numpy())
    """)
    r = subprocess.run([sys.executable, "-B", "-c", code], env=dict(os.environ, WS3D_FPS_PAIR="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for i, (ref, ref_temp) in enumerate(refs):
        np.testing.assert_array_equal(np.load(tmp_path / f"out{i}.npy"), ref)
        pcs = np.load(tmp_path / f"in{i}.npy")
        np.testing.assert_array_equal(np.load(tmp_path / f"xyz{i}.npy"),
                                      np.stack([pcs[b][ref[b]] for b in range(pcs.shape[0])]))
        np.testing.assert_array_equal(np.load(tmp_path / f"tmp{i}.npy"), ref_temp)


FPS_ENV_VARIANTS = [
    {"WS3D_FPS_PAIR": "1"},                              # two scenes per CU (the dense kernel's form for more scenes than CUs)
    {"WS3D_FPS_BUCKET": "0"},                            # dense sweep also where the pruned kernels are the default
    {"WS3D_FPS_BUCKET": "1"},                            # pruned kernels for every cloud of 4097..16384 points
    {"WS3D_FPS_BUCKET": "1", "WS3D_FPS_ROUNDS": "0"},    # ... one sample per record exchange (round 2's kernel; serves m > 6144 by default)
]


@pytest.mark.parametrize("env", FPS_ENV_VARIANTS, ids=lambda e: ",".join(f"{k[9:]}={v}" for k, v in e.items()))
def test_fps_kernel_variants_subprocess(oracle, tmp_path, env):
    """every selectable FPS kernel / geometry (environment switches are read once per process): indices, gathered centres
    and the final min-distance buffer against the oracle, over shapes that reach every template instance"""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [(1, 40000, 150, "lidar", 0.02), (1, 20000, 100, "uniform", 0.0), (2, 16384, 1500, "lidar", 0.02), (1, 12345, 400, "lidar", 0.3), (2, 8192, 300, "uniform", 0.0), (2, 4096, 500, "lidar", 0.05),
             (2, 3000, 200, "lidar", 0.0), (2, 2048, 256, "lidar", 0.05), (2, 1025, 100, "uniform", 0.0), (2, 1000, 250, "lidar", 0.1),
             (2, 512, 128, "lidar", 0.0), (3, 200, 60, "uniform", 0.2), (2, 100, 37, "uniform", 0.0), (2, 64, 64, "uniform", 0.0)]
    refs = []
    for i, (B, N, M, kind, dup) in enumerate(cases):
        pcs = synth.make_batch(kind, B, N, 13, dup_frac=dup)[:, :, :3].copy()
        np.save(tmp_path / f"in{i}.npy", pcs)
        refs.append(oracle.furthest_point_sample(pcs, M, return_temp=True))
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {root!r})
        from ws3d_amd import compat
        for i, M in enumerate({[c[2] for c in cases]!r}):
            x = torch.from_numpy(np.load({str(tmp_path)!r} + f"/in{{i}}.npy")).cuda()
            B, N = x.shape[0], x.shape[1]
            idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); nx = torch.empty((B, M, 3), device="cuda")
            temp = torch.full((B, N), 1e10, device="cuda")
            compat.furthest_point_sampling_gather(B, N, M, x, temp, idx, nx)
            np.save({str(tmp_path)!r} + f"/out{{i}}.npy", idx.cpu().numpy())
            np.save({str(tmp_path)!r} + f"/xyz{{i}}.npy", nx.cpu().numpy())
            np.save({str(tmp_path)!r} + f"/tmp{{i}}.npy", temp.cpu().numpy())
    """)
    r = subprocess.run([sys.executable, "-B", "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for i, (ref, ref_temp) in enumerate(refs):
        np.testing.assert_array_equal(np.load(tmp_path / f"out{i}.npy"), ref, err_msg=str(cases[i]))
        pcs = np.load(tmp_path / f"in{i}.npy")
        np.testing.assert_array_equal(np.load(tmp_path / f"xyz{i}.npy"), np.stack([pcs[b][ref[b]] for b in range(pcs.shape[0])]))
        np.testing.assert_array_equal(np.load(tmp_path / f"tmp{i}.npy"), ref_temp, err_msg=str(cases[i]))


@pytest.mark.parametrize("mode", [1, 2])
def test_alternative_distance_conventions_subprocess(tmp_path, mode):
    """libws3d_hip_dm<N>.so (WS3D_DIST_MODE=N: the squared distance spelled without / with the other FMA contraction) against
    the oracle built under the SAME convention: FPS (every kernel family), ball query (grid, slabs, brute force), 3-NN"""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {root!r})
        import oracle
        from ws3d_amd import compat, synth, _lib
        assert _lib.load().ws3d_dist_mode() == {mode} and oracle.dist_mode() == {mode}
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        for (B, N, M) in [(2, 16384, 1200), (2, 4096, 600), (2, 1000, 250), (3, 200, 60)]:
            pcs = synth.make_batch("lidar", B, N, 21, dup_frac=0.02)[:, :, :3].copy()
            ref = oracle.furthest_point_sample(pcs, M)
            idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); nx = torch.empty((B, M, 3), device="cuda")
            compat.furthest_point_sampling_gather(B, N, M, dev(pcs), None, idx, nx)
            assert np.array_equal(idx.cpu().numpy(), ref), ("fps", N)
            new = np.stack([pcs[b][ref[b]] for b in range(B)])
            for r, ns in ((0.1, 16), (0.7, 32)):
                want = oracle.ball_query(r, ns, pcs, new)
                x, c = dev(pcs), dev(new)
                for srt in ((compat.sort_points_x(x, grid=True), compat.sort_points_x(x, grid=False), None) if N >= 2048 else (None,)):
                    got = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
                    compat.ball_query_wrapper(B, N, M, r, ns, c, x, got, srt)
                    assert np.array_equal(got.cpu().numpy(), want), ("ball_query", N, r)
            d2, i3 = oracle.three_nn_dist2(pcs, new)
            gd = torch.empty((B, N, 3), device="cuda"); gi = torch.empty((B, N, 3), dtype=torch.int32, device="cuda")
            for srt in (compat.sort_points_xz(dev(new)), None):
                compat.three_nn_wrapper(B, N, M, dev(pcs), dev(new), gd, gi, srt)
                assert np.array_equal(gi.cpu().numpy(), i3) and np.array_equal(gd.cpu().numpy(), d2), ("three_nn", N)
        print("DIST_MODE_OK")
    """)
    r = subprocess.run([sys.executable, "-B", "-c", code], env=dict(os.environ, WS3D_DIST_MODE=str(mode)), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "DIST_MODE_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_fps_temp_contract(ops, oracle):
    """the wrapper-level entry point takes the caller's temp (pre-filled 1e10) and leaves the
    final running min-distance in it, like the reference kernel does (sampling_gpu.cu:134-135)."""
    pcs = synth.make_batch("lidar", 2, 3000, 11)[:, :, :3].copy()
    idx_ref, temp_ref = oracle.furthest_point_sample(pcs, 99, return_temp=True)
    x = dev(pcs)
    temp = torch.full((2, 3000), 1e10, device="cuda")
    idx = torch.empty((2, 99), dtype=torch.int32, device="cuda")
    ops.c.furthest_point_sampling_wrapper(2, 3000, 99, x, temp, idx)
    np.testing.assert_array_equal(host(idx), idx_ref)
    np.testing.assert_array_equal(host(temp), temp_ref)


# ------------------------------------------------------------------------------- ball query / group
# (the shapes of the ball-query tests live in tests/helpers.py: tests/test_ballquery_plan.py checks on the CPU that they reach every search kernel)
@pytest.mark.parametrize("B,N,M,r,ns,kind", H.BQ_CASES)
def test_ball_query_and_group_bit_exact(ops, oracle, B, N, M, r, ns, kind):
    pc = synth.make_batch(kind, B, N, 21)
    xyz = pc[:, :, :3].copy()
    feats = np.ascontiguousarray(np.transpose(
        np.concatenate([pc[:, :, 3:], np.random.default_rng(1).standard_normal((B, N, 4)).astype(np.float32)], 2),
        (0, 2, 1)))
    cidx = oracle.furthest_point_sample(xyz, M)
    new_xyz = np.stack([xyz[b][cidx[b]] for b in range(B)])
    ref_idx = oracle.ball_query(r, ns, xyz, new_xyz)
    got_idx = ops.pn.ball_query(r, ns, dev(xyz), dev(new_xyz))
    np.testing.assert_array_equal(host(got_idx), ref_idx)
    # grouping_operation (pure copy)
    ref_g = oracle.grouping_operation(feats, ref_idx)
    got_g = ops.pn.grouping_operation(dev(feats), got_idx)
    np.testing.assert_array_equal(host(got_g), ref_g)
    # fused QueryAndGroup == reference composition (pointnet2_utils.py:241-264)
    xyz_t = np.ascontiguousarray(np.transpose(xyz, (0, 2, 1)))
    ref_xyz = oracle.grouping_operation(xyz_t, ref_idx) - np.transpose(new_xyz, (0, 2, 1))[..., None]
    ref_fused = np.concatenate([ref_xyz, ref_g], 1)
    fused, idx_f = ops.pn.query_and_group(r, ns, dev(xyz), dev(new_xyz), dev(feats), True, return_idx=True)
    np.testing.assert_array_equal(host(idx_f), ref_idx)
    np.testing.assert_array_equal(host(fused), ref_fused)
    qg = ops.pn.QueryAndGroup(r, ns, use_xyz=True)
    np.testing.assert_array_equal(host(qg(dev(xyz), dev(new_xyz), dev(feats))), ref_fused)
    np.testing.assert_array_equal(host(qg(dev(xyz), dev(new_xyz), None)), ref_xyz)
    qg2 = ops.pn.QueryAndGroup(r, ns, use_xyz=False)
    np.testing.assert_array_equal(host(qg2(dev(xyz), dev(new_xyz), dev(feats))), ref_g)


@pytest.mark.parametrize("N,M,r,ns,kind", H.BQ_SLAB_CASES)
def test_ball_query_sorted_slab_equals_bruteforce(ops, oracle, N, M, r, ns, kind):
    """the x-sorted slab path, the LDS-tiled brute-force path and the oracle agree bit for bit,
    including slabs longer than the fallback threshold (r=50) and heavy duplication"""
    if kind == "dups":
        base = synth.lidar_cloud(64, 3)[:, :3]
        xyz = base[np.random.default_rng(0).integers(0, 64, N)][None].copy()
    else:
        xyz = synth.make_batch(kind, 1, N, 33)[:, :, :3].copy()
    xyz = np.ascontiguousarray(np.concatenate([xyz, xyz[:, ::-1]], 0))  # 2 scenes
    cidx = oracle.furthest_point_sample(xyz, M)
    new_xyz = np.stack([xyz[b][cidx[b]] for b in range(2)])
    ref = oracle.ball_query(r, ns, xyz, new_xyz)
    x, c = dev(xyz), dev(new_xyz)
    # fine (x, z) grid flavour (the default of sort_points_x): permutation of the scene, 16-bit cell starts non-decreasing
    grid = ops.c.sort_points_x(x, grid=True)
    assert grid is not None
    gstride = grid.numel() // 2
    for sc in range(2):
        raw = host(grid[sc * gstride:(sc + 1) * gstride])
        pts = raw[:N * 16].view(np.float32).reshape(N, 4)
        np.testing.assert_array_equal(np.sort(pts[:, 3].view(np.int32)), np.arange(N))
        np.testing.assert_array_equal(pts[:, :3], xyz[sc][pts[:, 3].view(np.int32)])
        hdr = raw[N * 16:N * 16 + 16]
        gx = -int(hdr[12:16].view(np.int32)[0])
        gz = int(raw[N * 16 + 16 + 65540:N * 16 + 16 + 65552].view(np.int32)[2])
        assert gx > 0 and gz > 0 and gx * gz <= 32768
        start16 = raw[N * 16 + 16:N * 16 + 16 + 2 * (gx * gz + 1)].view(np.uint16).astype(np.int64)
        assert start16[0] == 0 and start16[-1] == N and (np.diff(start16) >= 0).all()
    g = torch.zeros((2, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(2, N, M, r, ns, c, x, g, grid)
    np.testing.assert_array_equal(host(g), ref)
    d3 = torch.empty((2, M, 3), device="cuda"); i3 = torch.empty((2, M, 3), dtype=torch.int32, device="cuda")
    ops.c.three_nn_wrapper(2, M, N, c, x, d3, i3, grid)          # a grid-flavour buffer handed to three_nn stays exact
    rd, ri = oracle.three_nn_dist2(new_xyz, xyz)
    np.testing.assert_array_equal(host(i3), ri)
    np.testing.assert_array_equal(host(d3), rd)
    srt = ops.c.sort_points_x(x, grid=False)
    assert srt is not None
    stride = srt.numel() // 2
    for sc in range(2):  # binned copy: a permutation of the scene, cell starts non-decreasing, x grouped by cell
        raw = host(srt[sc * stride:(sc + 1) * stride])
        pts = raw[:N * 16].view(np.float32).reshape(N, 4)
        np.testing.assert_array_equal(np.sort(pts[:, 3].view(np.int32)), np.arange(N))
        np.testing.assert_array_equal(pts[:, :3], xyz[sc][pts[:, 3].view(np.int32)])
        start = raw[N * 16 + 16:N * 16 + 16 + 2049 * 4].view(np.int32)
        assert start[0] == 0 and start[-1] == N and (np.diff(start) >= 0).all()
        cell_of = np.searchsorted(start, np.arange(N), side="right") - 1
        xmax_per_cell = np.maximum.accumulate(np.where(np.diff(start) > 0, np.maximum.reduceat(
            pts[:, 0], np.minimum(start[:-1], N - 1)), -np.inf))
        assert (pts[:, 0] >= np.concatenate([[-np.inf], xmax_per_cell[:-1]])[cell_of] - 1e-3).all()
    a = torch.zeros((2, M, ns), dtype=torch.int32, device="cuda")
    bb = torch.zeros((2, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(2, N, M, r, ns, c, x, a, srt)
    ops.c.ball_query_wrapper(2, N, M, r, ns, c, x, bb, None)
    np.testing.assert_array_equal(host(a), ref)
    np.testing.assert_array_equal(host(bb), ref)


@pytest.mark.parametrize("N,M,r,ns,kind", H.BQ_DENSE_CASES)
def test_ball_query_grid_one_wave_per_centre_dense_lists(ops, oracle, N, M, r, ns, kind):
    """the fine-grid ball query with one WAVE per centre (threshold selection of the nsample smallest indices) on clouds with KITTI's
    density -- tens to hundreds of hits per ball -- against the oracle: lists bit-exact, through the plain and the fill entry, the
    fused grouping and the brute-force kernel.  'clump': 7000 points inside a 0.5 m cube (more hits than the wave's LDS list holds ->
    the ordered 64-wide scan); r = 60: more candidates than the grid walk accepts; 'narrow': a 2 m wide strip (many grid rows per ball)"""
    rng = np.random.default_rng(7)
    if kind == "dups":
        base = synth.hdl64_cloud(16384, 3)[:64, :3]
        xyz = base[rng.integers(0, 64, N)][None].copy()
    elif kind == "clump":
        xyz = synth.hdl64_cloud(N, 41)[None, :, :3].copy()
        where = rng.choice(N, 7000, replace=False)
        xyz[0, where] = (np.array([3.0, 1.0, 12.0]) + rng.uniform(-0.25, 0.25, (7000, 3))).astype(np.float32)
    elif kind == "narrow":
        xyz = synth.hdl64_cloud(N, 43)[None, :, :3].copy()
        xyz[0, :, 0] = (xyz[0, :, 0] * np.float32(0.025)).astype(np.float32)
    else:
        xyz = synth.hdl64_cloud(N, 40)[None, :, :3].copy() if N == 16384 else synth.hdl64_cloud(16384, 40)[None, :N, :3].copy()
    xyz = np.ascontiguousarray(np.concatenate([xyz, xyz[:, ::-1]], 0))  # 2 scenes
    cidx = oracle.furthest_point_sample(xyz, M)
    new_xyz = np.stack([xyz[b][cidx[b]] for b in range(2)])
    ref = oracle.ball_query(r, ns, xyz, new_xyz)
    distinct = (np.diff(ref, axis=2) > 0).sum(2) + 1
    x, c = dev(xyz), dev(new_xyz)
    grid = ops.c.sort_points_x(x, grid=True)
    assert grid is not None
    g = torch.zeros((2, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(2, N, M, r, ns, c, x, g, grid)
    np.testing.assert_array_equal(host(g), ref)
    np.testing.assert_array_equal(host(ops.c.ball_query_lists(r, ns, x, c, grid)), ref)
    # lists + their distinct (centre, source) pairs in one launch == ball_query_lists + compact_pairs
    both = ops.c.ball_query_pairs(r, ns, x, c, grid)
    assert both is not None
    np.testing.assert_array_equal(host(both[0]), ref)
    rc_, rs_, tot_ = both[1]
    T = int(tot_.item())
    want_pairs = sorted((cm, int(v)) for cm in range(2 * M) for v in ref.reshape(2 * M, ns)[cm][:distinct.reshape(-1)[cm]])
    got_pairs = list(zip(host(rc_)[:T].tolist(), host(rs_)[:T].tolist()))
    assert T == len(want_pairs) and sorted(got_pairs) == want_pairs
    pos = {}
    for i_, (cm, _) in enumerate(got_pairs):
        pos.setdefault(cm, []).append(i_)
    assert all(v == list(range(v[0], v[0] + len(v))) for v in pos.values())        # a centre's compact rows are contiguous
    # both scales of a level in ONE launch (ws3d_ball_query_pairs2): this scale beside a second one of another radius / nsample, in
    # either slot -- the lists of both and their pair tables are those of the single-scale calls
    r2, ns2 = (r * 3.0, 16) if ns != 16 else (r * 0.5, 32)
    ref2 = oracle.ball_query(r2, ns2, xyz, new_xyz)
    for order in ((0, 1), (1, 0)):
        rr, nn = [(r, r2)[k] for k in order], [(ns, ns2)[k] for k in order]
        dual = ops.c.ball_query_pairs2(rr, nn, x, c, grid)
        assert dual is not None
        for k, (lst, (rc2, rs2, tot2)) in zip(order, dual):
            want_l = (ref, ref2)[k]
            np.testing.assert_array_equal(host(lst), want_l)
            d2_ = (np.diff(want_l, axis=2) > 0).sum(2) + 1
            n2_ = (ns, ns2)[k]
            wp = sorted((cm, int(v)) for cm in range(2 * M) for v in want_l.reshape(2 * M, n2_)[cm][:d2_.reshape(-1)[cm]])
            T2 = int(tot2.item())
            assert T2 == len(wp) and sorted(zip(host(rc2)[:T2].tolist(), host(rs2)[:T2].tolist())) == wp
    bb = torch.zeros((2, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(2, N, M, r, ns, c, x, bb, None)
    np.testing.assert_array_equal(host(bb), ref)
    feat = dev(rng.standard_normal((2, N, 8)).astype(np.float32))
    gl = ops.c.query_and_group_nlc(r, ns, x, c, feat, True, grid)                # fused emit behind the same search
    li = torch.from_numpy(ref.astype(np.int64)).cuda().view(2, M * ns, 1)
    want = torch.cat((torch.gather(x, 1, li.expand(2, M * ns, 3)).view(2, M, ns, 3) - c.unsqueeze(2),
                      torch.gather(feat, 1, li.expand(2, M * ns, 8)).view(2, M, ns, 8)), dim=3)
    assert torch.equal(gl, want)
    if kind == "hdl64" and N == 16384 and r == 0.5 and ns == 32:
        assert distinct.mean() > 8 and (distinct == ns).mean() > 0.05, "this cloud is supposed to be dense"


def test_ball_query_binned_buffer_of_another_flavour_on_a_noted_address(ops, oracle):
    """the host picks the ball-query kernel from the flavour it noted per buffer ADDRESS; x-slab contents copied into a buffer noted
    as fine-grid (a clone, a recycled allocation) must not be walked as a grid: the kernel reads the header and scans in order"""
    xyz = synth.hdl64_cloud(16384, 44)[None, :, :3].copy()
    cidx = oracle.furthest_point_sample(xyz, 300)
    new_xyz = np.stack([xyz[0][cidx[0]]])
    x, c = dev(xyz), dev(new_xyz)
    grid = ops.c.sort_points_x(x, grid=True)
    slabs = ops.c.sort_points_x(x, grid=False)
    grid.copy_(slabs)
    for ns in H.BQ_FLAVOUR_NS:          # 32: one wave per centre; 72: one lane per centre (ball_query_grid_kernel reads the header too)
        np.testing.assert_array_equal(host(ops.c.ball_query_lists(0.5, ns, x, c, grid)), oracle.ball_query(0.5, ns, xyz, new_xyz))


def _grouped_ref(oracle, xyz, new_xyz, feats_ncl, ref_idx):
    """the reference composition (pointnet2_utils.py:241-264): (B, 3 + C, M, ns) from the oracle's lists"""
    xyz_t = np.ascontiguousarray(np.transpose(xyz, (0, 2, 1)))
    return np.concatenate([oracle.grouping_operation(xyz_t, ref_idx) - np.transpose(new_xyz, (0, 2, 1))[..., None],
                           oracle.grouping_operation(feats_ncl, ref_idx)], 1)


def _pair_set(rowc, rowsrc, total):
    """the compact (centre, source) table as a sorted (total, 2) array: its row order depends on an atomic"""
    t = int(total.item())
    pairs = np.stack([host(rowc[:t]), host(rowsrc[:t])], 1)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def _want_pairs(ref):
    """the distinct entries of every list (the padding repeats the first; a centre without a hit pairs with point 0), sorted"""
    flat = ref.reshape(-1, ref.shape[2])
    distinct = (np.diff(flat, axis=1) > 0).sum(1) + 1
    keep = np.arange(flat.shape[1])[None, :] < distinct[:, None]
    return np.stack([np.broadcast_to(np.arange(flat.shape[0])[:, None], flat.shape)[keep], flat[keep]], 1)


@pytest.fixture(scope="module")
def bq_lane_scenes(oracle):
    """(xyz, new_xyz, 1-channel features, 8-channel rows) per (B, N, M) of H.BQ_LANE_CASES, computed once"""
    out = {}
    for B, N, M, r, ns in H.BQ_LANE_CASES:
        if (B, N, M) not in out:
            base = synth.hdl64_cloud(16384, 46)
            pc = np.stack([base[b::B][:N] for b in range(B)])           # B interleaved sub-scans of one scan: KITTI's density pattern
            xyz = np.ascontiguousarray(pc[:, :, :3])
            cidx = oracle.furthest_point_sample(xyz, M)
            rows = np.random.default_rng(8).standard_normal((B, N, 8)).astype(np.float32)
            out[(B, N, M)] = (xyz, np.stack([xyz[b][cidx[b]] for b in range(B)]), np.ascontiguousarray(np.transpose(pc[:, :, 3:4], (0, 2, 1))), rows)
    return out


@pytest.mark.parametrize("B,N,M,r,ns", H.BQ_LANE_CASES)
def test_ball_query_fine_grid_one_lane_per_centre(ops, oracle, bq_lane_scenes, B, N, M, r, ns):
    """lists longer than 64 entries on a fine-grid buffer take ball_query_grid_kernel (one lane per centre, wave 0 searches): the oracle's
    lists through the plain and the fill entry, the reference composition through both fused entries.  70 centres: a ragged second tile;
    8 / 3 scenes: the XCD-aware and the plain tile decode; r = 60 on 4096 points: more candidates than the grid walk accepts -> the
    ordered scan (tests/test_ballquery_plan.py: these shapes take that kernel)"""
    xyz, new_xyz, feats, rows = bq_lane_scenes[(B, N, M)]
    ref = oracle.ball_query(r, ns, xyz, new_xyz)
    x, c = dev(xyz), dev(new_xyz)
    grid = ops.c.sort_points_x(x, min_n=1, grid=True)
    assert grid is not None
    g = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, c, x, g, grid)
    np.testing.assert_array_equal(host(g), ref)
    np.testing.assert_array_equal(host(ops.c.ball_query_lists(r, ns, x, c, grid)), ref)
    nbr = torch.full((B, M, ns), -7, dtype=torch.int32, device="cuda")
    out = torch.full((B, 4, M, ns), float("nan"), device="cuda")
    ops.c.query_and_group(B, N, M, 1, r, ns, True, x, c, dev(feats), nbr, out, grid)
    np.testing.assert_array_equal(host(nbr), ref)
    np.testing.assert_array_equal(host(out), _grouped_ref(oracle, xyz, new_xyz, feats, ref))
    gl = ops.c.query_and_group_nlc(r, ns, x, c, dev(rows), True, grid)
    want = _grouped_ref(oracle, xyz, new_xyz, np.ascontiguousarray(np.transpose(rows, (0, 2, 1))), ref)
    np.testing.assert_array_equal(host(gl), np.transpose(want, (0, 2, 3, 1)))
    if B == 3 and ns == 72:
        # while a three-scene fine-grid buffer is at hand: the two-scale launch on 8 waves per tile with the plain tile decode
        prev = ops.c.tune("bq_wide_nw", 8)
        try:
            dual = ops.c.ball_query_pairs2((r, 2 * r), (16, 32), x, c, grid)
        finally:
            ops.c.tune("bq_wide_nw", prev)
        assert dual is not None
        for (lst, (rowc, rowsrc, total)), (r2, ns2) in zip(dual, ((r, 16), (2 * r, 32))):
            ref2 = oracle.ball_query(r2, ns2, xyz, new_xyz)
            np.testing.assert_array_equal(host(lst), ref2)
            np.testing.assert_array_equal(_pair_set(rowc, rowsrc, total), _want_pairs(ref2))


def test_ball_query_lists_of_32_bit_indices(ops, oracle):
    """more than 65536 points (no binned copy takes them): ball_query_kernel<int32_t, *> holds its lists as 32-bit indices in LDS --
    the oracle's lists, and the reference composition with 3 + 4 channels"""
    B, N, M, r, ns, C = H.BQ_WIDE_INDEX_CASE
    xyz = synth.hdl64_cloud(N, 47)[None, :, :3].copy()
    # the points past 65535 form a clump of their own, away from the scan: the lists of a centre in it hold indices of 17 bits only
    xyz[0, 65536:] = (np.array([200.0, 0.0, 30.0]) + np.random.default_rng(9).uniform(-0.3, 0.3, (N - 65536, 3))).astype(np.float32)
    new_xyz = np.ascontiguousarray(xyz[:, N - 1 - 911 * np.arange(M)])          # centres spread over the scan, the last point among them
    ref = oracle.ball_query(r, ns, xyz, new_xyz)
    assert ref[0, 0].min() >= 65536 and len(set(ref[0, 0])) == ns
    x, c = dev(xyz), dev(new_xyz)
    assert ops.c.sort_points_x(x) is None
    g = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, c, x, g, None)
    np.testing.assert_array_equal(host(g), ref)
    feats = np.random.default_rng(9).standard_normal((B, C, N)).astype(np.float32)
    nbr = torch.full((B, M, ns), -7, dtype=torch.int32, device="cuda")
    out = torch.full((B, 3 + C, M, ns), float("nan"), device="cuda")
    ops.c.query_and_group(B, N, M, C, r, ns, True, x, c, dev(feats), nbr, out, None)
    np.testing.assert_array_equal(host(nbr), ref)
    np.testing.assert_array_equal(host(out), _grouped_ref(oracle, xyz, new_xyz, feats, ref))


@pytest.mark.parametrize("B,N,M,r,ns", H.BQ_MANY_SCENES_CASES)
def test_ball_query_on_more_tiles_than_the_wide_launch_takes(ops, oracle, B, N, M, r, ns):
    """2048 tiles of 64 centres and more: the one-wave-per-centre kernel on four waves per tile (ball_query_grid_coop_kernel<*, 4>, the
    geometry of the c2 block), lists only, both scales in one launch and fused -- many small scenes, the smallest shape that gets there"""
    base = synth.hdl64_cloud(16384, 48)
    pick = np.random.default_rng(10).integers(0, 16384, (B, N))
    xyz = np.ascontiguousarray(base[pick][:, :, :3])
    feats = np.ascontiguousarray(np.transpose(base[pick][:, :, 3:4], (0, 2, 1)))
    new_xyz = np.ascontiguousarray(xyz[:, ::2][:, :M])
    ref = oracle.ball_query(r, ns, xyz, new_xyz)
    x, c = dev(xyz), dev(new_xyz)
    grid = ops.c.sort_points_x(x, min_n=1, grid=True)
    assert grid is not None
    g = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, c, x, g, grid)
    np.testing.assert_array_equal(host(g), ref)
    dual = ops.c.ball_query_pairs2((r, 2 * r), (ns, 32), x, c, grid)
    assert dual is not None
    for (lst, (rowc, rowsrc, total)), (r2, ns2) in zip(dual, ((r, ns), (2 * r, 32))):
        ref2 = oracle.ball_query(r2, ns2, xyz, new_xyz)
        np.testing.assert_array_equal(host(lst), ref2)
        np.testing.assert_array_equal(_pair_set(rowc, rowsrc, total), _want_pairs(ref2))
    nbr = torch.full((B, M, ns), -7, dtype=torch.int32, device="cuda")
    out = torch.full((B, 4, M, ns), float("nan"), device="cuda")
    ops.c.query_and_group(B, N, M, 1, r, ns, True, x, c, dev(feats), nbr, out, grid)
    np.testing.assert_array_equal(host(nbr), ref)
    np.testing.assert_array_equal(host(out), _grouped_ref(oracle, xyz, new_xyz, feats, ref))


def test_ball_query_no_hit_rows_untouched(ops, oracle):
    xyz = synth.uniform_cloud(300, 5)[None, :, :3].copy()
    far = (xyz[:, :10] + np.float32(1000.0)).copy()
    x, f = dev(xyz), dev(far)
    idx = torch.full((1, 10, 8), 7, dtype=torch.int32, device="cuda")  # NOT zeroed on purpose
    ops.c.ball_query_wrapper(1, 300, 10, 0.5, 8, f, x, idx)
    assert (host(idx) == 7).all()
    assert (host(ops.pn.ball_query(0.5, 8, x, f)) == 0).all()
    # strict '<' at exactly r; fused path groups index 0 for no-hit rows
    p = np.array([[[0, 0, 0], [0.5, 0, 0], [0.25, 0, 0]]], dtype=np.float32)
    got = host(ops.pn.ball_query(0.5, 4, dev(p), dev(p[:, :1])))
    np.testing.assert_array_equal(got[0, 0], [0, 2, 0, 0])
    fused = host(ops.pn.query_and_group(0.5, 8, x, f, None, True))
    np.testing.assert_array_equal(fused, (xyz[0, 0][None, :, None, None] - np.transpose(far, (0, 2, 1))[..., None]) *
                                  np.ones((1, 3, 10, 8), dtype=np.float32))


def test_gather_and_backward_ops(ops, oracle):
    rng = np.random.default_rng(3)
    feat = rng.standard_normal((2, 21, 333)).astype(np.float32)
    gi = rng.integers(0, 333, (2, 50)).astype(np.int32)
    np.testing.assert_array_equal(host(ops.pn.gather_operation(dev(feat), dev(gi))), oracle.gather_operation(feat, gi))
    idx = rng.integers(0, 333, (2, 40, 7)).astype(np.int32)
    f = dev(feat).requires_grad_(True)
    out = ops.pn.grouping_operation(f, dev(idx))
    g = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(dev(g))
    np.testing.assert_allclose(host(f.grad), oracle.grouping_operation_grad(g, idx, 333), rtol=1e-4, atol=1e-5)
    f2 = dev(feat).requires_grad_(True)
    o2 = ops.pn.gather_operation(f2, dev(gi))
    g2 = rng.standard_normal(tuple(o2.shape)).astype(np.float32)
    o2.backward(dev(g2))
    np.testing.assert_allclose(host(f2.grad), oracle.gather_operation_grad(g2, gi, 333), rtol=1e-4, atol=1e-5)
    # fused QueryAndGroup backward == grouping backward on the feature channels
    xyz = synth.lidar_cloud(333, 4)[None, :, :3].repeat(2, 0).copy()
    new_xyz = xyz[:, :40].copy()
    f3 = dev(feat).requires_grad_(True)
    o3, idx3 = ops.pn.query_and_group(1.0, 7, dev(xyz), dev(new_xyz), f3, True, return_idx=True)
    g3 = rng.standard_normal(tuple(o3.shape)).astype(np.float32)
    o3.backward(dev(g3))
    np.testing.assert_allclose(host(f3.grad), oracle.grouping_operation_grad(g3[:, 3:], host(idx3), 333),
                               rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------- three_nn / interpolate
@pytest.mark.parametrize("B,n,m,seed", [(2, 700, 64, 1), (1, 1024, 256, 2), (2, 50, 3, 3), (1, 40, 2, 4),
                                        (1, 10, 1, 5), (1, 16384, 4096, 6), (2, 4096, 1024, 7), (1, 3000, 1500, 8)])
def test_three_nn_bit_exact(ops, oracle, B, n, m, seed):
    unk = synth.make_batch("lidar", B, n, seed)[:, :, :3].copy()
    kidx = oracle.furthest_point_sample(unk, m)
    kn = np.stack([unk[b][kidx[b]] for b in range(B)])
    d2_ref, idx_ref = oracle.three_nn_dist2(unk, kn)
    dist, idx = ops.pn.three_nn(dev(unk), dev(kn))
    np.testing.assert_array_equal(host(idx), idx_ref)
    np.testing.assert_allclose(host(dist), np.sqrt(d2_ref), rtol=1e-6, atol=0)
    d2 = torch.empty((B, n, 3), device="cuda")
    i2 = torch.empty((B, n, 3), dtype=torch.int32, device="cuda")
    ops.c.three_nn_wrapper(B, n, m, dev(unk), dev(kn), d2, i2)
    np.testing.assert_array_equal(host(d2), d2_ref)  # squared distances: bit-exact


@pytest.mark.parametrize("B,n,m,kind,seed", [(2, 4096, 2048, "lidar", 1), (1, 16384, 4096, "lidar", 2), (2, 3000, 2500, "uniform", 3),
                                             (1, 5000, 2048, "dups", 4), (1, 4096, 2100, "line", 5), (1, 2500, 2048, "outside", 6),
                                             (1, 2048, 2048, "samex", 7), (1, 7000, 6000, "lidar", 8),
                                             (1, 500, 3, "uniform", 9), (2, 700, 64, "lidar", 10), (1, 3000, 300, "lattice", 11),
                                             (1, 2048, 2048, "samez", 12), (1, 300, 40, "point", 13), (1, 1200, 1000, "lattice", 14)])
def test_three_nn_binned_search_bit_exact(ops, oracle, B, n, m, kind, seed):
    """the x-binned 3-NN == the full ascending scan, including equal-distance tie-breaks (duplicated
    known points), unknown points outside the known x range (clamped cells), a degenerate x
    extent (one cell) and points strung along x"""
    rng = np.random.default_rng(seed)
    base = synth.make_batch("uniform" if kind == "uniform" else "lidar", B, n, seed + 20)[:, :, :3].copy()
    unk = base
    kn = np.stack([base[b][rng.permutation(n)[:m]] for b in range(B)])
    if kind == "dups":      # every known point 4 times at scattered indices: ties on all three slots
        kn[:, m // 4:] = np.tile(kn[:, :m // 4], (1, 3, 1))[:, :m - m // 4]
        kn = np.stack([kn[b][rng.permutation(m)] for b in range(B)])
    if kind == "line":      # y = z = 0: distance = |dx| only, many exact ties from a regular grid
        kn[:, :, 1:] = 0
        kn[:, :, 0] = (rng.integers(0, 400, (B, m)) * 0.25).astype(np.float32)
        unk[:, :, 1:] = 0
        unk[:, :, 0] = (rng.integers(0, 800, (B, n)) * 0.125).astype(np.float32)
    if kind == "outside":   # unknown x range is 3x the known one
        unk[:, :, 0] *= 3.0
    if kind == "samex":     # all known points share one x: zero-width binning
        kn[:, :, 0] = 1.25
    if kind == "samez":     # ... or one z: a one-row grid
        kn[:, :, 2] = 30.0
    if kind == "point":     # every known point at the same place: a 1 x 1 grid, all distances tie
        kn[:] = kn[:, :1]
    if kind == "lattice":   # integer lattice in (x, z): exact ties between cells of the grid, queries on lattice points too
        kn[:, :, 0] = rng.integers(-20, 20, (B, m)); kn[:, :, 2] = rng.integers(0, 40, (B, m)); kn[:, :, 1] = rng.integers(0, 2, (B, m))
        unk[:, :, 0] = rng.integers(-25, 25, (B, n)) * 0.5; unk[:, :, 2] = rng.integers(-5, 90, (B, n)) * 0.5; unk[:, :, 1] = 0.5
    kn = np.ascontiguousarray(kn.astype(np.float32)); unk = np.ascontiguousarray(unk.astype(np.float32))
    d2_ref, idx_ref = oracle.three_nn_dist2(unk, kn)
    srt = ops.c.sort_points_x(dev(kn), min_n=1)
    grid = ops.c.sort_points_xz(dev(kn), min_n=1)           # the (x, z) grid flavour of the binned known set
    assert srt is not None and grid is not None
    for binned in (srt, grid):
        d2 = torch.full((B, n, 3), float("nan"), device="cuda"); i2 = torch.full((B, n, 3), -7, dtype=torch.int32, device="cuda")
        ops.c.three_nn_wrapper(B, n, m, dev(unk), dev(kn), d2, i2, binned)
        np.testing.assert_array_equal(host(i2), idx_ref)
        np.testing.assert_array_equal(host(d2), d2_ref)
    d2b = torch.empty_like(d2); i2b = torch.empty_like(i2)
    ops.c.three_nn_wrapper(B, n, m, dev(unk), dev(kn), d2b, i2b)          # full scan kernel
    np.testing.assert_array_equal(host(i2b), host(i2))
    dist, idx = ops.pn.three_nn(dev(unk), dev(kn), srt)
    np.testing.assert_array_equal(host(idx), idx_ref)
    # queries taken in the cell order of a binned copy of the UNKNOWN set (ws3d_three_nn_wq), every flavour of that copy: the rows
    # of idx / weight are those of the plain call, bit for bit
    i_plain, w_plain = ops.c.three_nn_with_weights(dev(unk), dev(kn), grid)
    np.testing.assert_array_equal(host(i_plain), idx_ref)
    for q_order in (ops.c.sort_points_x(dev(unk), min_n=1), ops.c.sort_points_x(dev(unk), min_n=1, grid=False), ops.c.sort_points_xz(dev(unk), min_n=1)):
        if q_order is None:
            continue
        for binned in (srt, grid):
            i_q, w_q = ops.c.three_nn_with_weights(dev(unk), dev(kn), binned, q_order)
            assert torch.equal(i_q, i_plain) and torch.equal(w_q, w_plain)


def test_three_interpolate_and_grad(ops, oracle):
    rng = np.random.default_rng(0)
    feat = rng.standard_normal((2, 37, 64)).astype(np.float32)
    idx = rng.integers(0, 64, (2, 600, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (2, 600, 3)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    f = dev(feat).requires_grad_(True)
    out = ops.pn.three_interpolate(f, dev(idx), dev(w))
    ref = oracle.three_interpolate(feat, idx, w)
    np.testing.assert_allclose(host(out), ref, atol=1e-5, rtol=0)
    np.testing.assert_array_equal(host(out), ref)  # same contraction as the oracle: bit-exact in practice
    g = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(dev(g))
    np.testing.assert_allclose(host(f.grad), oracle.three_interpolate_grad(g, idx, w, 64), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,C,M,N", [(2, 5, 300, 2048), (1, 9, 4097, 1024), (2, 3, 64, 1028), (1, 4, 7, 603),
                                     (1, 130, 1024, 4096)])
def test_three_interpolate_kernel_variants(ops, oracle, B, C, M, N):
    """rows-in-LDS (n >= 1024, n % 4 == 0, row fits), 4-points-per-lane and scalar kernels: all
    bit-equal to the oracle's fmaf expression"""
    rng = np.random.default_rng(N + M)
    feat = rng.standard_normal((B, C, M)).astype(np.float32)
    idx = rng.integers(0, M, (B, N, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    out = torch.empty((B, C, N), device="cuda")
    ops.c.three_interpolate_wrapper(B, C, M, N, dev(feat), dev(idx), dev(w), out)
    np.testing.assert_array_equal(host(out), oracle.three_interpolate(feat, idx, w))


# ------------------------------------------------------------------------------- roipool3d
def _roi_scene(B, n, m, c, cfg):
    pc = synth.make_batch("lidar", B, n, cfg)
    boxes = synth.proposal_boxes(B, m, cfg)
    for b in range(B):  # put some boxes exactly on the synthetic cars
        cars = synth.random_boxes3d(15, (1000 * cfg + b) * 7919 + 13)
        k = min(m // 2, 15)
        boxes[b, :k] = cars[:k]
    feat = np.random.default_rng(cfg).standard_normal((B, n, c)).astype(np.float32)
    return pc[:, :, :3].copy(), boxes, feat


@pytest.mark.parametrize("B,n,m,c,s,cfg", H.ROI_BIT_EXACT_CASES)
def test_roipool3d_bit_exact(ops, oracle, B, n, m, c, s, cfg):
    xyz, boxes, feat = _roi_scene(B, n, m, c, cfg)
    from ws3d_amd import kitti_utils
    enl = kitti_utils.enlarge_box3d(boxes.reshape(-1, 7), 1.0).reshape(B, m, 7)
    ref_pooled, ref_empty, ref_sel = oracle.roipool3d(xyz, enl, feat, s, return_idx=True)
    pooled, empty = ops.roi.roipool3d_gpu(dev(xyz), dev(feat), dev(boxes), 1.0, sampled_pt_num=s)
    assert empty.dtype == torch.int32
    np.testing.assert_array_equal(host(empty), ref_empty)
    np.testing.assert_array_equal(host(pooled), ref_pooled)
    assert (ref_empty == 0).any()
    # selected indices (the reference's internal pts_idx)
    pf = torch.zeros((B, m, s, 3 + c), device="cuda")
    ef = torch.zeros((B, m), dtype=torch.int32, device="cuda")
    sel = torch.full((B, m, s), -5, dtype=torch.int32, device="cuda")
    ops.c.roipool3d_forward(dev(xyz), dev(enl), dev(feat), pf, ef, sel)
    np.testing.assert_array_equal(host(sel), ref_sel)
    # ball variant
    rng = np.zeros_like(boxes)
    rng[..., 0], rng[..., 2], rng[..., 3:6] = boxes[..., 0], boxes[..., 2], 6.0
    rp, re = oracle.roipool3d(xyz, rng, feat, s)
    bp, be = ops.roi.roipool3dball_gpu(dev(xyz), dev(feat), dev(boxes), 1.0, sampled_pt_num=s)
    np.testing.assert_array_equal(host(be), re)
    np.testing.assert_array_equal(host(bp), rp)


def test_roipool3d_degenerate_scenes(ops, oracle):
    """scenes that stress the binned variant's grid and its radix select (and are just as valid for the scanning kernels): all points
    on one x / one z / one spot, NaN and inf coordinates, exact duplicates, a box far outside the cloud, boxes holding far more than
    S points whose indices are scattered (the first S BY INDEX must come out, wrap-padded when fewer), S not a power of two"""
    rng = np.random.default_rng(77)
    N, M, C = 40000, 24, 8
    base = synth.make_batch("lidar", 1, N, 45)[0, :, :3].copy()
    car = synth.random_boxes3d(15, (1000 * 45) * 7919 + 13)
    scenes = []
    a = base.copy(); a[:, 0] = 3.25; scenes.append(a)                                  # one x: a single grid column
    a = base.copy(); a[:, 2] = 30.0; scenes.append(a)                                  # one z: a single grid row
    a = base.copy(); a[:] = (1.0, 1.2, 20.0); scenes.append(a)                          # one spot
    a = base.copy(); a[::7, 0] = np.nan; a[3::11, 2] = np.inf; a[5::13, 1] = -np.inf; a[9::17, 0] = -np.inf; scenes.append(a)
    a = base.copy(); a[N // 2:] = a[:N // 2][rng.permutation(N // 2)]; scenes.append(a)       # every point twice, scattered
    a = base.copy(); k = rng.permutation(N)[:6000]; a[k] = car[0, :3] + rng.uniform(-0.4, 0.4, (6000, 3)).astype(np.float32) - (0, 0.8, 0); scenes.append(a)   # 6000 scattered indices inside one box
    xyz = np.ascontiguousarray(np.stack(scenes).astype(np.float32))
    B = xyz.shape[0]
    boxes = synth.proposal_boxes(B, M, 45)
    boxes[:, :8] = car[:8]
    boxes[:, 8] = (3.25, 1.7, 30.0, 1.6, 1.7, 4.0, 0.3)
    boxes[:, 9] = (1.0, 2.0, 20.0, 1.6, 1.7, 4.0, -1.2)
    boxes[:, 10] = (500.0, 1.7, -300.0, 1.6, 1.7, 4.0, 0.0)                          # nowhere near the cloud
    boxes[:, 11] = (0.0, 1.7, 30.0, 2.0, 19.0, 19.0, 0.7)                            # wider than the 10 m window
    boxes[:, 12] = (0.0, 1.7, 30.0, 2.0, 3.0, 5.0, np.pi / 2)                        # cos = 6e-8: one constraint per axis
    boxes[:, 13] = (0.0, 1.7, 30.0, 2.0, 3.0, 5.0, 0.0)
    boxes[0, 14, 6] = np.nan
    boxes[0, 15, 0] = np.inf
    feat = rng.standard_normal((B, N, C)).astype(np.float32)
    for S in (512, 4, 700):
        ref_p, ref_e, ref_s = oracle.roipool3d(xyz, boxes, feat, S, return_idx=True)
        for fn, init in ((ops.c.roipool3d_forward, 0.0), (ops.c.roipool3d_forward_fill, float("nan"))):
            pooled = torch.full((B, M, S, 3 + C), init, device="cuda")
            empty = torch.zeros((B, M), dtype=torch.int32, device="cuda")
            sel = torch.full((B, M, S), -5, dtype=torch.int32, device="cuda")
            fn(dev(xyz), dev(boxes), dev(feat), pooled, empty, sel)
            np.testing.assert_array_equal(host(empty), ref_e)
            np.testing.assert_array_equal(host(sel), ref_s)
            got = host(pooled)
            assert np.array_equal(got, ref_p, equal_nan=True)
    assert (ref_e == 0).any() and (ref_e == 1).any()


@pytest.mark.parametrize("min_n", ["64", "0"])
def test_roipool3d_other_variant_subprocess(min_n):
    """every roipool3d test of this file once more with the OTHER kernel family on all sizes: WS3D_ROI_BINNED=64 sends every scene of
    >= 64 points through roi_bin_kernel + roipool3d_binned_kernel (default: from 16384 points on), WS3D_ROI_BINNED=0 none"""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "roipool3d and not subprocess"],
                       env=dict(os.environ, WS3D_ROI_BINNED=min_n), capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-500:]


def test_roipool3d_boxes_wider_than_the_ten_metre_window(ops, oracle):
    """pt_in_box3d drops points more than 10 m from the box centre in x or z before the rotated test (roipool3d_kernel.cu:18-20).
    The kernels leave those two terms out for boxes whose BEV half-diagonal is under 9.9 m (they cannot decide anything there);
    boxes beyond that -- mixed with small ones in one workgroup, and at the threshold -- must still apply them"""
    B, N, M, C, S = 2, 20000, 16, 128, 512
    pc = synth.make_batch("lidar", B, N, 44)[:, :, :3].copy()
    boxes = synth.proposal_boxes(B, M, 44)
    boxes[:, 0::4, 3:6] = (3.0, 30.0, 44.0)                 # h, w, l: far wider than the window
    boxes[:, 1::4, 3:6] = (3.0, 13.0, 15.0)                 # half-diagonal 9.92 m: just above the threshold
    boxes[:, 2::4, 3:6] = (3.0, 12.9, 15.0)                 # 9.89 m: just below
    boxes[0, 3, 3:6] = (3.0, float("nan"), 4.0)
    feat = np.random.default_rng(5).standard_normal((B, N, C)).astype(np.float32)
    ref_p, ref_e, ref_s = oracle.roipool3d(pc, boxes, feat, S, return_idx=True)
    # the wide boxes hold points of the rotated rectangle that the window drops: the full cloud passes the rotated test far more often
    rot_only = oracle.pts_in_boxes3d(pc[0], boxes[0, 0:1])[0].sum() if hasattr(oracle, "pts_in_boxes3d") else 0
    assert len(np.unique(ref_s[0, 0])) > 100 and ref_e[0, 3] == 1 and rot_only >= 0
    for fn, init in ((ops.c.roipool3d_forward, 0.0), (ops.c.roipool3d_forward_fill, float("nan"))):
        pooled = torch.full((B, M, S, 3 + C), init, device="cuda")
        empty = torch.zeros((B, M), dtype=torch.int32, device="cuda")
        sel = torch.full((B, M, S), -5, dtype=torch.int32, device="cuda")
        fn(dev(pc), dev(boxes), dev(feat), pooled, empty, sel)
        np.testing.assert_array_equal(host(empty), ref_e)
        np.testing.assert_array_equal(host(sel), ref_s)
        np.testing.assert_array_equal(host(pooled), ref_p)


@pytest.fixture(scope="module")
def roi_variant_refs(oracle, tmp_path_factory):
    """the scenes of H.ROI_VARIANT_CASES as in<i>.npz in one directory, and the oracle's (pooled, empty, idx) of each: built once,
    shared by every variant"""
    d = tmp_path_factory.mktemp("roi_variants")
    refs = []
    for i, ((B, N, M, C, S), seed) in enumerate(zip(H.ROI_VARIANT_CASES, H.ROI_VARIANT_SEEDS)):
        pc = synth.make_batch("lidar", B, N, seed)[:, :, :3].copy()
        boxes = synth.proposal_boxes(B, M, seed)
        boxes[0, 1:3, 0] += 400.0                                             # empty boxes
        boxes[-1, 3::5, 4:6] = (25.0, 30.0)                                   # wider than the +-10 m window of pt_in_box3d
        if i >= 5:                                                            # a tiny box on a point of the cloud: a wrap-padded list
            boxes[0, 4] = (*pc[0, N // 3], 0.5, 0.5, 0.5, 0.3)
            boxes[0, 4, 1] += 0.25
        feat = np.random.default_rng(i).standard_normal((B, N, C)).astype(np.float32)
        np.savez(d / f"in{i}.npz", pc=pc, boxes=boxes, feat=feat)
        refs.append(oracle.roipool3d(pc, boxes, feat, S, return_idx=True))
    return d, refs


@pytest.mark.parametrize("env", H.ROI_ENV_VARIANTS, ids=H.roi_env_id)
def test_roipool3d_kernel_variants_subprocess(roi_variant_refs, tmp_path, env):
    """every selectable roipool3d kernel (boxes per workgroup, direct / LDS-staged copy, the variant that overlaps scan and
    copy -- reached only with WS3D_ROI_BINNED=0, tests/test_roipool_plan.py checks which kernel each variant takes): pooled rows,
    empty flags and selected indices against the oracle; scenes above and below the 16384-point switch, box counts that leave a
    ragged last workgroup, empty, wrap-padded and truncated boxes in every scene, pre-zeroed and fill entry points"""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = H.ROI_VARIANT_CASES
    src, refs = roi_variant_refs
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {root!r})
        from ws3d_amd import compat
        for i, S in enumerate({[c[4] for c in cases]!r}):
            d = np.load({str(src)!r} + f"/in{{i}}.npz")
            pc, boxes, feat = (torch.from_numpy(d[k]).cuda() for k in ("pc", "boxes", "feat"))
            B, M, C = boxes.shape[0], boxes.shape[1], feat.shape[2]
            out = {{}}
            for name, fn, init in (("z", compat.roipool3d_forward, 0.0), ("f", compat.roipool3d_forward_fill, float("nan"))):
                pooled = torch.full((B, M, S, 3 + C), init, device="cuda")
                empty = torch.full((B, M), 0 if name == "z" else 77, dtype=torch.int32, device="cuda")
                sel = torch.full((B, M, S), -5, dtype=torch.int32, device="cuda")
                fn(pc, boxes, feat, pooled, empty, sel)
                out.update({{name + "p": pooled.cpu().numpy(), name + "e": empty.cpu().numpy(), name + "s": sel.cpu().numpy()}})
            np.savez({str(tmp_path)!r} + f"/out{{i}}.npz", **out)
    """)
    r = subprocess.run([sys.executable, "-B", "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for i, (rp, re, rs) in enumerate(refs):
        got = np.load(tmp_path / f"out{i}.npz")
        S = cases[i][4]
        distinct = np.array([len(np.unique(row)) for row in rs.reshape(-1, S)])[re.reshape(-1) == 0]
        assert (re == 1).sum() >= 2
        if i >= 5:      # the two small cases: a wrap-padded list and a truncated one beside the empty boxes
            assert ((distinct >= 1) & (distinct < S)).sum() >= 1 and (distinct == S).sum() >= 1, (cases[i], distinct)
        for k in "zf":
            np.testing.assert_array_equal(got[k + "e"], re, err_msg=str((cases[i], k)))
            np.testing.assert_array_equal(got[k + "p"], rp, err_msg=str((cases[i], k)))
            np.testing.assert_array_equal(got[k + "s"], rs, err_msg=str((cases[i], k)))


def test_roipool3d_cpu_twins(ops, oracle):
    xyz, boxes, feat = _roi_scene(1, 3000, 20, 6, 9)
    flags = ops.roi.pts_in_boxes3d_cpu(torch.from_numpy(xyz[0]), torch.from_numpy(boxes[0]))
    ref = oracle.pts_in_boxes3d(xyz[0], boxes[0])
    np.testing.assert_array_equal(np.stack([f.numpy() for f in flags]).astype(np.int64), ref)
    pp, pf, pe = ops.roi.roipool_pc_cpu(torch.from_numpy(xyz[0]), torch.from_numpy(feat[0]), torch.from_numpy(boxes[0]), 128)
    rp, rf, re = oracle.roipool3d_cpu(xyz[0], boxes[0], feat[0], 128)
    np.testing.assert_array_equal(pe.numpy(), re)
    np.testing.assert_array_equal(pp.numpy(), rp)
    np.testing.assert_array_equal(pf.numpy(), rf)


# ------------------------------------------------------------------------------- iou3d
def _bev(n, seed, spread):
    rng = np.random.default_rng(seed)
    b3 = synth.random_boxes3d(n, seed)
    b3[:, 0] = rng.uniform(-spread, spread, n)
    b3[:, 2] = 30 + rng.uniform(-spread, spread, n)
    return synth.boxes3d_to_bev(b3), b3


@pytest.mark.parametrize("na,nb,spread", [(40, 50, 6.0), (130, 77, 10.0), (1, 1, 0.5), (64, 64, 3.0), (300, 5, 30.0)])
def test_overlap_and_iou(ops, oracle, na, nb, spread):
    A, A3 = _bev(na, 1, spread)
    B, B3 = _bev(nb, 2, spread)
    ov_ref, iou_ref = oracle.boxes_overlap_bev(A, B), oracle.boxes_iou_bev(A, B)
    ov = torch.zeros((na, nb), device="cuda")
    ops.c.boxes_overlap_bev_gpu(dev(A), dev(B), ov)
    np.testing.assert_allclose(host(ov), ov_ref, atol=1e-5, rtol=0)
    np.testing.assert_allclose(host(ops.iou.boxes_iou_bev(dev(A), dev(B))), iou_ref, atol=1e-5, rtol=0)
    # same IEEE op sequence + correctly rounded trig on both sides: expect bit equality
    np.testing.assert_array_equal(host(ov), ov_ref)
    iou2d, iou3d = ops.iou.boxes_iou3d_gpu(dev(A3), dev(B3))
    # composition (iou3d_utils.py:21-56) re-derived in numpy from the oracle overlap
    hmin_a, hmax_a = (A3[:, 1] - A3[:, 3])[:, None], A3[:, 1][:, None]
    hmin_b, hmax_b = (B3[:, 1] - B3[:, 3])[None], B3[:, 1][None]
    oh = np.clip(np.minimum(hmax_a, hmax_b) - np.maximum(hmin_a, hmin_b), 0, None)
    sa, sb = (A3[:, 4] * A3[:, 5])[:, None], (B3[:, 4] * B3[:, 5])[None]
    np.testing.assert_allclose(host(iou2d), ov_ref / np.clip(sa + sb - ov_ref, 1e-7, None), atol=1e-5)
    o3 = ov_ref * oh
    va, vb = (A3[:, 3] * A3[:, 4] * A3[:, 5])[:, None], (B3[:, 3] * B3[:, 4] * B3[:, 5])[None]
    np.testing.assert_allclose(host(iou3d), o3 / np.clip(va + vb - o3, 1e-7, None), atol=1e-5)


@pytest.mark.parametrize("n,thresh,normal,spread", [(64, 0.5, False, 4.0), (65, 0.3, False, 4.0), (300, 0.7, False, 5.0),
                                                    (200, 0.5, True, 4.0), (1, 0.5, False, 1.0), (129, 0.1, True, 4.0),
                                                    (2000, 0.8, False, 12.0), (512, 0.7, False, 8.0)])
def test_nms_mask_and_keep(ops, oracle, n, thresh, normal, spread):
    boxes, _ = _bev(n, 3, spread)
    scores = synth.distinct_scores(n, 3)
    order = np.argsort(-scores, kind="stable")
    sorted_boxes = np.ascontiguousarray(boxes[order])
    ref_mask = oracle.nms_mask(sorted_boxes, thresh, normal)
    got_full = host(ops.c.nms_mask(dev(sorted_boxes), thresh, normal, full_grid=True)).view(np.uint64)
    np.testing.assert_array_equal(got_full, ref_mask)
    got_tri = host(ops.c.nms_mask(dev(sorted_boxes), thresh, normal, full_grid=False)).view(np.uint64)
    cb = (n + 63) // 64
    upper = (np.arange(cb)[None, :] >= (np.arange(n) // 64)[:, None])
    np.testing.assert_array_equal(got_tri, np.where(upper, ref_mask, 0))
    ref_keep = oracle.nms_sorted(sorted_boxes, thresh, normal)
    keep, num = ops.c.nms_device(dev(sorted_boxes), thresh, normal)
    assert int(num.item()) == len(ref_keep)
    np.testing.assert_array_equal(host(keep)[:len(ref_keep)], ref_keep)
    fn = ops.iou.nms_normal_gpu if normal else ops.iou.nms_gpu
    np.testing.assert_array_equal(host(fn(dev(boxes), dev(scores), thresh)), oracle.nms(boxes, scores, thresh, normal))
    # reference ext signature: CPU int64 keep tensor + returned count (iou3d.cpp:73-120)
    keep_cpu = torch.zeros(n, dtype=torch.int64)
    cnt = (ops.c.nms_normal_gpu if normal else ops.c.nms_gpu)(dev(sorted_boxes), keep_cpu, thresh)
    assert cnt == len(ref_keep)
    np.testing.assert_array_equal(keep_cpu.numpy()[:cnt], ref_keep)


@pytest.mark.parametrize("thresh", [0.3, 0.5, 0.7, 0.8, 0.9])
@pytest.mark.parametrize("same_size", [True, False])
def test_nms_mask_of_near_threshold_clusters(ops, oracle, thresh, same_size):
    """the mask kernel drops a pair without running the polygon clipping when an upper bound of the intersection area proves
    iou <= thresh (iou3d.hip iou_surely_not_above): clusters of car-sized boxes a few centimetres to decimetres and a few degrees
    apart put thousands of pairs right at the threshold -- every bit must still be the oracle's"""
    rng = np.random.default_rng(int(thresh * 100) + (7 if same_size else 0))
    n, per = 640, 40
    centres = rng.uniform(-8, 8, (n // per, 2)) + np.array([0.0, 30.0])
    b3 = np.zeros((n, 7), np.float32)
    for c in range(n // per):
        sl = slice(c * per, (c + 1) * per)
        spread = [0.05, 0.15, 0.4, 1.0][c % 4]
        b3[sl, 0] = centres[c, 0] + rng.normal(0, spread, per)
        b3[sl, 2] = centres[c, 1] + rng.normal(0, spread, per)
        b3[sl, 1] = 1.0
        b3[sl, 3] = 1.5
        b3[sl, 4] = 1.6 if same_size else 1.6 * rng.uniform(0.85, 1.15, per)
        b3[sl, 5] = 3.9 if same_size else 3.9 * rng.uniform(0.85, 1.15, per)
        b3[sl, 6] = rng.uniform(-np.pi, np.pi) + rng.normal(0, [0.02, 0.1, 0.3, 1.0][(c // 4) % 4], per) + (np.pi / 2) * rng.integers(0, 2, per)
    boxes = np.ascontiguousarray(synth.boxes3d_to_bev(b3)[rng.permutation(n)])
    ref_mask = oracle.nms_mask(boxes, thresh, False)
    got = host(ops.c.nms_mask(dev(boxes), thresh, False, full_grid=True)).view(np.uint64)
    np.testing.assert_array_equal(got, ref_mask)
    bits = int(sum(bin(int(w)).count("1") for w in ref_mask.ravel()))
    assert bits > 40                                         # (the clusters do suppress each other: the test is not vacuous)
    ref_keep = oracle.nms_sorted(boxes, thresh, False)
    keep, num = ops.c.nms_device(dev(boxes), thresh, False)
    np.testing.assert_array_equal(host(keep)[:int(num.item())], ref_keep)


def test_nms_batched_and_proposal_stage(ops, oracle):
    """one launch pair for a batch of scenes == per-scene NMS == oracle; the vectorised proposal
    stage == a per-scene composition of the reference-named wrappers"""
    from ws3d_amd import kitti_utils, stage1
    B, n = 3, 700
    boxes = np.stack([_bev(n, 10 + b, 6.0)[0] for b in range(B)])
    scores = np.stack([synth.distinct_scores(n, 20 + b) for b in range(B)])
    order = np.argsort(-scores, axis=1, kind="stable")
    sorted_boxes = np.ascontiguousarray(np.take_along_axis(boxes, order[:, :, None], 1))
    keep, num = ops.c.nms_device_batched(dev(sorted_boxes), 0.5, False, 0)
    for b in range(B):
        ref = oracle.nms_sorted(sorted_boxes[b], 0.5, False)
        assert int(num[b]) == len(ref)
        np.testing.assert_array_equal(host(keep[b])[:len(ref)], ref)
    idx, cnt = ops.iou.nms_gpu_padded_batched(dev(boxes), dev(scores), 0.5, 40)
    for b in range(B):
        ref = oracle.nms(boxes[b], scores[b], 0.5, False)[:40]
        assert int(cnt[b]) == len(ref)
        np.testing.assert_array_equal(host(idx[b])[:len(ref)], ref)
        assert (host(idx[b])[len(ref):] == -1).all()
    # proposal stage on a synthetic rpn output
    rng = np.random.default_rng(0)
    N = 2048
    cfg = stage1.RPNConfig(rpn_pre_nms_top_n=1500, rpn_post_nms_top_n=30)
    pc = synth.make_batch("lidar", 2, N, 55)
    out = {"backbone_xyz": dev(pc[:, :, :3].copy()),
           "rpn_reg": dev(rng.standard_normal((2, N, 40)).astype(np.float32)),
           "rpn_cls": dev((rng.permutation(2 * N).reshape(2, N, 1) / (2 * N) * 8 - 4).astype(np.float32))}
    pb, ps, pcnt, penl = stage1.proposals_from_rpn(out, cfg, with_pool_boxes=True)
    # the fused glue (ws3d_gather_boxes_bev / ws3d_select_proposals) is bit-identical to the torch composition it replaces
    tb, ts, tcnt, tenl = stage1.proposals_from_rpn(out, cfg, with_pool_boxes=True, fused=False)
    assert torch.equal(pb, tb) and torch.equal(ps, ts) and torch.equal(pcnt, tcnt) and torch.equal(penl, tenl)
    assert pb.view(torch.int32).eq(tb.view(torch.int32)).all()          # including the sign of the zero padding
    h, w, l = cfg.cls_mean_size
    for b in range(2):
        score = torch.sigmoid(out["rpn_cls"][b, :, 0])
        ctr = stage1.decode_center_target(out["backbone_xyz"][b], out["rpn_reg"][b], cfg.loc_scope, cfg.loc_bin_size)
        box = torch.stack((ctr[:, 0], out["backbone_xyz"][b, :, 1] + h / 2, ctr[:, 2], torch.full_like(score, h),
                           torch.full_like(score, w), torch.full_like(score, l),
                           stage1.synthetic_orientation(N, score.device)), 1)
        sc, o = torch.topk(score, 1500, sorted=True)
        box = box[o]
        k = ops.iou.nms_gpu(kitti_utils.boxes3d_to_bev_torch(box), sc, cfg.rpn_nms_thresh)[:30]
        assert int(pcnt[b]) == len(k)
        np.testing.assert_array_equal(host(pb[b, :len(k)]), host(box[k]))
        np.testing.assert_array_equal(host(ps[b, :len(k)]), host(sc[k]))
        assert (host(pb[b, len(k):]) == 0).all()


@pytest.mark.parametrize("normal", [False, True])
@pytest.mark.parametrize("max_keep", [1, 5, 40, 200])
def test_nms_max_keep_leading_block_ladder(ops, oracle, normal, max_keep):
    """max_keep > 0 builds only a leading block of the mask and widens it when the sweep runs out
    of rows; scenes of one batch finish at different levels (sparse: first level, crowded: all
    levels).  The result must be the full greedy sweep's first max_keep survivors."""
    n = 3000
    scenes = [_bev(n, 31, 40.0)[0], _bev(n, 32, 1.5)[0], _bev(n, 33, 6.0)[0]]
    scenes[1][:, 4] = 0.0 if normal else scenes[1][:, 4]
    boxes = np.ascontiguousarray(np.stack(scenes))
    thresh = 0.05
    keep, num = ops.c.nms_device_batched(dev(boxes), thresh, normal, max_keep)
    full = [oracle.nms_sorted(boxes[b], thresh, normal) for b in range(3)]
    assert len(full[1]) < len(full[2]) < len(full[0])      # crowded < medium < sparse
    for b in range(3):
        ref = full[b][:max_keep]
        assert int(num[b]) == len(ref)
        np.testing.assert_array_equal(host(keep[b])[:len(ref)], ref)


def test_radius_nms_max_keep_ladder(ops, oracle):
    rng = np.random.default_rng(5)
    n = 2500
    c = np.stack([rng.uniform(-40, 40, (n, 2)), rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-3, 3, (n, 2))]).astype(np.float32)
    for max_keep in (1, 6, 50):
        keep, num = ops.c.radius_nms_device_batched(dev(c), 0.3, max_keep=max_keep)
        for b in range(3):
            ref = oracle.radius_nms_sorted(c[b], 0.3)[:max_keep]
            assert int(num[b]) == len(ref)
            np.testing.assert_array_equal(host(keep[b])[:len(ref)], ref)


@pytest.mark.parametrize("B,n,r", [(1, 1, 0.3), (2, 300, 0.3), (3, 1000, 1.0), (1, 4000, 0.3), (2, 65, 0.05)])
def test_radius_nms_bit_exact(ops, oracle, B, n, r):
    rng = np.random.default_rng(n)
    c = (rng.uniform(-4, 4, (B, n, 2)) + rng.integers(0, 3, (B, n, 1)) * 0.2).astype(np.float32)
    if n > 10:
        c[:, 5] = c[:, 2]
        c[:, 7] = c[:, 3] + np.float32([r, 0])
    keep, num = ops.c.radius_nms_device_batched(dev(c), r)
    for b in range(B):
        ref = oracle.radius_nms_sorted(c[b], r)
        assert int(num[b]) == len(ref)
        np.testing.assert_array_equal(host(keep[b])[:len(ref)], ref)
    keep2, num2 = ops.c.radius_nms_device_batched(dev(c), r, max_keep=7)
    for b in range(B):
        ref = oracle.radius_nms_sorted(c[b], r)[:7]
        assert int(num2[b]) == len(ref)
        np.testing.assert_array_equal(host(keep2[b])[:len(ref)], ref)


def test_center_proposal_stage_matches_reference_loop(ops):
    """stage1.center_proposals == the reference's inline proposal code (generate_box_dataset.py:
    92-140) restated with torch ops + its Python keep loop"""
    from ws3d_amd import stage1
    rng = np.random.default_rng(3)
    N = 3000
    pc = synth.make_batch("lidar", 1, N, 77)
    out = {"backbone_xyz": dev(pc[:, :, :3].copy()),
           "rpn_reg": dev(rng.standard_normal((1, N, 40)).astype(np.float32)),
           "rpn_cls": dev(rng.normal(-0.5, 1.5, (1, N, 1)).astype(np.float32))}
    cfg = stage1.DEFAULT_CFG
    ctr, norm, raw = stage1.center_proposals(out, cfg)
    xyz = out["backbone_xyz"].view(-1, 3)
    s_raw = out["rpn_cls"].view(-1)
    s_norm = torch.sigmoid(s_raw)
    rois = stage1.decode_center_target(xyz, out["rpn_reg"].view(-1, 40), cfg.loc_scope, cfg.loc_bin_size).view(-1, 3)
    reg_dist = rois - xyz
    mask = (s_norm > cfg.score_thresh) & (reg_dist[:, [0, 2]].pow(2).sum(-1).sqrt() > 0.2)
    rois, s_norm, s_raw = rois[mask], s_norm[mask], s_raw[mask]
    order = torch.argsort(-s_norm, stable=True)
    rois, s_norm, s_raw = rois[order], s_norm[order], s_raw[order]
    a = rois[:, [0, 2]]
    d = torch.sqrt(torch.sum((a[None, :] - a[:, None]) ** 2, dim=2))
    keep = [0]
    for i in range(1, rois.shape[0]):
        if torch.min(d[keep, i], dim=-1)[0] > 0.3:
            keep.append(i)
    assert 10 < len(keep) < rois.shape[0]
    np.testing.assert_array_equal(host(ctr), host(rois[keep]))
    np.testing.assert_array_equal(host(norm), host(s_norm[keep]))
    np.testing.assert_array_equal(host(raw), host(s_raw[keep]))


# ------------------------------------------------------------------------------- error behaviour
def test_errors_are_exceptions_not_exit(ops):
    from ws3d_amd._lib import Ws3dError
    with pytest.raises(Ws3dError):
        ops.pn.furthest_point_sample(torch.zeros((1, 16, 3)), 4)  # CPU tensor: no fallback
    with pytest.raises(Ws3dError):
        ops.c.ball_query_wrapper(1, 16, 4, 0.5, 0, torch.zeros((1, 4, 3), device="cuda"),
                                 torch.zeros((1, 16, 3), device="cuda"),
                                 torch.zeros((1, 4, 1), dtype=torch.int32, device="cuda"))
    with pytest.raises(AssertionError):
        ops.pn.furthest_point_sample(torch.zeros((1, 16, 6), device="cuda")[:, :, :3], 4)  # non-contiguous


@pytest.mark.parametrize("B,O,M,S", [(2, 5, 7, 16), (1, 3, 33, 32), (2, 4, 9, 5), (1, 2, 3, 4), (1, 1, 5, 64), (2, 3, 4, 256)])
def test_mlp_epilogues_bit_exact(ops, B, O, M, S):
    """SharedMLP epilogue kernels == the torch ops they replace (single fp32 add / max: bit-exact)"""
    g = torch.Generator().manual_seed(B * 100 + S)
    y = torch.randn((B, O, M, S), generator=g).cuda()
    y[0, 0, 0, 1] = float("nan")
    bias = torch.randn(O, generator=g).cuda()
    for relu in (True, False):
        ref = y.amax(dim=3) + bias[None, :, None]
        ref = torch.relu(ref) if relu else ref
        got = ops.c.rowmax_bias_act(y, bias, relu=relu)
        np.testing.assert_array_equal(host(got), host(ref))
        ref2 = y + bias[None, :, None, None]
        ref2 = torch.relu(ref2) if relu else ref2
        got2 = ops.c.bias_act_inplace(y.clone(), bias, relu=relu)
        np.testing.assert_array_equal(host(got2), host(ref2))
    np.testing.assert_array_equal(host(ops.c.rowmax_bias_act(y, None, relu=False)), host(y.amax(dim=3)))


def test_kitti_directory_to_result_files(ops, tmp_path):
    """ingest -> Stage-1 forward -> proposals -> KITTI result files on a synthetic KITTI tree"""
    from ws3d_amd import infer_kitti, kitti_io
    root, out = str(tmp_path / "kitti"), str(tmp_path / "res")
    synth.write_kitti_tree(root, [(7, 60000, 1), (8, 9000, 2), (11, 30000, 3)])
    files = infer_kitti.run(root, "val", out, batch=2)
    assert [os.path.basename(f) for f in files] == ["000007.txt", "000008.txt", "000011.txt"]
    for f in files:
        objs = kitti_io.read_label_file(f)
        assert len(objs) <= 100
        for o in objs:
            assert o.cls_type == "Car" and np.isfinite(o.box3d()).all() and 0.0 <= o.box2d[0] <= o.box2d[2] <= 1241.0
    again = infer_kitti.run(root, "val", str(tmp_path / "res2"), batch=3)
    for a, b in zip(files, again):   # another batch size: same proposals (GEMM kernels differ in the last ulps)
        oa, ob = kitti_io.read_label_file(a), kitti_io.read_label_file(b)
        assert len(oa) == len(ob)
        for x, y in zip(oa, ob):
            np.testing.assert_allclose(x.box3d(), y.box3d(), atol=2e-3)
            np.testing.assert_allclose(x.box2d, y.box2d, atol=5e-2)
    # loader processes + a deeper pipeline: every scene still gets its file (the 16384-point sampler then
    # draws from per-process random streams, so the proposals are those of another sampling of the scan)
    par = infer_kitti.run(root, "val", str(tmp_path / "res3"), batch=1, depth=3, workers=2)
    assert [os.path.basename(f) for f in par] == ["000007.txt", "000008.txt", "000011.txt"]
    for f in par:
        objs = kitti_io.read_label_file(f)
        assert 0 < len(objs) <= 100 and all(np.isfinite(o.box3d()).all() for o in objs)


# ------------------------------------------------------------------------------- Stage-2 (RCNN) shapes, SURVEY 8f.3
@pytest.mark.parametrize("B", [3, 96])
def test_stage2_sa_shapes_bit_exact(ops, oracle, B):
    """thousands-of-tiny-clouds regime (lib/config.py:122-129): npoint 128/32/None, r 0.2/0.4/100,
    nsample 64 on 512-point RoI clouds -- FPS runs one wave per cloud, the fused group emits
    (B,131,128,64); everything bit-equal to the oracle, and PointnetSAModule(npoint=None) == GroupAll"""
    from ws3d_amd import pn2_modules
    pts = synth.roi_clouds(B, 512, 9)
    pts[0, 10] = pts[0, 3]                       # exact duplicate: FPS / ball-query tie rules
    feat = np.random.default_rng(B).standard_normal((B, 128, 512)).astype(np.float32)
    i1 = oracle.furthest_point_sample(pts, 128)
    n1 = np.stack([pts[b][i1[b]] for b in range(B)])
    q1 = oracle.ball_query(0.2, 64, pts, n1)
    g1 = oracle.grouping_operation(feat, q1)
    gx1 = oracle.grouping_operation(np.ascontiguousarray(pts.transpose(0, 2, 1)), q1) - n1.transpose(0, 2, 1)[..., None]
    idx1 = ops.pn.furthest_point_sample(dev(pts), 128)
    np.testing.assert_array_equal(host(idx1), i1)
    out1 = ops.pn.QueryAndGroup(0.2, 64, use_xyz=True)(dev(pts), dev(n1), dev(feat))
    assert tuple(out1.shape) == (B, 131, 128, 64)
    np.testing.assert_array_equal(host(out1[:, 3:]), g1)
    np.testing.assert_array_equal(host(out1[:, :3]), gx1)
    i2 = oracle.furthest_point_sample(n1, 32)
    n2 = np.stack([n1[b][i2[b]] for b in range(B)])
    np.testing.assert_array_equal(host(ops.pn.furthest_point_sample(dev(n1), 32)), i2)
    q2 = oracle.ball_query(0.4, 64, n1, n2)
    idx2 = ops.pn.ball_query(0.4, 64, dev(n1), dev(n2))
    np.testing.assert_array_equal(host(idx2), q2)
    # third level: npoint=None -> GroupAll + SharedMLP + max over all 32 points
    f3 = np.random.default_rng(1).standard_normal((B, 16, 32)).astype(np.float32)
    ga = ops.pn.GroupAll(use_xyz=True)(dev(n2), None, dev(f3))
    np.testing.assert_array_equal(host(ga), np.concatenate([n2.transpose(0, 2, 1), f3], 1)[:, :, None, :])
    sa = pn2_modules.PointnetSAModule(mlp=[16, 8], npoint=None, radius=None, nsample=None, use_xyz=True, bn=True).cuda().eval()
    with torch.no_grad():
        xyz3, out3 = sa(dev(n2), dev(f3))
        ref3 = sa.mlps[0](ga).amax(dim=3)           # SharedMLP on the GroupAll tensor, pooled over the 32 points
    assert xyz3 is None and tuple(out3.shape) == (B, 8, 1)
    np.testing.assert_allclose(host(out3), host(ref3), atol=1e-5)


# ------------------------------------------------------------------------------- deterministic backward, SURVEY 8f.2
@pytest.mark.parametrize("B,C,N,M,ns", [(2, 5, 300, 40, 16), (1, 19, 4096, 1024, 32), (3, 8, 64, 64, 1), (1, 3, 10, 0, 4),
                                        # c >= 32: rows copy + 1 / 2 / 4 / 8 channel chunks per lane, c > 512: two passes
                                        (2, 32, 64, 64, 1), (2, 96, 500, 64, 16), (1, 130, 777, 100, 5), (1, 256, 300, 50, 8),
                                        (1, 515, 100, 30, 4), (1, 700, 50, 20, 3), (1, 64, 9, 100, 32)])
def test_group_and_gather_grad_deterministic_bit_exact(ops, oracle, B, C, N, M, ns):
    """sorted-segment accumulation == the sequential loop `dst[idx[slot]] += g[slot]` (oracle),
    bit for bit, and identical across repeated launches (the atomic kernel is neither)"""
    rng = np.random.default_rng(N + M)
    idx = rng.integers(0, max(N // 3, 1), (B, M, ns)).astype(np.int32)        # heavy collisions
    g = (rng.standard_normal((B, C, M, ns)) * 10 ** rng.uniform(-3, 3, (B, C, M, ns))).astype(np.float32)
    ref = oracle.grouping_operation_grad(g, idx, N)
    outs = []
    for _ in range(3):
        out = torch.full((B, C, N), float("nan"), device="cuda")
        ops.c.group_points_grad_det(B, C, N, M, ns, dev(g), dev(idx), out)
        outs.append(host(out))
    np.testing.assert_array_equal(outs[0], ref)
    np.testing.assert_array_equal(outs[0], outs[1]); np.testing.assert_array_equal(outs[0], outs[2])
    if M > 0:   # the atomic kernel agrees up to summation order
        at = torch.zeros((B, C, N), device="cuda")
        ops.c.group_points_grad_wrapper(B, C, N, M, ns, dev(g), dev(idx), at)
        np.testing.assert_allclose(host(at), ref, rtol=1e-4, atol=1e-3 * np.abs(g).max())


@pytest.mark.parametrize("B,C,n,m", [(2, 21, 1500, 90), (2, 64, 1500, 90), (1, 130, 333, 7), (1, 600, 200, 50), (3, 256, 64, 64)])
def test_three_interpolate_grad_deterministic_bit_exact(ops, oracle, B, C, n, m):
    rng = np.random.default_rng(4 + C)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
    g = rng.standard_normal((B, C, n)).astype(np.float32)
    ref = oracle.three_interpolate_grad(g, idx, w, m)
    out = torch.empty((B, C, m), device="cuda")
    ops.c.three_interpolate_grad_det(B, C, n, m, dev(g), dev(idx), dev(w), out)
    np.testing.assert_array_equal(host(out), ref)


def test_sa_module_avg_pool_equals_the_reference_composition(ops, oracle):
    """pool_method='avg_pool' (pointnet2_modules.py:45-46; unused by the Stage-1 network): the module's output is the reference's own
    composition -- ball_query -> grouping_operation -> subtract / cat -> SharedMLP -> F.avg_pool2d over the samples -- on the ORACLE's
    lists and grouped tensors, with the module's own weights (the grouped inputs are bit-equal; the SharedMLP is the same torch /
    library call on both sides)"""
    import torch.nn.functional as F
    from ws3d_amd import pn2_modules
    torch.manual_seed(3)
    sa = pn2_modules.PointnetSAModuleMSG(npoint=128, radii=[0.6, 1.2], nsamples=[8, 16], mlps=[[4, 8, 8], [4, 8, 16]], use_xyz=True, bn=True,
                                         pool_method='avg_pool').cuda().eval()
    pc = synth.make_batch("lidar", 2, 2048, 5)
    xyz = pc[:, :, :3].copy()
    feats = np.ascontiguousarray(np.repeat(pc[:, :, 3:], 4, axis=2).transpose(0, 2, 1))
    with torch.no_grad():
        nx, nf = sa(dev(xyz), dev(feats))
    cidx = oracle.furthest_point_sample(xyz, 128)
    new_xyz = np.stack([xyz[b][cidx[b]] for b in range(2)])
    np.testing.assert_array_equal(host(nx), new_xyz)
    xyz_t = np.ascontiguousarray(np.transpose(xyz, (0, 2, 1)))
    parts = []
    with torch.no_grad():
        for (r, ns), mlp in zip(((0.6, 8), (1.2, 16)), sa.mlps):
            idx = oracle.ball_query(r, ns, xyz, new_xyz)
            g = np.concatenate([oracle.grouping_operation(xyz_t, idx) - np.transpose(new_xyz, (0, 2, 1))[..., None],
                                oracle.grouping_operation(feats, idx)], 1)
            y = mlp(dev(g))
            parts.append(F.avg_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1))
    np.testing.assert_allclose(host(nf), host(torch.cat(parts, 1)), rtol=1e-6, atol=1e-6)
    assert nf.shape == (2, 24, 128)


def test_autograd_backward_is_reproducible(ops):
    """a small SA + FP stack: two backward passes give bit-identical parameter gradients with the
    deterministic kernels"""
    from ws3d_amd import pn2_modules
    assert ops.pn.DETERMINISTIC_BACKWARD
    torch.manual_seed(0)
    sa = pn2_modules.PointnetSAModuleMSG(npoint=256, radii=[0.5, 1.0], nsamples=[16, 32], mlps=[[4, 8, 8], [4, 8, 16]],
                                         use_xyz=True, bn=False).cuda()
    fp = pn2_modules.PointnetFPModule(mlp=[24 + 4, 16], bn=False).cuda()
    pc = synth.make_batch("lidar", 2, 2048, 3)
    xyz = dev(pc[:, :, :3].copy())
    feat = dev(np.ascontiguousarray(np.repeat(pc[:, :, 3:], 4, axis=2).transpose(0, 2, 1)))
    grads = []
    for _ in range(2):
        f = feat.clone().requires_grad_(True)
        for p in list(sa.parameters()) + list(fp.parameters()):
            p.grad = None
        nx, nf = sa(xyz, f)
        up = fp(xyz, nx, f, nf)
        (up * up).sum().backward()
        grads.append([host(f.grad)] + [host(p.grad) for p in list(sa.parameters()) + list(fp.parameters())])
    # the gradient w.r.t. the input features flows through group_points_grad (both scales),
    # three_interpolate_grad and the data-gradient convolutions; the conv WEIGHT gradients through
    # ws3d_conv1x1_wgrad (fixed-order slices) instead of the library's atomic split-K: everything bit-identical
    for a, b in zip(grads[0], grads[1]):
        np.testing.assert_array_equal(a, b)
    ops.pn.DETERMINISTIC_BACKWARD = False
    try:
        f = feat.clone().requires_grad_(True)
        nx, nf = sa(xyz, f)
        (fp(xyz, nx, f, nf) ** 2).sum().backward()
        np.testing.assert_allclose(host(f.grad), grads[0][0], rtol=1e-3, atol=1e-3)   # atomic path: same up to order
    finally:
        ops.pn.DETERMINISTIC_BACKWARD = True


# ------------------------------------------------------------------------------- Stage-1 trainer, SURVEY 8f.2
def test_trainer_learns_resumes_and_is_reproducible(ops, tmp_path):
    """a short run of the train_rpn counterpart on synthetic centre labels: the loss goes down, a
    checkpoint resumes at the saved iteration with the saved weights, the checkpoint loads into
    the inference network, and two runs from the same seed produce identical losses"""
    from ws3d_amd import stage1
    from ws3d_amd.train_rpn import SyntheticCenters, load_checkpoint, train
    cfg = stage1.RPNConfig(num_points=4096, npoints=(1024, 256, 64, 16))
    ds = SyntheticCenters(8, npoints=4096)
    res = train(ds, total_iters=24, batch_size=4, output_dir=str(tmp_path / "run"), seed=3, net_cfg=cfg, ckpt_save_interval=2)
    h = res["history"]
    assert len(h) == 24 and np.isfinite(h).all()
    assert np.mean(h[-6:]) < 0.7 * np.mean(h[:3]), h
    assert res["checkpoints"] and res["checkpoints"][-1].endswith("checkpoint_iter_00024.pth")
    # resume: continues from it=24 for 4 more iterations
    res2 = train(ds, total_iters=28, batch_size=4, output_dir=str(tmp_path / "run2"), seed=3, net_cfg=cfg,
                 ckpt=res["checkpoints"][-1])
    assert res2["it"] == 28 and len(res2["history"]) == 4
    # inference network accepts the training checkpoint (same keys as the reference's model_state)
    net = stage1.Stage1Net(mode="TEST", cfg=cfg).cuda().eval()
    it, _ = load_checkpoint(net, None, res["checkpoints"][-1])
    assert it == 24
    pts = torch.from_numpy(np.stack([ds[0]["pts_input"]])).cuda()
    out = net.rpn_forward({"pts_input": pts})
    score = torch.sigmoid(out["rpn_cls"][0, :, 0])
    lab = torch.from_numpy(ds[0]["rpn_cls_label"]).cuda()
    assert score[lab > 0.5].mean() > score[lab < 0.05].mean()          # it learnt where the centres are
    # evaluation pass (Trainer.eval_epoch_rpn): the trained net finds the annotated centres
    from ws3d_amd.train_rpn import evaluate
    ev = evaluate(res["model"], ds, cfg, max_scenes=3)
    assert set(ev) == {"val_loss", "point_precision", "gt_recall", "mean_offset"} and np.isfinite(ev["val_loss"])
    fresh = evaluate(stage1.Stage1Net(mode="TRAIN", cfg=cfg).cuda(), ds, cfg, max_scenes=3)
    assert ev["val_loss"] < fresh["val_loss"]
    # augmented training data (rotation / scaling / flip) runs through the same loop
    aug = train(SyntheticCenters(8, npoints=4096, augment=True, rng=np.random.RandomState(1)), total_iters=3, batch_size=4,
                seed=3, net_cfg=cfg)
    assert np.isfinite(aug["history"]).all()
    # same seed, same data order, same schedule: the loss curve repeats BIT FOR BIT -- scatter, norm, pool and
    # the convolutions' weight gradients all add in a fixed order (the library's split-K weight gradient was
    # the last source of run-to-run noise)
    res3 = train(ds, total_iters=24, batch_size=4, seed=3, net_cfg=cfg)
    assert res3["history"] == h


# ------------------------------------------------------------------------------- channels-last variants / fast path
@pytest.mark.parametrize("B,N,M,C,r,ns,srt", [(2, 4096, 512, 1, 0.5, 16, True), (2, 4096, 500, 96, 1.0, 32, True),
                                               (1, 1000, 77, 8, 2.0, 16, False), (1, 600, 40, 5, 2.0, 8, False),
                                               (2, 2048, 256, 0, 1.0, 16, True), (1, 64, 16, 512, 4.0, 32, False),
                                               (3, 70, 5, 12, 100.0, 64, False)])
def test_channels_last_query_and_group(ops, B, N, M, C, r, ns, srt):
    """ws3d_query_and_group_nlc == the channels-first fused kernel, transposed (bit for bit)"""
    pc = synth.make_batch("lidar", B, N, 41)
    xyz = dev(pc[:, :, :3].copy())
    feat = torch.randn((B, C, N), generator=torch.Generator().manual_seed(C)).cuda() if C else None
    _, new_xyz = ops.pn.furthest_point_sample_gather(xyz, M)
    sorted_xyz = ops.c.sort_points_x(xyz) if srt else None
    ref = ops.pn.query_and_group(r, ns, xyz, new_xyz, feat, use_xyz=True, sorted_xyz=sorted_xyz)      # (B,3+C,M,ns)
    got = ops.c.query_and_group_nlc(r, ns, xyz, new_xyz, None if feat is None else feat.transpose(1, 2).contiguous(),
                                    True, sorted_xyz)                                                  # (B,M,ns,3+C)
    assert tuple(got.shape) == (B, M, ns, 3 + C)
    assert torch.equal(got.permute(0, 3, 1, 2), ref)


def test_channels_last_interpolate_and_rowmax(ops, oracle):
    rng = np.random.default_rng(2)
    B, C, M, N = 2, 20, 90, 700
    feat = rng.standard_normal((B, C, M)).astype(np.float32)
    idx = rng.integers(0, M, (B, N, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
    ref = oracle.three_interpolate(feat, idx, w)                                  # (B,C,N)
    got = ops.c.three_interpolate_nlc(dev(np.ascontiguousarray(feat.transpose(0, 2, 1))), dev(idx), dev(w))
    np.testing.assert_array_equal(host(got), ref.transpose(0, 2, 1))
    buf = torch.full((B, N, C + 8), -7.0, device="cuda")                          # into the left part of a wider buffer
    ops.c.three_interpolate_nlc(dev(np.ascontiguousarray(feat.transpose(0, 2, 1))), dev(idx), dev(w), buf)
    np.testing.assert_array_equal(host(buf[:, :, :C]), ref.transpose(0, 2, 1))
    assert (buf[:, :, C:] == -7.0).all()
    y = torch.randn((50 * 16, 24), generator=torch.Generator().manual_seed(1)).cuda()
    y[3, 5] = float("nan")
    out = torch.zeros((50, 40), device="cuda")
    ops.c.rowmax_rows(y, 16, out, 8)
    np.testing.assert_array_equal(host(out[:, 8:32]), host(y.view(50, 16, 24).amax(dim=1)))
    assert (out[:, :8] == 0).all() and (out[:, 32:] == 0).all()


def test_channels_last_fast_path_equals_reference_layout_path(ops):
    """the eval-mode (B,N,C) pipeline and the reference-layout pipeline run the same weights through
    the same operators: identical sampling / neighbour decisions, outputs equal to GEMM rounding"""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.seeded import seeded_state_dict
    model = stage1.Stage1Net(mode="TEST").eval()
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 7))
    model = model.cuda()
    assert fastpath.supported(model)
    pts = dev(synth.make_batch("lidar", 2, 16384, 3))
    fast = model.rpn_forward({"pts_input": pts})
    assert "backbone_features_nlc" in fast
    stage1.CHANNELS_LAST_FASTPATH = False
    try:
        slow = model.rpn_forward({"pts_input": pts})
    finally:
        stage1.CHANNELS_LAST_FASTPATH = True
    assert "backbone_features_nlc" not in slow
    for k in ("rpn_cls", "rpn_reg", "backbone_xyz", "backbone_features"):
        assert fast[k].shape == slow[k].shape, k
        scale = float(slow[k].abs().max())
        np.testing.assert_allclose(host(fast[k]), host(slow[k]), atol=2e-5 * max(scale, 1.0), rtol=0, err_msg=k)
    f = fast["backbone_features"].transpose(1, 2).contiguous()
    assert f.data_ptr() == fast["backbone_features_nlc"].data_ptr()          # the (B,C,N) view costs nothing to undo


@pytest.mark.parametrize("c1,c2,c3,ns,R", [(16, 16, 32, 16, 777), (32, 32, 64, 32, 300), (16, 16, 32, 32, 64), (32, 32, 64, 16, 1),
                                          (32, 32, 64, 16, 5002), (32, 32, 64, 32, 40001), (16, 16, 32, 16, 30000)])   # (matrix-core kernel, many tiles per wave)
def test_fused_sa_mlp_pool_matches_gemm_chain(ops, c1, c2, c3, ns, R):
    """ws3d_sa_mlp3_pool == three (row GEMM + bias + ReLU) layers + max over nsample, to fp32
    summation-order rounding (a float64 evaluation sits between the two)"""
    g = torch.Generator().manual_seed(c3 + ns)
    x = (torch.randn((R * ns, 4), generator=g) * 2).cuda()
    layers = []
    cin = 4
    for cout in (c1, c2, c3):
        layers.append((torch.randn((cin, cout), generator=g).mul_(cin ** -0.5).cuda().contiguous(),
                       torch.randn(cout, generator=g).mul_(0.3).cuda(), True))
        cin = cout
    out = torch.full((R, c3 + 8), -3.0, device="cuda")
    assert ops.c.sa_mlp3_pool(x, ns, layers, out, 4)
    h = x.double()
    for w, b, _ in layers:
        h = torch.relu(h @ w.double() + b.double())
    ref = h.view(R, ns, c3).amax(dim=1)
    np.testing.assert_allclose(host(out[:, 4:4 + c3]), host(ref), rtol=2e-5, atol=2e-5)
    assert (out[:, :4] == -3.0).all() and (out[:, 4 + c3:] == -3.0).all()
    # unsupported widths: the caller is told to take the GEMM chain
    bad = [(torch.zeros((4, 8), device="cuda"), torch.zeros(8, device="cuda"), True),
           (torch.zeros((8, 8), device="cuda"), torch.zeros(8, device="cuda"), True),
           (torch.zeros((8, 16), device="cuda"), torch.zeros(16, device="cuda"), True)]
    assert ops.c.sa_mlp3_pool(x, ns, bad, out, 0) is False


# ------------------------------------------------------------------------------- non-finite inputs
def _poison(a, rng, k=4):
    """a few NaN / +inf / -inf coordinates at random places (in place)"""
    flat = a.reshape(-1, a.shape[-1])
    rows = rng.choice(flat.shape[0], 3 * k, replace=False)
    for j, r in enumerate(rows):
        flat[r, rng.integers(0, min(3, a.shape[-1]))] = (np.nan, np.inf, -np.inf)[j % 3]
    return a


def test_nonfinite_coordinates_follow_the_reference_semantics(ops, oracle):
    """NaN / inf coordinates take whatever path the reference's comparisons send them down (the
    oracle restates those comparisons literally): FPS, ball query (both searches), 3-NN (both
    searches), roipool3d and the NMS mask must agree with it bit for bit"""
    rng = np.random.default_rng(77)
    pc = synth.make_batch("lidar", 2, 3000, 5)[:, :, :3].copy()
    _poison(pc, rng)
    # FPS (register kernel) + gathered centres
    ref_idx = oracle.furthest_point_sample(pc, 200)
    idx, new_xyz = ops.pn.furthest_point_sample_gather(dev(pc), 200)
    np.testing.assert_array_equal(host(idx), ref_idx)
    centres = np.stack([pc[b][ref_idx[b]] for b in range(2)])
    np.testing.assert_array_equal(host(new_xyz), centres)                      # NaN == NaN position-wise
    # ball query: brute force and x-binned
    big = synth.make_batch("lidar", 2, 4096, 6)[:, :, :3].copy()
    _poison(big, rng)
    cen = _poison(big[:, :512].copy(), rng, k=2)
    ref_bq = oracle.ball_query(1.0, 16, big, cen)
    np.testing.assert_array_equal(host(ops.pn.ball_query(1.0, 16, dev(big), dev(cen))), ref_bq)
    srt = ops.c.sort_points_x(dev(big))
    got = torch.zeros((2, 512, 16), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(2, 4096, 512, 1.0, 16, dev(cen), dev(big), got, srt)
    np.testing.assert_array_equal(host(got), ref_bq)
    # three_nn: full scan and binned
    kn = _poison(big[:, :2048].copy(), rng, k=2)
    unk = _poison(big[:, 1000:3500].copy(), rng, k=2)
    d2_ref, i_ref = oracle.three_nn_dist2(unk, kn)
    for sorted_known in (None, ops.c.sort_points_x(dev(kn)), ops.c.sort_points_xz(dev(kn))):
        d2 = torch.empty((2, 2500, 3), device="cuda"); i3 = torch.empty((2, 2500, 3), dtype=torch.int32, device="cuda")
        ops.c.three_nn_wrapper(2, 2500, 2048, dev(unk), dev(kn), d2, i3, sorted_known)
        np.testing.assert_array_equal(host(i3), i_ref)
        np.testing.assert_array_equal(host(d2), d2_ref)
    # roipool3d: poisoned points and boxes (NaN heading, infinite extent, NaN centre)
    boxes = synth.proposal_boxes(2, 24, 9)
    boxes[0, 1, 6] = np.nan; boxes[0, 2, 5] = np.inf; boxes[1, 3, 0] = np.nan; boxes[1, 4, 3] = -np.inf
    feat = rng.standard_normal((2, 3000, 8)).astype(np.float32)
    ref_p, ref_e = oracle.roipool3d(pc, boxes, feat, 64)
    pooled = torch.zeros((2, 24, 64, 11), device="cuda"); empty = torch.zeros((2, 24), dtype=torch.int32, device="cuda")
    ops.c.roipool3d_forward(dev(pc), dev(boxes), dev(feat), pooled, empty)
    np.testing.assert_array_equal(host(empty), ref_e)
    np.testing.assert_array_equal(host(pooled), ref_p)
    # NMS mask with a NaN box and an infinite one
    bev = np.ascontiguousarray(synth.boxes3d_to_bev(synth.proposal_boxes(1, 200, 4)[0]))
    bev[5, 0] = np.nan; bev[9, 2] = np.inf; bev[11, 4] = np.nan
    for normal in (False, True):
        ref_mask = oracle.nms_mask(bev, 0.3, normal)
        got_mask = host(ops.c.nms_mask(dev(bev), 0.3, normal, full_grid=True)).view(np.uint64)
        np.testing.assert_array_equal(got_mask, ref_mask)
        ref_keep = oracle.nms_sorted(bev, 0.3, normal)
        keep, num = ops.c.nms_device(dev(bev), 0.3, normal)
        assert int(num.item()) == len(ref_keep)
        np.testing.assert_array_equal(host(keep)[:len(ref_keep)], ref_keep)


@pytest.mark.parametrize("B,n,k", [(3, 16384, 9000), (2, 5000, 5000), (1, 1, 1), (4, 700, 10), (2, 4096, 0), (8, 16384, 16384), (2, 2049, 2049),
                                   (3, 9000, 100), (1, 12289, 9000), (5, 4097, 4000)])
@pytest.mark.parametrize("segments", [True, False])
def test_topk_sorted_kernel(ops, B, n, k, segments):
    """segments: the sort of a scene spread over its CUs (2048-key segments + ranking, ws3d_topk_sorted_ws; n > 2048) against one
    workgroup per scene (ws3d_topk_sorted) -- both are torch's stable descending sort"""
    g = torch.Generator().manual_seed(n)
    s = torch.randn((B, n), generator=g).cuda()
    if n > 300:
        s[0, 100:200] = s[0, 7]                      # ties: ascending index order
        s[-1, 5] = float("inf"); s[-1, 9] = float("-inf"); s[0, 3] = -0.0; s[0, 4] = 0.0
    if n > 4000:
        s[0, 3000:3300] = s[0, 7]                    # the same value in another segment
        s[-1, 2047] = s[-1, 2048] = s[-1, 4095]
    vals, idx = ops.c.topk_sorted(s, k, spread=segments)
    ref_v, ref_i = torch.sort(s, dim=1, descending=True, stable=True)
    assert torch.equal(idx, ref_i[:, :k])
    assert torch.equal(vals, ref_v[:, :k])


@pytest.mark.parametrize("B,n,k,segments", [(3, 16384, 9000, False), (3, 16384, 9000, True), (2, 5000, 5000, False), (2, 5000, 3000, True), (4, 700, 10, False),
                                            (1, 1024, 1024, False), (2, 2049, 100, True)])
def test_topk_sorted_over_the_sigmoid_of_logits(ops, B, n, k, segments):
    """ws3d_topk_sorted_sigmoid[_ws]: the sort over 1 / (1 + exp(-x)) evaluated in the kernel == the sort of torch.sigmoid(x) --
    the same fp32 values bit for bit (torch evaluates the same expression with the same device library), hence the same order
    incl. the ties that the sigmoid's rounding creates between distinct logits (ascending index)"""
    g = torch.Generator().manual_seed(7 * n + k)
    x = (torch.randn((B, n), generator=g) * 6).cuda()
    x[0, :min(n, 40)] = torch.linspace(-104.0, 104.0, min(n, 40))          # saturation on both sides, subnormal results
    if n > 300:
        x[-1, 100:130] = torch.linspace(17.0, 17.00001, 30)              # distinct logits, equal sigmoids
        x[-1, 5] = float("inf"); x[-1, 9] = float("-inf"); x[0, 203] = -0.0; x[0, 204] = 0.0
    ref = torch.sigmoid(x)
    want_v, want_i = ops.c.topk_sorted(ref, k, spread=segments)
    vals, idx = ops.c.topk_sorted(x, k, spread=segments, sigmoid=True)
    assert torch.equal(vals.view(torch.int32), want_v.view(torch.int32))
    assert torch.equal(idx, want_i)


def test_proposal_glue_kernels_of_round_5(ops):
    """ws3d_decode_gather_boxes_bev == ws3d_decode_center_boxes + ws3d_gather_boxes_bev; ws3d_select_proposals_packed's extra rows ==
    cat(boxes, scores); ws3d_split_points_clear == the two strided copies + a fill -- each bit for bit"""
    rng = np.random.default_rng(3)
    B, N, top = 3, 5000, 1200
    xyz = dev(rng.uniform(-40, 40, size=(B, N, 3)).astype(np.float32))
    reg = dev(rng.standard_normal((B, N, 48)).astype(np.float32))
    reg[0, 7, 3] = float("nan")
    order = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(b))[:top] for b in range(B)]).cuda()
    box = ops.c.decode_center_boxes(xyz, reg, 3.0, 0.5, (1.5, 1.6, 3.9))
    want_rows, want_bev = ops.c.gather_boxes_bev(box, order)
    rows, bev = ops.c.decode_gather_boxes_bev(xyz, reg, order, 3.0, 0.5, (1.5, 1.6, 3.9))
    assert torch.equal(rows.view(torch.int32), want_rows.view(torch.int32)) and torch.equal(bev.view(torch.int32), want_bev.view(torch.int32))
    sc = torch.sort(torch.rand((B, top), device="cuda"), dim=1, descending=True)[0]
    keep = torch.stack([torch.randperm(top, generator=torch.Generator().manual_seed(9 + b)) for b in range(B)]).cuda()
    num = torch.tensor([0, 17, 900], dtype=torch.int32, device="cuda")
    a = ops.c.select_proposals(rows, sc, keep, num, 64, 1.0)
    b_ = ops.c.select_proposals(rows, sc, keep, num, 64, 1.0, packed=True)
    assert len(b_) == 5 and all(torch.equal(x_, y_) for x_, y_ in zip(a, b_[:4]))
    assert torch.equal(b_[4].view(torch.int32), torch.cat([a[0], a[1].unsqueeze(-1)], dim=-1).view(torch.int32))
    for C_ in (4, 3, 7):
        pc = dev(rng.standard_normal((2, 1237, C_)).astype(np.float32))
        junk = torch.full((4099 * 4,), float("nan"), device="cuda")
        x_, f_ = ops.c.split_points_clear(pc, junk)
        assert torch.equal(x_, pc[..., :3].contiguous()) and (f_ is None if C_ == 3 else torch.equal(f_, pc[..., 3:].contiguous()))
        assert bool((junk.view(torch.int32) == 0).all())
        x_, f_ = ops.c.split_points_clear(pc, None)
        assert torch.equal(x_, pc[..., :3].contiguous())
    with pytest.raises(ValueError):
        ops.c.split_points_clear(dev(np.zeros((1, 8, 4), np.float32)), torch.zeros(3, device="cuda"))


def test_three_nn_weights_kernel_equals_torch_composition(ops):
    pc = synth.make_batch("lidar", 2, 3000, 12)[:, :, :3].copy()
    kn = pc[:, :700].copy()
    kn[0, 5] = pc[0, 1000]                                  # a zero distance: weight ~ 1e8 / norm
    idx, w = ops.c.three_nn_with_weights(dev(pc), dev(kn))
    dist, ref_idx = ops.pn.three_nn(dev(pc), dev(kn))
    r = 1.0 / (dist + 1e-8)
    ref_w = r / torch.sum(r, dim=2, keepdim=True)
    assert torch.equal(idx, ref_idx)
    np.testing.assert_allclose(host(w), host(ref_w), rtol=3e-7, atol=0)
    np.testing.assert_allclose(host(w.sum(dim=2)), 1.0, rtol=1e-6)
    # the one-launch form (weights in the search kernel's epilogue) == search + ws3d_three_nn_weights, bit for bit, behind every
    # flavour of the binned known set (none: brute force; x slabs; the 3-NN (x, z) grid; the ball query's fine grid)
    from ws3d_amd import _lib
    big = dev(synth.make_batch("hdl64", 2, 16384, 13)[:, :, :3].copy())
    for unknown, known in ((dev(pc), dev(kn)), (big, big[:, :4096].contiguous())):
        B, n, m = unknown.size(0), unknown.size(1), known.size(1)
        for srt in (None, ops.c.sort_points_x(known, min_n=256, grid=False), ops.c.sort_points_xz(known), ops.c.sort_points_x(known, min_n=256, grid=True)):
            d2 = torch.empty((B, n, 3), device="cuda"); i3 = torch.empty((B, n, 3), dtype=torch.int32, device="cuda")
            ops.c.three_nn_wrapper(B, n, m, unknown, known, d2, i3, srt)
            w2 = torch.empty((B, n, 3), device="cuda")
            _lib.check(_lib.load().ws3d_three_nn_weights(B * n, d2.data_ptr(), w2.data_ptr(), torch.cuda.current_stream().cuda_stream))
            i1, w1 = ops.c.three_nn_with_weights(unknown, known, srt)
            assert torch.equal(i1, i3) and torch.equal(w1, w2)


# ------------------------------------------------------------------------------- SA pool (training path)
@pytest.mark.parametrize("ns", [1, 4, 5, 12, 16, 32, 64, 100])
def test_pool_nsample_equals_max_pool2d_forward_and_backward(ops, ns):
    """pool_nsample is the SA module's F.max_pool2d(kernel=[1, nsample]) (pointnet2_modules.py:50):
    values, the argmax the gradient goes to (first maximum; ties, +-inf and NaN rows included) and
    the gradient itself bit-equal to the library op"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(ns)
    x = torch.randn((3, 7, 33, ns), generator=g)
    x = torch.round(x * 2) / 2                     # many exact ties
    x[0, 0, 0, :] = -float("inf")                  # nothing is ever taken: position 0
    x[0, 0, 1, :] = 1.25                           # all equal: first position
    if ns > 2:
        x[0, 1, 2, ns // 2] = float("nan")         # NaN wins ...
        x[0, 1, 3, 1] = float("nan"); x[0, 1, 3, ns - 1] = float("nan")   # ... and the last NaN is recorded
        x[0, 1, 4, ns - 1] = float("inf")
    xa = x.cuda().requires_grad_(True)
    xb = x.cuda().requires_grad_(True)
    ya = ops.pn.pool_nsample(xa)
    yb = F.max_pool2d(xb, kernel_size=[1, ns]).squeeze(-1)
    assert ya.shape == yb.shape
    assert torch.equal(torch.nan_to_num(ya, nan=1e30), torch.nan_to_num(yb, nan=1e30))
    assert torch.equal(torch.isnan(ya), torch.isnan(yb))
    go = torch.randn(ya.shape, generator=g).cuda()
    ya.backward(go)
    yb.backward(go)
    assert torch.equal(xa.grad, xb.grad)


def test_pool_nsample_rejects_wide_windows_and_cpu_tensors(ops):
    with pytest.raises(Exception):
        ops.c.pool_nsample(torch.zeros((4, 300), device="cuda"))
    with pytest.raises(Exception):
        ops.c.pool_nsample(torch.zeros((4, 16)))


# ------------------------------------------------------------------------------- sampling one step ahead
def test_sampling_plan_equals_sampling_inside_the_modules(ops):
    """the FPS chain computed ahead of time (train_rpn.DevicePrefetcher) and handed to the SA
    modules through new_xyz gives the same network output as sampling inside the modules"""
    from ws3d_amd import stage1
    cfg = stage1.RPNConfig(num_points=4096, npoints=(1024, 256, 64, 16))
    torch.manual_seed(0)
    net = stage1.Stage1Net(mode="TRAIN", cfg=cfg).cuda().train()
    pts = torch.from_numpy(np.stack([synth.velodyne_scan(4096, seed=s) for s in (1, 2)])).cuda()
    plan = ops.pn.sampling_plan(pts[..., 0:3].contiguous(), cfg.npoints)
    assert [tuple(p.shape) for p in plan] == [(2, m, 3) for m in cfg.npoints]
    cur = pts[..., 0:3].contiguous()
    for lvl in plan:
        _, cur = ops.pn.furthest_point_sample_gather(cur, lvl.size(1))
        assert torch.equal(cur, lvl)
    # NO warm-up pass (round 3 added one after a single unexplained failure in a full run): the two passes below are the first two
    # forward passes of this network.  The output of EVERY module that returns a tensor is recorded (in training mode a Conv block runs
    # conv1x1_train + bn_relu_train as functions: its conv / bn / activation children are never called, the block itself is), so a
    # mismatch names the first block that differs.
    rec, names = [], {m: n for n, m in net.named_modules()}
    hooks = [m.register_forward_hook(lambda m, i, o: rec[-1].append((names[m], o.detach().clone())) if isinstance(o, torch.Tensor) else None)
             for m in net.modules()]
    rec.append([])
    torch.manual_seed(1)                                     # the heads' Dropout draws from the global generator
    a = net({"pts_input": pts})
    rec.append([])
    torch.manual_seed(1)
    b = net({"pts_input": pts, "sampling_plan": plan})
    for h in hooks:
        h.remove()
    first = next(((n, float((x - y).abs().max())) for (n, x), (_, y) in zip(rec[0], rec[1]) if not torch.equal(x, y)), None)
    assert [n for n, _ in rec[0]] == [n for n, _ in rec[1]] and len(rec[0]) > 40, "the hooks did not see the same modules in both passes"
    assert first is None, "first module whose output differs between the two passes (name, max abs difference): %s" % (first,)
    # (rpn_cls is a VIEW of its head's output -- (B, 1, N) transposed is contiguous as it stands -- so it can be compared with the
    # clone the hook took of that very buffer: a difference says the buffer changed AFTER the head had produced it)
    def diagnose(key, head):
        last = {p: [o for n_, o in rec[p] if n_ == "rpn." + head][-1].transpose(1, 2) for p in (0, 1)}
        out = []
        for p, t in ((0, a[key]), (1, b[key])):
            bad = (t != last[p]).flatten().nonzero().flatten()
            if bad.numel():
                out.append("pass %d: %s differs from the clone taken at its head's exit in %d of %d elements, flat positions %s .. %s, first values now / then %s / %s"
                           % (p, key, bad.numel(), t.numel(), bad[:4].tolist(), bad[-4:].tolist(), t.flatten()[bad[:4]].tolist(), last[p].flatten()[bad[:4]].tolist()))
        return out or ["%s: both passes still equal their head-exit clones; the passes differ in %d elements"
                       % (key, int((a[key] != b[key]).sum()))]
    same = torch.equal(a["rpn_cls"], b["rpn_cls"]) and torch.equal(a["rpn_reg"], b["rpn_reg"])
    assert same, "; ".join(diagnose("rpn_cls", "rpn_cls_layer") + diagnose("rpn_reg", "rpn_reg_layer"))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_consecutive_forward_passes_of_a_cold_process_are_bit_equal(mode):
    """a fresh process, nothing warmed up: passes 0 .. 3 of the TRAIN-mode (library convolutions + own BN / pooling kernels) and the
    inference (fast path) network on the same input are bit-equal in every leaf module (scripts/cold_forward_bits.py)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-B", os.path.join(root, "scripts", "cold_forward_bits.py"), "4", mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RESULT mode=%s passes=4 differing=0" % mode in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("mode", ["train", "eval", "eval_nofast"])
def test_forward_pass_does_not_depend_on_what_recycled_memory_holds(mode):
    """the caching allocator's free blocks filled with zeros / NaN / 3e38 / -7.5 before each pass (torch.empty hands them out as they
    are): a kernel that reads memory it never wrote, or an accumulate-into output that was never cleared, would show here
    (scripts/poison_forward.py)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-B", os.path.join(root, "scripts", "poison_forward.py"), mode], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RESULT mode=%s differing=0" % mode in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_prefetching_trainer_matches_the_inline_loop(ops):
    from ws3d_amd import stage1
    from ws3d_amd.train_rpn import DevicePrefetcher, SyntheticCenters, batches, train
    cfg = stage1.RPNConfig(num_points=4096, npoints=(1024, 256, 64, 16))
    ds = SyntheticCenters(8, npoints=4096)
    on = train(ds, total_iters=8, batch_size=4, seed=5, net_cfg=cfg, prefetch=True)
    off = train(ds, total_iters=8, batch_size=4, seed=5, net_cfg=cfg, prefetch=False)
    np.testing.assert_allclose(on["history"][:4], off["history"][:4], rtol=2e-3)
    # the prefetcher hands out device tensors in the source's order and surfaces its errors
    pf = DevicePrefetcher(batches(ds, 4, np.random.RandomState(5)), "cuda:0", cfg.npoints)
    ref = batches(ds, 4, np.random.RandomState(5))
    for _ in range(3):
        got, want = next(pf), next(ref)
        assert got["sample_id"] == want["sample_id"]
        assert torch.equal(got["pts_input"].cpu(), torch.from_numpy(want["pts_input"]))
        assert got["sampling_plan"][0].shape == (4, 1024, 3) and got["rpn_cls_label"].dtype == torch.float32
    pf.close()

    def broken():
        yield next(batches(ds, 4, np.random.RandomState(5)))
        raise RuntimeError("loader failed")
    pf = DevicePrefetcher(broken(), "cuda:0", cfg.npoints)
    next(pf)
    pf.advance()                                   # the failure is held until the batch is asked for
    with pytest.raises(RuntimeError, match="loader failed"):
        next(pf)
    finite = DevicePrefetcher(iter([next(batches(ds, 4, np.random.RandomState(5)))]), "cuda:0", cfg.npoints)
    assert len(list(finite)) == 1


# ------------------------------------------------------------------------------- BatchNorm + ReLU (training step)
@pytest.mark.parametrize("shape,relu", [((2, 16, 64, 16), True), ((3, 5, 1000), True), ((2, 7, 333), True),
                                         ((2, 3, 5), False), ((4, 32, 4096, 8), True), ((2, 64, 20000), False)])
def test_bn_relu_train_kernels_match_the_library_pair(ops, shape, relu):
    """ws3d_bn_relu_train_fwd/bwd against nn.BatchNorm(train) + ReLU (pytorch_utils.py:35-101): outputs,
    running statistics and all three gradients to fp32 round-off, and bit-identical run to run"""
    import torch.nn as nn
    from ws3d_amd import nn_blocks
    g = torch.Generator().manual_seed(len(shape) * 100 + shape[1])
    c = shape[1]
    x = (torch.randn(shape, generator=g) * 2.0 + 0.7).cuda()
    go = torch.randn(shape, generator=g).cuda()
    cls = nn.BatchNorm2d if len(shape) == 4 else nn.BatchNorm1d
    ref, own = cls(c, momentum=0.3).cuda().train(), cls(c, momentum=0.3).cuda().train()
    with torch.no_grad():
        for m in (ref, own):
            m.weight.copy_(torch.linspace(0.5, 1.5, c)); m.bias.copy_(torch.linspace(-0.3, 0.3, c))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = ref(xa)
    ya = torch.relu(ya) if relu else ya
    yb = nn_blocks.bn_relu_train(xb, own, relu)
    scale = float(ya.detach().abs().max()) + 1e-6
    assert float((ya - yb).detach().abs().max()) <= 2e-6 * scale + 1e-6
    np.testing.assert_allclose(host(own.running_mean), host(ref.running_mean), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(own.running_var), host(ref.running_var), rtol=1e-5, atol=1e-6)
    assert int(own.num_batches_tracked) == 1
    ya.backward(go); yb.backward(go)
    for a, b in ((xa.grad, xb.grad), (ref.weight.grad, own.weight.grad), (ref.bias.grad, own.bias.grad)):
        tol = 2e-5 * (float(a.abs().max()) + 1e-6)
        # an element whose pre-activation rounds to the other side of 0 flips its ReLU mask: allow a handful
        bad = int(((a - b).abs() > tol).sum())
        assert bad <= max(2, a.numel() // 100000), (bad, a.numel())
    own2 = cls(c, momentum=0.3).cuda().train()
    own2.load_state_dict(ref.state_dict() | {"running_mean": torch.zeros(c), "running_var": torch.ones(c),
                                              "num_batches_tracked": torch.tensor(0)})
    own2.weight.data.copy_(own.weight.data); own2.bias.data.copy_(own.bias.data)
    xc = x.clone().requires_grad_(True)
    yc = nn_blocks.bn_relu_train(xc, own2, relu)
    yc.backward(go)
    assert torch.equal(yc, yb) and torch.equal(xc.grad, xb.grad) and torch.equal(own2.weight.grad, own.weight.grad)


def test_conv_block_training_path_uses_the_fused_norm(ops):
    import torch.nn as nn
    from ws3d_amd import nn_blocks
    torch.manual_seed(4)
    blk = nn_blocks.Conv2d(12, 24, bn=True).cuda().train()
    x = torch.randn(2, 12, 50, 16, device="cuda")
    outs = []
    for fused in (True, False):
        nn_blocks.FUSED_BN_TRAIN = fused
        try:
            blk.zero_grad()
            blk.bn[0].running_mean.zero_(); blk.bn[0].running_var.fill_(1.0)
            xi = x.clone().requires_grad_(True)
            y = blk(xi)
            y.square().sum().backward()
            outs.append((y.detach(), xi.grad, blk.conv.weight.grad.clone(), blk.bn[0].weight.grad.clone(),
                         blk.bn[0].running_var.clone()))
        finally:
            nn_blocks.FUSED_BN_TRAIN = True
    for a, b in zip(*outs):
        np.testing.assert_allclose(host(a), host(b), rtol=2e-4, atol=2e-5 * float(b.abs().max()))
    with pytest.raises(Exception):
        ops.c.bn_relu_train_fwd(torch.zeros((1, 4, 1), device="cuda"), torch.ones(4, device="cuda"), torch.zeros(4, device="cuda"),
                                None, None, 0.1, 1e-5)


# ------------------------------------------------------------------------------- batches in flight
def test_stage1_pipeline_equals_the_plain_step(ops):
    """ws3d_amd.pipeline.Stage1Pipeline (hipGraph per slot, several batches in flight, padded last
    batch) returns what the plain forward + proposal stage returns for every batch"""
    from ws3d_amd import stage1
    from ws3d_amd.pipeline import Stage1Pipeline
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.RPNConfig(num_points=4096, npoints=(1024, 256, 64, 16), rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=20)
    model = stage1.Stage1Net(mode="TEST", cfg=cfg)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 3))
    model = model.cuda().eval()
    batches = [np.stack([synth.velodyne_scan(4096, seed=10 * i + j) for j in range(n)]) for i, n in enumerate((3, 3, 3, 3, 2))]
    want = []
    with torch.no_grad():
        for b in batches:
            out = model.rpn_forward({"pts_input": dev(b)})
            boxes, scores, count = stage1.proposals_from_rpn(out, cfg)
            want.append((host(boxes), host(scores), host(count)))
    for use_graph, depth in ((True, 3), (False, 2), (True, 1)):
        pipe = Stage1Pipeline(model, cfg, batch=3, n_points=4096, depth=depth, use_graph=use_graph)
        got = [(f0, nv, host(o["boxes"]), host(o["scores"]), host(o["count"])) for f0, nv, o in pipe.map(batches)]
        assert pipe.graph_error is None
        assert [g[0] for g in got] == [0, 3, 6, 9, 12] and [g[1] for g in got] == [3, 3, 3, 3, 2]
        for (f0, nv, boxes, scores, count), (wb, ws, wc) in zip(got, want):
            np.testing.assert_array_equal(count[:nv], wc)
            for j in range(nv):
                k = int(wc[j])
                np.testing.assert_allclose(boxes[j, :k], wb[j, :k], atol=1e-4)
                np.testing.assert_allclose(scores[j, :k], ws[j, :k], atol=1e-4)
    with pytest.raises(ValueError):
        pipe.submit(np.zeros((4, 4096, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        pipe.result(99)


def test_sort_points_jobs_equals_one_call_per_job(ops, oracle):
    """ws3d_sort_points_jobs (several clouds / both flavours binned by ONE launch) fills every buffer as the single calls do: the
    same cell tables and headers byte for byte, the same records per scene (inside a cell their order is the arrival order of an
    LDS atomic in either form: compared as sets), and the searches on them return the same lists"""
    rng = np.random.default_rng(11)
    B = 3
    clouds = [dev(np.stack([synth.cloud("hdl64", 16384, 900 + j)[:, :3] for j in range(B)])[:, :n].copy()) for n in (4096, 1024, 256)]
    clouds.append(dev(rng.uniform(-3, 3, size=(B, 700, 3)).astype(np.float32)))
    jobs = [(c, "grid") for c in clouds] + [(c, "xz") for c in clouds]
    bufs = ops.c.sort_points_jobs(jobs)
    assert len(bufs) == len(jobs) and all(b is not None for b in bufs)
    for (c, kind), buf in zip(jobs, bufs):
        single = ops.c.sort_points_x(c, 1, grid=True) if kind == "grid" else ops.c.sort_points_xz(c, 1)
        n = c.size(1)
        a, b_ = host(buf).reshape(B, -1), host(single).reshape(B, -1)
        assert a.shape == b_.shape
        np.testing.assert_array_equal(a[:, n * 16:n * 16 + 16], b_[:, n * 16:n * 16 + 16])     # the header (the cell tables' unused tail is not written: checked through the searches below)
        for s_ in range(B):
            ra = np.ascontiguousarray(a[s_, :n * 16]).view(np.uint32).reshape(n, 4)
            rb = np.ascontiguousarray(b_[s_, :n * 16]).view(np.uint32).reshape(n, 4)
            np.testing.assert_array_equal(ra[np.argsort(ra[:, 3], kind="stable")], rb[np.argsort(rb[:, 3], kind="stable")])
    # the searches on the jobs' buffers: every cloud against the centres / queries of the next smaller one
    for k in range(3):
        x, c_ = clouds[k], clouds[k + 1][:, :256].contiguous()
        want = oracle.ball_query(0.8, 16, host(x), host(c_))
        got = torch.zeros((B, c_.size(1), 16), dtype=torch.int32, device="cuda")
        ops.c.ball_query_wrapper(B, x.size(1), c_.size(1), 0.8, 16, c_, x, got, bufs[k])
        np.testing.assert_array_equal(host(got), want)
        _d2, idx = oracle.three_nn_dist2(host(c_), host(x))
        idx_g, _w = ops.c.three_nn_with_weights(c_, x, bufs[4 + k], None)
        np.testing.assert_array_equal(host(idx_g), idx)
    with pytest.raises(ValueError):
        ops.c.sort_points_jobs([(clouds[0], "slab")])


def test_three_nn_jobs_equals_one_call_per_job(ops, oracle):
    """ws3d_three_nn_jobs (the searches of several FP modules in ONE launch) == three_nn_with_weights per module, bit for bit, with
    and without the queries in cell order, and == the oracle's indices"""
    B = 2
    l0 = dev(np.stack([synth.cloud("hdl64", 16384, 1300 + j)[:, :3] for j in range(B)]))
    levels = [l0, l0[:, ::4].contiguous(), l0[:, ::16].contiguous(), l0[:, ::64].contiguous()]         # 16384, 4096, 1024, 256
    xz = [None] + [ops.c.sort_points_xz(x) for x in levels[1:]]
    grid = [ops.c.sort_points_x(x, 1, grid=True) for x in levels]
    for cell_order in (True, False):
        jobs = [(levels[k], levels[k + 1], xz[k + 1], grid[k] if cell_order else None) for k in range(3)]
        got = ops.c.three_nn_jobs(jobs)
        assert got is not None and len(got) == 3
        for (un, kn, sk, su), (idx, w) in zip(jobs, got):
            want_i, want_w = ops.c.three_nn_with_weights(un, kn, sk, su)
            assert torch.equal(idx, want_i) and torch.equal(w.view(torch.int32), want_w.view(torch.int32))
            if un.size(1) <= 4096:
                np.testing.assert_array_equal(host(idx), oracle.three_nn_dist2(host(un), host(kn))[1])
    assert ops.c.three_nn_jobs([(levels[0], levels[1], None, None)]) is None              # not binned: the caller keeps its own call
    assert ops.c.three_nn_jobs([(levels[1], levels[0], grid[0], None)]) is None           # 16384 known points: beyond the LDS copy


def test_pipeline_primed_pair_dispatch_keeps_the_bits(ops):
    """Stage1Pipeline(pair_dispatch="primed") drops the gated dense twins of the scales its priming batch shows far below the fill
    threshold (fastpath.primed_compact_scales); "device" keeps both forms in the graph.  Same bits either way -- on the sparse
    batches the pipeline was primed on AND on a dense batch (a cloud inside a 3 m cube: every list full) sent through the graphs
    primed on sparse ones, where the compact kernels now run above the threshold the dense form would have taken over at."""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.pipeline import Stage1Pipeline
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.RPNConfig(rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=50)
    model = stage1.Stage1Net(mode="TEST", cfg=cfg).eval()
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 7))
    model = model.cuda()
    sparse = [np.stack([synth.cloud("hdl64", 16384, 6100 + 2 * i + j) for j in range(2)]) for i in range(2)]
    rng = np.random.default_rng(5)
    cube = rng.uniform(-1.5, 1.5, size=(2, 16384, 4)).astype(np.float32)
    cube[:, :, 2] += 20.0
    batches = sparse + [cube]
    keys_sparse = fastpath.primed_compact_scales(model.rpn.backbone_net, dev(sparse[0]))
    keys_dense = fastpath.primed_compact_scales(model.rpn.backbone_net, dev(cube))
    assert len(keys_sparse) >= 6 and len(keys_dense) < len(keys_sparse), (keys_sparse, keys_dense)
    outs = {}
    for mode in ("device", "primed"):
        pipe = Stage1Pipeline(model, cfg, batch=2, n_points=16384, depth=2, roipool=True, tune_gemms=False, pair_dispatch=mode)
        got = []
        for b in batches:
            o = pipe.result(pipe.submit(b))
            got.append([o[k].clone() for k in ("boxes", "scores", "count", "pooled", "empty")] + [o["rpn"]["rpn_cls"].clone(), o["rpn"]["rpn_reg"].clone()])
        assert pipe.graph_error is None
        assert pipe.compact_only == (keys_sparse if mode == "primed" else frozenset())
        outs[mode] = got
    for a, b in zip(outs["device"], outs["primed"]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        Stage1Pipeline(model, cfg, batch=2, n_points=16384, depth=1, pair_dispatch="host")


def test_every_launch_mode_of_the_step_gives_the_same_bits(ops):
    """eager on one stream, eager with the coordinate-only work on side streams, a single-stream hipGraph and a hipGraph with the
    side streams forked and joined INSIDE the capture produce bit-identical outputs -- also on their second and third replay and
    with another stream hammering the chip (a missing dependency would show as a race).  Round 2 saw the fork/join graph return
    other proposals: the compact / dense choice was then latched on the host per process (from whatever batch came first) and
    SA4's dense form runs a library GEMM with another summation order; the choice is now taken on the device (launch gates) and the
    same in every mode.  scripts/graph_fork_debug.py is the long form of this test (every SA / FP output, batch 8)."""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.RPNConfig(rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=50)
    model = stage1.Stage1Net(mode="TEST", cfg=cfg).eval()
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 7))
    model = model.cuda()
    pts = dev(np.stack([synth.cloud("hdl64", 16384, 5000 + j) for j in range(2)]))

    @torch.no_grad()
    def body():
        # (defer_reg_join: in the side-stream mode the regression head runs beside the classification head and the top-k; the
        # proposal stage waits for it -- reading rpn_reg below is ordered behind that wait)
        out = model.rpn_forward({"pts_input": pts, "defer_reg_join": True})
        boxes, scores, count = stage1.proposals_from_rpn(out, cfg)
        return [out["rpn_cls"], out["rpn_reg"], out["backbone_features_nlc"], boxes, scores, count]

    saved = (fastpath.GEOMETRY_AHEAD, fastpath.GEOMETRY_IN_CAPTURE)
    try:
        fastpath.GEOMETRY_AHEAD = False
        body()
        ref = [t.clone() for t in body()]
        fastpath.GEOMETRY_AHEAD = True
        for _ in range(3):
            assert all(torch.equal(a, b) for a, b in zip(ref, body())), "eager side streams"
        other = torch.cuda.Stream()
        x = torch.randn(2048, 2048, device="cuda")
        for fork in (False, True):
            fastpath.GEOMETRY_IN_CAPTURE = fork
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                body()
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                res = body()
            for load in (False, False, True, True):
                if load:
                    with torch.cuda.stream(other):
                        for _ in range(10):
                            x = x @ x * 1e-3
                with torch.cuda.stream(s):
                    g.replay()
                torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(ref, res)), "graph, fork/join inside" if fork else "graph, single stream"
    finally:
        fastpath.GEOMETRY_AHEAD, fastpath.GEOMETRY_IN_CAPTURE = saved


def test_roipool3d_fill_writes_every_element(ops, oracle):
    """ws3d_roipool3d_fill: outputs poisoned with NaN / garbage beforehand come out equal to the oracle,
    empty boxes included (zeros), for row widths that are and are not multiples of 16 bytes"""
    pc = synth.make_batch("lidar", 2, 3000, 21)[:, :, :3].copy()
    for C, S in ((8, 64), (5, 33), (0, 16), (128, 512)):
        boxes = synth.proposal_boxes(2, 24, 21)
        boxes[0, 3:7, 0] += 400.0; boxes[1, 0, 2] -= 300.0          # empty boxes
        feat = np.random.default_rng(C + S).standard_normal((2, 3000, C)).astype(np.float32)
        ref_p, ref_e = oracle.roipool3d(pc, boxes, feat, S)
        pooled = torch.full((2, 24, S, 3 + C), float("nan"), device="cuda")
        empty = torch.full((2, 24), 77, dtype=torch.int32, device="cuda")
        pidx = torch.full((2, 24, S), -5, dtype=torch.int32, device="cuda")
        ops.c.roipool3d_forward_fill(dev(pc), dev(boxes), dev(feat), pooled, empty, pidx)
        np.testing.assert_array_equal(host(empty), ref_e)
        np.testing.assert_array_equal(host(pooled), ref_p)
        assert (ref_e == 1).sum() >= 5 and (host(pidx)[ref_e == 1] == 0).all() and (host(pidx) >= 0).all()


def test_three_interpolate_nlc_into_an_odd_stride_buffer(ops, oracle):
    """the FP concat buffer [interpolated | skip] may be 257 floats wide: the left columns are written with
    4-byte-aligned 16-byte stores and the skip column stays untouched"""
    rng = np.random.default_rng(3)
    B, n, m, C = 2, 700, 90, 8
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
    feats = rng.standard_normal((B, C, m)).astype(np.float32)
    ref = oracle.three_interpolate(feats, idx, w)                                  # (B, C, n)
    for extra in (1, 2, 3):
        buf = torch.full((B, n, C + extra), 9.5, device="cuda")
        ops.c.three_interpolate_nlc(dev(np.ascontiguousarray(feats.transpose(0, 2, 1))), dev(idx), dev(w), buf)
        np.testing.assert_array_equal(host(buf[:, :, :C]), ref.transpose(0, 2, 1))
        assert bool((buf[:, :, C:] == 9.5).all())


# ------------------------------------------------------------------------------- last SA layer + pool on the matrix cores
@pytest.mark.parametrize("rows,ns,k,o,relu,bias", [(128, 16, 64, 128, True, True), (256, 32, 96, 64, True, True), (64, 16, 196, 256, False, True),
                                                    (192, 32, 4, 64, True, False), (64, 32, 388, 512, True, True)])
def test_gemm_pool_matches_gemm_then_rowmax(ops, rows, ns, k, o, relu, bias):
    """ws3d_gemm_pool == addmm (+bias, +ReLU) followed by the max over each group of nsample rows, to fp32
    round-off (matrix-core summation order differs from the library GEMM's); written into a column slice"""
    g = torch.Generator().manual_seed(rows + k)
    x = torch.randn((rows, k), generator=g).cuda()
    wt = (torch.randn((k, o), generator=g) * 0.2).cuda()
    b = torch.randn((o,), generator=g).cuda() if bias else None
    y = x.double() @ wt.double()
    if b is not None:
        y = y + b.double()
    if relu:
        y = torch.relu(y)
    ref = y.view(rows // ns, ns, o).amax(dim=1)
    out = torch.full((rows // ns, o + 64), 7.0, device="cuda")
    assert ops.c.gemm_pool(x, wt, b, relu, ns, out, 64)
    assert bool((out[:, :64] == 7.0).all())
    np.testing.assert_allclose(host(out[:, 64:]), host(ref.float()), rtol=2e-5, atol=2e-5 * float(ref.abs().max()))
    # shapes the kernel does not cover are declined, not mis-computed
    assert ops.c.gemm_pool(x[:, :k], wt, b, relu, 8, out, 64) is False
    assert ops.c.gemm_pool(x[:rows - 1], wt, b, relu, ns, out, 64) is False


# ------------------------------------------------------------------------------- weight gradient of the 1x1 convolutions
@pytest.mark.parametrize("B,C,O,shape", [(2, 4, 16, (300, 16)), (3, 16, 16, (64, 4)), (2, 99, 64, (128, 16)), (2, 259, 130, (37,)),
                                          (1, 515, 256, (40, 2)), (2, 128, 1, (1000,)), (2, 33, 200, (5, 3))])
def test_conv1x1_wgrad_matches_the_library_and_is_reproducible(ops, B, C, O, shape):
    """ws3d_conv1x1_wgrad against the float64 contraction (and the library's weight gradient): fp32 round-off,
    and bit-identical from run to run; Conv1d and Conv2d shapes, channel counts off the tile sizes, l not a multiple of 4"""
    g = torch.Generator().manual_seed(C + O)
    x = torch.randn((B, C) + shape, generator=g).cuda()
    gy = torch.randn((B, O) + shape, generator=g).cuda()
    ref = torch.einsum("bol,bcl->oc", gy.reshape(B, O, -1).double(), x.reshape(B, C, -1).double())
    got = ops.c.conv1x1_wgrad(gy, x)
    scale = float(ref.abs().max())
    assert float((got.double() - ref).abs().max()) <= 3e-6 * scale
    for _ in range(3):
        assert torch.equal(ops.c.conv1x1_wgrad(gy, x), got)


def test_conv_block_backward_uses_our_weight_gradient(ops):
    import torch.nn as nn
    from ws3d_amd import nn_blocks
    torch.manual_seed(2)
    blk = nn_blocks.Conv2d(20, 48, bn=True).cuda().train()
    x = torch.randn(2, 20, 70, 16, device="cuda")
    grads = []
    for fused in (True, False, True):
        nn_blocks.FUSED_CONV_WGRAD = fused
        try:
            blk.zero_grad()
            xi = x.clone().requires_grad_(True)
            blk(xi).square().sum().backward()
            grads.append((blk.conv.weight.grad.clone(), xi.grad.clone()))
        finally:
            nn_blocks.FUSED_CONV_WGRAD = True
    np.testing.assert_allclose(host(grads[0][0]), host(grads[1][0]), rtol=2e-4, atol=2e-5 * float(grads[1][0].abs().max()))
    np.testing.assert_allclose(host(grads[0][1]), host(grads[1][1]), rtol=2e-4, atol=2e-5 * float(grads[1][1].abs().max()))
    assert torch.equal(grads[0][0], grads[2][0])          # our path: identical bits on the second run


@pytest.mark.parametrize("B,N,M,ns,C,O,r", [(2, 4096, 1024, 16, 96, 64, 0.5), (2, 4096, 1024, 32, 96, 64, 1.0), (1, 1024, 256, 16, 256, 128, 1.0),
                                           (2, 256, 64, 32, 512, 256, 4.0)])
def test_gather_gemm_equals_group_then_linear(ops, B, N, M, ns, C, O, r):
    """ws3d_gather_gemm (grouping fused into the first SharedMLP layer, fp32 matrix cores) against QueryAndGroup rows @ W + b:
    same neighbour lists (ball query, bit-exact), features within fp32 round-off of the float64 product"""
    rng = np.random.default_rng(4)
    pc = synth.make_batch("lidar", B, 16384, 61)[:, :N, :3].copy()
    xyz = dev(pc)
    feats = dev(rng.standard_normal((B, N, C)).astype(np.float32))
    idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); new_xyz = torch.empty((B, M, 3), device="cuda")
    ops.c.furthest_point_sampling_gather(B, N, M, xyz, None, idx, new_xyz)
    nbr = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, new_xyz, xyz, nbr, ops.c.sort_points_x(xyz))
    wt = dev((rng.standard_normal((C + 3, O)) / np.sqrt(C)).astype(np.float32))       # rows: features, then dx dy dz
    bias = dev(rng.standard_normal(O).astype(np.float32))
    got = ops.c.gather_gemm(feats, xyz, new_xyz, nbr, wt, bias, True)
    assert got is not None and tuple(got.shape) == (B * M * ns, O)
    li = nbr.long()
    gx = torch.gather(xyz, 1, li.view(B, M * ns, 1).expand(B, M * ns, 3)).view(B, M, ns, 3) - new_xyz.unsqueeze(2)
    gf = torch.gather(feats, 1, li.view(B, M * ns, 1).expand(B, M * ns, C)).view(B, M, ns, C)
    x = torch.cat((gf, gx), dim=3).view(-1, C + 3).double()
    want = torch.relu(x @ wt.double() + bias.double())
    err = (got.double() - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= 4e-6 * max(scale, 1.0) * np.sqrt(C / 96), (err, scale)
    assert ops.c.gather_gemm(feats[:, :, :C - 2].contiguous(), xyz, new_xyz, nbr, wt[:C + 1].contiguous(), bias, True) is None   # C % 4


@pytest.mark.parametrize("B,N,M,C2,C1,O", [(2, 4096, 1024, 256, 96, 128), (1, 16384, 4096, 128, 1, 128), (2, 1024, 256, 512, 256, 256),
                                           (2, 256, 64, 512, 512, 512), (2, 1024, 256, 128, 0, 64)])
def test_interp_gemm_equals_interpolate_then_linear(ops, B, N, M, C2, C1, O):
    """ws3d_interp_gemm (three_interpolate + skip concat fused into the first FP layer, fp32 matrix cores) against the bit-exact
    three_interpolate rows, concatenated with the skip features, @ W + b in float64"""
    rng = np.random.default_rng(9)
    pc = synth.make_batch("lidar", B, 16384, 62)[:, :N, :3].copy()
    unknown = dev(pc)
    known = unknown[:, ::N // M].contiguous()
    kf = dev(rng.standard_normal((B, M, C2)).astype(np.float32))
    uf = dev(rng.standard_normal((B, N, C1)).astype(np.float32)) if C1 else None
    idx, weight = ops.c.three_nn_with_weights(unknown, known, None)
    wt = dev((rng.standard_normal((C2 + C1, O)) / np.sqrt(C2 + C1)).astype(np.float32))
    bias = dev(rng.standard_normal(O).astype(np.float32))
    got = ops.c.interp_gemm(kf, uf, idx, weight, wt, bias, True)
    assert got is not None and tuple(got.shape) == (B * N, O)
    interp = torch.empty((B, N, C2), device="cuda")
    ops.c.three_interpolate_nlc(kf, idx, weight, interp)
    x = interp if uf is None else torch.cat((interp, uf), dim=2)
    want = torch.relu(x.view(-1, C2 + C1).double() @ wt.double() + bias.double())
    err = (got.double() - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= 4e-6 * max(scale, 1.0) * np.sqrt((C2 + C1) / 96), (err, scale)
    assert ops.c.interp_gemm(kf, uf, idx, weight, wt[:, :O - 8].contiguous(), bias[:O - 8], True) is None              # O % 64


def test_fps_nested_equals_plain_fps(ops, oracle):
    """ws3d_furthest_point_sampling_nested against the oracle's FPS on the same cloud: clouds in sampling order (the verified
    path: idx = arange), clouds in arbitrary order and sampling-ordered clouds with exact duplicates (ties: the per-scene
    fallback), mixed in one batch; ragged sizes, m = n, m = 1"""
    def sampled(kind, B, N, M, seed, dup=0.0):
        pc = synth.make_batch(kind, B, N, seed, dup_frac=dup)[:, :, :3].copy()
        ref = oracle.furthest_point_sample(pc, M)
        return np.stack([pc[b][ref[b]] for b in range(B)])
    clouds = [
        ("sampling order", sampled("lidar", 3, 16384, 4096, 71), 1024, True),
        ("sampling order, level 3", sampled("lidar", 2, 16384, 4096, 72)[:, :1024].copy(), 256, True),
        ("sampling order, uniform", sampled("uniform", 2, 5000, 1000, 73), 333, True),
        ("all of a cloud with duplicates, re-sampled completely", sampled("lidar", 2, 700, 700, 74, dup=0.3), 700, False),
        ("arbitrary order", synth.make_batch("lidar", 2, 4096, 75)[:, :, :3].copy(), 512, False),
        ("arbitrary order, ragged", synth.make_batch("uniform", 3, 3001, 76)[:, :, :3].copy(), 777, False),
        ("tiny", synth.make_batch("uniform", 2, 37, 77)[:, :, :3].copy(), 37, False),
        ("one point asked", synth.make_batch("uniform", 2, 50, 78)[:, :, :3].copy(), 1, True),
        ("single point", synth.make_batch("uniform", 1, 1, 79)[:, :, :3].copy(), 1, True),
    ]
    mixed = np.stack([sampled("lidar", 1, 8192, 2048, 80)[0], synth.make_batch("lidar", 1, 2048, 81)[0, :, :3]])
    clouds.append(("mixed batch: scene 0 in sampling order, scene 1 not", mixed, 600, None))
    for name, pc, M, expect_prefix in clouds:
        B, N = pc.shape[0], pc.shape[1]
        ref = oracle.furthest_point_sample(pc, M)
        idx = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
        nx = torch.full((B, M, 3), float("nan"), device="cuda")
        ops.c.furthest_point_sampling_nested(B, N, M, dev(pc), idx, nx)
        np.testing.assert_array_equal(host(idx), ref, err_msg=name)
        np.testing.assert_array_equal(host(nx), np.stack([pc[b][ref[b]] for b in range(B)]), err_msg=name)
        if expect_prefix:
            assert (ref == np.arange(M)[None]).all(), name          # the nesting property itself, on the oracle's output
        i2, x2 = ops.pn.furthest_point_sample_gather_nested(dev(pc), M)
        assert torch.equal(i2, idx) and torch.equal(x2, nx)
    assert (oracle.furthest_point_sample(mixed, 600)[0] == np.arange(600)).all()
    with pytest.raises(Exception):
        ops.c.furthest_point_sampling_nested(1, 5000, 10, torch.zeros((1, 5000, 3), device="cuda"),
                                             torch.zeros((1, 10), dtype=torch.int32, device="cuda"), torch.zeros((1, 10, 3), device="cuda"))


def test_fps_nested_chain_equals_level_by_level(ops, oracle):
    """ws3d_furthest_point_sampling_nested_chain (the levels below the first in four launches: when level 0 verifies, the deeper levels
    are verified with it and one kernel writes their prefixes; a scene that does not verify takes the literal restatement level by
    level) against the ORACLE's FPS applied level by level, and against chained calls of the one-level entry: sampling-ordered
    clouds, arbitrary order, duplicates, a mixed batch, one / two / four levels, equal counts, single points"""
    def sampled(kind, B, N, M, seed, dup=0.0):
        pc = synth.make_batch(kind, B, N, seed, dup_frac=dup)[:, :, :3].copy()
        ref = oracle.furthest_point_sample(pc, M)
        return np.stack([pc[b][ref[b]] for b in range(B)])
    mixed = np.stack([sampled("lidar", 1, 8192, 2048, 80)[0], synth.make_batch("lidar", 1, 2048, 81)[0, :, :3]])
    cases = [
        ("the network's chain", sampled("hdl64", 3, 16384, 4096, 171), [1024, 256, 64]),
        ("four levels", sampled("lidar", 2, 16384, 4096, 172), [2048, 512, 128, 7]),
        ("one level", sampled("lidar", 2, 16384, 4096, 173), [1000]),
        ("equal counts", sampled("uniform", 2, 5000, 1000, 174), [1000, 1000, 333]),
        ("duplicates: the fallback at every level", sampled("lidar", 2, 700, 700, 175, dup=0.3), [700, 300, 40]),
        ("arbitrary order", synth.make_batch("lidar", 2, 4096, 176)[:, :, :3].copy(), [512, 100, 9]),
        ("mixed batch: scene 0 in sampling order, scene 1 not", mixed, [600, 150, 30]),
        ("tiny", synth.make_batch("uniform", 2, 37, 177)[:, :, :3].copy(), [37, 5, 1]),
        ("single point", synth.make_batch("uniform", 1, 1, 178)[:, :, :3].copy(), [1, 1]),
    ]
    for name, pc, ms in cases:
        got = ops.pn.furthest_point_sample_gather_nested_chain(dev(pc), ms)
        assert len(got) == len(ms)
        cur_host, cur_dev = pc, dev(pc)
        for (idx, nx), m in zip(got, ms):
            ref = oracle.furthest_point_sample(cur_host, m)
            want = np.stack([cur_host[b][ref[b]] for b in range(pc.shape[0])])
            np.testing.assert_array_equal(host(idx), ref, err_msg="%s, level of %d" % (name, m))
            np.testing.assert_array_equal(host(nx), want, err_msg="%s, level of %d" % (name, m))
            i1, x1 = ops.pn.furthest_point_sample_gather_nested(cur_dev, m)
            assert torch.equal(i1, idx) and torch.equal(x1, nx), name
            cur_host, cur_dev = want, nx
    with pytest.raises(Exception):                   # counts must not grow along the chain
        ops.c.furthest_point_sampling_nested_chain(dev(cases[0][1]), [256, 1024])


@pytest.mark.parametrize("B,N,M,ns,C,O1,O2,r", [(2, 4096, 1024, 16, 96, 64, 64, 0.5), (2, 4096, 1024, 32, 96, 64, 96, 1.0), (1, 1024, 256, 16, 256, 128, 196, 1.0),
                                              (2, 256, 64, 32, 512, 256, 384, 4.0), (2, 256, 64, 16, 512, 256, 256, 2.0)])
def test_gather_gemm2_equals_two_layers(ops, B, N, M, ns, C, O1, O2, r):
    """ws3d_gather_gemm2 (layers 1 + 2 of a set-abstraction SharedMLP, the first activation on chip) against the float64
    product relu(relu([gf | gx] @ W1 + b1) @ W2 + b2), and against ws3d_gather_gemm followed by a GEMM"""
    rng = np.random.default_rng(14)
    pc = synth.make_batch("lidar", B, 16384, 63)[:, :N, :3].copy()
    xyz = dev(pc)
    feats = dev(rng.standard_normal((B, N, C)).astype(np.float32))
    idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); new_xyz = torch.empty((B, M, 3), device="cuda")
    ops.c.furthest_point_sampling_gather(B, N, M, xyz, None, idx, new_xyz)
    nbr = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, new_xyz, xyz, nbr, ops.c.sort_points_x(xyz))
    w1 = dev((rng.standard_normal((C + 3, O1)) / np.sqrt(C)).astype(np.float32))
    b1 = dev(rng.standard_normal(O1).astype(np.float32))
    w2 = dev((rng.standard_normal((O1, O2)) / np.sqrt(O1)).astype(np.float32))
    b2 = dev(rng.standard_normal(O2).astype(np.float32))
    got = ops.c.gather_gemm2(feats, xyz, new_xyz, nbr, w1, b1, True, w2, b2, True)
    assert got is not None and tuple(got.shape) == (B * M * ns, O2)
    li = nbr.long()
    gx = torch.gather(xyz, 1, li.view(B, M * ns, 1).expand(B, M * ns, 3)).view(B, M, ns, 3) - new_xyz.unsqueeze(2)
    gf = torch.gather(feats, 1, li.view(B, M * ns, 1).expand(B, M * ns, C)).view(B, M, ns, C)
    x = torch.cat((gf, gx), dim=3).view(-1, C + 3).double()
    h = torch.relu(x @ w1.double() + b1.double())
    want = torch.relu(h @ w2.double() + b2.double())
    err = (got.double() - want).abs().max().item()
    scale = max(want.abs().max().item(), 1.0)
    assert err <= 1e-5 * scale * np.sqrt(C / 96), (err, scale)
    two = torch.relu(ops.c.gather_gemm(feats, xyz, new_xyz, nbr, w1, b1, True) @ w2 + b2)
    assert (got - two).abs().max().item() <= 2e-5 * scale
    no_act = ops.c.gather_gemm2(feats, xyz, new_xyz, nbr, w1, None, False, w2, None, False)
    assert (no_act.double() - (x @ w1.double()) @ w2.double()).abs().max().item() <= 2e-5 * scale * np.sqrt(C / 96)
    assert ops.c.gather_gemm2(feats, xyz, new_xyz, nbr, w1[:, :O1 - 16].contiguous(), None, True, w2[:O1 - 16].contiguous(), b2, True) is None   # O1


def test_eager_side_streams_back_to_back_equal_the_single_stream_forward(ops):
    """the coordinate-only work of a forward pass runs on two side streams (fastpath._Geometry) and its tensors are allocated
    there: 24 different batches issued back to back WITHOUT host synchronisation -- plain calls on one stream, and through an
    eager 3-deep Stage1Pipeline whose slots share the side streams -- must reproduce the single-stream forward exactly
    (same kernels, same order per batch: any difference would be a cross-stream reuse of live memory)"""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.pipeline import Stage1Pipeline
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.RPNConfig(num_points=4096, npoints=(1024, 256, 64, 16), rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=20)
    model = stage1.Stage1Net(mode="TEST", cfg=cfg)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 5))
    model = model.cuda().eval()
    batches = [dev(np.stack([synth.velodyne_scan(4096, seed=100 + 2 * i + j) for j in range(2)])) for i in range(24)]
    keys = ("rpn_cls", "rpn_reg")
    prev = fastpath.GEOMETRY_AHEAD
    try:
        fastpath.GEOMETRY_AHEAD = False
        with torch.no_grad():
            want = []
            for b in batches:
                out = model.rpn_forward({"pts_input": b})
                boxes, scores, count = stage1.proposals_from_rpn(out, cfg)
                want.append([out[k].clone() for k in keys] + [boxes.clone(), count.clone()])
        torch.cuda.synchronize()
        fastpath.GEOMETRY_AHEAD = True
        with torch.no_grad():
            got = []
            for b in batches:                      # no synchronisation between the passes
                out = model.rpn_forward({"pts_input": b})
                boxes, scores, count = stage1.proposals_from_rpn(out, cfg)
                got.append([out[k].clone() for k in keys] + [boxes.clone(), count.clone()])
        torch.cuda.synchronize()
        for i, (g, w) in enumerate(zip(got, want)):
            for a, c in zip(g, w):
                assert torch.equal(a, c), i
        pipe = Stage1Pipeline(model, cfg, batch=2, n_points=4096, depth=3, use_graph=False)
        for i, (f0, nv, o) in enumerate(pipe.map(batches)):
            assert torch.equal(o["rpn"]["rpn_cls"], want[i][0]) and torch.equal(o["rpn"]["rpn_reg"], want[i][1]), i
            assert torch.equal(o["boxes"], want[i][2]) and torch.equal(o["count"], want[i][3]), i
    finally:
        fastpath.GEOMETRY_AHEAD = prev


@pytest.mark.parametrize("rows,o2,relu2,bias", [(32, 1, False, True), (4096, 40, False, True), (16384 + 32, 1, False, True),
                                                 (2048, 64, True, True), (1024, 33, True, False), (131072, 40, False, True)])
def test_mlp2_rows_matches_two_layers(rows, o2, relu2, bias):
    """ws3d_mlp2_rows (both layers of a head in one kernel, activation in registers) against the same two layers in float64"""
    import torch
    from ws3d_amd import compat as C
    g = torch.Generator().manual_seed(rows + o2)
    x = torch.randn(rows, 128, generator=g).cuda()
    w1t = (torch.randn(128, 128, generator=g) / 11).cuda()
    w2t = (torch.randn(128, o2, generator=g) / 11).cuda()
    b1 = torch.randn(128, generator=g).cuda() if bias else None
    b2 = torch.randn(o2, generator=g).cuda() if bias else None
    y = C.mlp2_rows(x, w1t, b1, True, w2t, b2, relu2)
    assert y is not None and y.shape == (rows, o2)
    h = x.double() @ w1t.double()
    if bias:
        h = h + b1.double()
    h = h.clamp_min(0)
    ref = h @ w2t.double()
    if bias:
        ref = ref + b2.double()
    if relu2:
        ref = ref.clamp_min(0)
    err = (y.double() - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err
    # shapes outside the kernel's cover: None, the caller runs two GEMMs
    assert C.mlp2_rows(x[:, :64].contiguous(), w1t[:64].contiguous(), b1, True, w2t, b2, relu2) is None
    assert C.mlp2_rows(x[:31], w1t, b1, True, w2t, b2, relu2) is None


def test_gemm_pool_both_output_tiles():
    """ws3d_gemm_pool against the float64 product + group max on shapes that take the 64 x 64 kernel and on one that takes the
    128 x 128 one (rows % 128 == 0, O % 128 == 0, >= 512 tiles: the last shape); in a child process like the other library-level checks"""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys, torch
        sys.path.insert(0, {root!r})
        from ws3d_amd import compat as c
        for rows, ns, k, o, relu in [(128, 16, 4, 128, True), (256, 32, 100, 256, False), (2048, 16, 196, 256, True), (4096, 32, 384, 512, True),
                                     (192, 32, 64, 64, True), (65536, 32, 96, 128, True)]:
            g = torch.Generator().manual_seed(rows + k)
            x = torch.randn((rows, k), generator=g).cuda(); wt = (torch.randn((k, o), generator=g) * 0.2).cuda(); b = torch.randn((o,), generator=g).cuda()
            y = x.double() @ wt.double() + b.double()
            if relu: y = torch.relu(y)
            ref = y.view(rows // ns, ns, o).amax(dim=1)
            out = torch.full((rows // ns, o + 64), 7.0, device="cuda")
            assert c.gemm_pool(x, wt, b, relu, ns, out, 64)
            assert bool((out[:, :64] == 7.0).all())
            err = float((out[:, 64:].double() - ref).abs().max())
            assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (rows, ns, k, o, err)
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_interp_gemm_both_output_tiles():
    """ws3d_interp_gemm against three_interpolate + concat + float64 product, including the c1 = 1 ragged skip block of FP1: shapes
    that take the 64 x 64 kernel and one that takes the 64 x 128 one (O % 128 == 0, >= 512 tiles: the last shape)"""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys, numpy as np, torch
        sys.path.insert(0, {root!r})
        from ws3d_amd import compat as c, synth
        rng = np.random.default_rng(9)
        for B, N, M, C2, C1, O in [(8, 1024, 256, 64, 1, 128), (2, 512, 128, 96, 32, 256), (8, 256, 64, 128, 0, 128), (1, 192, 48, 32, 5, 64),
                                   (16, 2048, 512, 256, 1, 128)]:
            pc = synth.make_batch("lidar", B, 16384, 62)[:, :N, :3].copy()
            unknown = torch.from_numpy(pc).cuda(); known = unknown[:, ::N // M].contiguous()
            kf = torch.from_numpy(rng.standard_normal((B, M, C2)).astype(np.float32)).cuda()
            uf = torch.from_numpy(rng.standard_normal((B, N, C1)).astype(np.float32)).cuda() if C1 else None
            idx, weight = c.three_nn_with_weights(unknown, known, None)
            wt = torch.from_numpy((rng.standard_normal((C2 + C1, O)) / np.sqrt(C2 + C1)).astype(np.float32)).cuda()
            bias = torch.from_numpy(rng.standard_normal(O).astype(np.float32)).cuda()
            got = c.interp_gemm(kf, uf, idx, weight, wt, bias, True)
            interp = torch.empty((B, N, C2), device="cuda"); c.three_interpolate_nlc(kf, idx, weight, interp)
            x = interp if uf is None else torch.cat((interp, uf), dim=2)
            want = torch.relu(x.view(-1, C2 + C1).double() @ wt.double() + bias.double())
            err = (got.double() - want).abs().max().item()
            assert err <= 4e-6 * max(want.abs().max().item(), 1.0) * np.sqrt((C2 + C1) / 96), (B, N, M, C2, C1, O, err)
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_fast_path_switches_agree(ops):
    """the optional fusions of the inference fast path (whole-SharedMLP kernel at SA2 / SA3, two-layer heads, two-layer
    gather-GEMM, fused interpolation) switched on and off: the network's outputs agree to fp32 round-off of the matrix products
    (different summation orders), i.e. every switch computes the same function"""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.RPNConfig(num_points=16384, rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=20)
    model = stage1.Stage1Net(mode="TEST", cfg=cfg)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 6))
    model = model.cuda().eval()
    pts = dev(np.stack([synth.velodyne_scan(16384, seed=300 + j) for j in range(8)]))
    names = ("FUSED_MLP2_ROWS", "FUSED_GATHER_GEMM2", "FUSED_INTERP_GEMM", "PER_POINT_L1", "PER_POINT_FP", "COMPACT_PAIRS", "SA1_FROM_LISTS", "PARALLEL_SCALES", "PARALLEL_HEADS",
             "FUSED_COMPACT3_MAX_LDS", "FUSED_QINTERP_GEMM_MIN_ROWS", "BIN_INPUT_AHEAD", "NESTED_CHAIN", "QUERY_CELL_ORDER", "DUAL_SCALE_SEARCH", "MERGED_BINNING", "FUSED_PROLOGUE", "MERGED_THREE_NN", "PAIRED_SCALES", "CHAIN_MLP")
    saved = {n: getattr(fastpath, n) for n in names}

    def run(**kw):
        for n, v in kw.items():
            setattr(fastpath, n, v)
        with torch.no_grad():
            out = model.rpn_forward({"pts_input": pts})
        return out["rpn_cls"].clone(), out["rpn_reg"].clone()
    try:
        off = {"FUSED_MLP2_ROWS": False, "FUSED_GATHER_GEMM2": False, "FUSED_INTERP_GEMM": False, "PER_POINT_L1": False, "PER_POINT_FP": False, "COMPACT_PAIRS": False,
               "SA1_FROM_LISTS": False, "PARALLEL_SCALES": False, "PARALLEL_HEADS": False, "FUSED_COMPACT3_MAX_LDS": 0, "FUSED_QINTERP_GEMM_MIN_ROWS": 1 << 60,
               "BIN_INPUT_AHEAD": False, "NESTED_CHAIN": False, "QUERY_CELL_ORDER": False, "DUAL_SCALE_SEARCH": False, "MERGED_BINNING": False, "FUSED_PROLOGUE": False}
        base = run(**off)
        scale = [float(t.abs().max()) for t in base]
        for kw in ({"FUSED_MLP2_ROWS": True}, {"FUSED_GATHER_GEMM2": True}, {"FUSED_INTERP_GEMM": True}, {"PER_POINT_L1": True}, {"PER_POINT_FP": True}, {"PER_POINT_L1": True, "PER_POINT_FP": True, "FUSED_MLP2_ROWS": True}, {"PER_POINT_L1": True, "COMPACT_PAIRS": True},
                   {"SA1_FROM_LISTS": True}, {"SA1_FROM_LISTS": True, "COMPACT_PAIRS": True, "PER_POINT_L1": True}, {"PARALLEL_SCALES": True, "PARALLEL_HEADS": True, "PER_POINT_L1": True, "COMPACT_PAIRS": True},
                   {"FUSED_MLP2_ROWS": True, "FUSED_GATHER_GEMM2": True, "FUSED_INTERP_GEMM": True},
                   {"PER_POINT_L1": True, "COMPACT_PAIRS": True, "FUSED_COMPACT3_MAX_LDS": 64 * 1024}, {"PER_POINT_L1": True, "COMPACT_PAIRS": True, "FUSED_COMPACT3_MAX_LDS": 160 * 1024},
                   {"PER_POINT_FP": True, "FUSED_QINTERP_GEMM_MIN_ROWS": 30000}, {"PER_POINT_FP": True, "FUSED_QINTERP_GEMM_MIN_ROWS": 1}, {"BIN_INPUT_AHEAD": True, "PARALLEL_SCALES": True},
                   {"NESTED_CHAIN": True}, {"QUERY_CELL_ORDER": True}, {"NESTED_CHAIN": True, "QUERY_CELL_ORDER": True, "PER_POINT_L1": True, "COMPACT_PAIRS": True},
                   {"DUAL_SCALE_SEARCH": True, "PER_POINT_L1": True, "COMPACT_PAIRS": True, "SA1_FROM_LISTS": True}):
            for n, v in saved.items():
                setattr(fastpath, n, v)
            got = run(**dict(off, **kw))
            for g, b, s in zip(got, base, scale):
                assert float((g - b).abs().max()) <= 2e-4 * max(s, 1.0), (kw, float((g - b).abs().max()), s)
        for n, v in saved.items():
            setattr(fastpath, n, v)
        with fastpath.geometry_ahead(False):      # the serial order Stage1Pipeline's graphs capture: one binning launch for levels 2.. or one per level and flavour
            one, per_level = run(MERGED_BINNING=True), run(MERGED_BINNING=False)
            split = run(FUSED_PROLOGUE=False)
            for n, v in saved.items():
                setattr(fastpath, n, v)
            assert all(torch.equal(x_, y_) for x_, y_ in zip(one, run(MERGED_THREE_NN=False)))
            for n, v in saved.items():
                setattr(fastpath, n, v)
            with fastpath.compact_only_scales({(l_, s_) for l_ in range(4) for s_ in range(2)}):       # (what a primed pipeline captures)
                assert all(torch.equal(x_, y_) for x_, y_ in zip(run(PAIRED_SCALES=True), run(PAIRED_SCALES=False)))
                for n, v in saved.items():
                    setattr(fastpath, n, v)
                # round 6: SA2's SharedMLP on the register-chained kernel (ws3d_chain_mlp3) or on ws3d_compact_mlp_pair(3): the same bits
                assert all(torch.equal(x_, y_) for x_, y_ in zip(run(CHAIN_MLP=True), run(CHAIN_MLP=False)))
                for n, v in saved.items():
                    setattr(fastpath, n, v)
        assert all(torch.equal(x_, y_) for x_, y_ in zip(one, per_level)) and all(torch.equal(x_, y_) for x_, y_ in zip(one, split))
        assert all(torch.equal(x_, y_) for x_, y_ in zip(run(FUSED_PROLOGUE=True), run(FUSED_PROLOGUE=False)))        # and with the side streams
    finally:
        for n, v in saved.items():
            setattr(fastpath, n, v)


@pytest.mark.parametrize("B,N,M,ns,C,O1,O2,r", [(2, 4096, 1024, 16, 96, 64, 64, 0.5), (2, 4096, 1024, 32, 96, 64, 96, 1.0), (1, 1024, 256, 16, 256, 128, 196, 1.0),
                                              (2, 256, 64, 32, 512, 256, 384, 4.0), (1, 512, 128, 16, 8, 64, 20, 1.0)])
def test_per_point_layer1_equals_the_grouped_product(ops, B, N, M, ns, C, O1, O2, r):
    """ws3d_pgather_gemm2 / ws3d_pgather_rows (layer 1 as feats @ W_f over the POINTS, gathered per pair, + the centred xyz term)
    against the float64 product over the grouped rows and against ws3d_gather_gemm(2); P carries a second scale's columns, so
    the column offset and the row stride are exercised"""
    rng = np.random.default_rng(16)
    pc = synth.make_batch("lidar", B, 16384, 65)[:, :N, :3].copy()
    xyz = dev(pc)
    feats = dev(rng.standard_normal((B, N, C)).astype(np.float32))
    idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); new_xyz = torch.empty((B, M, 3), device="cuda")
    ops.c.furthest_point_sampling_gather(B, N, M, xyz, None, idx, new_xyz)
    nbr = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, new_xyz, xyz, nbr, ops.c.sort_points_x(xyz))
    w1 = dev((rng.standard_normal((C + 3, O1)) / np.sqrt(C)).astype(np.float32)); b1 = dev(rng.standard_normal(O1).astype(np.float32))
    w2 = dev((rng.standard_normal((O1, O2)) / np.sqrt(O1)).astype(np.float32)); b2 = dev(rng.standard_normal(O2).astype(np.float32))
    other = dev(rng.standard_normal((C, 64)).astype(np.float32))                  # another scale's columns in front
    pmat = feats.view(B * N, C) @ torch.cat((other, w1[:C]), dim=1)
    w1x = w1[C:].contiguous()
    li = nbr.long()
    gx = torch.gather(xyz, 1, li.view(B, M * ns, 1).expand(B, M * ns, 3)).view(B, M, ns, 3) - new_xyz.unsqueeze(2)
    gf = torch.gather(feats, 1, li.view(B, M * ns, 1).expand(B, M * ns, C)).view(B, M, ns, C)
    x = torch.cat((gf, gx), dim=3).view(-1, C + 3).double()
    h = torch.relu(x @ w1.double() + b1.double())
    tol = 1e-5 * np.sqrt(max(C, 96) / 96)
    rows = ops.c.pgather_rows(pmat, 64, O1, xyz, new_xyz, nbr, w1x, b1, True)
    assert rows is not None and tuple(rows.shape) == (B * M * ns, O1)
    assert (rows.double() - h).abs().max().item() <= tol * max(h.abs().max().item(), 1.0)
    assert (rows - ops.c.gather_gemm(feats, xyz, new_xyz, nbr, w1, b1, True)).abs().max().item() <= 2 * tol * max(h.abs().max().item(), 1.0)
    if O1 <= 128:
        want = torch.relu(h @ w2.double() + b2.double())
        got = ops.c.pgather_gemm2(pmat, 64, O1, xyz, new_xyz, nbr, w1x, b1, True, w2, b2, True)
        assert got is not None and tuple(got.shape) == (B * M * ns, O2)
        assert (got.double() - want).abs().max().item() <= tol * max(want.abs().max().item(), 1.0)
        no_act = ops.c.pgather_gemm2(pmat, 64, O1, xyz, new_xyz, nbr, w1x, None, False, w2, None, False)
        assert (no_act.double() - (x @ w1.double()) @ w2.double()).abs().max().item() <= 2 * tol * max(want.abs().max().item(), 1.0)
    else:
        assert ops.c.pgather_gemm2(pmat, 64, O1, xyz, new_xyz, nbr, w1x, b1, True, w2, b2, True) is None


@pytest.mark.parametrize("B,N,M,C2,C1,O", [(2, 4096, 1024, 256, 96, 256), (1, 16384, 4096, 128, 1, 128), (2, 1024, 256, 512, 256, 512),
                                           (2, 256, 64, 512, 512, 512), (2, 1024, 256, 128, 0, 64), (1, 300, 70, 64, 3, 20)])
def test_qinterp_rows_equals_interpolate_then_linear(ops, B, N, M, C2, C1, O):
    """ws3d_qinterp_rows (first FP layer as the interpolation of Q = known_feats @ W_a + the skip channels' product) against
    three_interpolate + concat + float64 product, and against ws3d_interp_gemm where that applies; both skip forms (lin from
    a GEMM, <= 4 channels evaluated inside), no skip, no bias"""
    rng = np.random.default_rng(17)
    pc = synth.make_batch("lidar", B, 16384, 66)[:, :N, :3].copy()
    unknown = dev(pc)
    known = unknown[:, ::max(N // M, 1)][:, :M].contiguous()
    kf = dev(rng.standard_normal((B, M, C2)).astype(np.float32))
    uf = dev(rng.standard_normal((B, N, C1)).astype(np.float32)) if C1 else None
    idx, weight = ops.c.three_nn_with_weights(unknown, known, None)
    wt = dev((rng.standard_normal((C2 + C1, O)) / np.sqrt(C2 + C1)).astype(np.float32))
    bias = dev(rng.standard_normal(O).astype(np.float32))
    interp = torch.empty((B, N, C2), device="cuda")
    ops.c.three_interpolate_nlc(kf, idx, weight, interp)
    x = interp if uf is None else torch.cat((interp, uf), dim=2)
    want = torch.relu(x.view(-1, C2 + C1).double() @ wt.double() + bias.double())
    q = (kf.view(B * M, C2) @ wt[:C2]).view(B, M, O)
    tol = 6e-6 * max(want.abs().max().item(), 1.0) * np.sqrt((C2 + C1) / 96)
    if C1 > 4:
        lin = torch.addmm(bias, uf.view(B * N, C1), wt[C2:].contiguous())
        got = ops.c.qinterp_rows(q, idx, weight, lin=lin, relu=True)
    else:
        got = ops.c.qinterp_rows(q, idx, weight, skip=uf, wb=wt[C2:].contiguous() if C1 else None, bias=bias, relu=True)
    assert got is not None and tuple(got.shape) == (B * N, O)
    assert (got.double() - want).abs().max().item() <= tol
    if O % 64 == 0 and (B * N) % 64 == 0:
        fused = ops.c.interp_gemm(kf, uf, idx, weight, wt, bias, True)
        if fused is not None:
            assert (got - fused).abs().max().item() <= 2 * tol
    if C1 <= 4:
        nb = ops.c.qinterp_rows(q, idx, weight, skip=uf, wb=wt[C2:].contiguous() if C1 else None, bias=None, relu=False)
        assert (nb.double() - x.view(-1, C2 + C1).double() @ wt.double()).abs().max().item() <= tol
        assert ops.c.qinterp_rows(q[:, :, :O - 1].contiguous(), idx, weight, relu=True) is None if (O - 1) % 4 else True


@pytest.mark.parametrize("B,N,M,C2,C1,C,O,relu1", [(1, 16384, 4096, 256, 1, 128, 128, True), (2, 4096, 1024, 512, 96, 256, 256, True), (2, 1024, 256, 512, 256, 512, 512, True),
                                                     (2, 256, 64, 64, 0, 64, 128, False), (1, 1000, 256, 64, 3, 64, 128, True), (2, 1024, 256, 64, 2, 48, 64, True)])
def test_qinterp_gemm_is_qinterp_rows_followed_by_the_second_layer(ops, B, N, M, C2, C1, C, O, relu1):
    """ws3d_qinterp_gemm (both layers of a two-layer FP module in one kernel: the first layer's rows are built in the A operand of the
    second layer's product): with an identity second layer it returns ws3d_qinterp_rows' rows to the bit -- both skip forms -- and with a
    real one the float64 product of those rows; shapes outside its tiles are declined (the caller runs the two-launch form)"""
    rng = np.random.default_rng(29)
    pc = synth.make_batch("hdl64", B, 16384, 72)[:, :N, :3].copy()
    unknown = dev(pc)
    known = unknown[:, ::max(N // M, 1)][:, :M].contiguous()
    kf = dev(rng.standard_normal((B, M, C2)).astype(np.float32))
    uf = dev(rng.standard_normal((B, N, C1)).astype(np.float32)) if C1 else None
    idx, weight = ops.c.three_nn_with_weights(unknown, known, None)
    wa = dev((rng.standard_normal((C2, C)) / np.sqrt(C2)).astype(np.float32))
    wb = dev((rng.standard_normal((C1, C)) / np.sqrt(max(C1, 1))).astype(np.float32)) if C1 else None
    b1 = dev(rng.standard_normal(C).astype(np.float32))
    q = (kf.view(B * M, C2) @ wa).view(B, M, C)
    if C1 > 4:
        kw = dict(lin=torch.addmm(b1, uf.view(B * N, C1), wb))
    else:
        kw = dict(skip=uf, wb=wb, bias=b1)
    rows = ops.c.qinterp_rows(q, idx, weight, relu=relu1, **kw)
    w2 = dev((rng.standard_normal((C, O)) / np.sqrt(C)).astype(np.float32))
    b2 = dev(rng.standard_normal(O).astype(np.float32))
    got = ops.c.qinterp_gemm(q, idx, weight, w2, b2, True, relu=relu1, **kw)
    if (B * N) % 64 or C % 16 or O % 128:
        assert got is None
        return
    want = torch.relu(rows.double() @ w2.double() + b2.double())
    assert got is not None and tuple(got.shape) == (B * N, O)
    assert (got.double() - want).abs().max().item() <= 2e-5 * max(want.abs().max().item(), 1.0) * np.sqrt(max(C, 128) / 128)
    if C == O:
        eye = torch.eye(C, device="cuda")
        assert torch.equal(ops.c.qinterp_gemm(q, idx, weight, eye, None, False, relu=relu1, **kw), rows)


@pytest.mark.parametrize("B,N,M,C,O1,scales", [(2, 4096, 1024, 96, 64, ((16, 0.5, 64, 128), (32, 1.0, 96, 128))),          # SA2's two scales: the fused kernel
                                               (2, 1024, 256, 256, 128, ((16, 1.0, 128, 256), (32, 2.0, 196, 256))),      # SA3
                                               (2, 256, 64, 512, 256, ((16, 2.0, 256, 512), (32, 4.0, 384, 512))),        # SA4: first layer 256 wide, two-kernel form only
                                               (1, 512, 37, 8, 64, ((16, 0.01, 20, 64), (16, 3.0, 64, 192))),             # ragged: 37 centres, one-point lists beside full ones
                                               (3, 2048, 300, 12, 64, ((16, 0.3, 20, 128), (32, 2.5, 84, 128))),          # the register-chained kernel's ragged widths (o2 = 20, 84) and 300 centres
                                               (1, 1024, 256, 32, 64, ((32, 40.0, 96, 128), (16, 0.2, 32, 128)))])        # full lists beside sparse ones, widths 96 / 32
def test_compact_mlp_pair_equals_the_single_scale_launches(ops, B, N, M, C, O1, scales):
    """ws3d_compact_mlp_pair (both scales of a level in ONE launch: the fused three-layer kernel, or layers 1 + 2 then layer 3 + pool)
    == the single-scale launches, bit for bit, incl. the column slices of a shared output and scales of unequal pair counts"""
    rng = np.random.default_rng(23)
    pc = synth.make_batch("lidar", B, 16384, 71)[:, :N, :3].copy()
    xyz = dev(pc)
    feats = dev(rng.standard_normal((B, N, C)).astype(np.float32))
    idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); new_xyz = torch.empty((B, M, 3), device="cuda")
    ops.c.furthest_point_sampling_gather(B, N, M, xyz, None, idx, new_xyz)
    srt = ops.c.sort_points_x(xyz)
    w1s = [dev((rng.standard_normal((C + 3, O1)) / np.sqrt(C)).astype(np.float32)) for _ in scales]
    pmat = feats.view(B * N, C) @ torch.cat([w[:C] for w in w1s], dim=1)
    width = sum(sc[3] for sc in scales)
    args, col = [], 0
    for si, (ns, r, O2, O3) in enumerate(scales):
        nbr = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
        ops.c.ball_query_wrapper(B, N, M, r, ns, new_xyz, xyz, nbr, srt)
        args.append({"pmat": pmat, "col0": si * O1, "o1": O1, "xyz": xyz, "new_xyz": new_xyz, "pairs": ops.c.compact_pairs(nbr), "w1x": w1s[si][C:].contiguous(),
                     "b1": dev(rng.standard_normal(O1).astype(np.float32)), "relu1": True,
                     "w2t": dev((rng.standard_normal((O1, O2)) / np.sqrt(O1)).astype(np.float32)), "b2": dev(rng.standard_normal(O2).astype(np.float32)), "relu2": True,
                     "w3t": dev((rng.standard_normal((O2, O3)) / np.sqrt(O2)).astype(np.float32)), "b3": dev(rng.standard_normal(O3).astype(np.float32)),
                     "col_offset": col})
        col += O3
    want = torch.zeros((B * M, width), device="cuda")
    mids_want = []
    for a in args:
        yc = ops.c.pgather_gemm2_compact(a["pmat"], a["col0"], O1, xyz, new_xyz, a["pairs"], a["w1x"], a["b1"], True, a["w2t"], a["b2"], True)
        assert yc is not None and ops.c.gemm_pool_compact(yc, a["pairs"], a["w3t"], a["b3"], want, a["col_offset"])
        mids_want.append(yc)
    totals = [int(a["pairs"][2].item()) for a in args]
    # the two-kernel form, paired
    out2 = torch.zeros_like(want)
    for a in args:
        a["out2d"] = out2
    mids = ops.c.compact_mlp_pair(2, args)
    assert mids is not None and all(torch.equal(m_[:t_], w_[:t_]) for m_, w_, t_ in zip(mids, mids_want, totals))
    took1 = ops.c.compact_mlp_pair(1, args, mids=mids)
    assert took1 == all(sc[3] % 64 == 0 for sc in scales)
    if took1:
        assert torch.equal(out2, want)
    # the fused kernel, paired
    out3 = torch.zeros_like(want)
    for a in args:
        a["out2d"] = out3
    took3 = ops.c.compact_mlp_pair(3, args)
    assert took3 == (O1 in (64, 128) and all(sc[3] % 128 == 0 for sc in scales))
    if took3:
        assert torch.equal(out3, want)
        assert not ops.c.compact_mlp_pair(3, args, max_lds=16 * 1024) and torch.equal(out3, want)
    assert not ops.c.compact_mlp_pair(3, [args[0], dict(args[1], o1=O1 * 2)])            # unequal first-layer widths: the caller keeps the per-scale launches
    # the register-chained kernel of round 6 (ws3d_chain_mlp3: activations in registers, weights resident in LDS, ticketed tiles):
    # the same fmaf chains in the same k order -> the same bits; both scales in one launch, each scale alone, few and many workgroups
    covered = O1 == 64 and all(sc[2] <= 96 and sc[3] == 128 for sc in scales)
    for wgs in (0, 1, 7):
        out4 = torch.zeros_like(want)
        for a in args:
            a["out2d"] = out4
        ops.c.CHAIN_WORKGROUPS = wgs
        try:
            took4 = ops.c.chain_mlp3(args, torch.zeros(ops.c.chain_ticket_ints(), dtype=torch.int32, device="cuda"))
        finally:
            ops.c.CHAIN_WORKGROUPS = 0
        assert took4 == covered
        if took4:
            assert torch.equal(out4, want)
    if covered:
        out5 = torch.zeros_like(want)
        for a in args:
            a["out2d"] = out5
            assert ops.c.chain_mlp3([a], torch.zeros(ops.c.chain_ticket_ints(), dtype=torch.int32, device="cuda"))
        assert torch.equal(out5, want)
        # behind the launch gate's limit a scale does nothing (the dense twin runs instead)
        out6 = torch.zeros_like(want)
        for a in args:
            a["out2d"] = out6
        assert ops.c.chain_mlp3([dict(args[0], limit=0), args[1]], torch.zeros(ops.c.chain_ticket_ints(), dtype=torch.int32, device="cuda"))
        w0 = args[0]["col_offset"]
        assert not out6[:, w0:w0 + 128].any() and torch.equal(out6[:, args[1]["col_offset"]:args[1]["col_offset"] + 128], want[:, args[1]["col_offset"]:args[1]["col_offset"] + 128])


@pytest.mark.parametrize("B,N,M,ns,C,O1,O2,O3,r", [(2, 4096, 1024, 16, 96, 64, 64, 128, 0.5), (2, 4096, 1024, 32, 96, 64, 96, 128, 1.0),
                                                  (1, 1024, 256, 32, 256, 128, 196, 256, 2.0), (2, 4096, 1024, 32, 96, 64, 96, 128, 6.0),
                                                  (2, 256, 64, 32, 512, 256, 384, 512, 4.0), (1, 512, 37, 16, 8, 64, 20, 64, 0.01)])
def test_compact_pairs_path_is_bit_identical_to_the_dense_one(ops, B, N, M, ns, C, O1, O2, O3, r):
    """the SharedMLP over the DISTINCT (centre, sample) pairs (ws3d_compact_pairs_* / ws3d_pgather_gemm2_compact /
    ws3d_gemm_pool_compact) gives exactly the pooled rows of the dense kernels: padded rows repeat row 0 of their centre.  Radii
    from "every list is one point" (0.01) over the network's to "every list is full" (6.0); the pair table itself is checked
    against the lists"""
    rng = np.random.default_rng(18)
    pc = synth.make_batch("lidar", B, 16384, 67)[:, :N, :3].copy()
    xyz = dev(pc)
    feats = dev(rng.standard_normal((B, N, C)).astype(np.float32))
    idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); new_xyz = torch.empty((B, M, 3), device="cuda")
    ops.c.furthest_point_sampling_gather(B, N, M, xyz, None, idx, new_xyz)
    nbr = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, new_xyz, xyz, nbr, ops.c.sort_points_x(xyz))
    rowc, rowsrc, total = ops.c.compact_pairs(nbr, ordered=True)
    T = int(total.item())
    want_pairs = []
    nb = host(nbr).reshape(B * M, ns)
    for c_ in range(B * M):
        row = nb[c_]
        k = 1 + int((row[1:] > row[:-1]).sum())
        assert len(set(row[:k].tolist())) == k and set(row.tolist()) == set(row[:k].tolist())
        want_pairs += [(c_, int(v)) for v in row[:k]]
    assert T == len(want_pairs)
    assert list(zip(host(rowc)[:T].tolist(), host(rowsrc)[:T].tolist())) == want_pairs
    rc1, rs1, t1 = ops.c.compact_pairs(nbr)                          # one launch: same pairs, centres in arrival order
    assert int(t1.item()) == T
    got1 = list(zip(host(rc1)[:T].tolist(), host(rs1)[:T].tolist()))
    assert sorted(got1) == sorted(want_pairs)
    firsts = {}
    for i_, (c_, _) in enumerate(got1):
        firsts.setdefault(c_, []).append(i_)
    assert all(v == list(range(v[0], v[0] + len(v))) for v in firsts.values())       # a centre's rows are contiguous
    rowc, rowsrc, total = rc1, rs1, t1                                # the network uses this form
    w1 = dev((rng.standard_normal((C + 3, O1)) / np.sqrt(C)).astype(np.float32)); b1 = dev(rng.standard_normal(O1).astype(np.float32))
    w2 = dev((rng.standard_normal((O1, O2)) / np.sqrt(O1)).astype(np.float32)); b2 = dev(rng.standard_normal(O2).astype(np.float32))
    w3 = dev((rng.standard_normal((O2, O3)) / np.sqrt(O2)).astype(np.float32)); b3 = dev(rng.standard_normal(O3).astype(np.float32))
    pmat = feats.view(B * N, C) @ w1[:C]
    w1x = w1[C:].contiguous()
    dense = torch.empty((B * M, O3), device="cuda")
    y = ops.c.pgather_gemm2(pmat, 0, O1, xyz, new_xyz, nbr, w1x, b1, True, w2, b2, True) if (M * ns) % 64 == 0 else None
    if y is not None and ops.c.gemm_pool(y, w3, b3, True, ns, dense, 0):
        pass
    else:   # shapes the dense kernels decline: the float64 chain decides (round-off instead of bit-equality)
        dense = None
    out = torch.zeros((B * M, O3 + 64), device="cuda")
    yc = ops.c.pgather_gemm2_compact(pmat, 0, O1, xyz, new_xyz, (rowc, rowsrc, total), w1x, b1, True, w2, b2, True)
    assert yc is not None and ops.c.gemm_pool_compact(yc, (rowc, rowsrc, total), w3, b3, out, 64)
    assert bool((out[:, :64] == 0).all())
    # the same chain in ONE kernel (ws3d_pgather_gemm3_compact: layer 2's tile stays in LDS): bit-identical to the two-kernel form
    # wherever it takes the shape (o1 in {64, 128}, O3 % 128, the tiles within the LDS), gated by the same limit
    out3 = torch.zeros((B * M, O3 + 64), device="cuda")
    took = ops.c.pgather_gemm3_compact(pmat, 0, O1, xyz, new_xyz, (rowc, rowsrc, total), w1x, b1, True, w2, b2, True, w3, b3, out3, 64)
    assert took == (O1 in (64, 128) and O3 % 128 == 0)
    if took:
        assert torch.equal(out3, out)
        assert not ops.c.pgather_gemm3_compact(pmat, 0, O1, xyz, new_xyz, (rowc, rowsrc, total), w1x, b1, True, w2, b2, True, w3, b3, out3, 64, max_lds=16 * 1024)
        for limit, runs in ((T - 1, False), (T, True)):
            o3_ = torch.zeros((B * M, O3), device="cuda")
            assert ops.c.pgather_gemm3_compact(pmat, 0, O1, xyz, new_xyz, (rowc, rowsrc, total), w1x, b1, True, w2, b2, True, w3, b3, o3_, 0, limit=limit)
            assert torch.equal(o3_, out[:, 64:]) if runs else bool((o3_ == 0).all()), "the fused compact kernel ignored its limit"
    if dense is not None:
        assert torch.equal(out[:, 64:], dense)
        # device-side dispatch (launch gates): both forms launched into the same buffers, the pair total decides in the kernels'
        # prologues -- a limit below the total runs the dense form only, a limit at or above it the compact form only
        for limit, runs in ((T - 1, "dense"), (0, "dense"), (T, "compact"), (B * M * ns, "compact")):
            o2_ = torch.zeros((B * M, O3), device="cuda")
            buf = ops.c.pgather_gemm2_compact(pmat, 0, O1, xyz, new_xyz, (rowc, rowsrc, total), w1x, b1, True, w2, b2, True, limit=limit)
            if runs == "compact":
                assert torch.equal(buf[:T], yc[:T])
            assert ops.c.gemm_pool_compact(buf, (rowc, rowsrc, total), w3, b3, o2_, 0, limit=limit)
            assert bool((o2_ == 0).all()) == (runs == "dense"), "the compact last layer ignored its limit"
            yd = ops.c.pgather_gemm2(pmat, 0, O1, xyz, new_xyz, nbr, w1x, b1, True, w2, b2, True, out=buf, gate=(total, limit))
            assert yd is buf and ops.c.gemm_pool(yd, w3, b3, True, ns, o2_, 0, gate=(total, limit))
            assert torch.equal(o2_, dense), (limit, runs)
            assert torch.equal(buf, y) if runs == "dense" else torch.equal(buf[:T], yc[:T]), "a gated-off kernel wrote its output"
    li = nbr.long()
    gx = torch.gather(xyz, 1, li.view(B, M * ns, 1).expand(B, M * ns, 3)).view(B, M, ns, 3) - new_xyz.unsqueeze(2)
    gf = torch.gather(feats, 1, li.view(B, M * ns, 1).expand(B, M * ns, C)).view(B, M, ns, C)
    x = torch.cat((gf, gx), dim=3).view(-1, C + 3).double()
    h = torch.relu(torch.relu(x @ w1.double() + b1.double()) @ w2.double() + b2.double())
    want = torch.relu(h @ w3.double() + b3.double()).view(B * M, ns, O3).amax(dim=1)
    assert (out[:, 64:].double() - want).abs().max().item() <= 2e-5 * max(want.abs().max().item(), 1.0) * np.sqrt(max(C, 96) / 96)


SA1_CHAIN_CASES = [
    pytest.param(16, (16, 16, 32), 0.1, 2, 16384, 4096, 0, id="16-widths0-0.1"), pytest.param(32, (32, 32, 64), 0.5, 2, 16384, 4096, 0, id="32-widths1-0.5"),
    pytest.param(32, (32, 32, 64), 3.0, 2, 16384, 4096, 0, id="32-widths2-3.0"), pytest.param(16, (16, 16, 32), 0.001, 2, 16384, 4096, 0, id="16-widths3-0.001"),
    # the other two (widths, nsample) instantiations of the grouped and the list kernel
    pytest.param(16, (32, 32, 64), 0.3, 2, 16384, 4096, 0, id="16-wide-0.3"), pytest.param(32, (16, 16, 32), 0.3, 2, 16384, 4096, 0, id="32-narrow-0.3"),
    # 32 list rows = ONE tile: the compact total stays below a tile (rows behind the end repeat the last one), both prefetches of the
    # compact kernel run off the end, every wave but one leaves in the prologue
    pytest.param(16, (32, 32, 64), 1.0, 1, 256, 2, 0, id="one-tile-wide"), pytest.param(16, (16, 16, 32), 1.0, 1, 256, 2, 0, id="one-tile-narrow"),
    # eight tiles for ONE four-wave workgroup (ws3d_tune sa1_wgs = 1): each wave walks two tiles, the second prefetched under the first
    pytest.param(32, (32, 32, 64), 4.0, 1, 256, 8, 1, id="eight-tiles-wide"), pytest.param(32, (16, 16, 32), 4.0, 1, 256, 8, 1, id="eight-tiles-narrow")]


@pytest.mark.parametrize("ns,widths,r,B,N,M,wgs", SA1_CHAIN_CASES)
def test_sa1_compact_chain_is_bit_identical_to_the_grouped_one(ops, ns, widths, r, B, N, M, wgs):
    """ws3d_sa_mlp3_pool_compact (first level over the distinct pairs, rows built from xyz / new_xyz / the feature channel) gives
    exactly ws3d_sa_mlp3_pool on the grouped tensor of ws3d_query_and_group_nlc"""
    prev = ops.c.tune("sa1_wgs", wgs)
    try:
        _sa1_chain_forms_agree(ops, ns, widths, r, B, N, M)
    finally:
        ops.c.tune("sa1_wgs", prev)


def _sa1_chain_forms_agree(ops, ns, widths, r, B, N, M):
    rng = np.random.default_rng(19)
    pc = synth.make_batch("lidar", B, N, 68)
    xyz = dev(pc[:, :, :3].copy()); feat = dev(pc[:, :, 3:4].copy())
    idx = torch.empty((B, M), dtype=torch.int32, device="cuda"); new_xyz = torch.empty((B, M, 3), device="cuda")
    ops.c.furthest_point_sampling_gather(B, N, M, xyz, None, idx, new_xyz)
    srt = ops.c.sort_points_x(xyz)
    layers = []
    cin = 4
    for wdt in widths:
        layers.append((dev((rng.standard_normal((cin, wdt)) / np.sqrt(cin)).astype(np.float32)), dev(rng.standard_normal(wdt).astype(np.float32) * 0.1), True))
        cin = wdt
    g = ops.c.query_and_group_nlc(r, ns, xyz, new_xyz, feat, True, srt)
    dense = torch.empty((B * M, widths[2]), device="cuda")
    assert ops.c.sa_mlp3_pool(g.view(-1, 4), ns, layers, dense, 0)
    nbr = torch.zeros((B, M, ns), dtype=torch.int32, device="cuda")
    ops.c.ball_query_wrapper(B, N, M, r, ns, new_xyz, xyz, nbr, srt)
    out = torch.zeros((B * M, widths[2] + 32), device="cuda")
    assert ops.c.sa_mlp3_pool_compact(xyz, new_xyz, feat, ops.c.compact_pairs(nbr), layers, out, 32)
    assert bool((out[:, :32] == 0).all())
    assert torch.equal(out[:, 32:], dense)
    # the dense form without a grouped tensor (rows built from the lists), alone and under the launch gates
    lists = torch.full((B * M, widths[2] + 32), -7.0, device="cuda")
    assert ops.c.sa_mlp3_pool_lists(xyz, new_xyz, feat, nbr, layers, lists, 32)
    assert bool((lists[:, :32] == -7.0).all()) and torch.equal(lists[:, 32:], dense)
    pairs = ops.c.compact_pairs(nbr)
    T = int(pairs[2].item())
    assert B * M <= T <= B * M * ns and (B * M * ns > 32 or T < 32), T      # (the one-tile scene: fewer distinct pairs than a tile)
    for limit, runs in ((T - 1, "dense"), (T, "compact")):
        o2_ = torch.zeros((B * M, widths[2]), device="cuda")
        assert ops.c.sa_mlp3_pool_compact(xyz, new_xyz, feat, pairs, layers, o2_, 0, limit=limit)
        assert bool((o2_ == 0).all()) == (runs == "dense")
        assert ops.c.sa_mlp3_pool_lists(xyz, new_xyz, feat, nbr, layers, o2_, 0, gate=(pairs[2], limit))
        assert torch.equal(o2_, dense), (limit, runs)


def test_compact_and_dense_sharedmlps_give_the_same_network_outputs(ops):
    """the SharedMLPs over the distinct pairs compute what the dense kernels compute: the fill threshold that chooses between them
    (fastpath.COMPACT_MAX_FILL, applied on the device to every batch's pair total) is a speed decision only"""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.RPNConfig(num_points=16384, rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=20)
    model = stage1.Stage1Net(mode="TEST", cfg=cfg)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 7))
    model = model.cuda().eval()
    pts = dev(np.stack([synth.velodyne_scan(16384, seed=400 + j) for j in range(4)]))
    saved = (fastpath.COMPACT_MAX_FILL, fastpath.COMPACT_PAIRS, fastpath.PER_POINT_L1)
    try:
        fastpath.COMPACT_PAIRS, fastpath.PER_POINT_L1 = True, True
        outs = []
        for thr in (0.55, -1.0, 2.0, 0.1):               # the default / always dense / always compact / a threshold inside the fills seen
            fastpath.COMPACT_MAX_FILL = thr
            with torch.no_grad():
                o = model.rpn_forward({"pts_input": pts})
            outs.append((o["rpn_cls"].clone(), o["rpn_reg"].clone()))
        fills = fastpath.list_fill(model.rpn.backbone_net, pts)
        assert len(fills) == 8 and all(0.0 < f["fill"] <= 1.0 for f in fills)
        # every gated scale runs the same arithmetic row by row in either form (bit-identical pooled features, see the kernel-level
        # tests; SA4 has no gated dense form and stays compact): the network outputs do not depend on the threshold at all
        for a in outs[1:]:
            assert torch.equal(a[0], outs[0][0]) and torch.equal(a[1], outs[0][1])
        fastpath.COMPACT_PAIRS = False                      # WS3D_COMPACT_PAIRS=0: all rows, SA4's middle layer on the library GEMM (fp32 round-off)
        with torch.no_grad():
            o = model.rpn_forward({"pts_input": pts})
        for x_, y_ in zip((o["rpn_cls"], o["rpn_reg"]), outs[0]):
            assert float((x_ - y_).abs().max()) <= 2e-5 * max(float(y_.abs().max()), 1.0)
    finally:
        fastpath.COMPACT_MAX_FILL, fastpath.COMPACT_PAIRS, fastpath.PER_POINT_L1 = saved


@pytest.mark.parametrize("B,N,M,r,ns,kind,grid,misalign", H.BQ_ONE_CHANNEL_CASES)
def test_query_and_group_one_feature_channel_with_lists(ops, oracle, B, N, M, r, ns, kind, grid, misalign):
    """the (3 xyz + 1 feature channel) shape of the c2 block / the first SA level through ws3d_query_and_group with the lists written
    beside the grouped rows (round 6: four entries per lane as one 16-byte store, entry -> centre by a shift): list lengths that are
    and are not powers of two / multiples of four, centre counts that do not fill the last tile of 64, every search kernel behind it
    (fine grid, x slabs, brute force) and a list tensor that is only 4-byte aligned -- grouped rows and lists equal the reference
    composition (pointnet2_utils.py:241-264: ball_query -> grouping_operation -> subtract) bit for bit"""
    pc = synth.make_batch(kind, B, N, 57)
    xyz = pc[:, :, :3].copy()
    feats = np.ascontiguousarray(np.transpose(pc[:, :, 3:4], (0, 2, 1)))
    cidx = oracle.furthest_point_sample(xyz, M)
    new_xyz = np.stack([xyz[b][cidx[b]] for b in range(B)])
    ref_idx = oracle.ball_query(r, ns, xyz, new_xyz)
    xyz_t = np.ascontiguousarray(np.transpose(xyz, (0, 2, 1)))
    ref = np.concatenate([oracle.grouping_operation(xyz_t, ref_idx) - np.transpose(new_xyz, (0, 2, 1))[..., None],
                          oracle.grouping_operation(feats, ref_idx)], 1)
    x, c, f = dev(xyz), dev(new_xyz), dev(feats)
    srt = None if grid is None else ops.c.sort_points_x(x, grid=grid)
    flat = torch.full((B * M * ns + 4,), -7, dtype=torch.int32, device="cuda")
    nbr = flat[1:1 + B * M * ns].view(B, M, ns) if misalign else flat[4:].view(B, M, ns)
    out = torch.full((B, 4, M, ns), float("nan"), device="cuda")
    ops.c.query_and_group(B, N, M, 1, r, ns, True, x, c, f, nbr, out, srt)
    np.testing.assert_array_equal(host(nbr), ref_idx)
    np.testing.assert_array_equal(host(out), ref)
    assert int(flat[0].item()) == -7 and (misalign or bool((flat[:4] == -7).all().item()))
    # without the lists (idx_out = NULL): the same rows
    out2 = torch.full((B, 4, M, ns), float("nan"), device="cuda")
    ops.c.query_and_group(B, N, M, 1, r, ns, True, x, c, f, None, out2, srt)
    np.testing.assert_array_equal(host(out2), ref)
    # the list-only entry points take the same quad stores
    got = ops.pn.ball_query(r, ns, x, c)
    np.testing.assert_array_equal(host(got), ref_idx)


@pytest.mark.parametrize("N,M,radii,nss,kind", H.BQ_PAIRS2_NW8_CASES)
def test_ball_query_pairs2_on_eight_waves_per_tile(ops, oracle, N, M, radii, nss, kind):
    """ws3d_tune key 5 (round 6: Stage1Pipeline's throughput geometry): the two-scale search launch on 8 waves x 8 centres per tile instead of
    16 x 4 -- the oracle's lists, and the same SET of compact (centre, source) pairs with the same totals as the default launch"""
    B = 8
    xyz = synth.make_batch(kind, B, N, 77)[:, :, :3].copy()
    cidx = oracle.furthest_point_sample(xyz, M)
    new_xyz = np.stack([xyz[b][cidx[b]] for b in range(B)])
    x, c = dev(xyz), dev(new_xyz)
    grid = ops.c.sort_points_x(x, grid=True)
    res = {}
    for nw in (0, 8):
        prev = ops.c.tune("bq_wide_nw", nw)
        try:
            out = ops.c.ball_query_pairs2(radii, nss, x, c, grid)
        finally:
            ops.c.tune("bq_wide_nw", prev)
        assert out is not None
        res[nw] = []
        for (idx, (rowc, rowsrc, total)) in out:
            t = int(total.item())
            pairs = np.stack([host(rowc[:t]), host(rowsrc[:t])], 1)
            res[nw].append((host(idx), t, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]))
    for k in range(2):
        ref = oracle.ball_query(radii[k], nss[k], xyz, new_xyz)
        np.testing.assert_array_equal(res[8][k][0], ref)
        np.testing.assert_array_equal(res[0][k][0], ref)
        assert res[8][k][1] == res[0][k][1]
        np.testing.assert_array_equal(res[8][k][2], res[0][k][2])
    assert ops.c.tune("bq_wide_nw") == 0
    if N == 2048:
        # the fused emit behind the same search on these eight scenes (16 waves per tile, XCD-aware tile decode)
        ns = nss[0]
        feat = dev(np.random.default_rng(7).standard_normal((B, N, 8)).astype(np.float32))
        gl = ops.c.query_and_group_nlc(radii[0], ns, x, c, feat, True, grid)
        li = torch.from_numpy(res[0][0][0].astype(np.int64)).cuda().view(B, M * ns, 1)
        want = torch.cat((torch.gather(x, 1, li.expand(B, M * ns, 3)).view(B, M, ns, 3) - c.unsqueeze(2),
                          torch.gather(feat, 1, li.expand(B, M * ns, 8)).view(B, M, ns, 8)), dim=3)
        assert torch.equal(gl, want)


def test_ball_query_fill_equals_ball_query_on_a_cleared_tensor(ops):
    """ws3d_ball_query_fill into an UNCLEARED tensor == ws3d_ball_query into zeros, for every search kernel (grid, x slabs, brute
    force) and with centres that have no hit at all (NaN centres, a radius of 0)"""
    pc = synth.make_batch("lidar", 2, 16384, 69)[:, :, :3].copy()
    for n, m, r, ns in ((16384, 4096, 0.5, 32), (4096, 1024, 1.0, 16), (700, 100, 2.0, 8), (4096, 512, 0.0, 16)):
        xyz = dev(pc[:, :n].copy())
        new_xyz = xyz[:, :m].clone()
        new_xyz[0, 3] = float("nan")                       # a centre without any hit
        for srt in (ops.c.sort_points_x(xyz), ops.c.sort_points_x(xyz, grid=False), None):
            want = torch.zeros((2, m, ns), dtype=torch.int32, device="cuda")
            ops.c.ball_query_wrapper(2, n, m, r, ns, new_xyz, xyz, want, srt)
            got = ops.c.ball_query_lists(r, ns, xyz, new_xyz, srt)
            got2 = torch.full((2, m, ns), 123456, dtype=torch.int32, device="cuda")
            from ws3d_amd import _lib
            _lib.check(_lib.load().ws3d_ball_query_fill(2, n, m, float(r), ns, new_xyz.data_ptr(), xyz.data_ptr(), got2.data_ptr(),
                                                        srt.data_ptr() if srt is not None else None, torch.cuda.current_stream().cuda_stream))
            assert torch.equal(got, want) and torch.equal(got2, want)


@pytest.mark.gpu
def test_proposal_stage_writes_the_send_rows_of_the_exchange(ops):
    """stage1.proposals_from_rpn(with_packed=<send buffer of dist.ProposalExchange>): ws3d_select_proposals_send (ABI 6) writes the packed
    rows and, behind each scene's rows, its count straight into the buffer the step's one all-gather sends -- the same rows as
    ws3d_select_proposals_packed, the same boxes / scores / counts; the fifth result is a view of the buffer; nothing else packs"""
    from ws3d_amd import dist as wd
    from ws3d_amd import stage1
    cfg = stage1.DEFAULT_CFG
    g = torch.Generator().manual_seed(5)
    B, N, K = 3, 16384, cfg.rpn_post_nms_top_n
    bins = int(cfg.loc_scope / cfg.loc_bin_size) * 2
    pc = synth.make_batch("hdl64", B, N, 31)
    out = {"backbone_xyz": dev(pc[:, :, :3].copy()), "rpn_reg": (torch.randn(B, N, bins * 4, generator=g) * 0.5).cuda(), "rpn_cls": torch.randn(B, N, 1, generator=g).cuda()}
    boxes, scores, count, enl, packed = stage1.proposals_from_rpn(out, cfg, with_pool_boxes=True, with_packed=True)
    ex = wd.ProposalExchange(B, K, B + 2, "cuda", world=1, rank=0)          # (a send buffer with more rows than this rank's scenes)
    ex.send.fill_(7.0)
    b2, s2, c2, e2, view = stage1.proposals_from_rpn(out, cfg, with_pool_boxes=True, with_packed=ex.send)
    torch.cuda.synchronize()
    assert torch.equal(b2, boxes) and torch.equal(s2, scores) and torch.equal(c2, count) and torch.equal(e2, enl)
    assert view.data_ptr() == ex.send.data_ptr() and torch.equal(view, packed) and int(count.max()) > 0
    assert torch.equal(ex.send[:B, K * 8], count.to(torch.float32)) and torch.equal(ex.send[:B, :K * 8].reshape(B, K, 8), packed)
    assert bool((ex.send[B:] == 7.0).all())                                 # rows behind this rank's scenes are not touched
    got, cnt = ex.gather()                                                  # world 1: the send rows themselves, no collective
    assert torch.equal(got, packed) and torch.equal(cnt, count.to(torch.float32)) and ex.collectives == 0
    with pytest.raises(ValueError, match="send buffer"):
        stage1.proposals_from_rpn(out, cfg, with_packed=torch.zeros((B, K * 8), device="cuda"))


@pytest.mark.parametrize("B,C,N,M,ns", [(2, 96, 4096, 1024, 16), (3, 99, 4096, 1024, 32), (2, 7, 1024, 600, 12), (1, 4, 512, 300, 4), (2, 96, 8192, 1024, 32), (1, 5, 100, 64, 16)])
def test_group_points_with_the_rows_staged_in_lds(ops, B, C, N, M, ns):
    """group_points_wrapper (group_points_gpu.cu:47-66): the round-6 kernel that stages a channel group's source rows in LDS (n <= 4096,
    plane >= 2 n, c >= 4) and the gather kernel it replaces there (other shapes) are exact copies: compared with torch's own indexing"""
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + C)
    pts = torch.randn((B, C, N), device="cuda", generator=g)
    idx = torch.randint(0, N, (B, M, ns), device="cuda", generator=g, dtype=torch.int32)
    out = torch.full((B, C, M, ns), float("nan"), device="cuda")
    ops.c.group_points_wrapper(B, C, N, M, ns, pts, idx, out)
    want = torch.gather(pts, 2, idx.long().view(B, 1, M * ns).expand(B, C, M * ns)).view(B, C, M, ns)
    assert torch.equal(out, want)


def test_the_zero_arena_serves_every_take_of_the_forward_pass(ops):
    """one cleared buffer per forward pass (fastpath._ZeroArena) holds every pooled output, pair total and ticket block of the default
    network: a take it cannot serve falls back to a fill launch of its own (round 6 found one: the tickets of ws3d_chain_mlp3 were taken
    for levels the kernel does not cover) -- asserted zero for the eager dispatch and for what a primed pipeline captures"""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.seeded import seeded_state_dict
    model = stage1.Stage1Net(mode='TEST').eval()
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 7))
    model.cuda()
    pts = dev(synth.make_batch("hdl64", 8, 16384, 3))
    with torch.no_grad():
        model.rpn_forward({"pts_input": pts})
        assert fastpath.LAST_ARENA_FALLBACKS == 0, fastpath.LAST_ARENA_FALLBACKS
        keys = fastpath.primed_compact_scales(model.rpn.backbone_net, pts)
        with fastpath.geometry_ahead(False), fastpath.compact_only_scales(keys):
            model.rpn_forward({"pts_input": pts})
        assert fastpath.LAST_ARENA_FALLBACKS == 0, fastpath.LAST_ARENA_FALLBACKS
