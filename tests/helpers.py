"""Independent numpy re-derivations used to cross-check the C oracle (and, on the
GPU box, the HIP kernels).  Nothing here shares code with oracle/ws3d_oracle.c."""
from __future__ import annotations

import numpy as np


# ----------------------------------------------------------------------------- exact fmaf
def fmaf_np(a, b, c):
    """Correctly rounded float32 fma(a,b,c), vectorised.

    a*b is exact in float64 (24+24 <= 53 bits).  The float64 sum s = fl(p + c) is
    corrected to ROUND-TO-ODD with the exact TwoSum error term, after which the
    final float64 -> float32 rounding cannot double-round (53 >= 24 + 2)."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # exact: p + c = s + err
    s_arr = np.atleast_1d(s)
    e_arr = np.atleast_1d(err)
    si = s_arr.view(np.int64).copy()
    inexact = e_arr != 0
    even = (si & 1) == 0
    # the exact value lies strictly between s and its neighbour in the direction of err;
    # of those two doubles exactly one has an odd mantissa: pick it.
    toward_inf = (e_arr > 0) == (s_arr > 0)  # neighbour has larger magnitude
    adj = np.where(toward_inf, 1, -1)
    si = np.where(inexact & even, si + adj, si)
    out = si.view(np.float64).astype(np.float32)
    return out.reshape(np.shape(s))


def sqdist_np(p, q):
    """d = fmaf(dz,dz, fmaf(dx,dx, dy*dy)) with d* = p* - q* in float32."""
    p = np.asarray(p, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    dx = p[..., 0] - q[..., 0]
    dy = p[..., 1] - q[..., 1]
    dz = p[..., 2] - q[..., 2]
    return fmaf_np(dz, dz, fmaf_np(dx, dx, dy * dy))


# ----------------------------------------------------------------------------- FPS
def bitrev(v: np.ndarray, bits: int) -> np.ndarray:
    v = np.asarray(v, dtype=np.int64)
    r = np.zeros_like(v)
    for i in range(bits):
        r |= ((v >> i) & 1) << (bits - 1 - i)
    return r


def opt_n_threads(n: int) -> int:
    p = 1
    while p * 2 <= n:
        p *= 2
    return max(min(p, 1024), 1)


def fps_np(xyz: np.ndarray, m: int) -> np.ndarray:
    """Rank formulation of the reference FPS: every step takes the
    argmax of the running min-distance; exact ties go to the candidate whose owner thread
    (k mod bs) has the smallest bit-reversed id, then to the smallest k."""
    xyz = np.asarray(xyz, dtype=np.float32)
    n = xyz.shape[0]
    bs = opt_n_threads(n)
    bits = bs.bit_length() - 1
    k = np.arange(n)
    rank = bitrev(k % bs, bits) * (n // bs + 1) + k // bs  # smaller rank wins ties
    temp = np.full(n, 1e10, dtype=np.float32)
    idx = np.zeros(m, dtype=np.int32)
    old = 0
    for j in range(1, m):
        d = sqdist_np(xyz, xyz[old][None, :])
        temp = np.minimum(d, temp)
        mx = temp.max()
        cand = np.nonzero(temp == mx)[0]
        old = int(cand[np.argmin(rank[cand])])
        idx[j] = old
    return idx


# ----------------------------------------------------------------------------- ball query / knn
def ball_query_np(radius: float, nsample: int, xyz: np.ndarray, new_xyz: np.ndarray) -> np.ndarray:
    xyz = np.asarray(xyz, dtype=np.float32)
    new_xyz = np.asarray(new_xyz, dtype=np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    out = np.zeros((new_xyz.shape[0], nsample), dtype=np.int32)
    for i, c in enumerate(new_xyz):
        d2 = sqdist_np(c[None, :], xyz)
        hit = np.nonzero(d2 < r2)[0][:nsample]
        if hit.size:
            out[i, :] = hit[0]
            out[i, :hit.size] = hit
    return out


def three_nn_np(unknown: np.ndarray, known: np.ndarray):
    unknown = np.asarray(unknown, dtype=np.float32)
    known = np.asarray(known, dtype=np.float32)
    n, m = unknown.shape[0], known.shape[0]
    d2 = np.full((n, 3), np.inf, dtype=np.float32)
    idx = np.zeros((n, 3), dtype=np.int32)
    for i, u in enumerate(unknown):
        d = sqdist_np(u[None, :], known)
        order = np.argsort(d, kind="stable")[:3]
        d2[i, :order.size] = d[order]
        idx[i, :order.size] = order
    return d2, idx


# ----------------------------------------------------------------------------- rotated boxes
def bev_corners(box):
    """[x1,y1,x2,y2,ry] -> 4 corners rotated like iou3d_kernel.cu:98-102 (float64)."""
    x1, y1, x2, y2, a = [float(v) for v in box]
    cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
    c, s = np.cos(a), np.sin(a)
    pts = []
    for (px, py) in ((x1, y1), (x2, y1), (x2, y2), (x1, y2)):
        dx, dy = px - cx, py - cy
        pts.append((dx * c + dy * s + cx, -dx * s + dy * c + cy))
    return pts


def _clip(subject, a, b):
    def inside(p):
        return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) >= 0

    def inter(p, q):
        x1, y1, x2, y2 = p[0], p[1], q[0], q[1]
        x3, y3, x4, y4 = a[0], a[1], b[0], b[1]
        den = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
        t = ((x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4)) / den
        return (x1 + t * (x2 - x1), y1 + t * (y2 - y1))

    out = []
    for i in range(len(subject)):
        cur, prev = subject[i], subject[i - 1]
        if inside(cur):
            if not inside(prev):
                out.append(inter(prev, cur))
            out.append(cur)
        elif inside(prev):
            out.append(inter(prev, cur))
    return out


def poly_area(p):
    a = 0.0
    for i in range(len(p)):
        a += p[i - 1][0] * p[i][1] - p[i][0] * p[i - 1][1]
    return abs(a) / 2


def overlap_sh(box_a, box_b) -> float:
    """Sutherland-Hodgman rotated-rectangle intersection area in float64 (independent of
    the reference's vertex-collect + atan2-sort + fan algorithm)."""
    pa, pb = bev_corners(box_a), bev_corners(box_b)

    def ccw(p):
        s = 0.0
        for i in range(len(p)):
            s += p[i - 1][0] * p[i][1] - p[i][0] * p[i - 1][1]
        return p if s > 0 else p[::-1]

    pa, pb = ccw(pa), ccw(pb)
    out = pa
    for i in range(4):
        if not out:
            return 0.0
        out = _clip(out, pb[i - 1], pb[i])
    return poly_area(out) if len(out) >= 3 else 0.0


def greedy_nms_from_iou(iou: np.ndarray, thresh: float) -> np.ndarray:
    n = iou.shape[0]
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= iou[i, i + 1:] > thresh
    return np.asarray(keep, dtype=np.int64)


# ----------------------------------------------------------------------------- roipool3d launch variants
# The environment knobs of csrc/roipool3d.hip (read once per process) under which tests/test_gpu_parity.py runs every pooling kernel on
# the GPU and tests/test_roipool_plan.py asks the launcher's plan on the CPU.  compat hands a workspace to every scene of >= 16384
# points, and a launch with a workspace takes the binned kernel before it looks at WS3D_ROI_PIPE: only the variants with
# WS3D_ROI_BINNED=0 reach roipool3d_pipe_kernel there.
def _roi_env(**kw):
    return {"WS3D_ROI_" + k: str(v) for k, v in kw.items()}


ROI_ENV_VARIANTS = [
    _roi_env(BG=4, PIPE=0, STAGE=0),      # round-1 copy: aligned loads, row-shifted stores
    _roi_env(BG=4, PIPE=0, STAGE=16), _roi_env(BG=4, PIPE=0, STAGE=32),
    _roi_env(BG=4, PIPE=2), _roi_env(BG=4, PIPE=2, STAGE=32),
    _roi_env(BG=4, PIPE=1), _roi_env(BG=4, PIPE=1, STAGE=32),
    _roi_env(BG=1, STAGE=16), _roi_env(BG=2),
    # without the binned kernel: the four roipool3d_pipe_kernel instantiations, and roipool3d_kernel<4, 32> / <2, 16> on large scenes
    _roi_env(BINNED=0, BG=4, PIPE=2), _roi_env(BINNED=0, BG=4, PIPE=2, STAGE=32),
    _roi_env(BINNED=0, BG=4, PIPE=1), _roi_env(BINNED=0, BG=4, PIPE=1, STAGE=32),
    _roi_env(BINNED=0, BG=4, PIPE=0, STAGE=32),
    _roi_env(BG=2, STAGE=16),
]
ROI_PIPE_VARIANTS = [v for v in ROI_ENV_VARIANTS if v.get("WS3D_ROI_BINNED") == "0" and v["WS3D_ROI_PIPE"] != "0"]


def roi_env_id(env):
    return ",".join(f"{k[9:]}={v}" for k, v in env.items())


# (B, N, M, C, S) and the synth seed of each case.  The last two are the smallest shapes at which the shared phases of the kernels can
# still go wrong: N at and just past the 16384-point switch (16400 is no multiple of 256), M % 4 == 3 (a last workgroup of three boxes:
# with two boxes per pass the second pass scans one box and one dummy), C = 4 (one lane per row carries features), S = 8 below one
# stretch of 16 rows, S = 20 one full stretch and a ragged one of 4 rows.
ROI_VARIANT_CASES = [(2, 20000, 37, 128, 512), (1, 40000, 9, 128, 64), (2, 3000, 24, 128, 512), (2, 20000, 18, 8, 36), (1, 17000, 6, 5, 33),
                     (1, 16384, 7, 4, 8), (1, 16400, 11, 4, 20)]
ROI_VARIANT_SEEDS = [30, 31, 32, 33, 34, 60, 61]
# (B, n, m, c, s, cfg) of test_roipool3d_bit_exact (default environment)
ROI_BIT_EXACT_CASES = [(2, 2048, 24, 8, 64, 1), (2, 16384, 100, 128, 512, 3), (1, 4096, 40, 16, 512, 2), (1, 512, 8, 3, 16, 4),
                       (1, 65536, 64, 128, 512, 5), (1, 1000, 5, 1, 700, 6)]


# ----------------------------------------------------------------------------- ball-query launch coverage
# The shapes of the ball-query tests of tests/test_gpu_parity.py, kept here so that tests/test_ballquery_plan.py can ask the launcher's
# plan (ws3d_ball_query_plan) on the CPU which search kernel each of their calls takes.
# (B, N, M, r, ns, kind) of test_ball_query_and_group_bit_exact
BQ_CASES = [
    (2, 2048, 256, 0.5, 16, "lidar"), (2, 4096, 300, 1.0, 32, "lidar"), (1, 1024, 128, 0.1, 64, "lidar"),
    (3, 500, 77, 4.0, 8, "uniform"), (2, 16384, 4096, 0.1, 64, "lidar"), (1, 16384, 4096, 0.5, 32, "lidar"),
    (1, 16384, 4096, 0.1, 16, "uniform"), (1, 4096, 1024, 2.0, 32, "lidar"), (1, 777, 5, 100.0, 64, "lidar"),
    (1, 300, 129, 1.0, 3, "uniform"),
]
# (N, M, r, ns, kind), two scenes each: test_ball_query_sorted_slab_equals_bruteforce, test_ball_query_grid_one_wave_per_centre_dense_lists
BQ_SLAB_CASES = [(16384, 4096, 0.1, 64, "lidar"), (16384, 1024, 0.5, 32, "uniform"), (4096, 1024, 1.0, 16, "lidar"), (2048, 300, 50.0, 8, "lidar"),
                 (8192, 500, 0.3, 5, "dups")]
BQ_DENSE_CASES = [(16384, 4096, 0.5, 32, "hdl64"), (16384, 4096, 0.1, 16, "hdl64"), (16384, 4096, 0.1, 64, "hdl64"),
                  (4096, 1024, 1.0, 32, "hdl64"), (4096, 1024, 0.5, 16, "hdl64"), (16384, 512, 2.5, 64, "hdl64"),
                  (16384, 777, 0.4, 32, "clump"), (16384, 300, 60.0, 32, "hdl64"), (8192, 500, 0.3, 5, "dups"),
                  (16384, 2048, 0.5, 1, "hdl64"), (16384, 1000, 0.5, 33, "narrow")]
# (B, N, M, r, ns, kind, grid, misalign) of test_query_and_group_one_feature_channel_with_lists
BQ_ONE_CHANNEL_CASES = [
    (2, 16384, 4096, 0.1, 64, "hdl64", True, False), (1, 16384, 4096, 0.5, 32, "hdl64", True, False), (2, 4096, 1000, 0.5, 16, "lidar", True, False),
    (1, 2048, 333, 1.0, 12, "lidar", True, False), (1, 2048, 333, 1.0, 12, "lidar", False, False), (2, 3000, 257, 0.8, 20, "uniform", True, True),
    (1, 900, 70, 2.0, 8, "lidar", None, False), (1, 4096, 1024, 0.5, 6, "lidar", True, False)]
# (N, M, radii, nss, kind), eight scenes each: test_ball_query_pairs2_on_eight_waves_per_tile
BQ_PAIRS2_NW8_CASES = [(16384, 4096, (0.1, 0.5), (16, 32), "hdl64"), (4096, 1024, (0.5, 1.0), (16, 32), "hdl64"),
                       (4096, 1000, (1.0, 2.0), (16, 32), "lidar"), (2048, 64, (2.0, 4.0), (8, 64), "lidar")]
# (B, N, M, r, ns) of test_ball_query_fine_grid_one_lane_per_centre: lists longer than the 64 entries the one-wave-per-centre kernel
# takes, on a fine-grid buffer -> ball_query_grid_kernel.  M = 70: a ragged second tile; B = 8 / 3: the XCD-aware and the plain tile
# decode; r = 60 on 4096 points: every point a candidate, more than the grid walk accepts (BQS_MAX_SLAB = 3072) -> the ordered scan.
BQ_LANE_CASES = [(3, 2048, 70, 0.5, 72), (3, 2048, 70, 0.5, 128), (8, 2048, 70, 0.5, 72), (8, 2048, 70, 0.5, 128), (1, 4096, 70, 60.0, 72)]
BQ_FLAVOUR_NS = (32, 72)            # test_ball_query_binned_buffer_of_another_flavour_on_a_noted_address (1 scene, 16384 -> 300)
# (B, N, M, r, ns, C) of test_ball_query_lists_of_32_bit_indices: more than 65536 points, no binned copy -> ball_query_kernel<int32_t, *>
BQ_WIDE_INDEX_CASE = (1, 65600, 70, 1.0, 8, 4)
# (B, N, M, r, ns) of test_ball_query_on_more_tiles_than_the_wide_launch_takes: 2048 tiles of 64 centres and more -> four waves per tile
# (ball_query_grid_coop_kernel<*, 4>), with the XCD-aware (B % 8 == 0) and the plain tile decode
BQ_MANY_SCENES_CASES = [(2048, 128, 64, 4.0, 16), (2049, 128, 64, 4.0, 16)]


def bq_plan_calls():
    """[(b, n, m, c, nsample, fused, nlc, flavour, pairs, scales, wide_nw)]: the arguments of ws3d_ball_query_plan for the searches the
    tests above launch (flavour 1: a fine-grid buffer, 0: x slabs, -1: no binned copy)"""
    calls = []

    def lists(b, n, m, ns, flavour, pairs=0, scales=1, nw=0):
        calls.append((b, n, m, 0, ns, 0, 0, flavour, pairs, scales, nw))

    def fused(b, n, m, c, ns, flavour, nlc=0):
        calls.append((b, n, m, c, ns, 1, nlc, flavour, 0, 1, 0))

    def auto(n):                                       # pn2_ops bins the scene itself where compat.sort_points_x takes it
        return 1 if 2048 <= n <= 16384 else -1

    for B, N, M, r, ns, kind in BQ_CASES:
        lists(B, N, M, ns, auto(N))
        for c in (5, 0):
            fused(B, N, M, c, ns, auto(N))
    for N, M, r, ns, kind in BQ_SLAB_CASES:
        for flavour in (1, 0, -1):
            lists(2, N, M, ns, flavour)
    for N, M, r, ns, kind in BQ_DENSE_CASES:
        lists(2, N, M, ns, 1)
        lists(2, N, M, ns, 1, pairs=1)
        lists(2, N, M, max(ns, 16 if ns != 16 else 32), 1, pairs=1, scales=2)
        lists(2, N, M, ns, -1)
        fused(2, N, M, 8, ns, 1, nlc=1)
    for ns in BQ_FLAVOUR_NS:
        lists(1, 16384, 300, ns, 1)
    for B, N, M, r, ns, kind, grid, misalign in BQ_ONE_CHANNEL_CASES:
        fused(B, N, M, 1, ns, {True: 1, False: 0, None: -1}[grid])
        lists(B, N, M, ns, auto(N))
    for N, M, radii, nss, kind in BQ_PAIRS2_NW8_CASES:
        for nw in (0, 8):
            lists(8, N, M, max(nss), 1, pairs=1, scales=2, nw=nw)
        if N == 2048:
            fused(8, N, M, 8, nss[0], 1, nlc=1)
    for B, N, M, r, ns in BQ_LANE_CASES:
        lists(B, N, M, ns, 1)
        fused(B, N, M, 1, ns, 1)
        fused(B, N, M, 8, ns, 1, nlc=1)
        if B == 3:
            lists(B, N, M, 32, 1, pairs=1, scales=2, nw=8)
    B, N, M, r, ns, C = BQ_WIDE_INDEX_CASE
    lists(B, N, M, ns, -1)
    fused(B, N, M, C, ns, -1)
    for B, N, M, r, ns in BQ_MANY_SCENES_CASES:
        lists(B, N, M, ns, 1)
        lists(B, N, M, 32, 1, pairs=1, scales=2)
        fused(B, N, M, 1, ns, 1)
    return calls
