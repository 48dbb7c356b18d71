"""Furthest point sampling on the host, in numpy: the CPU route of ``pn2_ops.furthest_point_sample_ragged``.

It is what the loader processes use (they are forked and never touch the device) and what builds the ground-truth database on
a machine without a device.  Same indices as the HIP kernels, bit for bit:
  * the squared distance follows the library's convention (``_lib.DIST_MODE``, csrc/common.h ``sqdist3``) in float32, the fused
    multiply-adds evaluated exactly (product in float64, sum rounded to odd, one final rounding to float32);
  * every step takes the arg-max of the running minimum; among exact ties the winner is the point whose owner thread
    ``k mod bs`` of the reference launch (``bs = opt_n_threads(n)``: the largest power of two <= n, at most 1024) has the
    smallest bit-reversed id, then the smallest k (sampling_gpu.cu:93-253, csrc/fps.hip header).
"""
from __future__ import annotations

import numpy as np


def _fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, correctly rounded: a*b is exact in float64; the float64 sum is forced to an odd
    last bit whenever it was inexact (TwoSum gives the exact error), so the rounding to float32 sees the true value's side"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    v = s - p
    err = (p - (s - v)) + (c - v)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)                     # the true value lies beyond s in magnitude
    bits = np.where(fix, bits + np.where(away, 1, -1), bits)
    return bits.view(np.float64).astype(np.float32)


def sqdist(points: np.ndarray, q: np.ndarray, dist_mode: int = 0) -> np.ndarray:
    """squared distance of float32 points (n,3) to q (3,) under csrc/common.h's WS3D_DIST_MODE"""
    dx, dy, dz = points[:, 0] - q[0], points[:, 1] - q[1], points[:, 2] - q[2]
    if dist_mode == 0:
        return _fma32(dz, dz, _fma32(dx, dx, dy * dy))
    if dist_mode == 1:
        return (dx * dx + dy * dy) + dz * dz
    return _fma32(dz, dz, _fma32(dy, dy, dx * dx))


def block_size(n: int) -> int:
    """opt_n_threads of the reference launcher (cuda_utils.h:10-14)"""
    bs = 1
    while bs * 2 <= n and bs < 1024:
        bs *= 2
    return bs


def tie_rank(n: int) -> np.ndarray:
    """smaller rank wins an exact tie: bit-reversed owner thread first, then the point index"""
    bs = block_size(n)
    bits = bs.bit_length() - 1
    k = np.arange(n, dtype=np.int64)
    t, rev = k % bs, np.zeros(n, dtype=np.int64)
    for i in range(bits):
        rev |= ((t >> i) & 1) << (bits - 1 - i)
    return rev * (n // bs + 1) + k // bs


def furthest_point_sample(xyz: np.ndarray, m: int, dist_mode: int = 0) -> np.ndarray:
    """xyz (n,3) -> (m,) int32 indices, idx[0] = 0"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    if n < 1 or m > n or m < 0:
        raise ValueError(f"furthest_point_sample: cannot take {m} of {n} points")
    rank = tie_rank(n)
    running = np.full(n, 1e10, dtype=np.float32)
    idx = np.zeros(m, dtype=np.int32)
    last = 0
    for j in range(1, m):
        running = np.minimum(sqdist(xyz, xyz[last], dist_mode), running)
        cand = np.flatnonzero(running == running.max())
        last = int(cand[0]) if cand.size == 1 else int(cand[np.argmin(rank[cand])])
        idx[j] = last
    return idx


def furthest_point_sample_ragged(xyz: np.ndarray, offsets: np.ndarray, m: int, dist_mode: int = 0) -> np.ndarray:
    """xyz (T,3) packed, offsets (C+1,) -> (C, m) int32, indices local to each cloud"""
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    out = np.zeros((max(offsets.size - 1, 0), m), dtype=np.int32)
    for c in range(out.shape[0]):
        out[c] = furthest_point_sample(xyz[offsets[c]:offsets[c + 1]], m, dist_mode)
    return out
