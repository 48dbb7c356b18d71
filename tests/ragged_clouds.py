"""The clouds and oracle picks shared by tests/test_fps_ragged.py (numpy route) and tests/test_gpu_fps_ragged.py (HIP kernel).

Sizes on both sides of every power of two up to the 1024 cap of the reference's block size, and on both sides of the ragged
kernel's on-chip limit; per size a car-shaped cloud and a copy in which 30 % of the points duplicate other points (exact ties, so
the size-dependent tie rule decides), plus one cloud of identical points (every step is a tie of all points)."""
import functools

import numpy as np

MS = (1, 2, 100)


def sizes(limit):
    return [100, 101, 127, 128, 129, 255, 256, 513, 1023, 1024, 1025, 1500, 2049, limit, limit + 1]


@functools.lru_cache(maxsize=None)
def clouds(limit):
    """list of (n_i, 3) float32 arrays"""
    from ws3d_amd import synth
    rng = np.random.default_rng(2049)
    out = []
    for j, n in enumerate(sizes(limit)):
        car = synth.roi_clouds(1, n, 40 + j)[0]
        dup = car.copy()
        dst = rng.choice(n, int(0.3 * n), replace=False)
        dup[dst] = car[rng.integers(0, n, dst.size)]
        out += [car, dup]
    out.append(np.tile(np.array([[1.5, -0.25, 0.75]], dtype=np.float32), (300, 1)))
    for c in out:
        c.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(limit, m):
    """(C, m) int32: the C oracle on every cloud alone"""
    import oracle
    return np.stack([oracle.furthest_point_sample(c[None], m)[0] for c in clouds(limit)])


def packed(cs):
    """-> xyz (T,3) float32, offsets (C+1,) int32"""
    offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in cs])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(cs, 0), dtype=np.float32), offsets
