"""NumPy restatements of the few host lines of the reference's click-driven annotation (tools/eval_active.py:198-272), shared by
test_annotate.py and test_gpu_annotate.py.  Nothing here imports the product's kernels."""
import numpy as np

SIDE = 5
OFFSETS = [np.float32(0.1 * i) for i in (-2, -1, 0, 1, 2)]       # what torch adds to an fp32 tensor in `sample[:, 0] += 0.1 * i`


def candidates_np(clicks, centre_y=1.65):
    """clicks (n,3) fp32 -> (25 n, 3): eval_active.py:202-209, i outer, j inner, whole click lists concatenated; y set to centre_y"""
    xz = np.asarray(clicks, dtype=np.float32)[:, [0, 2]]
    out = []
    for i in range(SIDE):
        for j in range(SIDE):
            sample = xz.copy()
            sample[:, 0] += OFFSETS[i]
            sample[:, 1] += OFFSETS[j]
            out.append(sample)
    out = np.concatenate(out, axis=0) if out else np.zeros((0, 2), np.float32)
    return np.stack([out[:, 0], np.full(out.shape[0], centre_y, np.float32), out[:, 1]], axis=1).astype(np.float32)


def padded_candidates_np(clicks, num, centre_y=1.65):
    """clicks (B,K,3), num (B) -> cand (B,25K,3) zero padded, cand_num (B) int32"""
    B, K = clicks.shape[0], clicks.shape[1]
    cand = np.zeros((B, SIDE * SIDE * K, 3), dtype=np.float32)
    for b in range(B):
        c = candidates_np(clicks[b, :num[b]], centre_y)
        cand[b, :c.shape[0]] = c
    return cand, (SIDE * SIDE * np.asarray(num)).astype(np.int32)


def cloud_np(pts, score64, centre, S, radius=4.0):
    """one candidate's Stage-2 input (eval_active.py:248-267 + the first-S-cyclic rule of kitti_boxplace_dataset.py:327-337):
    pts (N,4) fp32, score64 (N,) float64, centre (3,) fp32 (x, ground y, z) -> rows (S,5) fp32, the member count, the (S,) scene indices of the rows
    (empty for an empty cylinder)"""
    pts = np.asarray(pts, dtype=np.float32)
    dx, dz = centre[0] - pts[:, 0], centre[2] - pts[:, 2]
    member = np.sqrt(dx * dx + dz * dz) < np.float32(radius)
    idx = np.nonzero(member)[0]
    rows = np.zeros((S, 5), dtype=np.float32)
    sel = idx[:0]
    if idx.size:
        sel = idx[:S][np.arange(S) % min(idx.size, S)]
        rows[:, 0] = pts[sel, 0] - centre[0]
        rows[:, 1] = pts[sel, 1] - centre[1]
        rows[:, 2] = pts[sel, 2] - centre[2]
        rows[:, 3] = pts[sel, 3]
        rows[:, 4] = (score64[sel] > 0.5).astype(np.float32) - np.float32(0.5)
    return rows, int(idx.size), sel
