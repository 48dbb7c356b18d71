#!/usr/bin/env python
"""Golden record for tests/test_oracle_vs_ref.py: the reference's own CPU roipool3d (lib/utils/roipool3d/src/roipool3d.cpp:82-195,
compiled into oracle/_ref/ by oracle/build_ref.py where the reference tree is mounted) run on the test's inputs:
``python -B tests/golden/make_golden_roipool3d_ref.py``.

Fixture = data only (roipool3d_ref.npz): per case a digest of the inputs, the in-box flags bit-packed along the points axis, the
empty flags, and SHA-256 digests of the pooled points / features (26 MB of features for the largest case: the digest pins them bit
for bit at 64 bytes)."""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import build_ref  # noqa: E402
from tests.test_oracle_vs_ref import POOL_CASES, PIB_CASES, _boundary_inputs, _key, _scene, digest  # noqa: E402


def flags(ref, pts, boxes):
    f = torch.zeros((len(boxes), len(pts)), dtype=torch.int64)
    ref.pts_in_boxes3d_cpu(f, torch.from_numpy(pts), torch.from_numpy(boxes))
    return np.packbits(f.numpy().astype(bool), axis=1)


def main():
    ref = build_ref.load()
    if ref is None:
        raise SystemExit("oracle/_ref/roipool3d_ref.so is not built (oracle/build_ref.py needs the reference tree)")
    rec = {}
    for n, m, seed in PIB_CASES:
        pts, boxes, _ = _scene(n, m, 4, seed)
        k = _key("pib", n, m, seed)
        rec[k + "_inputs"] = np.array(digest(pts, boxes))
        rec[k + "_flag"] = flags(ref, pts, boxes)
    for n, m, c, s, seed in POOL_CASES:
        pts, boxes, feat = _scene(n, m, c, seed)
        k = _key("pool", n, m, c, s, seed)
        pp, pf, pe = torch.zeros((m, s, 3)), torch.zeros((m, s, c)), torch.zeros((m,), dtype=torch.int64)
        ref.roipool3d_cpu(torch.from_numpy(pts), torch.from_numpy(boxes), torch.from_numpy(feat), pp, pf, pe)
        rec[k + "_inputs"] = np.array(digest(pts, boxes, feat))
        rec[k + "_empty"] = pe.numpy().astype(np.int8)
        rec[k + "_pooled_pts"] = np.array(digest(pp.numpy()))
        rec[k + "_pooled_feat"] = np.array(digest(pf.numpy()))
    (pts, box), (p2, big) = _boundary_inputs()
    rec["boundary_flag"] = flags(ref, pts, box)
    rec["prefilter_flag"] = flags(ref, p2, big)
    out = os.path.join(HERE, "roipool3d_ref.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
