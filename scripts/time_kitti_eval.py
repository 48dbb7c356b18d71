#!/usr/bin/env python
"""Wall time of ws3d_amd.kitti_eval.get_official_eval_result on a KITTI-val-sized synthetic set built in memory:
3,769 frames, 100 Car detections and ~8 labels per frame (Stage-1's output size).  Device times of the overlap and
counting launches: run it under ``rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/time_kitti_eval.py``.

    python scripts/time_kitti_eval.py [--frames 3769] [--dets 100] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def synthetic_annos(frames, dets, seed=0):
    rng = np.random.default_rng(seed)
    gt, dt = [], []
    for _ in range(frames):
        n = int(rng.integers(4, 13))
        names = rng.choice(["Car", "Car", "Car", "Van", "Pedestrian", "Cyclist", "DontCare"], n)
        loc = np.stack([rng.uniform(-20, 20, n), rng.uniform(1, 2, n), rng.uniform(5, 70, n)], 1)
        dims = np.stack([rng.uniform(3.5, 4.5, n), rng.uniform(1.4, 1.7, n), rng.uniform(1.5, 1.8, n)], 1)   # l, h, w
        ry = rng.uniform(-np.pi, np.pi, n)
        top = rng.uniform(150, 200, n)
        hgt = rng.uniform(15, 120, n)
        left = rng.uniform(0, 1100, n)
        bbox = np.stack([left, top, left + 1.5 * hgt, top + hgt], 1)
        gt.append({"name": names, "truncated": rng.choice([0.0, 0.2, 0.4], n), "occluded": rng.integers(0, 3, n),
                   "alpha": rng.uniform(-np.pi, np.pi, n), "bbox": bbox, "dimensions": dims, "location": loc, "rotation_y": ry,
                   "score": np.zeros(n)})
        src = rng.integers(0, n, dets)
        near = rng.uniform(0, 1, dets) < 0.3            # 30 % near a label, the rest anywhere
        dloc = np.where(near[:, None], loc[src] + rng.normal(0, 0.3, (dets, 3)),
                        np.stack([rng.uniform(-20, 20, dets), rng.uniform(1, 2, dets), rng.uniform(5, 70, dets)], 1))
        dbox = np.where(near[:, None], bbox[src] + rng.normal(0, 5, (dets, 4)), bbox[rng.integers(0, n, dets)] + rng.normal(0, 80, (dets, 4)))
        dt.append({"name": np.array(["Car"] * dets), "truncated": -np.ones(dets), "occluded": -np.ones(dets, dtype=np.int64),
                   "alpha": rng.uniform(-np.pi, np.pi, dets), "bbox": dbox, "dimensions": dims[src] * rng.uniform(0.9, 1.1, (dets, 3)),
                   "location": dloc, "rotation_y": ry[src] + rng.normal(0, 0.1, dets), "score": np.round(rng.uniform(0, 1, dets), 4)})
    return gt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch
    from ws3d_amd import kitti_eval
    gt, dt = synthetic_annos(a.frames, a.dets)
    times, result, ret = [], None, None
    for _ in range(a.repeat + 1):        # the first run loads the library and warms the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result, ret = kitti_eval.get_official_eval_result(gt, dt, 0)
        times.append(time.perf_counter() - t0)
    print(result, end="")
    print(json.dumps({"frames": a.frames, "dets_per_frame": a.dets, "labels": int(sum(len(g["name"]) for g in gt)),
                      "get_official_eval_result_s": [round(t, 4) for t in times[1:]], "first_call_s": round(times[0], 4),
                      "Car_3d_moderate": float(ret["Car_3d_moderate"])}))


if __name__ == "__main__":
    main()
