#!/usr/bin/env python
"""Device time of Stage 2 on WHOLE instance clouds: ``python scripts/time_stage2_ragged.py [--out profiles/stage2_ragged.txt]``.

The clouds of eight ``synth.hdl64_cloud(16384, seed)`` scenes (seeds 3000 .. 3007): the 4 m cylinders around the cars that hold at
least 16 points within 2 m, x and z shifted to the car, y lowered by 1.65 -- what tools/eval_auto.py:286-403 feeds.  Seeded weights.
  * the ragged route ``Stage2Net.rcnn_forward_ragged`` (all clouds in one call);
  * the per-cloud loop of ``rcnn_forward`` on (1, n_i, .) inputs: the reference's form, existing code;
  * the fixed route: every cloud cut to / repeated up to 512 rows, one ``rcnn_forward``;
  * the three kernels of csrc/stage2_ragged.hip on their own (level 1's npoint, radius and nsample);
  * the share of clouds the fixed route truncates, and how many final boxes differ between the fixed and the ragged route.
HIP events around each call on one stream, warm-up calls, then timed calls one by one; median with p10 / p90.
No figure here is a pass criterion."""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ws3d_amd import compat as C, pn2_ops, stage2, synth  # noqa: E402
from ws3d_amd.seeded import seeded_state_dict  # noqa: E402

SEEDS = tuple(range(3000, 3008))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.percentile(ms, 50), np.percentile(ms, 10), np.percentile(ms, 90)


def scene_clouds(seed, radius=4.0, ground_y=1.65):
    """-> [(rows (n,5), centre (3,))] of one scene"""
    pc, boxes = synth.hdl64_cloud(16384, seed, return_boxes=True)
    d2 = (pc[:, None, 0] - boxes[None, :, 0]) ** 2 + (pc[:, None, 2] - boxes[None, :, 2]) ** 2
    out = []
    for k in range(boxes.shape[0]):
        if (d2[:, k] < 4.0).sum() < 16:
            continue
        rows = np.nonzero(d2[:, k] < radius * radius)[0]
        p = np.zeros((rows.size, 5), dtype=np.float32)
        p[:, 0], p[:, 1], p[:, 2] = pc[rows, 0] - boxes[k, 0], pc[rows, 1] - np.float32(ground_y), pc[rows, 2] - boxes[k, 2]
        p[:, 3] = pc[rows, 3]
        p[:, 4] = np.where(d2[rows, k] < 4.0, 0.5, -0.5)
        out.append((p, np.array([boxes[k, 0], ground_y, boxes[k, 2]], dtype=np.float32)))
    return out


def as_inputs(t):
    return {"cur_box_point": t[..., 0:3].contiguous(), "cur_box_reflect": t[..., 3:4].contiguous(), "train_mask": t[..., 4:5].contiguous()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    s2 = stage2.Stage2Net()
    sd = seeded_state_dict({k: tuple(v.shape) for k, v in s2.rcnn_net.state_dict().items()}, 12)
    for k in ("reg_layer.3.conv.weight", "reg_layer.3.conv.bias", "ref_layer.0.3.conv.weight", "ref_layer.0.3.conv.bias"):
        sd[k] = sd[k] * 0.05
    s2.rcnn_net.load_state_dict(sd)
    s2 = s2.cuda().eval()
    scenes = [scene_clouds(s) for s in SEEDS]
    clouds = [p for sc in scenes for p, _ in sc]
    sizes = [p.shape[0] for p in clouds]
    Cn = len(sizes)
    packed = torch.from_numpy(np.concatenate(clouds)).cuda()
    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)).cuda()
    ragged = dict(as_inputs(packed), offsets=offsets)
    singles = [as_inputs(torch.from_numpy(p[None].copy()).cuda()) for p in clouds]
    fixed = as_inputs(torch.from_numpy(np.stack([p[np.arange(512) % p.shape[0]] for p in clouds])).cuda())
    lines = ["Stage 2 on whole instance clouds, device time (HIP events, warm-up calls, then timed calls: median [p10 .. p90])",
             "device: %s" % torch.cuda.get_device_name(0),
             "%d clouds of %d scenes: %d .. %d points, median %d, %d rows in all; %.0f %% exceed 512 points (the fixed route truncates them), "
             "%.0f %% hold fewer than level 1's %d centres, %d exceed 4096" % (Cn, len(SEEDS), min(sizes), max(sizes), int(np.median(sizes)), sum(sizes),
                                                                               100.0 * np.mean(np.array(sizes) > 512),
                                                                               100.0 * np.mean(np.array(sizes) < s2.rcnn_net.SA_modules[0].npoint),
                                                                               s2.rcnn_net.SA_modules[0].npoint, int((np.array(sizes) > 4096).sum())), ""]
    with torch.no_grad():
        routes = (("ragged route (one rcnn_forward_ragged)", lambda: s2.rcnn_forward_ragged(ragged, sizes=sizes), a.iters, 3),
                  ("per-cloud loop of rcnn_forward", lambda: [s2.rcnn_forward(d) for d in singles], max(2, a.iters // 4), 1),
                  ("fixed route (512 rows a cloud)", lambda: s2.rcnn_forward(fixed), a.iters, 3))
        res = {}
        for name, fn, iters, warm in routes:
            res[name] = timed(fn, iters, warm)
            med, lo, hi = res[name]
            lines.append("%-42s %9.3f ms [%8.3f .. %8.3f]  = %8.2f us per cloud" % (name + ":", med, lo, hi, 1e3 * med / Cn))
        names = [r[0] for r in routes]
        lines.append("loop / ragged: %.1f x    ragged / fixed: %.2f x" % (res[names[1]][0] / res[names[0]][0], res[names[0]][0] / res[names[2]][0]))
        lines.append("")
        # the three kernels on their own
        sa = s2.rcnn_net.SA_modules[0]
        m, r, ns = sa.npoint, sa.groupers[0].radius, sa.groupers[0].nsample
        xyz = packed[:, 0:3].contiguous()
        box = s2.rcnn_forward_ragged(ragged, sizes=sizes)["box_ce"].contiguous()
        can = C.stage2_canonical_ragged(packed, offsets, sizes, box)
        can_xyz = can[:, 0:3].contiguous()
        zeroed = float((can_xyz.abs().amax(dim=1) == 0).float().mean())
        for label, pts in (("raw cylinders", xyz), ("canonical, %.0f %% of the rows zeroed" % (100 * zeroed), can_xyz)):
            idx, new_xyz = pn2_ops.furthest_point_sample_gather_ragged(pts, offsets, m, sizes=sizes)
            t_fps = timed(lambda: pn2_ops.furthest_point_sample_gather_ragged(pts, offsets, m, sizes=sizes), a.iters, 3)
            t_bq = timed(lambda: pn2_ops.ball_query_ragged(r, ns, pts, offsets, new_xyz, sizes=sizes, global_rows=True), a.iters, 3)
            lines.append("%-44s sampling + gather (m = %d) %8.3f ms [%7.3f .. %7.3f]   ball query (r = %.1f, ns = %d) %8.3f ms [%7.3f .. %7.3f]"
                         % (label + ":", m, *t_fps, r, ns, *t_bq))
        t_can = timed(lambda: C.stage2_canonical_ragged(packed, offsets, sizes, box), a.iters, 3)
        lines.append("%-44s %8.3f ms [%7.3f .. %7.3f]" % ("canonical transform (%d rows):" % packed.shape[0], *t_can))
        lines.append("")
        # final boxes of the two routes (the seeded IoU head scores below IOUN.SCORE_THRESH: the threshold is lowered to keep boxes)
        cfg = dataclasses.replace(stage2.DEFAULT_CFG, ioun_score_thresh=-1e9)
        B, K = len(scenes), max(len(sc) for sc in scenes)
        num = torch.tensor([len(sc) for sc in scenes], dtype=torch.int32).cuda()
        center = torch.zeros((B, K, 3))
        slot = []
        for b, sc in enumerate(scenes):
            for k, (_, ctr) in enumerate(sc):
                center[b, k] = torch.from_numpy(ctr)
                slot.append(b * K + k)
        center, slot = center.cuda(), torch.tensor(slot).cuda()
        found = {}
        for name, out in (("ragged", s2.rcnn_forward_ragged(ragged, sizes=sizes)), ("fixed", s2.rcnn_forward(fixed))):
            full = {k: torch.zeros((B * K, w), device="cuda") for k, w in (("rcnn_cls", 1), ("rcnn_iou", 1), ("rcnn_ref", 7), ("box_ce", 7))}
            for k in full:
                full[k][slot] = out[k].reshape(Cn, -1)
            boxes, _, count, index = stage2.detections(full, center, num, cfg, return_index=True)
            found[name] = {(b, int(index[b, j])): boxes[b, j].cpu().numpy() for b in range(B) for j in range(int(count[b]))}
        both = set(found["ragged"]) & set(found["fixed"])
        moved = [float(np.abs(found["ragged"][s][:6] - found["fixed"][s][:6]).max()) for s in both]
        lines.append("final boxes (IOUN.SCORE_THRESH lowered to keep the seeded head's boxes): ragged %d, fixed %d, from the same centre %d; of those %d "
                     "differ by more than 1 cm in a coordinate or size (largest difference %.3f m), %d by more than 10 cm"
                     % (len(found["ragged"]), len(found["fixed"]), len(both), sum(d > 0.01 for d in moved), max(moved) if moved else 0.0,
                        sum(d > 0.1 for d in moved)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
