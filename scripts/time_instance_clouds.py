#!/usr/bin/env python
"""Device time of the Stage-2 instance-cloud cut (ws3d_amd.instance_ops) at B = 8, N = 16384 on the ``hdl64`` and ``lidar``
generators, with the centres ``stage1.center_proposals`` keeps on the seeded weights (and, for scale, K = 100 jittered scene
points per scene, the proposal count of the c3 bench).  The seeded heads are untrained and keep thousands of centres per scene;
the best-scored --max_centres of each scene are timed:

  fixed            ws3d_instance_clouds, S = 512, no features           (B,K,S,5)
  fixed+feats      ... with the C = 128 backbone features               (B,K,S,5) + (B,K,S,128)
  ragged           ws3d_instance_clouds_count + cumsum + one host sync + ws3d_instance_clouds_emit
  ragged+feats     ... with features
  reference loop   generate_box_dataset.py:200, 203-227 / eval_auto.py:324-367 restated in torch on the same device and inputs:
                   the (N x K) distance matrix, then per centre a boolean mask, an emptiness test (one sync) and the indexing
  roipool3d_fill   ws3d_roipool3d_fill at the same B, K, S, C (mean-size boxes on the centres): the same kind of ordered
                   select-and-copy, (B,K,S,3+128) output

Every shape is warmed up, the variants alternate inside one run and are repeated; each time is a pair of device events around
the call (the reference loop and the ragged pair synchronise inside, their host time is part of what they cost).  Kernel times:
run it under ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/time_instance_clouds.py --repeat 3
--skip_reference``.

    python scripts/time_instance_clouds.py [--repeat 7] [--batch 8] [--npoints 16384]
"""
import argparse
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def reference_loop(pts, scores, centres, num, feats):
    """the reference's per-scene code, on the device; returns the number of rows it produced"""
    import torch
    rows = 0
    for b in range(pts.shape[0]):
        inputs, sc = pts[b], scores[b]
        ctr = centres[b, :int(num[b])]
        d = torch.sqrt(torch.sum((ctr[:, [0, 2]][None, :] - inputs[:, [0, 2]][:, None]) ** 2, dim=2))      # (N, K)
        for i in range(ctr.shape[0]):
            flag = d[:, i].view(-1) < 4.0
            if flag.long().sum() == 0:
                continue
            xyz = inputs[flag, :3] - ctr[i].view(1, 3)
            refl = inputs[flag, 3].view(-1, 1)
            mask = (sc[flag] > 0.5).view(-1, 1).float() - 0.5
            held = (xyz, refl, mask, feats[b][flag] if feats is not None else None)      # what the reference hands on per centre
            rows += held[0].shape[0]
    return rows


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--npoints", type=int, default=16384)
    ap.add_argument("--sampled", type=int, default=512)
    ap.add_argument("--max_centres", type=int, default=512, help="time at most this many kept centres per scene, the best-scored ones (0: all)")
    ap.add_argument("--skip_reference", action="store_true", help="leave the reference loop out (kernel-trace runs: it makes ~10^5 launches)")
    a = ap.parse_args()
    import torch
    from ws3d_amd import compat, instance_ops, stage1, synth
    from ws3d_amd.seeded import seeded_state_dict
    dev = torch.device("cuda:0")
    B, N, S = a.batch, a.npoints, a.sampled
    model = stage1.Stage1Net(mode="TEST").to(dev).eval()
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0))
    h, w, l = stage1.DEFAULT_CFG.cls_mean_size
    for kind in ("hdl64", "lidar"):
        pc = synth.make_batch(kind, B, N, 3)
        pts = torch.from_numpy(pc).to(dev)
        with torch.no_grad():
            out = model.rpn_forward({"pts_input": pts})
        scores = torch.sigmoid(out["rpn_cls"].reshape(B, N)).contiguous()
        feats = out.get("backbone_features_nlc")
        feats = (out["backbone_features"].transpose(1, 2) if feats is None else feats).contiguous()
        C = feats.shape[2]
        # the seeded heads are untrained (scores near the focal prior): lower SCORE_THRESH until centres are kept, and say so
        for thresh in (0.3, 0.1, 0.03, 0.01, 0.003, 0.0):
            cfg = dataclasses.replace(stage1.DEFAULT_CFG, score_thresh=thresh)
            centre, _, num = stage1.kept_centres(out, cfg, y=1.65)
            if int(num.sum()) >= 8 * B:
                break
        kept = num.cpu().numpy().tolist()
        if a.max_centres and centre.shape[1] > a.max_centres:      # (the untrained heads keep far more centres than a trained Stage 1 does)
            centre, num = centre[:, :a.max_centres].contiguous(), num.clamp(max=a.max_centres)
        rng = np.random.default_rng(5)
        jit = np.zeros((B, 100, 3), dtype=np.float32)
        for b in range(B):
            pick = rng.integers(0, N, 100)
            jit[b, :, 0] = pc[b, pick, 0] + rng.normal(0, 1.0, 100)
            jit[b, :, 2] = pc[b, pick, 2] + rng.normal(0, 1.0, 100)
        jit[:, :, 1] = 1.65
        sets = [("center_proposals(score_thresh=%g) kept %s, first %d of each timed" % (thresh, kept, centre.shape[1]), centre, num),
                ("100 jittered scene points per scene", torch.from_numpy(jit).to(dev), torch.full((B,), 100, dtype=torch.int32, device=dev))]
        for label, ctr, num in sets:
            K = ctr.shape[1]
            num_h = num.cpu().numpy()
            boxes = torch.zeros((B, K, 7), device=dev)
            boxes[..., 0], boxes[..., 2], boxes[..., 1] = ctr[..., 0], ctr[..., 2], 1.65
            boxes[..., 3], boxes[..., 4], boxes[..., 5] = h + 2.0, w + 2.0, l + 2.0
            xyz = pts[..., :3].contiguous()
            pooled = torch.empty((B, K, S, 3 + C), device=dev)
            empty = torch.empty((B, K), dtype=torch.int32, device=dev)
            variants = {
                "fixed": lambda: instance_ops.instance_clouds(pts, scores, ctr, num, sampled_pt_num=S, mask_mode=1),
                "fixed+feats": lambda: instance_ops.instance_clouds(pts, scores, ctr, num, sampled_pt_num=S, mask_mode=1, features=feats),
                "ragged": lambda: instance_ops.instance_clouds_ragged(pts, scores, ctr, num, mask_mode=1),
                "ragged+feats": lambda: instance_ops.instance_clouds_ragged(pts, scores, ctr, num, mask_mode=1, features=feats),
                "reference loop": lambda: reference_loop(pts, scores, ctr, num_h, None),
                "reference loop+feats": lambda: reference_loop(pts, scores, ctr, num_h, feats),
                "roipool3d_fill": lambda: compat.roipool3d_forward_fill(xyz, boxes, feats, pooled, empty),
            }
            if a.skip_reference:
                variants = {k: v for k, v in variants.items() if not k.startswith("reference")}
            for fn in variants.values():          # warm-up of every shape
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(a.repeat):             # alternated
                for k, fn in variants.items():
                    times[k].append(timed(fn)[0])
            count = instance_ops.instance_clouds(pts, scores, ctr, num, sampled_pt_num=S)[2]
            total = int(count.sum())
            out_bytes = {"fixed": B * K * S * 5 * 4, "fixed+feats": B * K * S * (5 + C) * 4, "ragged": total * 5 * 4,
                         "ragged+feats": total * (5 + C) * 4, "roipool3d_fill": B * K * S * (3 + C) * 4}
            print(f"== {kind}  B={B} N={N} S={S} C={C}  centres: {label}  K={K} num={num_h.tolist()}")
            print(f"   members per centre: min {int(count.min())} median {int(count.float().median())} max {int(count.max())}, total rows {total}")
            res = {}
            for k, t in times.items():
                t = sorted(t)
                med = t[len(t) // 2]
                line = f"   {k:22s} median {med:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}"
                if k in out_bytes:
                    line += f"   output {out_bytes[k] / 1e6:8.1f} MB  {out_bytes[k] / med / 1e9:7.3f} TB/s effective"
                print(line)
                res[k] = med
            if a.skip_reference:
                continue
            print("   " + json.dumps({"kind": kind, "centres": label, "K": K, "reference_loop_over_fixed": round(res["reference loop"] / res["fixed"], 1),
                                      "reference_loop_feats_over_fixed_feats": round(res["reference loop+feats"] / res["fixed+feats"], 1),
                                      "fixed_feats_rate_over_roipool3d_fill_rate": round((out_bytes["fixed+feats"] / res["fixed+feats"]) /
                                                                                         (out_bytes["roipool3d_fill"] / res["roipool3d_fill"]), 3)}))


if __name__ == "__main__":
    main()
