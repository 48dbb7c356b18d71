#!/usr/bin/env python
"""Device time of click-driven annotation (ws3d_amd.annotate) on the ``hdl64`` generator at B = 8, N = 16384, with one click on
every car of the generator that has scene points within 4 m of its centre, on the seeded Stage-2 weights:

  click_prepare    ws3d_click_prepare: the click score over (points x clicks) and the 25 jittered candidates per click
  cut              ws3d_instance_clouds around the candidates, S = 512
  stage 2          Stage2Net.rcnn_forward over the real candidates in chunks of --rcnn_batch clouds (detect_kitti.rcnn_over_real_slots)
  tail             stage2.detections(ANNOTATE_CFG, return_index=True)
  annotate_batch   the four together, as the public entry runs them
  reference loop   tools/eval_active.py:187-324, 463-499 restated on the same device and inputs: the click score on the host
                   (losses.gaussian_center_labels), the candidate list by 25 clones, the (N x 25K) distance matrix, per candidate a
                   boolean mask and an emptiness test (one synchronisation), then ONE rcnn_forward call at R = 1 -- over the same
                   512-row cloud the batched route feeds, so both routes run the network on the same inputs -- and the host sweep
                   (stage2.detections_loop)

Every shape is warmed up, the variants alternate inside one run and are repeated; each time is a pair of device events around
the call (whatever synchronises inside pays its host time).  Nothing here asserts a ratio: the file records what was measured.

    python scripts/time_annotate.py [--out profiles/annotate.txt] [--repeat 7] [--batch 8] [--npoints 16384] [--skip_reference]

--out: the lines from ``MARKER`` on are replaced, whatever stands before it (the compiler's resource remarks) is kept.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

MARKER = "== measured (scripts/time_annotate.py)"


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def visible_clicks(pc, boxes, radius=4.0):
    """per scene the centres of the generator's cars with at least one scene point within `radius` in (x, z) -> (B,K,3) zero padded, (B,)"""
    rows = []
    for p, b in zip(pc, boxes):
        d = np.sqrt((p[:, None, 0] - b[None, :, 0]) ** 2 + (p[:, None, 2] - b[None, :, 2]) ** 2)
        rows.append(b[(d < radius).any(axis=0), :3].astype(np.float32))
    K = max(r.shape[0] for r in rows)
    clicks = np.zeros((len(rows), K, 3), dtype=np.float32)
    for i, r in enumerate(rows):
        clicks[i, :r.shape[0]] = r
    return clicks, np.array([r.shape[0] for r in rows], dtype=np.int32)


def reference_loop(s2, pts, clicks, num_h, clouds, cfg):
    """the reference's per-scene, per-candidate code on the device; clouds: annotate_inputs' dict (the R = 1 forwards read its rows)"""
    import torch
    from ws3d_amd import losses, stage2
    B, Kc = clouds["center"].shape[0], clouds["center"].shape[1]
    full = {k: torch.zeros((B * Kc, w), device=pts.device) for k, w in (("rcnn_cls", 1), ("rcnn_iou", 1), ("rcnn_ref", 7), ("box_ce", 7))}
    for b in range(B):
        n = int(num_h[b])
        if n == 0:
            continue
        inputs = pts[b]
        mask = losses.gaussian_center_labels(inputs[:, :3].cpu().numpy(), clicks[b, :n].cpu().numpy())[0]       # click_gaussian_mask, on the host
        score = torch.from_numpy(np.asarray(mask, dtype=np.float32)).to(pts.device)
        centre = clicks[b, :n][:, [0, 2]].contiguous()
        grid = []
        for i in (-2, -1, 0, 1, 2):
            for j in (-2, -1, 0, 1, 2):
                sample = torch.clone(centre)
                sample[:, 0] += 0.1 * i
                sample[:, 1] += 0.1 * j
                grid.append(sample)
        centre = torch.cat(grid, dim=0)
        d = torch.sqrt(torch.sum((centre[None, :] - inputs[:, [0, 2]][:, None]) ** 2, dim=2))      # (N, 25 n)
        near = d.min(dim=-1)[0] < 4.0
        d, inputs, score = d[near], inputs[near], score[near]
        for c in range(centre.shape[0]):
            flag = d[:, c].view(-1) < 4.0
            if flag.long().sum() == 0:
                continue
            held = (inputs[flag, :3], inputs[flag, 3].view(-1, 1), (score[flag] > 0.5).view(-1, 1).float() - 0.5)   # noqa: F841 (what the reference builds per candidate)
            slot = b * Kc + c
            res = s2.rcnn_forward({k: clouds[k].reshape(B * Kc, *clouds[k].shape[2:])[slot:slot + 1].contiguous()
                                   for k in ("cur_box_point", "cur_box_reflect", "train_mask")})
            for k in full:
                full[k][slot] = res[k].reshape(-1)
    sel = stage2.select_boxes(full["box_ce"].view(B, Kc, 7), full["rcnn_ref"].view(B, Kc, 7), full["rcnn_cls"].view(B, Kc), full["rcnn_iou"].view(B, Kc),
                              clouds["center"], clouds["num"], cfg)
    return stage2.detections_loop(*sel, cfg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--npoints", type=int, default=16384)
    ap.add_argument("--rcnn_batch", type=int, default=800)
    ap.add_argument("--skip_reference", action="store_true", help="leave the reference loop out (it makes one Stage-2 forward per candidate)")
    a = ap.parse_args()
    import torch
    from ws3d_amd import annotate, detect_kitti, instance_ops, stage2, synth
    dev = torch.device("cuda:0")
    B, N = a.batch, a.npoints
    cfg = annotate.ANNOTATE_CFG
    s2 = detect_kitti.load_stage2(device="cuda:0")
    scenes = [synth.hdl64_cloud(N, 1000 * 3 + s, return_boxes=True) for s in range(B)]      # synth.make_batch('hdl64', B, N, 3)'s scenes
    pc = np.stack([s[0] for s in scenes])
    clicks_h, num_h = visible_clicks(pc, [s[1] for s in scenes])
    pts, clicks, num = torch.from_numpy(pc).to(dev), torch.from_numpy(clicks_h).to(dev), torch.from_numpy(num_h).to(dev)
    with torch.no_grad():
        score, cand, cand_num = annotate._click_prepare(pts, clicks, num, 5, 0.1, cfg.ground_y)
        inp = annotate.annotate_inputs(pts, clicks, num, ground_y=cfg.ground_y)
        full = detect_kitti.rcnn_over_real_slots(s2, inp, a.rcnn_batch)
        variants = {
            "click_prepare": lambda: annotate._click_prepare(pts, clicks, num, 5, 0.1, cfg.ground_y),
            "cut": lambda: instance_ops.instance_clouds(pts, score, cand, cand_num, 4.0, 512, mask_mode=1, mask_thresh=0.5),
            "stage 2": lambda: detect_kitti.rcnn_over_real_slots(s2, inp, a.rcnn_batch),
            "tail": lambda: stage2.detections(full, inp["center"], inp["num"], cfg, return_index=True),
            "annotate_batch": lambda: annotate.annotate_batch(s2, pts, clicks, num, cfg, a.rcnn_batch),
            "reference loop": lambda: reference_loop(s2, pts, clicks, num_h, inp, cfg),
        }
        if a.skip_reference:
            del variants["reference loop"]
        for fn in variants.values():          # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.repeat):             # alternated
            for k, fn in variants.items():
                times[k].append(timed(fn)[0])
        kept = annotate.annotate_batch(s2, pts, clicks, num, cfg, a.rcnn_batch)[2].cpu().tolist()
    count = inp["count"]
    lines = [MARKER,
             f"{torch.cuda.get_device_name(0)}  hdl64  B={B} N={N} S=512  clicks per scene {num_h.tolist()} (K={clicks.shape[1]}), "
             f"{int(cand_num.sum())} candidates, rcnn_batch={a.rcnn_batch}, seeded Stage-2 weights, repeat={a.repeat}",
             f"members per candidate: min {int(count.min())} median {int(count.float().median())} max {int(count.max())}; kept boxes per scene {kept}"]
    for k, t in times.items():
        t = sorted(t)
        lines.append(f"   {k:16s} median {t[len(t) // 2]:10.3f} ms  min {t[0]:10.3f}  max {t[-1]:10.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        head = ""
        if os.path.exists(a.out):
            head = open(a.out).read().split(MARKER)[0]
        with open(a.out, "w") as f:
            f.write(head + text)


if __name__ == "__main__":
    main()
