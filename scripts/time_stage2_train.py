#!/usr/bin/env python
"""Device time of Stage-2 training at R = 800: ``python scripts/time_stage2_train.py [--out profiles/stage2_train.txt]``.

  1. ``boxes_iou3d_paired`` against the route to the same numbers before it existed: ``boxes_iou3d_gpu`` plus the diagonal;
  2. each fused loss, forward + backward, against the torch restatement on the GPU with the reference's N x N IoU route
     (a record of what the fusion buys: both sides are this package's code);
  3. one training step per phase split into forward / loss / backward / optimizer, and the host synchronisations in it;
  4. whether two seeded three-step runs end with bit-equal weights.
Every part runs in a child process of its own under a time limit; a part that fails ends the run.  HIP events around each call on
one stream, warm-up calls first, the two sides of a comparison alternated, medians.  No figure here is a pass criterion."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 800
PARTS = (("iou", 120), ("losses", 180), ("step", 420), ("repro", 420))


def alternated(fns, iters, warmup=5):
    """median ms of each callable, the callables taking turns"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [float(np.median(m)) for m in ms]


def loss_inputs(seed=5):
    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor([1.5, 1.6, 3.9])
    gt = torch.cat((torch.rand((R, 1), generator=g) * 2 - 1, torch.rand((R, 1), generator=g) * 0.5 + 0.5, torch.rand((R, 1), generator=g) * 2 - 1,
                    mean * (0.8 + 0.45 * torch.rand((R, 3), generator=g)), (torch.rand((R, 1), generator=g) * 2 - 1) * np.pi), dim=1)
    pred = gt + torch.randn((R, 7), generator=g) * torch.tensor([0.3, 0.3, 0.3, 0.1, 0.1, 0.1, 0.2]) * torch.rand((R, 1), generator=g)
    cls = (torch.rand((R,), generator=g) < 0.5).float()
    gt = gt * (cls.view(-1, 1) + (torch.rand((R, 1), generator=g) < 0.5).float()).clamp(max=1)
    ref = torch.randn((R, 7), generator=g) * 0.05
    refined = torch.cat((pred[:, :3] + pred[:, 3:6] * ref[:, :3], pred[:, 3:6] * (1 + ref[:, 3:6]), pred[:, 6:7] + ref[:, 6:7]), dim=1)
    t = {"cls": cls, "gt": gt, "pred": pred, "refined": refined, "ref": ref, "rcnn_cls": torch.randn((R,), generator=g) * 2,
         "reg": torch.randn((R, 52), generator=g) * 0.8, "iou": torch.rand((R,), generator=g)}
    return {k: v.cuda().contiguous() for k, v in t.items()}


def part_iou(iters):
    from ws3d_amd import iou3d_ops
    t = loss_inputs()
    paired = lambda: iou3d_ops.boxes_iou3d_paired(t["pred"], t["gt"])                       # noqa: E731
    matrix = lambda: torch.diagonal(iou3d_ops.boxes_iou3d_gpu(t["pred"], t["gt"])[1]).contiguous()   # noqa: E731
    assert torch.equal(paired()[1], matrix())
    a, b = alternated([paired, matrix], iters)
    return ["paired 3-D IoU, %d pairs: boxes_iou3d_paired %.4f ms, boxes_iou3d_gpu + diagonal %.4f ms (%.1fx), outputs bit-equal" % (R, a, b, b / a)]


def part_losses(iters):
    from ws3d_amd import stage2_losses as sl
    t = loss_inputs()
    lines = []
    for phase in ("rcnn", "ioun"):
        heads = [t["rcnn_cls"], t["reg"]] if phase == "rcnn" else [t["iou"], t["ref"]]
        heads = [h.clone().requires_grad_(True) for h in heads]
        rest = (t["pred"], t["gt"], t["cls"]) if phase == "rcnn" else (t["pred"], t["refined"], t["gt"], t["cls"])

        def fused():
            loss, _ = (sl.rcnn_loss if phase == "rcnn" else sl.ioun_loss)(*heads, *rest)
            torch.autograd.grad(loss, heads)

        def restated():
            loss, _ = (sl.rcnn_loss_torch if phase == "rcnn" else sl.ioun_loss_torch)(*heads, *rest, full_matrix=True)
            torch.autograd.grad(loss, heads)

        a, b = alternated([fused, restated], iters)
        lines.append("%s loss forward + backward, R = %d: fused kernel %.4f ms, torch restatement with the N x N IoU route %.4f ms (%.1fx)" % (phase, R, a, b, b / a))
    return lines


def _setup(phase, seed=0, batch=R):
    from ws3d_amd import train_rcnn as t2
    torch.manual_seed(seed)
    model = t2.build_model(phase, torch.device("cuda"))
    opt = t2.AdamOneCycle(t2.trained_parameters(model, phase), 100, t2.STAGE2_TRAIN)
    ds = t2.BoxDataset(t2.SyntheticBoxes(max(batch // 4, 8), seed), "TRAIN", seed, phase)
    return t2, model, opt, t2.batches(ds, batch)


def part_step(iters):
    from ws3d_amd import stage2_losses as sl
    lines = []
    for phase in ("rcnn", "ioun"):
        t2, model, opt, stream = _setup(phase)
        batch = next(stream)
        for it in range(2):
            t2.train_step(model, opt, batch, it, phase)
        # the step again, piece by piece, events between the pieces
        model.train()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        parts = []
        for it in range(max(iters // 3, 3)):
            opt.schedule(it); opt.zero_grad()
            ev[0].record()
            data = t2.prepare_batch(batch, "cuda")
            inputs = {k: data[k] for k in ("cur_box_point", "cur_box_reflect", "train_mask") + t2.IOU_KEYS if k in data}
            ev[1].record()
            out = model.rcnn_forward(inputs, towers="rcnn" if phase == "rcnn" else "both")
            ev[2].record()
            if phase == "rcnn":
                loss, _ = sl.rcnn_loss(out["rcnn_cls"], out["rcnn_reg"], out["pred_boxes3d"], data["gt_boxes"], data["cls"])
            else:
                loss, _ = sl.ioun_loss(out["rcnn_iou"], out["rcnn_ref"], out["pred_boxes3d"], out["refined_box"], data["gt_boxes"], data["cls"])
            ev[3].record()
            loss.backward()
            ev[4].record()
            torch.nn.utils.clip_grad_norm_(t2.trained_parameters(model, phase), 1.0)
            opt.step()
            ev[5].record()
            torch.cuda.synchronize()
            parts.append([ev[i].elapsed_time(ev[i + 1]) for i in range(5)])
        med = np.median(np.array(parts), axis=0)
        torch.cuda.set_sync_debug_mode(1)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            t2.train_step(model, opt, batch, 5, phase)
        torch.cuda.set_sync_debug_mode(0)
        syncs = sum("synchroniz" in str(w.message) for w in caught)
        lines.append("%s step, R = %d (module route): prepare %.2f ms, forward %.2f ms, loss %.3f ms, backward %.2f ms, clip + optimizer %.2f ms; "
                     "loss share %.2f %%; host synchronisations in train_step: %d" % (phase, R, *med, 100 * med[2] / med.sum(), syncs))
        stream.close()
    return lines


def part_repro(iters):
    lines = []
    for phase in ("rcnn", "ioun"):
        ends = []
        for _ in range(2):
            t2, model, opt, stream = _setup(phase, seed=3, batch=64)
            for it in range(3):
                t2.train_step(model, opt, next(stream), it, phase)
            ends.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
            stream.close()
        same = all(torch.equal(ends[0][k], ends[1][k]) for k in ends[0])
        lines.append("%s: two seeded three-step runs (batch 64) end with bit-equal weights: %s" % (phase, same))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--part", default=None, choices=[p for p, _ in PARTS])
    a = ap.parse_args()
    if a.part:
        for line in globals()["part_" + a.part](a.iters):
            print("RESULT " + line, flush=True)
        return 0
    lines = ["Stage-2 training, device time (HIP events, 5 warm-up calls, medians of %d alternated calls)" % a.iters]
    for part, limit in PARTS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--iters", str(a.iters)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s: no result within %d s; stopping here" % (part, limit))
            break
        lines += [l[len("RESULT "):] for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0:
            lines.append("%s: exit status %d; stopping here\n%s" % (part, r.returncode, r.stderr[-1500:]))
            break
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
