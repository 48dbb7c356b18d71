#!/usr/bin/env python
"""Stage-1 targets and loss, host route against device route: ``python scripts/time_rpn_targets.py [--out profiles/rpn_targets.txt]``.

At B = 8 and B = 25 scenes of 16384 points with 15 centres each:
  1. labels: ``losses.center_labels_batch`` on the device (one launch) against ``losses.gaussian_center_labels`` scene by scene on the host;
  2. loss: ``losses.rpn_loss_fused`` forward + backward against ``losses.rpn_loss(lazy=True)`` forward + backward on the device, and the
     host synchronisations in each;
  3. host: milliseconds the training process spends building one batch at ``--workers 0``, labels made on the host or left to the device
     (augmented scenes, so nothing is cached);
  4. step: one ``train_step`` on either loss (B = 2, N = 4096) and the torch route's own distance from float64, the figures
     tests/test_gpu_rpn_targets.py bounds;
  5. train: ms / iteration of ``train_rpn --synthetic 64 --total_iters 60`` with and without ``--device_targets``.
Every part runs in a child process of its own under a time limit; a part that fails ends the run.  HIP events around each call on one
stream, warm-up calls first, the two sides of a comparison alternated, medians.  No figure here is a pass criterion."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, BATCHES = 16384, 15, (8, 25)
PARTS = (("labels", 180), ("loss", 180), ("host", 240), ("step", 240), ("train", 420))


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


def scenes(batch, seed=40):
    from ws3d_amd import synth
    pts = np.stack([synth.lidar_cloud(N, 1000 * seed + b) for b in range(batch)]).astype(np.float32)
    centres = np.stack([synth.random_boxes3d(K, (1000 * seed + b) * 7919 + 13)[:, :3] for b in range(batch)]).astype(np.float32)
    return pts, centres, np.full((batch,), K, dtype=np.int32)


def part_labels(iters):
    from ws3d_amd import losses
    lines = []
    for batch in BATCHES:
        pts, centres, count = scenes(batch)
        dev = [torch.from_numpy(a).cuda() for a in (pts, centres, count)]
        (ms,) = alternated([lambda: losses.center_labels_batch(*dev)], iters)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = [losses.gaussian_center_labels(pts[b, :, :3], centres[b]) for b in range(batch)]
            host.append((time.perf_counter() - t0) * 1e3)
        cls, reg = (t.cpu().numpy() for t in losses.center_labels_batch(*dev))
        want_cls = np.stack([w[0].astype(np.float32) for w in want])
        same = np.array_equal(reg, np.stack([w[1] for w in want])) and np.array_equal(cls > 0, want_cls > 0)
        ulp = int(np.abs(cls.view(np.int32).astype(np.int64) - want_cls.view(np.int32).astype(np.int64)).max())
        lines.append("labels, B = %d: device %.4f ms (one launch), host numpy %.1f ms (%.1f ms per scene); reg_label and label > 0 bit-equal: %s, "
                     "cls_label within %d fp32 unit(s); foreground %d of %d, %d of them fp32 denormals"
                     % (batch, ms, float(np.median(host)), float(np.median(host)) / batch, same, ulp, int((cls > 0).sum()), cls.size,
                        int(((cls > 0) & (cls < np.finfo(np.float32).tiny)).sum())))
    return lines


def _syncs(fn):
    torch.cuda.set_sync_debug_mode(1)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fn()
    torch.cuda.set_sync_debug_mode(0)
    return sum("synchroniz" in str(w.message) for w in caught)


def part_loss(iters):
    from ws3d_amd import losses
    lines = []
    for batch in BATCHES:
        pts, centres, count = scenes(batch)
        cls, reg = losses.center_labels_batch(*[torch.from_numpy(a).cuda() for a in (pts, centres, count)])
        g = torch.Generator().manual_seed(batch)
        heads = [(torch.randn((batch, N, 1), generator=g) * 1.5 - 2.0).cuda().requires_grad_(True), torch.randn((batch, N, 40), generator=g).cuda().requires_grad_(True)]

        def fused():
            loss, _ = losses.rpn_loss_fused(*heads, cls, reg, 4.0, 0.8)
            torch.autograd.grad(loss, heads)

        def plain():
            loss, _ = losses.rpn_loss(*heads, cls, reg, 4.0, 0.8, lazy=True)
            torch.autograd.grad(loss, heads)

        a, b = alternated([fused, plain], iters)
        lines.append("loss forward + backward, B = %d (%d rows): fused HIP %.4f ms (3 launches + the backward's 2 scalings), torch route %.4f ms (%.1fx); "
                     "host synchronisations: fused %d, torch route %d" % (batch, batch * N, a, b, b / a, _syncs(fused), _syncs(plain)))
    return lines


def part_host(iters):
    from ws3d_amd import train_rpn
    lines = []
    for batch in BATCHES:
        ms = {}
        for flag in (True, False):
            ds = train_rpn.SyntheticCenters(2 * batch, augment=True, rng=np.random.RandomState(1), labels=flag)
            for i in range(len(ds)):
                ds[i]                                   # the scans are generated once and kept: the first pass is not what a step pays
            src = train_rpn.batches(ds, batch, np.random.RandomState(0), collate=train_rpn._collate if flag else train_rpn._collate_centers)
            t = []
            for _ in range(max(iters // 5, 4)):
                t0 = time.perf_counter()
                next(src)
                t.append((time.perf_counter() - t0) * 1e3)
            src.close()
            ms[flag] = float(np.median(t))
        lines.append("host work per batch at --workers 0, B = %d (augmented scenes): labels on the host %.1f ms, labels left to the device %.1f ms"
                     % (batch, ms[True], ms[False]))
    return lines


def part_step(iters):
    from tests.test_gpu_rpn_targets import step_deviation
    f = step_deviation()
    return ["train_step, B = %d, N = %d, same weights / batch / dropout seed: loss %.9g (torch route) %.9g (fused), float64 loss of the head outputs %.12g; "
            "grad_norm %.9g (torch route) %.9g (fused)" % (f["batch"], f["npoints"], f["loss_torch"], f["loss_fused"], f["fp64_loss"], f["grad_norm_torch"],
                                                            f["grad_norm_fused"]),
            "  the yardstick: the fp32 torch loss route is %.3g from its float64 CPU run in the loss and %.3g (relative l2) in d loss / d heads; "
            "the two steps differ by %.3g in the loss and %.3g (relative) in grad_norm"
            % (f["torch_route_loss_deviation"], f["torch_route_grad_deviation_rel"], abs(f["loss_fused"] - f["loss_torch"]),
               abs(f["grad_norm_fused"] - f["grad_norm_torch"]) / f["grad_norm_torch"]),
            "  " + json.dumps(f)]


def part_train(iters):
    import logging
    from ws3d_amd import train_rpn
    logging.disable(logging.CRITICAL)
    lines = []
    for batch in BATCHES:
        ms = {}
        for flag in (False, True):
            ds = train_rpn.SyntheticCenters(64, labels=not flag)
            res = train_rpn.train(ds, 60, batch, output_dir=None, device_targets=flag)
            ms[flag] = (float(np.median(res["step_ms"][2:])), res["history"][-1])
        lines.append("train_rpn --synthetic 64 --total_iters 60 --batch_size %d: %.1f ms/it (last loss %.4f), with --device_targets %.1f ms/it (last loss %.4f); "
                     "medians over iterations 21-60 (the 64 un-augmented scenes and their host labels are cached after the first epoch)"
                     % (batch, ms[False][0], ms[False][1], ms[True][0], ms[True][1]))
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
    lines = ["Stage-1 targets and loss, N = %d, K = %d (HIP events, 5 warm-up calls, medians of %d alternated calls)" % (N, K, a.iters)]
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
