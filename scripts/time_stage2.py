#!/usr/bin/env python
"""Device time of the Stage-2 box network per instance cloud: ``python scripts/time_stage2.py [--out profiles/stage2.txt]``.

R = 800 (the reference's Stage-2 batch) and R = 64 clouds of 512 points (synth.roi_clouds in the Stage-2 frame, seeded weights):
  * RCNNNet forward by the channels-last route and by the module route;
  * ws3d_stage2_embed (with and without a box) against the same five layers as a chain of library GEMMs on channels-last rows
    (torch addmm + relu, the canonical transform as torch ops).
HIP events around each call on one stream, 5 warm-up calls, then `--iters` timed calls one by one; median with p10 / p90.
No figure here is a pass criterion."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ws3d_amd import compat as C, stage2, synth  # noqa: E402
from ws3d_amd.seeded import seeded_state_dict  # noqa: E402


def timed(fn, iters, warmup=5):
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


def clouds(R, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    xyz = synth.roi_clouds(R, 512, seed) - np.array([0.0, -0.2, 0.0], dtype=np.float32)
    refl = rng.uniform(0, 1, (R, 512, 1)).astype(np.float32)
    mask = np.where(rng.uniform(0, 1, (R, 512, 1)) < 0.5, 0.5, -0.5).astype(np.float32)
    t = torch.from_numpy(np.concatenate((xyz * 0.5, refl, mask), axis=-1).astype(np.float32)).cuda()
    return {"cur_box_point": t[..., 0:3].contiguous(), "cur_box_reflect": t[..., 3:4].contiguous(), "train_mask": t[..., 4:5].contiguous()}, t.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    net = stage2.RCNNNet()
    sd = seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 12)
    for k in ("reg_layer.3.conv.weight", "reg_layer.3.conv.bias", "ref_layer.0.3.conv.weight", "ref_layer.0.3.conv.bias"):
        sd[k] = sd[k] * 0.05
    net.load_state_dict(sd)
    net = net.cuda().eval()
    lines = ["Stage-2 box network, device time (HIP events, 5 warm-up calls, %d timed calls: median [p10 .. p90])" % a.iters,
             "device: %s" % torch.cuda.get_device_name(0), ""]
    for R in (800, 64):
        data, pts5 = clouds(R)
        res = {}
        for name, fast in (("channels-last route", True), ("module route", False)):
            stage2.CHANNELS_LAST_FASTPATH = fast
            with torch.no_grad():
                res[name] = timed(lambda: net(data), a.iters if fast else max(5, a.iters // 3))
        stage2.CHANNELS_LAST_FASTPATH = True
        for name, (med, lo, hi) in res.items():
            lines.append("R = %3d  RCNNNet forward, %-20s %9.3f ms [%8.3f .. %8.3f]  = %8.2f us per cloud" % (R, name + ":", med, lo, hi, 1e3 * med / R))
        lines.append("R = %3d  module / channels-last: %.2f x" % (R, res["module route"][0] / res["channels-last route"][0]))
        # the tower front alone
        with torch.no_grad():
            box = net(data)["box_ce"].contiguous()
        for label, b, mods in (("no box ", None, (net.xyz_up_layer, net.feature_up_layer, net.merge_down_layer)),
                               ("canonical", box, (net.can_xyz_up_layer[0], net.can_feature_up_layer[0], net.can_merge_down_layer[0]))):
            layers = [mods[0].layer0, mods[0].layer1, mods[1].layer0, mods[1].layer1, mods[2].layer0]
            wt = [l.conv.weight.detach().reshape(l.conv.weight.shape[0], -1).t().contiguous() for l in layers]
            bs = [l.conv.bias.detach().contiguous() for l in layers]
            packed = [t for pair in zip(wt, bs) for t in pair]

            def kernel():
                return C.stage2_embed(pts5, b, *packed)

            def chain():
                xyz = pts5[..., 0:3] if b is None else stage2.canonical_points(pts5[..., 0:3], b)
                ux = torch.relu_(torch.addmm(bs[1], torch.relu_(torch.addmm(bs[0], xyz.reshape(-1, 3), wt[0])), wt[1]))
                uf = torch.relu_(torch.addmm(bs[3], torch.relu_(torch.addmm(bs[2], pts5[..., 3:5].reshape(-1, 2), wt[2])), wt[3]))
                return xyz, torch.relu_(torch.addmm(bs[4], torch.cat((ux, uf), dim=1), wt[4]))

            with torch.no_grad():
                k_ms, c_ms = timed(kernel, a.iters), timed(chain, a.iters)
                d = float((kernel()[1] - chain()[1]).abs().max())
            lines.append("R = %3d  tower front (%s): ws3d_stage2_embed %8.3f ms [%7.3f .. %7.3f]   library GEMM chain %8.3f ms [%7.3f .. %7.3f]   "
                         "chain / kernel %.2f x   max |difference| %.2g" % (R, label, *k_ms, *c_ms, c_ms[0] / k_ms[0], d))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
