"""Timings of the ground-truth paste augmentation on the device it is built for.

    python scripts/time_gt_paste.py --out profiles/gt_paste.txt

  1. the ragged furthest-point-sampling launch against a loop of per-cloud launches (all there was before it): 512 clouds with a
     database-like size mix of 513-4096 points, m = 100; device time between events, the two alternated, outputs compared;
  2. database build time per scan on the device and on the host route;
  3. host ms per scene of ``gt_paste.paste_scene`` with stored and with per-draw picks;
  4. the share of augmented draws whose per-draw picks equal the stored ones (reported, not asserted);
  5. ``train_rpn`` ms per iteration on synthetic scenes with and without the paste, with 0 and 4 loader processes.
Needs a HIP device: there is no fallback, a host timing says nothing about it."""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ws3d_amd import fps_host, gt_database as gdb, gt_paste, losses, pn2_ops, synth, train_rpn  # noqa: E402


def _events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def ragged_vs_loop(lines, clouds=512, m=100, reps=7):
    rng = np.random.default_rng(0)
    sizes = np.exp(rng.uniform(np.log(513), np.log(4096), clouds)).astype(np.int64).clip(513, 4096)   # many small, few large
    cs = [synth.roi_clouds(1, int(n), 100 + i)[0] for i, n in enumerate(sizes)]
    xyz = torch.from_numpy(np.concatenate(cs)).cuda()
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).cuda()
    views = [xyz[int(a):int(b)][None] for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
    res = {}

    def ragged():
        res["ragged"] = pn2_ops.furthest_point_sample_ragged(xyz, offsets, m)

    def loop():
        res["loop"] = [pn2_ops.furthest_point_sample(v, m) for v in views]

    ragged(); loop(); torch.cuda.synchronize()                  # warm-up: code objects loaded, every shape seen
    same = bool(torch.equal(res["ragged"], torch.cat(res["loop"])))
    t = {"ragged": [], "loop": []}
    for _ in range(reps):                                       # alternated, so that a busy neighbour hits both
        t["ragged"] += _events(ragged, 1)
        t["loop"] += _events(loop, 1)
    lines.append("1. furthest point sampling of %d clouds (513-4096 points, median %d, %d points in all), m = %d; device ms between events,"
                 % (clouds, int(np.median(sizes)), int(sizes.sum()), m))
    lines.append("   %d alternated repetitions after a warm-up; the loop also allocates its (1, n) temp and (1, m) output per cloud, as the op does" % reps)
    for k in ("ragged", "loop"):
        lines.append("   %-28s median %8.3f ms   min %8.3f   max %8.3f" % ("one ragged launch" if k == "ragged" else "%d per-cloud launches" % clouds,
                                                                          statistics.median(t[k]), min(t[k]), max(t[k])))
    lines.append("   outputs identical: %s   ratio of medians (loop / ragged): %.1f" % (same, statistics.median(t["loop"]) / statistics.median(t["ragged"])))


def build_times(lines, scans=8):
    scenes = list(gdb.synthetic_scenes(scans))
    kw = dict(easy_min_points=gdb.SYNTHETIC_EASY_MIN_POINTS)
    out = {}
    for name, dev in (("device", torch.device("cuda:0")), ("host", None)):
        gdb.build_gt_database(scenes[:2], device=dev, **kw)     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[name] = gdb.build_gt_database(scenes, device=dev, **kw)
        torch.cuda.synchronize()
        lines.append("2. database build, %d ray-cast scans (%d points each on average), %s route: %.1f ms per scan (host clock, synchronised)"
                     % (scans, int(np.mean([s[1].shape[0] for s in scenes])), name, (time.perf_counter() - t0) * 1e3 / scans))
    easy = [r for r in out["device"] if r["presampling_flag"]]
    lines.append("   %d objects, %d easy (more than %d points; sizes %d-%d), %d hard" % (len(out["device"]), len(easy), gdb.SYNTHETIC_EASY_MIN_POINTS,
                 min(r["points"].shape[0] for r in easy), max(r["points"].shape[0] for r in easy), len(out["device"]) - len(easy)))
    return out["device"], scenes


def paste_times(lines, records, scenes, draws=40):
    db = gdb.GtDatabase(records)
    for mode in ("stored", "draw"):
        rng, py = np.random.RandomState(1), random.Random(1)
        t0 = time.perf_counter()
        for k in range(draws):
            sid, pts, inten, objs = scenes[k % len(scenes)]
            own = np.array([o.pos for o in objs if gdb.keep_object(o)], dtype=np.float32).reshape(-1, 3)
            gt_paste.paste_scene(pts.astype(np.float32), inten, own, db, rng, py, mimic=mode)
        lines.append("3. paste_scene, mimic=%-6s: %.2f ms per scene on the host (%d scenes of ~%d points)"
                     % (mode, (time.perf_counter() - t0) * 1e3 / draws, draws, scenes[0][1].shape[0]))
    return db


def pick_agreement(lines, db, draws=10):
    rng = np.random.RandomState(2)
    same = total = 0
    for r in db.easy:
        for _ in range(draws):
            p, _, _ = losses.scene_augmentation(r["points"], r["gt_box3d"].reshape(-1, 7), rng)
            got = fps_host.furthest_point_sample(np.ascontiguousarray(p[r["sampled_mask"]], dtype=np.float32), db.mimic_points)
            same += int(np.array_equal(got, r["mimic_index"]))
            total += 1
    lines.append("4. per-draw picks equal to the stored picks: %d of %d augmented draws (%d easy objects x %d draws of rotation / scaling / flip)"
                 % (same, total, len(db.easy), draws))


def train_times(lines, db, scenes=32, batch=8, iters=60):
    for workers in (0, 4):
        for paste in (False, True):
            ds = train_rpn.SyntheticCenters(scenes, gt_database=db if paste else None)
            res = train_rpn.train(ds, iters, batch, None, workers=workers)
            torch.cuda.synchronize()
            lines.append("5. train_rpn --synthetic %d --batch_size %d%s --workers %d: median %.1f ms/it over the last %d reports of 10 iterations"
                         % (scenes, batch, " --gt_aug synthetic" if paste else "                    ", workers,
                            statistics.median(res["step_ms"][2:]), len(res["step_ms"][2:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_train", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gt_paste.py needs a HIP device")
    arch = str(getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")).split(":")[0]
    lines = ["ground-truth paste augmentation on %s (%s)" % (torch.cuda.get_device_name(0), arch)]
    ragged_vs_loop(lines)
    records, scenes = build_times(lines)
    db = paste_times(lines, records, scenes)
    pick_agreement(lines, db)
    if not a.skip_train:
        train_times(lines, db)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
