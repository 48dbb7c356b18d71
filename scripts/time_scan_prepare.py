"""Timings of scan preparation (ws3d_amd.scan_prepare) on the device it is built for.

    python scripts/time_scan_prepare.py --out profiles/scan_prepare.txt

  1. host ``kitti_io.rpn_input_from_scan`` ms per scene on the host this runs on, file reads not counted;
  2. the device route per scene for the same scans: packing + upload (host clock, synchronised) and the two kernels of
     ``ws3d_scan_prepare`` (device ms between events), separately, for a batch of 8; the host restatement next to them;
  3. ``infer_kitti`` scenes/s on a synthetic tree of 64 scans on the three ingest routes with 0 and 8 loader processes.  A run also builds
     the network and primes the pipeline, so each figure comes from the difference between a run over the tree listed four times and a
     run over its first 8 scenes (medians of alternated rounds).  'off' is the driver's unchanged default: the comparison every other line is read against.
Needs a HIP device: there is no fallback, a host timing says nothing about it."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ws3d_amd import infer_kitti, kitti_io, scan_prepare as sp, synth  # noqa: E402

PASSES = 4                          # the driver runs list every scan this often: a fraction of a second measures the scheduler
SIZES = (40000, 60000, 85000)      # the synthetic scan puts 18 % of its points beyond 40 m: larger ones do not fit 16384 rows


def per_scene(lines, cam, reps=7, batch=8):
    calib, shape = cam
    for n in SIZES:
        scans = [synth.velodyne_scan(n, 50 + k) for k in range(batch)]
        keys = list(range(batch))
        rng = np.random.RandomState(666)
        kitti_io.rpn_input_from_scan(scans[0], calib, shape, rng=rng)                     # warm-up
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for s in scans:
                kitti_io.rpn_input_from_scan(s, calib, shape, rng=rng)
            host.append((time.perf_counter() - t0) * 1e3 / batch)
        t0 = time.perf_counter()
        ref = sp.prepare_scans_host(scans, [calib] * batch, [shape] * batch, keys)
        restated = (time.perf_counter() - t0) * 1e3 / batch
        up = sp.upload_packed(sp.pack_scans(scans, [calib] * batch, [shape] * batch, keys), "cuda:0")
        res = sp.launch_packed(up, 16384)                                                # warm-up: code object loaded, LDS cap raised
        torch.cuda.synchronize()
        same = all(np.array_equal(res[k].cpu().numpy(), ref[k]) for k in ref)
        upload, kernel = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            up = sp.upload_packed(sp.pack_scans(scans, [calib] * batch, [shape] * batch, keys), "cuda:0")
            torch.cuda.synchronize()
            upload.append((time.perf_counter() - t0) * 1e3 / batch)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sp.launch_packed(up, 16384)
            b.record()
            torch.cuda.synchronize()
            kernel.append(a.elapsed_time(b) / batch)
        V = ref["valid_count"]
        lines.append("%6d raw points (V %d-%d), batch of %d, ms per scene, median of %d (min-max):" % (n, V.min(), V.max(), batch, reps))
        lines.append("   1. host rpn_input_from_scan          %8.3f (%.3f-%.3f)" % (statistics.median(host), min(host), max(host)))
        lines.append("   2. device: pack + upload             %8.3f (%.3f-%.3f)" % (statistics.median(upload), min(upload), max(upload)))
        lines.append("      device: ws3d_scan_prepare         %8.3f (%.3f-%.3f)" % (statistics.median(kernel), min(kernel), max(kernel)))
        lines.append("      host restatement (one run)        %8.3f   device outputs bit-equal to it: %s" % (restated, same))


def driver_rates(lines, root, rounds=5):
    combos = [(route, w) for w in (0, 8) for route in sp.ROUTES]
    out = tempfile.mkdtemp(prefix="scan_prepare_out")
    infer_kitti.run(root, "warm", out, batch=8)                                           # every code object loaded once
    t = {(c, split): [] for c in combos for split in ("warm", "val")}
    for _ in range(rounds):                                                               # alternated, so that a busy neighbour hits all
        for route, w in combos:
            for split in ("warm", "val"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                infer_kitti.run(root, split, out, batch=8, workers=w, device_ingest=route)
                torch.cuda.synchronize()
                t[((route, w), split)].append(time.perf_counter() - t0)
    lines.append("3. infer_kitti --batch 8 over a tree of 64 scans of %s raw points in turn, listed %d times (%d scenes) and its first 8 scenes;"
                 % ("/".join(str(s) for s in SIZES), PASSES, 64 * PASSES))
    lines.append("   seconds per run, median of %d alternated rounds (min-max); scenes/s = %d / (median long - median short): set-up cancels"
                 % (rounds, 64 * PASSES - 8))
    for c in combos:
        long, short = t[(c, "val")], t[(c, "warm")]
        rate = (64 * PASSES - 8) / max(statistics.median(long) - statistics.median(short), 1e-9)
        lines.append("   --device_ingest %-6s --workers %d: %6.3f (%.3f-%.3f) s, short %6.3f (%.3f-%.3f) s -> %8.1f scenes/s"
                     % (c[0], c[1], statistics.median(long), min(long), max(long), statistics.median(short), min(short), max(short), rate))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_drivers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_scan_prepare.py needs a HIP device")
    arch = str(getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")).split(":")[0]
    lines = ["scan preparation on %s (%s)" % (torch.cuda.get_device_name(0), arch)]
    root = tempfile.mkdtemp(prefix="scan_prepare_tree")
    synth.write_kitti_tree(root, [(i, SIZES[i % len(SIZES)], 100 + i) for i in range(64)])
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("\n".join("%06d" % i for _ in range(PASSES) for i in range(64)) + "\n")
    with open(os.path.join(root, "ImageSets", "warm.txt"), "w") as f:
        f.write("\n".join("%06d" % i for i in range(8)) + "\n")
    ds = kitti_io.KittiScenes(root, "val")
    per_scene(lines, (ds.get_calib(0), ds.get_image_shape(0)))
    if not a.skip_drivers:
        driver_rates(lines, root)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
