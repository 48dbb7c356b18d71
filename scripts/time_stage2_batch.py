"""Where a Stage-2 training batch comes from and what it costs: the host route (``BoxDataset.sample`` x batch, ``collate``,
``prepare_batch``) against the device route (``stage2_batch``: parameter blocks on the host, one upload, one launch).

    python scripts/time_stage2_batch.py --out profiles/stage2_batch.txt [--batch 800] [--records 256] [--train_runs 3] [--train_iters 8]

One GPU, at most 16 host threads.  Records: ``SyntheticBoxes`` with 640 points (batch / 4 of them for the per-batch figures, so
that every batch is full), phase rcnn.  Host figures: wall clock, median of `--reps` batches after one warm-up.  Device figure: HIP events around upload + launch, median of 30 after 5 warm-ups.  Training:
``python -m ws3d_amd.train_rcnn --synthetic 256 --batch_size 800`` in child processes, ``--device_batches off`` and ``device`` in
turn, seconds per iteration as the driver logs them (batch preparation included), the first two iterations of a run left out.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def train_run(route, args):
    cmd = [sys.executable, "-m", "ws3d_amd.train_rcnn", "--synthetic", str(args.records), "--batch_size", str(args.batch), "--phase", "rcnn",
           "--total_iters", str(args.train_iters), "--device_batches", route]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, check=True, timeout=600).stdout
    secs = [float(m.group(1)) for m in re.finditer(r"^it \d+/\d+ .* (\d+\.\d+) s$", out, re.M)]
    assert len(secs) == args.train_iters, out[-2000:]
    return statistics.median(secs[2:])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=800)
    ap.add_argument("--records", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train_runs", type=int, default=3, help="runs per route, alternated; 0 skips the training comparison")
    ap.add_argument("--train_iters", type=int, default=8)
    a = ap.parse_args()

    import torch
    from ws3d_amd import stage2_batch as sb, train_rcnn as t2
    dev = torch.device("cuda:0")
    lines = ["Stage-2 batch preparation: batch %d, %d SyntheticBoxes records of 640 points, phase rcnn, %s, %d host threads"
             % (a.batch, a.batch // 4, torch.cuda.get_device_name(0), torch.get_num_threads())]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # batch / 4 records: an epoch (every record under its four aug_flags) is exactly one batch, so every timed batch has `batch` samples
    source = t2.SyntheticBoxes(a.batch // 4)
    for workers in (0, 8):
        ds = t2.BoxDataset(source, "TRAIN", 0, "rcnn")
        stream = t2.batches(ds, a.batch, workers)

        def host_route():
            d = t2.prepare_batch(next(stream), dev)
            torch.cuda.synchronize()
            return d
        say("host route, batches(workers=%d) + prepare_batch:   median %8.2f ms per batch  (min %.2f, max %.2f)" % ((workers,) + median_ms(host_route, a.reps)))
        stream.close()

    ds = t2.BoxDataset(source, "TRAIN", 0, "rcnn")
    plan = sb.batch_plan(ds, a.batch)
    ids, seeds = next(plan)
    say("host twin, prepare_boxes_host:                      median %8.2f ms per batch  (min %.2f, max %.2f)"
        % median_ms(lambda: sb.prepare_boxes_host(ds, ids, seeds), a.reps))
    say("device route, parameter blocks on the host:         median %8.2f ms per batch  (min %.2f, max %.2f)"
        % median_ms(lambda: sb.param_blocks(ds, ids, seeds), a.reps))

    boxes = sb.DeviceBoxes(ds, dev)
    blocks, plans = sb.param_blocks(ds, ids, seeds)
    host = sb._collate_plans(plans)
    times = []
    for rep in range(35):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sb.launch_blocks(boxes, blocks, host)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 5:
            times.append(e0.elapsed_time(e1))
    say("device route, upload + kernel (HIP events):         median %8.3f ms per batch  (min %.3f, max %.3f; 30 after 5 warm-ups)"
        % (statistics.median(times), min(times), max(times)))

    def device_route():
        i, s = next(plan)
        d = sb.prepare_boxes(boxes, i, s)
        torch.cuda.synchronize()
        return d
    say("device route, prepare_boxes end to end:             median %8.2f ms per batch  (min %.2f, max %.2f)" % median_ms(device_route, a.reps))
    want, got = sb.prepare_boxes_host(ds, ids, seeds), sb.prepare_boxes(boxes, ids, seeds)
    same = all(np.array_equal(want[k], got[k].cpu().numpy()) for k in ("cur_box_point", "cur_box_reflect", "train_mask", "gt_boxes", "cls"))
    say("device route against the host twin on that batch:   %s" % ("bit-equal" if same else "DIFFERENT"))
    del boxes
    torch.cuda.empty_cache()

    if a.train_runs > 0:
        say("training, %d runs per route in turn, %d iterations each, the first two left out (an epoch is %d samples: batches of %s alternate on both routes)"
            % (a.train_runs, a.train_iters, 4 * a.records, " and ".join(str(v) for v in sorted({min(a.batch, 4 * a.records - i) for i in range(0, 4 * a.records, a.batch)}, reverse=True))))
        res = {"off": [], "device": []}
        for _ in range(a.train_runs):
            for route in ("off", "device"):
                res[route].append(train_run(route, a))
        for route in ("off", "device"):
            say("train_rcnn --synthetic %d --batch_size %d --device_batches %-6s  median %.3f s per iteration  (runs: %s; spread %.3f)"
                % (a.records, a.batch, route, statistics.median(res[route]), " ".join("%.3f" % v for v in res[route]), max(res[route]) - min(res[route])))
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
