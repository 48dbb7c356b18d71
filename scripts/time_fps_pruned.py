"""Timings of furthest point sampling above 16384 points: the plain entry (fps_big_kernel of csrc/fps.hip) against
ws3d_furthest_point_sampling_ws (the pruned kernels of csrc/fps_pruned.hip) on the same buffers.

    python scripts/time_fps_pruned.py --out profiles/fps_pruned.txt [--prof_lib PATH]

Device time between HIP events, 7 repetitions after a warm-up of both routes, the two routes alternated.  Per row: median (min-max)
of both, us per sample, the part of the _ws entry that does not depend on m (a call with m = 1: the setup kernel, plus the sampling
kernel's bucket records and the scatter of the min-distance buffer), whether idx / temp / new_xyz of the two routes are identical,
and the decision rule of DESIGN.md 5.1c: the pruned kernels are the default of a row's size class only if their median beats the plain
entry's by more than the plain entry's own (max - min) / median.
--prof_lib: a library built with -DWS3D_FPP_PROF (the sampling kernel counts its bucket updates into the workspace): adds the mean
number of surviving buckets per step.  Needs a HIP device: there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ws3d_amd import _lib, synth  # noqa: E402

ROWS = [(65536, 16384, 1), (65536, 16384, 8), (65536, 4096, 8), (32768, 8192, 8), (20000, 4096, 8)]     # (n, m, batch)
REPS = 7


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = fn()
    b.record()
    torch.cuda.synchronize()
    assert rc == 0, rc
    return a.elapsed_time(b)


def row(lib, prof, kind, n, m, batch):
    xyz = torch.from_numpy(np.ascontiguousarray(synth.make_batch(kind, batch, n, 61)[:, :, :3])).cuda()
    st = torch.cuda.current_stream().cuda_stream
    nbytes = int(lib.ws3d_fps_workspace_bytes(batch, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = {}
    for route in ("plain", "ws"):
        out[route] = (torch.empty((batch, n), device="cuda"), torch.empty((batch, m), dtype=torch.int32, device="cuda"),
                      torch.empty((batch, m, 3), device="cuda"))

    def plain():
        t, i, x = out["plain"]
        t.fill_(1e10)
        return lambda: lib.ws3d_furthest_point_sampling_gather(batch, n, m, xyz.data_ptr(), t.data_ptr(), i.data_ptr(), x.data_ptr(), st)

    def pruned(mm=m, handle=lib):
        t, i, x = out["ws"]
        t.fill_(1e10)
        return lambda: handle.ws3d_furthest_point_sampling_ws(batch, n, mm, xyz.data_ptr(), t.data_ptr(), i.data_ptr(), x.data_ptr(), ws.data_ptr(),
                                                              nbytes, st)

    _timed(plain()); _timed(pruned())                        # warm-up: code objects loaded, LDS cap raised
    tp, tw, tf = [], [], []
    for _ in range(REPS):
        tp.append(_timed(plain()))
        tw.append(_timed(pruned()))
    same = all(torch.equal(a, b) for a, b in zip(out["plain"], out["ws"]))
    for _ in range(REPS):
        tf.append(_timed(pruned(1)))
    mp, mw, mf = statistics.median(tp), statistics.median(tw), statistics.median(tf)
    spread = (max(tp) - min(tp)) / mp
    wins = mw < mp * (1.0 - spread)
    text = ("%-5s %5d -> %5d x %d   plain %8.3f (%.3f-%.3f) ms %6.3f us/sample | pruned %8.3f (%.3f-%.3f) ms %6.3f us/sample, m-independent part "
            "%6.3f ms (%4.1f %%) | %5.2fx, plain spread %4.1f %% -> %s | outputs identical: %s"
            % (kind, n, m, batch, mp, min(tp), max(tp), mp * 1e3 / m, mw, min(tw), max(tw), mw * 1e3 / m, mf, 100.0 * mf / mw, mp / mw, 100.0 * spread,
               "pruned" if wins else "plain", same))
    if prof is not None:
        _timed(pruned(m, prof))
        per_scene = nbytes // batch
        upd = sum(int(ws[s * per_scene:s * per_scene + 8].cpu().numpy().view(np.uint64)[0]) for s in range(batch))
        text += " | surviving buckets per step %.2f of %d" % (upd / (batch * max(m - 1, 1)), (n + 63) // 64)
    return text, wins, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--prof_lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fps_pruned.py needs a HIP device")
    lib = _lib.load()
    prof = None
    if a.prof_lib:
        prof = ctypes.CDLL(a.prof_lib)
        prof.ws3d_furthest_point_sampling_ws.restype, prof.ws3d_furthest_point_sampling_ws.argtypes = _lib.SIGNATURES["ws3d_furthest_point_sampling_ws"]
    arch = str(getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")).split(":")[0]
    lines = ["furthest point sampling above 16384 points on %s (%s): plain entry (fps_big_kernel) vs ws3d_furthest_point_sampling_ws (fps_pruned.hip)"
             % (torch.cuda.get_device_name(0), arch),
             "device ms between HIP events, median (min-max) of %d alternated repetitions after a warm-up" % REPS]
    ok, lost = True, []
    for kind in ("hdl64", "lidar"):
        for n, m, batch in ROWS:
            text, wins, same = row(lib, prof, kind, n, m, batch)
            ok = ok and same
            if not wins:
                lost.append("%s %d -> %d x %d" % (kind, n, m, batch))
            lines.append(text)
    lines.append("default route by the rule above: %s" % ("the pruned kernels on every row, so on the whole range 16385-65536" if not lost else
                                                          "the plain entry wins or ties on: " + "; ".join(lost)))
    lines.append("goal (VERDICT.md item 6): 65536 -> 16384 x 8 scenes in <= 30 ms -- see the two x 8 rows")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if not ok:
        raise SystemExit("outputs of the two routes differ")


if __name__ == "__main__":
    main()
