#!/usr/bin/env python
"""Achieved error of the Stage-2 box network against the float64 run of the reference's RCNNNet (tests/golden/stage2_forward.*), per
quantity, route (module / channels-last) and mode (IoU tower teacher-forced with the fixture's box_ce / free-running), beside the
bound the tests assert (4 x the reference's own fp32 error): ``python scripts/stage2_parity.py [--out profiles/stage2_parity.txt]``."""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import stage2_reference as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arrays, meta, keys = ref.fixture()
    net = ref.fixture_model(meta, keys)
    lines = ["Stage-2 parity: max |this code - reference float64 run| over the fixture's %d clouds (seed %d), on %s" % (
             arrays["pts"].shape[0], meta["seed"], torch.cuda.get_device_name(0)),
             "bound = 4 x e_ref, e_ref = the reference's own single-thread fp32 run against its float64 run", "",
             "%-14s %-15s %-13s %10s %10s %10s %10s" % ("route", "mode", "quantity", "error", "bound", "e_ref", "max|value|")]
    for fast in (False, True):
        for teacher in (True, False):
            err, same, _ = ref.parity_run(net, arrays, fast, teacher)
            for k in sorted(err):
                lines.append("%-14s %-15s %-13s %10.3g %10.3g %10.3g %10.3g%s" % ("channels-last" if fast else "modules", "teacher-forced" if teacher else "free-running",
                             k, err[k], 4 * meta["e_ref"][k], meta["e_ref"][k], meta["max_abs"][k], "" if err[k] <= 4 * meta["e_ref"][k] else "   ABOVE THE BOUND"))
            lines.append("%-14s %-15s index tensors (6 FPS + 6 ball query), zero pattern of the canonical cloud, centres: %s" % (
                         "channels-last" if fast else "modules", "teacher-forced" if teacher else "free-running",
                         "all equal" if all(same.values()) else "DIFFER: %s" % [k for k, v in same.items() if not v]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
