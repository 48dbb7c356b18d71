"""CPU check of ws3d_rpn_heads' resources: csrc/rpn_heads.hip compiled for gfx950 with the library's flags has no spills, no scratch
and keeps two waves per SIMD (the kernel's latency hiding assumes it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rpn_heads_kernel_has_no_spills_and_no_scratch(tmp_path):
    from ws3d_amd import build
    src = os.path.join(ROOT, "ws3d_amd", "csrc", "rpn_heads.hip")
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "rpn_heads.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    report = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
        if m and name:
            report[name][m.group(1).strip()] = m.group(2)
    kernels = [k for k in report if "rpn_heads_kernel" in k]
    assert len(kernels) == 2 and any("pack" in k for k in report), sorted(report)
    for k, v in report.items():
        assert v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0", (k, v)
        assert v["ScratchSize [bytes/lane]"] == "0", (k, v)
    for k in kernels:
        assert int(report[k]["Occupancy [waves/SIMD]"]) >= 2, (k, report[k])
