"""CPU check of ws3d_gemm_rows_split's resources: csrc/gemm_rows.hip compiled for gfx950 with the library's flags has no spills, no
scratch, and its GEMM kernels keep the two waves per SIMD (two workgroups of four waves per CU) the kernel's latency hiding assumes;
the 64-row tiles stay within 128 VGPRs (four waves per SIMD)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_rows_kernels_have_no_spills_no_scratch_and_two_waves_per_simd(tmp_path):
    from ws3d_amd import build
    assert "gemm_rows.hip" in build.SOURCES
    src = os.path.join(ROOT, "ws3d_amd", "csrc", "gemm_rows.hip")
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "gemm_rows.o")]
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
    kernels = [k for k in report if "gemm_rows_kernel" in k]
    assert len(kernels) == 3 and any("pack" in k for k in report), sorted(report)
    for k, v in report.items():
        assert v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0", (k, v)
        assert v["ScratchSize [bytes/lane]"] == "0", (k, v)
    for k in kernels:
        assert int(report[k]["Occupancy [waves/SIMD]"]) >= 2, (k, report[k])
        if "ILi4ELi4E" not in k:          # (the 128-row tile holds four accumulators: 192 VGPRs, two waves per SIMD)
            assert int(report[k]["VGPRs"]) + int(report[k]["AGPRs"]) <= 128, (k, report[k])
