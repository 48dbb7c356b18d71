"""CPU check of the resources of csrc/stage2_batch.hip compiled for gfx950 with the library's flags: one kernel, no scratch, no VGPR
spills, and the static LDS size its header comment states (512 keys of 8 bytes, a 256-bin histogram, 10 ints)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ws3d_amd", "csrc", "stage2_batch.hip")


def test_stage2_batch_kernel_has_no_scratch_no_spills_and_the_lds_it_states(tmp_path):
    from ws3d_amd import build
    assert "stage2_batch.hip" in build.SOURCES
    with open(SRC) as f:
        stated = re.search(r"^// Static LDS: (\d+) bytes", f.read(), re.M)
    assert stated and int(stated.group(1)) == 512 * 8 + 256 * 4 + 10 * 4 <= 8192
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o",
           str(tmp_path / "stage2_batch.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    report, kernel = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:.*Function Name: (\S+)", line)
        if m:
            kernel = re.match(r"_ZN4ws3d\d+(\w+?_kernel)E", m.group(1)).group(1)
            report[kernel] = {}
            continue
        m = re.search(r"remark:.*?\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
        if m and kernel:
            report[kernel][m.group(1).strip()] = m.group(2)
    assert set(report) == {"stage2_batch_kernel"}, sorted(report)
    v = report["stage2_batch_kernel"]
    assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, v
    assert v["Dynamic Stack"] == "False", v
    assert int(v["LDS Size [bytes/block]"]) == int(stated.group(1)), v
