"""CPU check of the resources of the register-chained kernels: csrc/sa_mlp.hip (SA1's SharedMLP chain in its three forms, the VALU
kernel, the two-layer row kernel) and csrc/rpn_heads.hip compiled for gfx950 with the library's flags have no spills, no scratch,
and no kernel runs at fewer waves per SIMD than it did before the three SA1 chains and the two split-bf16 files were built from
shared cores.  The floors are the figures of the files as they were written out in full (profiles/chain_cores_refactor.txt, the
"parent" rows), not of the code under test."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kernel, leading template integers) -> waves per SIMD.  The SA1 kernels are keyed by their widths <C1, C2, C3> (either nsample),
# mlp2_rows_kernel and rpn_heads_kernel by their 32-column blocks.
FLOORS = {
    "sa_mlp.hip": {
        ("sa_mlp3_pool_mfma_kernel", (32, 32, 64)): 3, ("sa_mlp3_pool_mfma_kernel", (16, 16, 32)): 6,
        ("sa_mlp3_compact_mfma_kernel", (32, 32, 64)): 2, ("sa_mlp3_compact_mfma_kernel", (16, 16, 32)): 4,
        ("sa_mlp3_lists_mfma_kernel", (32, 32, 64)): 3, ("sa_mlp3_lists_mfma_kernel", (16, 16, 32)): 5,
        ("mlp2_rows_kernel", (1,)): 3, ("mlp2_rows_kernel", (2,)): 2,
        ("sa_mlp3_pool_kernel", (32, 32, 64)): 6, ("sa_mlp3_pool_kernel", (16, 16, 32)): 8,
    },
    "rpn_heads.hip": {("rpn_heads_kernel", (1,)): 2, ("rpn_heads_kernel", (2,)): 2, ("rpn_heads_pack_kernel", ()): 8},
}
KERNELS = {"sa_mlp.hip": 16, "rpn_heads.hip": 3}      # instantiations: 4 + 2 + 4 of the three chains, 4 VALU, 2 row kernels; 2 + pack


def _kernel_key(mangled):
    """_ZN4ws3d16mlp2_rows_kernelILi1EEEv... -> ("mlp2_rows_kernel", (1,))"""
    m = re.match(r"_ZN4ws3d\d+(\w+?_kernel)(?:I((?:Li\d+E)+)E)?E", mangled)
    assert m, mangled
    return m.group(1), tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(2) or ""))


@pytest.mark.parametrize("name", sorted(FLOORS))
def test_chain_kernels_have_no_spills_no_scratch_and_keep_their_occupancy(tmp_path, name):
    from ws3d_amd import build
    assert name in build.SOURCES
    src = os.path.join(ROOT, "ws3d_amd", "csrc", name)
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / (name + ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    report = {}
    kernel = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:.*Function Name: (\S+)", line)
        if m:
            kernel = m.group(1)
            report[kernel] = {}
            continue
        m = re.search(r"remark:.*?\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
        if m and kernel:
            report[kernel][m.group(1).strip()] = m.group(2)
    assert len(report) == KERNELS[name], sorted(report)
    floors = FLOORS[name]
    seen = set()
    for k, v in report.items():
        assert v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0", (k, v)
        assert v["ScratchSize [bytes/lane]"] == "0", (k, v)
        base, ints = _kernel_key(k)
        key = next((f for f in floors if f[0] == base and ints[:len(f[1])] == f[1]), None)
        assert key is not None, ("no floor recorded for", k)
        seen.add(key)
        assert int(v["Occupancy [waves/SIMD]"]) >= floors[key], (k, v, floors[key])
    assert seen == set(floors), set(floors) - seen
