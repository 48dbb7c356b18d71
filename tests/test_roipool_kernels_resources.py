"""CPU check of the resources of csrc/roipool3d.hip compiled for gfx950 with the library's flags: 16 kernels, none with more scratch
or VGPR spills, fewer waves per SIMD or another static LDS size than the file had when its three pooling kernels were written out in
full (profiles/roipool_phases_refactor.txt, the "parent" rows -- the floors are those figures, not the ones of the code under test).
The ablation builds of scripts/ablate_roi.sh, scripts/ablate_roi_scan.sh and scripts/ubench/roi_prof.hip must keep compiling."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ws3d_amd", "csrc", "roipool3d.hip")

# (kernel, template integers) -> (scratch bytes per lane, VGPR spills, waves per SIMD, static LDS bytes)
PARENT = {
    ("roi_bin_kernel", ()): (0, 0, 5, 16704), ("pts_in_boxes3d_kernel", ()): (0, 0, 8, 0),
    ("roipool3d_binned_kernel", (16,)): (0, 0, 8, 6160),
    ("roipool3d_pipe_kernel", (1, 16)): (0, 0, 4, 32), ("roipool3d_pipe_kernel", (1, 32)): (12, 4, 4, 32),
    ("roipool3d_pipe_kernel", (2, 16)): (0, 0, 4, 48), ("roipool3d_pipe_kernel", (2, 32)): (56, 17, 4, 48),
    ("roipool3d_kernel", (4, 32)): (0, 0, 5, 64), ("roipool3d_kernel", (2, 32)): (0, 0, 5, 32), ("roipool3d_kernel", (1, 32)): (0, 0, 8, 16),
    ("roipool3d_kernel", (4, 16)): (0, 0, 5, 64), ("roipool3d_kernel", (2, 16)): (0, 0, 7, 32), ("roipool3d_kernel", (1, 16)): (0, 0, 8, 16),
    ("roipool3d_kernel", (4, 0)): (0, 0, 4, 64), ("roipool3d_kernel", (2, 0)): (0, 0, 5, 32), ("roipool3d_kernel", (1, 0)): (0, 0, 8, 16),
}
ABLATIONS = [["-DWS3D_ROI_NO_SCAN"], ["-DWS3D_ROI_NO_COPY"], ["-DWS3D_ROI_NO_COPY", "-DWS3D_ROI_SCAN_ABL=1"],
             ["-DWS3D_ROI_NO_COPY", "-DWS3D_ROI_SCAN_ABL=2"], ["-DWS3D_ROI_PROF"]]


def _compile(tmp_path, name, extra):
    from ws3d_amd import build
    assert "roipool3d.hip" in build.SOURCES
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, *extra, "-c", SRC, "-o", str(tmp_path / (name + ".o"))]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _kernel_key(mangled):
    """_ZN4ws3d16roipool3d_kernelILi4ELi32EEEv... -> ("roipool3d_kernel", (4, 32))"""
    m = re.match(r"_ZN4ws3d\d+(\w+?_kernel)(?:I((?:Li\d+E)+)E)?(?:E|v)", mangled)
    assert m, mangled
    return m.group(1), tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(2) or ""))


def test_roipool_kernels_keep_the_parents_resources_and_the_ablations_compile(tmp_path):
    procs = [_compile(tmp_path, "lib", ["-Rpass-analysis=kernel-resource-usage"])] + [_compile(tmp_path, f"abl{i}", d) for i, d in enumerate(ABLATIONS)]
    outs = [p.communicate() + (p.returncode,) for p in procs]       # side by side: the test takes as long as one compilation
    for defs, (_, err, rc) in zip([[]] + ABLATIONS, outs):
        assert rc == 0, (defs, err)
    report = {}
    kernel = None
    for line in outs[0][1].splitlines():
        m = re.search(r"remark:.*Function Name: (\S+)", line)
        if m:
            kernel = _kernel_key(m.group(1))
            report[kernel] = {}
            continue
        m = re.search(r"remark:.*?\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
        if m and kernel:
            report[kernel][m.group(1).strip()] = m.group(2)
    assert len(report) == 16 and set(report) == set(PARENT), sorted(set(report) ^ set(PARENT))
    for k, (scratch, vspill, occ, lds) in PARENT.items():
        v = report[k]
        assert int(v["ScratchSize [bytes/lane]"]) <= scratch and int(v["VGPRs Spill"]) <= vspill, (k, v)
        assert int(v["Occupancy [waves/SIMD]"]) >= occ, (k, v)
        assert int(v["LDS Size [bytes/block]"]) == lds, (k, v)
