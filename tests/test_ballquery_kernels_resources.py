"""CPU check of the resources of csrc/ballquery_group.hip compiled for gfx950 with the library's flags: 20 kernels, none with more
scratch or VGPR spills, fewer waves per SIMD or another static LDS size than the file had when its four generations of search kernel
were written out in full (profiles/ballquery_phases_refactor.txt, the "parent" rows -- the floors are those figures, not the ones of
the code under test).  The ablation and tuning builds of scripts/ablate_bq.sh, scripts/r06/bq_variants.sh, scripts/r06/bq_variants2.sh
(its switches arrive as arguments: the ones profiles/ and the kernel comments name) and scripts/ubench/bq_wide_threshold.sh must keep
compiling."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ws3d_amd", "csrc", "ballquery_group.hip")

# (kernel, template arguments as mangled) -> (scratch bytes per lane, VGPR spills, waves per SIMD, static LDS bytes)
PARENT = {
    ("bin_points_x_kernel", ""): (0, 0, 8, 8384), ("bin_points_grid_kernel", ""): (92, 22, 4, 69952),
    ("bin_points_jobs_kernel", ""): (88, 21, 4, 78464),
    ("group_points_kernel", ""): (0, 0, 8, 0), ("group_points_vec4_kernel", ""): (0, 0, 8, 0), ("group_points_lds_kernel", ""): (0, 0, 8, 0),
    ("group_points_grad_kernel", ""): (0, 0, 8, 0),
    ("ball_query_kernel", "tLb0E"): (0, 0, 8, 0), ("ball_query_kernel", "tLb1E"): (0, 0, 8, 0),               # <uint16_t, FUSED>
    ("ball_query_kernel", "iLb0E"): (0, 0, 8, 0), ("ball_query_kernel", "iLb1E"): (0, 0, 8, 0),               # <int32_t, FUSED>
    ("ball_query_sorted_kernel", "Lb0E"): (0, 0, 8, 0), ("ball_query_sorted_kernel", "Lb1E"): (0, 0, 8, 0),
    ("ball_query_grid_kernel", "Lb0E"): (0, 0, 8, 0), ("ball_query_grid_kernel", "Lb1E"): (0, 0, 8, 0),
    ("ball_query_grid_coop_kernel", "Lb0ELi4E"): (0, 0, 5, 0), ("ball_query_grid_coop_kernel", "Lb0ELi8E"): (0, 0, 8, 0),
    ("ball_query_grid_coop_kernel", "Lb0ELi16E"): (0, 0, 8, 0),
    ("ball_query_grid_coop_kernel", "Lb1ELi4E"): (0, 0, 5, 0), ("ball_query_grid_coop_kernel", "Lb1ELi16E"): (0, 0, 8, 0),
}
ABLATIONS = [
    # scripts/ablate_bq.sh
    ["-DWS3D_BQS_NO_SEARCH", "-DWS3D_BQG_NO_SEARCH"], ["-DWS3D_BQS_NO_EMIT", "-DWS3D_BQG_NO_EMIT"], ["-DWS3D_BQS_PACKED_ABL", "-DWS3D_BQG_PACKED_ABL"],
    # scripts/r06/bq_variants.sh (its -DBQC_LARGE_NW=2 has not compiled since the search deals one lane per (centre, row): 32 centres x 4 rows)
    ["-DWS3D_BQ_NO_NT"], ["-DBQC_LARGE_NW=8"], ["-DBQC_LARGE_NW=16"], ["-DWS3D_BQC_NO_SEARCH"], ["-DWS3D_BQC_NO_EMIT"],
    ["-DWS3D_BQC_NO_SEARCH", "-DWS3D_BQ_NO_NT"],
    # scripts/r06/bq_variants2.sh, scripts/r06/bq_c3_ab.sh
    ["-DWS3D_BQC_NO_SEARCH2"], ["-DWS3D_BQC_NO_BATCH"], ["-DWS3D_BQC_EXTRA_LDS=8192", "-DBQC_FUSED_WPE=2"], ["-DBQC_ROWS_PER_BATCH=8", "-DBQC_LARGE_NW=8"],
    ["-DWS3D_BQG_ALL_PAD"], ["-DWS3D_BQG_NO_IDS"], ["-DBQC_HCAP=512", "-DBQS_UNROLL=4"],
    # scripts/ubench/bq_wide_threshold.sh
    ["-DBQC_WIDE_BELOW=2000000000"],
]


def _compile(tmp_path, name, extra):
    from ws3d_amd import build
    assert "ballquery_group.hip" in build.SOURCES
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-DWS3D_DIST_MODE=0", *extra, "-c", SRC, "-o", str(tmp_path / (name + ".o"))]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _kernel_key(mangled):
    """_ZN4ws3d27ball_query_grid_coop_kernelILb0ELi16EEEviiii... -> ("ball_query_grid_coop_kernel", "Lb0ELi16E")"""
    m = re.match(r"_ZN4ws3d\d+(\w+?_kernel)(?:I(\w+?)E(?=Ev))?", mangled)
    assert m, mangled
    return m.group(1), m.group(2) or ""


def test_ballquery_kernels_keep_the_parents_resources_and_the_ablations_compile(tmp_path):
    procs = [_compile(tmp_path, "lib", ["-Rpass-analysis=kernel-resource-usage"])] + [_compile(tmp_path, f"abl{i}", d) for i, d in enumerate(ABLATIONS)]
    outs = [p.communicate() + (p.returncode,) for p in procs]       # side by side: the test takes about as long as one compilation
    for defs, (_, err, rc) in zip([[]] + ABLATIONS, outs):
        assert rc == 0, (defs, err[-3000:])
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
    assert len(report) == 20 and set(report) == set(PARENT), sorted(set(report) ^ set(PARENT))
    for k, (scratch, vspill, occ, lds) in PARENT.items():
        v = report[k]
        assert int(v["ScratchSize [bytes/lane]"]) <= scratch and int(v["VGPRs Spill"]) <= vspill, (k, v)
        assert int(v["Occupancy [waves/SIMD]"]) >= occ, (k, v)
        assert int(v["LDS Size [bytes/block]"]) == lds, (k, v)
