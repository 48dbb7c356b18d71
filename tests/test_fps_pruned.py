"""CPU checks of the pruned furthest point sampling for 16385 .. 65536 points (csrc/fps_pruned.hip): the two entries are exported,
declared and bound; ws3d_fps_workspace_bytes is a pure host function with the documented values; the file compiles for gfx950 with
the library's flags under all three distance conventions, and none of its kernels uses scratch or spills a VGPR."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ws3d_amd", "csrc", "fps_pruned.hip")
ENTRIES = ("ws3d_fps_workspace_bytes", "ws3d_furthest_point_sampling_ws")


@pytest.fixture(scope="module")
def lib():
    from ws3d_amd import build
    handle = ctypes.CDLL(build.build())
    handle.ws3d_fps_workspace_bytes.restype = ctypes.c_size_t
    handle.ws3d_fps_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    return handle


def test_entries_are_exported_declared_and_bound(lib):
    from ws3d_amd import _lib, build
    assert "fps_pruned.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "ws3d_ops.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"WS3D_API\s+[\w\s\*]+?\b%s\s*\(" % name, header), f"{name} is not declared in ws3d_ops.h"
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+WS3D_ABI_VERSION\s+6\b", header)


def test_workspace_bytes_without_a_device(lib):
    f = lib.ws3d_fps_workspace_bytes
    assert f(1, 16384) == 0 and f(8, 16384) == 0 and f(1, 65537) == 0 and f(0, 20000) == 0 and f(-1, 20000) == 0
    for n in (16385, 65536):
        one = f(1, n)
        assert one > 0 and one % 16 == 0
        assert f(8, n) == 8 * one and f(8, n) % 16 == 0
    assert f(3, 20000) == 3 * f(1, 20000)


def _compile(tmp_path, name, extra):
    from ws3d_amd import build
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, *extra, "-c", SRC, "-o", str(tmp_path / (name + ".o"))]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_kernels_use_no_scratch_and_every_distance_mode_compiles(tmp_path):
    procs = [_compile(tmp_path, "dm0", ["-DWS3D_DIST_MODE=0", "-Rpass-analysis=kernel-resource-usage"]),
             _compile(tmp_path, "dm1", ["-DWS3D_DIST_MODE=1", "-Rpass-analysis=kernel-resource-usage"]),
             _compile(tmp_path, "dm2", ["-DWS3D_DIST_MODE=2", "-Rpass-analysis=kernel-resource-usage"])]
    outs = [p.communicate() + (p.returncode,) for p in procs]       # side by side: the test takes as long as one compilation
    for mode, (_, err, rc) in enumerate(outs):
        assert rc == 0, (mode, err)
        report, kernel = {}, None
        for line in err.splitlines():
            m = re.search(r"remark:.*Function Name: (\S+)", line)
            if m:
                kernel = m.group(1)
                report[kernel] = {}
                continue
            m = re.search(r"remark:.*?\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
            if m and kernel:
                report[kernel][m.group(1).strip()] = m.group(2)
        assert len(report) == 2 and all("fps_pruned" in k for k in report), (mode, sorted(report))
        for k, v in report.items():
            assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0, (mode, k, v)
            assert int(v["VGPRs"]) <= 128, (mode, k, v)              # 1024 threads per workgroup: 4 waves per SIMD
