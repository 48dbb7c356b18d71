"""CPU check of which roipool3d kernel every tested (environment, shape) pair launches: ws3d_roipool3d_plan is the launcher's own
decision (csrc/roipool3d.hip roi_plan) without the launch.  The variants of tests/test_gpu_parity.py's
test_roipool3d_kernel_variants_subprocess and the default-environment shapes of test_roipool3d_bit_exact together must reach every
pooling instantiation of the file -- a variant list that names a kernel the launcher never takes fails here, without a GPU."""
import json
import os
import subprocess
import sys

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 1000 * family + 100 * G + CR: roipool3d_kernel<BG, CR> (9), roipool3d_pipe_kernel<SG, CR> (4), roipool3d_binned_kernel<16>
INSTANTIATIONS = {100 * g + cr for g in (1, 2, 4) for cr in (0, 16, 32)} | {1000 + 100 * sg + cr for sg in (1, 2) for cr in (16, 32)} | {2116}

# one child process per environment (the knobs are read once per process); the workspace size is the one compat._roipool3d passes
CHILD = """
import json, sys
sys.path.insert(0, %r)
from ws3d_amd import _lib
lib = _lib.load()
shapes = json.loads(sys.argv[1])
print(json.dumps([lib.ws3d_roipool3d_plan(B, N, M, C, S, 1, lib.ws3d_roipool3d_workspace_bytes(B, N)) for B, N, M, C, S in shapes]))
""" % ROOT


def _plans(jobs):
    """[(env, shapes)] -> [plans], the children running side by side"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("WS3D_ROI_")}
    procs = [subprocess.Popen([sys.executable, "-B", "-c", CHILD, json.dumps(shapes)], env=dict(base, **env), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for env, shapes in jobs]
    out = []
    for p in procs:
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, se[-2000:]
        out.append(json.loads(so.strip().splitlines()[-1]))
    return out


def test_the_tested_variants_reach_every_pooling_kernel():
    cases = [list(c) for c in H.ROI_VARIANT_CASES]
    jobs = [(env, cases) for env in H.ROI_ENV_VARIANTS] + [({}, [list(c[:5]) for c in H.ROI_BIT_EXACT_CASES])]
    plans = _plans(jobs)
    assert all(p > 0 for ps in plans for p in ps), plans
    assert {p for ps in plans for p in ps} == INSTANTIATIONS, sorted({p for ps in plans for p in ps} ^ INSTANTIATIONS)
    # the variants meant for the pipe kernel reach it on every scene it covers
    assert len(H.ROI_PIPE_VARIANTS) == 4
    for env, ps in zip(H.ROI_ENV_VARIANTS, plans):
        if env not in H.ROI_PIPE_VARIANTS:
            continue
        sg, cr = int(env["WS3D_ROI_PIPE"]), int(env.get("WS3D_ROI_STAGE", 16))
        covered = [p for (B, N, M, C, S), p in zip(H.ROI_VARIANT_CASES, ps) if N >= 16384 and S % 4 == 0]
        assert len(covered) >= 5 and all(p == 1000 + 100 * sg + cr for p in covered), (env, ps)


def test_the_plan_refuses_what_the_launcher_refuses():
    (ps,) = _plans([({}, [[1, 1000, 5, 1, 0], [-1, 1000, 5, 1, 8], [0, 1000, 5, 1, 8], [1, 1000, 0, 1, 8], [1, 1000, 5, 1, 40000], [65536, 64, 1, 4, 8]])])
    assert ps == [-1, -1, 0, 0, -4, -4]         # WS3D_E_INVALID, nothing to launch, WS3D_E_UNSUPPORTED (LDS, batch)
