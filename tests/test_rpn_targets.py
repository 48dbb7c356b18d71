"""CPU checks of the device route to the Stage-1 targets and loss (csrc/rpn_targets.hip): the three entry points are declared,
exported, bound and validate their arguments before any HIP call; the Python surface falls back to the host functions off the GPU; the
label-free datasets and the padding collate; and the kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ws3d_rpn_center_labels", "ws3d_rpn_loss_workspace_bytes", "ws3d_rpn_loss")


@pytest.fixture(scope="module")
def lib():
    from ws3d_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from ws3d_amd import _lib, build, compat
    header = open(os.path.join(ROOT, "include", "ws3d_ops.h")).read()
    assert "rpn_targets.hip" in build.SOURCES
    for name in NAMES:
        assert re.search(r"WS3D_API\s+[\w\s\*]+?\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for cite in ("kitti_rcnn_dataset.py:529-573", "train_functions.py:163-228", "loss_utils.py:25-156"):
        assert cite in header, cite
    assert callable(compat.rpn_center_labels) and callable(compat.rpn_loss)
    assert _lib.ABI_VERSION == 6 == lib.ws3d_abi_version()
    # a slot per 128 rows and per 4096 rows: grows with the rows, never zero
    assert 0 < lib.ws3d_rpn_loss_workspace_bytes(0) <= lib.ws3d_rpn_loss_workspace_bytes(1) < lib.ws3d_rpn_loss_workspace_bytes(131072)
    assert lib.ws3d_rpn_loss_workspace_bytes(131072) >= (131072 // 128) * 7 * 8


def test_invalid_arguments_are_refused_before_any_hip_call(lib):
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int32 * 4)()
    p, ip = ctypes.addressof(buf), ctypes.addressof(ibuf)

    def loss(rows, bins, ptrs=(p,) * 4, outs=(p, ip, p, p), ws=p, ws_bytes=1 << 20):
        return lib.ws3d_rpn_loss(rows, bins, 4.0, 0.8, 0.25, 2.0, 1.0, 1.0, *ptrs, *outs, ws, ws_bytes, None)

    assert loss(-1, 10) == -1 and b"invalid" in lib.ws3d_last_error()
    assert loss(1, 0) == -1 and loss(1, -3) == -1 and loss(1, 33) == -1
    for k in range(4):
        assert loss(1, 10, ptrs=tuple(None if j == k else p for j in range(4))) == -1
        assert loss(1, 10, outs=tuple(None if j == k else q for j, q in enumerate((p, ip, p, p)))) == -1
    assert loss(1, 10, ws=None) == -1
    assert loss(0, 10, ptrs=(None,) * 4, outs=(None,) * 4, ws=None, ws_bytes=0) == 0      # no rows: nothing to do

    def labels(batch, n, kmax, stride=4, pts=p, centres=p, count=ip, cls=p, reg=p):
        return lib.ws3d_rpn_center_labels(batch, n, kmax, stride, 0.707, 0.7, 1.5, pts, centres, count, cls, reg, None)

    assert labels(-1, 4, 1) == -1 and b"invalid" in lib.ws3d_last_error()
    assert labels(1, -4, 1) == -1 and labels(1, 4, -1) == -1 and labels(1, 4, 1, stride=2) == -1
    for name in ("pts", "centres", "count", "cls", "reg"):
        assert labels(1, 4, 1, **{name: None}) == -1, name
    assert labels(0, 4, 1, pts=None, centres=None, count=None, cls=None, reg=None) == 0   # no scene: nothing to do


def _scenes(counts, n, seed):
    from ws3d_amd import synth
    rng = np.random.default_rng(seed)
    pts = np.stack([synth.lidar_cloud(n, seed + b) for b in range(len(counts))]).astype(np.float32)
    kmax = max(max(counts), 1)
    centres = rng.uniform(-40, 40, (len(counts), kmax, 3)).astype(np.float32)     # the padding holds plausible centres: it must be ignored
    for b, k in enumerate(counts):
        if k:
            centres[b, :k, [0, 2]] = pts[b, rng.integers(0, n, k)][:, [0, 2]].T + rng.normal(0, 1.0, (2, k)).astype(np.float32)
    return pts, centres, np.asarray(counts, dtype=np.int32)


def test_center_labels_batch_on_cpu_is_the_per_scene_function():
    from ws3d_amd import losses
    pts, centres, count = _scenes([3, 0, 7], 500, 11)
    cls, reg = losses.center_labels_batch(torch.from_numpy(pts), torch.from_numpy(centres), torch.from_numpy(count))
    assert cls.dtype == torch.float32 and tuple(cls.shape) == (3, 500) and tuple(reg.shape) == (3, 500, 3)
    for b in range(3):
        want_cls, want_reg = losses.gaussian_center_labels(pts[b, :, :3], centres[b, :count[b]])
        assert np.array_equal(cls[b].numpy(), want_cls.astype(np.float32)) and np.array_equal(reg[b].numpy(), want_reg)
    assert float(cls[1].abs().max()) == 0.0 and float(reg[1].abs().max()) == 0.0 and float(cls[0].max()) > 0.5


def test_rpn_loss_fused_on_cpu_is_rpn_loss():
    from ws3d_amd import losses
    pts, centres, count = _scenes([4, 2], 300, 5)
    cls, reg = losses.center_labels_batch(torch.from_numpy(pts), torch.from_numpy(centres), torch.from_numpy(count))
    g = torch.Generator().manual_seed(3)
    outs = []
    for fn in (losses.rpn_loss_fused, lambda *a: losses.rpn_loss(*a, lazy=True)):
        rpn_cls = torch.randn((2, 300, 1), generator=g.manual_seed(3)).requires_grad_(True)
        rpn_reg = torch.randn((2, 300, 40), generator=g).requires_grad_(True)
        loss, tb = fn(rpn_cls, rpn_reg, cls, reg, 4.0, 0.8)
        loss.backward()
        outs.append((loss.detach(), losses.resolve_scalars(dict(tb)), rpn_cls.grad, rpn_reg.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][1]["rpn_fg_sum"] > 0
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])
    assert set(outs[0][1]) == {"rpn_loss_cls_pos", "rpn_loss_cls_neg", "rpn_loss_cls", "rpn_loss_reg", "rpn_loss", "rpn_fg_sum"}


def test_label_free_datasets_and_the_padding_collate():
    from ws3d_amd import train_rpn
    with_labels = train_rpn.SyntheticCenters(6, npoints=256)
    without = train_rpn.SyntheticCenters(6, npoints=256, labels=False)
    item = without[2]
    assert set(item) == {"sample_id", "pts_input", "gt_centers"}
    assert np.array_equal(item["pts_input"], with_labels[2]["pts_input"]) and np.array_equal(item["gt_centers"], with_labels[2]["gt_centers"])
    # augmentation draws from the same stream whether or not labels are made
    aug = [train_rpn.SyntheticCenters(6, npoints=256, augment=True, rng=np.random.RandomState(4), labels=flag) for flag in (True, False)]
    for i in (1, 4):
        a, b = aug[0][i], aug[1][i]
        assert np.array_equal(a["pts_input"], b["pts_input"]) and np.array_equal(a["gt_centers"], b["gt_centers"]) and "rpn_cls_label" not in b

    # batch composition at one seed: the same scenes in the same order
    ids = []
    for ds, collate in ((with_labels, train_rpn._collate), (without, train_rpn._collate_centers)):
        src = train_rpn.batches(ds, 2, np.random.RandomState(9), collate=collate)
        ids.append([next(src) for _ in range(4)])
        src.close()
    assert [b["sample_id"] for b in ids[0]] == [b["sample_id"] for b in ids[1]]
    for a, b in zip(*ids):
        assert np.array_equal(a["pts_input"], b["pts_input"])
        assert tuple(b["gt_centers"].shape) == (2, 15, 3) and b["gt_count"].dtype == np.int32 and b["gt_count"].tolist() == [15, 15]
        assert "rpn_cls_label" not in b

    # ragged counts, a scene without any centre, and a batch without any
    def scene(sid, k):
        return {"sample_id": sid, "pts_input": np.full((8, 4), sid, np.float32), "gt_centers": np.arange(3 * k, dtype=np.float32).reshape(k, 3) + 1}

    b = train_rpn._collate_centers([scene(0, 2), scene(1, 0), scene(2, 3)])
    assert tuple(b["gt_centers"].shape) == (3, 3, 3) and b["gt_count"].tolist() == [2, 0, 3] and tuple(b["pts_input"].shape) == (3, 8, 4)
    assert np.array_equal(b["gt_centers"][0, :2], scene(0, 2)["gt_centers"]) and not b["gt_centers"][0, 2:].any() and not b["gt_centers"][1].any()
    e = train_rpn._collate_centers([scene(0, 0), scene(1, 0)])
    assert tuple(e["gt_centers"].shape) == (2, 0, 3) and e["gt_count"].tolist() == [0, 0]
    out = train_rpn.device_labels(e, "cpu")
    assert tuple(out["rpn_cls_label"].shape) == (2, 8) and not out["rpn_cls_label"].any() and not out["rpn_reg_label"].any()
    out = train_rpn.device_labels(b, "cpu")
    assert tuple(out["rpn_reg_label"].shape) == (3, 8, 3) and out["pts_input"].dtype == torch.float32


def test_rpn_targets_kernels_have_no_spills_and_no_scratch(tmp_path):
    from ws3d_amd import build
    src = os.path.join(ROOT, "ws3d_amd", "csrc", "rpn_targets.hip")
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "rpn_targets.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    report, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
        if m and name:
            report[name][m.group(1).strip()] = m.group(2)
    for want in ("rpn_center_labels_kernel", "rpn_loss_counts_kernel", "rpn_loss_rows_kernel", "rpn_loss_fold_kernel"):
        assert sum(want in k for k in report) == 1, (want, sorted(report))
    assert len(report) == 4, sorted(report)
    for k, v in report.items():
        assert v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0", (k, v)
        assert v["ScratchSize [bytes/lane]"] == "0", (k, v)
        assert int(v["Occupancy [waves/SIMD]"]) >= 4, (k, v)      # element-wise kernels: latency is hidden by waves in flight
