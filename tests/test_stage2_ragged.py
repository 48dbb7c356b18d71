"""CPU checks of Stage 2 on whole instance clouds: the three entries of csrc/stage2_ragged.hip are declared, bound and built, the
file's kernels compile to what its comments claim, and ``detect_kitti.rcnn_over_real_clouds_ragged`` puts every cloud's rows into
its own (scene, slot) and never lets a dropped slot through ``stage2.detections``."""
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ws3d_stage2_canonical_ragged", "ws3d_furthest_point_sampling_ragged_gather", "ws3d_ball_query_ragged")


def test_entries_are_declared_bound_exported_and_built():
    from ws3d_amd import _lib, build, compat, pn2_ops
    hdr = open(os.path.join(ROOT, "include", "ws3d_ops.h")).read()
    assert "#define WS3D_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6          # additive: the version stays
    assert "stage2_ragged.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "ws3d_amd", "csrc", "stage2_ragged.hip")).read()
    exports = open(os.path.join(ROOT, "ws3d_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ws3d_\*;", exports)                               # the map exports the whole ws3d_ prefix
    for name in ENTRIES:
        assert re.search(r"WS3D_API int %s\(" % name, hdr), name
        assert re.search(r'extern "C" int %s\(' % name, src), name
        assert name in _lib.SIGNATURES and name.startswith("ws3d_"), name
        n_args = len(re.search(r"WS3D_API int %s\(([^;]*)\);" % name, hdr).group(1).split(","))
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    for fn in ("stage2_canonical_ragged", "furthest_point_sampling_ragged_gather", "ball_query_ragged"):
        assert callable(getattr(compat, fn))
    assert callable(pn2_ops.furthest_point_sample_gather_ragged) and callable(pn2_ops.ball_query_ragged)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in ENTRIES:
            assert hasattr(lib, name)
        # host-side validation needs no device: nothing to do, and an nsample the kernel does not hold
        assert lib.ws3d_ball_query_ragged(0, None, 128, 0.2, 64, None, None, 0, None, None) == 0
        assert lib.ws3d_ball_query_ragged(0, None, 128, 0.2, 65, None, None, 0, None, None) == _lib.E_UNSUPPORTED
        assert lib.ws3d_furthest_point_sampling_ragged_gather(0, None, None, 8, None, None, None, None) == 0
        assert lib.ws3d_stage2_canonical_ragged(0, 0, None, None, None, 1.2, None, None) == 0


def test_the_old_file_keeps_its_kernel():
    """the shared device code moved into fps_ragged.h; fps_ragged.hip still holds fps_ragged_kernel, its entry and its n < m gate"""
    text = open(os.path.join(ROOT, "ws3d_amd", "csrc", "fps_ragged.hip")).read()
    assert '#include "fps_ragged.h"' in text and "void fps_ragged_kernel(" in text and "n < m" in text
    assert "ragged_cloud(" in open(os.path.join(ROOT, "ws3d_amd", "csrc", "fps_ragged.h")).read()


def test_kernels_have_no_spills_no_scratch_and_the_claimed_figures(tmp_path):
    from ws3d_amd import build
    src = os.path.join(ROOT, "ws3d_amd", "csrc", "stage2_ragged.hip")
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "stage2_ragged.o")]
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
    kernels = {"canonical": "stage2_canonical_ragged_kernel", "fps": "fps_ragged_gather_kernel", "bq": "ball_query_ragged_kernel"}
    assert len(report) == 3 and all(any(v in k for k in report) for v in kernels.values()), sorted(report)
    by = {short: next(v for k, v in report.items() if full in k) for short, full in kernels.items()}
    for k, v in by.items():
        assert v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0" and v["ScratchSize [bytes/lane]"] == "0", (k, v)
    text = open(src).read()
    assert "16,400 bytes" in text and (3 * 1024 + 16 * 64 + 4) * 4 == 16400
    assert int(by["bq"]["LDS Size [bytes/block]"]) == 16400 and int(by["fps"]["LDS Size [bytes/block]"]) == 640
    assert int(by["canonical"]["LDS Size [bytes/block]"]) == 0
    assert int(by["bq"]["Occupancy [waves/SIMD]"]) >= 8 and int(by["canonical"]["Occupancy [waves/SIMD]"]) >= 8
    assert int(by["fps"]["Occupancy [waves/SIMD]"]) >= 6
    assert "8 waves per SIMD" in text and "6 in the sampler" in text and 160 * 1024 // 16400 == 9


class _FakeStage2:
    """records what it is given; every cloud's outputs encode the cloud's first reflectance value and its size"""

    def __init__(self):
        self.calls = []

    def rcnn_forward_ragged(self, sub, sizes=None):
        off = sub["offsets"].tolist()
        assert off[0] == 0 and [b - a for a, b in zip(off, off[1:])] == list(sizes) and off[-1] == sub["cur_box_point"].shape[0]
        assert sub["cur_box_reflect"].shape == (off[-1], 1) and sub["train_mask"].shape == (off[-1], 1)
        self.calls.append(list(sizes))
        tag = torch.stack([sub["cur_box_reflect"][a, 0] for a in off[:-1]])
        for a, b in zip(off, off[1:]):
            assert bool((sub["cur_box_reflect"][a:b, 0] == sub["cur_box_reflect"][a, 0]).all())       # a cloud's rows stay together
        n = torch.tensor(sizes, dtype=torch.float32)
        return {"rcnn_cls": tag.view(-1, 1), "rcnn_iou": (tag + 0.5).view(-1, 1), "rcnn_ref": tag.view(-1, 1).expand(-1, 7) * 0 + n.view(-1, 1),
                "box_ce": tag.view(-1, 1).expand(-1, 7).clone()}


@pytest.mark.parametrize("rcnn_batch", [800, 2])
def test_driver_slot_bookkeeping(rcnn_batch):
    """B = 2 scenes, K = 4 slots.  Scene 0: slots 0, 2 hold points, slot 1 is an EMPTY cylinder, slot 3 is padding (num = 3) that carries rows.  Scene 1:
    num = 2, slot 0 and 1 hold points; the padding slot 2 carries rows all the same (a count that ignores num must not leak in)"""
    from ws3d_amd import detect_kitti, stage2
    B, K = 2, 4
    count = np.array([[3, 0, 5, 6], [2, 70, 4, 0]])
    num = np.array([3, 2], dtype=np.int32)
    offsets = np.concatenate(([0], np.cumsum(count.reshape(-1))))
    T = int(offsets[-1])
    tag = np.repeat(np.arange(B * K, dtype=np.float32) + 1, count.reshape(-1))                # every row knows its slot (1-based)
    inp = {"cur_box_point": torch.zeros(T, 3), "cur_box_reflect": torch.from_numpy(tag).view(T, 1), "train_mask": torch.zeros(T, 1),
           "offsets": torch.from_numpy(offsets), "count": torch.from_numpy(count.astype(np.int32)), "center": torch.zeros(B, K, 3),
           "num": torch.from_numpy(num)}
    fake = _FakeStage2()
    full = detect_kitti.rcnn_over_real_clouds_ragged(fake, inp, rcnn_batch)
    real = [0, 2, 4, 5]
    assert [n for call in fake.calls for n in call] == [3, 5, 2, 70]
    assert all(len(call) <= min(rcnn_batch, 511) for call in fake.calls) and len(fake.calls) == (1 if rcnn_batch == 800 else 2)
    for k in detect_kitti.OUT_KEYS:
        assert full[k].shape[0] == B * K
    for s in range(B * K):
        if s in real:
            assert float(full["rcnn_cls"][s, 0]) == s + 1 and float(full["rcnn_iou"][s, 0]) == s + 1.5
            assert full["rcnn_ref"][s].tolist() == [float(count.reshape(-1)[s])] * 7 and full["box_ce"][s].tolist() == [s + 1.0] * 7
        else:
            assert float(full["rcnn_cls"][s, 0]) == float("-inf") and float(full["rcnn_iou"][s, 0]) == float("-inf")
            assert not full["rcnn_ref"][s].any() and not full["box_ce"][s].any()
    # no threshold lets a dropped slot through the selection, not even one far below every score
    import dataclasses
    cfg = dataclasses.replace(stage2.DEFAULT_CFG, ioun_score_thresh=-1e30, rcnn_score_thresh=-1.0, size_window=((-9, 9), (-9, 9), (-9, 9)))
    _, keep, _ = stage2.select_boxes(full["box_ce"].view(B, K, 7), full["rcnn_ref"].view(B, K, 7) * 0, full["rcnn_cls"].view(B, K),
                                     full["rcnn_iou"].view(B, K), inp["center"], inp["num"].to(torch.int32), cfg)
    assert keep.reshape(-1).nonzero().reshape(-1).tolist() == real


def test_detect_batch_refuses_an_unknown_route_and_keeps_its_default():
    import inspect
    from ws3d_amd import detect_kitti
    assert inspect.signature(detect_kitti.detect_batch).parameters["clouds"].default == "fixed"
    assert inspect.signature(detect_kitti.run).parameters["clouds"].default == "fixed"
    with pytest.raises(ValueError):
        detect_kitti.detect_batch(None, None, torch.zeros(1, 8, 4), clouds="whole")


def test_rcnn_forward_ragged_refuses_an_empty_cloud_and_bad_sizes():
    from ws3d_amd import stage2
    net = stage2.Stage2Net()
    d = {"cur_box_point": torch.zeros(5, 3), "cur_box_reflect": torch.zeros(5, 1), "train_mask": torch.zeros(5, 1),
         "offsets": torch.tensor([0, 3, 3, 5])}
    with pytest.raises(ValueError, match="empty"):
        net.rcnn_forward_ragged(d)
    d["offsets"] = torch.tensor([0, 3, 4])
    with pytest.raises(ValueError, match="add up"):
        net.rcnn_forward_ragged(d)
    assert stage2.ragged_max_clouds(net.rcnn_net) == 511


def test_fixture_is_well_formed():
    import json
    from tests import stage2_reference as ref
    path = os.path.join(ref.GOLDEN, "stage2_ragged.npz")
    a = dict(np.load(path))
    meta = json.load(open(os.path.join(ref.GOLDEN, "stage2_ragged.json")))
    fixed = json.load(open(os.path.join(ref.GOLDEN, "stage2_forward.json")))
    assert os.path.getsize(path) < 300 * 1024 and meta["generator"] == "tests/golden/make_golden_stage2_ragged.py"
    sizes = [1, 37, 127, 128, 129, 513, 1100, 1500]
    assert meta["sizes"] == sizes and a["offsets"].tolist() == np.concatenate(([0], np.cumsum(sizes))).tolist() and a["offsets"].dtype == np.int32
    T, C = sum(sizes), len(sizes)
    assert a["pts"].shape == (T, 5) and a["pts"].dtype == np.float32 and a["can_xyz"].shape == (T, 3) and a["box_ce"].shape == (C, 7)
    assert (meta["seed"], meta["last_layer_scale"], meta["scaled_keys"]) == (fixed["seed"], fixed["last_layer_scale"], fixed["scaled_keys"])
    for k in ref.OUTPUTS + ("box_ce", "can_xyz"):
        assert 0 < meta["e_ref"][k] < 1e-5 and meta["max_abs"][k] > 0, k
        assert a[k].shape[0] == (T if k == "can_xyz" else C) and (a[k].dtype == np.float64 or k == "can_xyz")
    for (fps, bq), m, ns in zip(ref.INDEX_NAMES, (256, 128, 32) * 2, (16, 32, 64) * 2):
        assert a[fps].shape == (C, m) and a[bq].shape == (C, m, ns) and fps in meta["index_tensors"] and bq in meta["index_tensors"]
    o = a["offsets"]
    for i, n in enumerate(sizes):
        assert a["rcnn_fps_0"][i].max() < n and a["rcnn_bq_0"][i].max() < n and a["ioun_fps_0"][i].max() < n      # local indices
        inside = int((np.abs(a["can_xyz"][o[i]:o[i + 1]]).max(-1) > 0).sum())
        assert inside == meta["points_inside_box"][i]
    # a cloud below level 1's npoint: its distinct points first, then index 0 (the reference's tie rule)
    assert len(set(a["rcnn_fps_0"][1][:37].tolist())) == 37 and not a["rcnn_fps_0"][1][37:].any()
    # the real cylinders: most points outside the 1.2 x box, zeroed for the IoU tower
    assert meta["cylinders"] == [6, 7] and all(meta["points_inside_box"][i] < sizes[i] // 2 for i in (6, 7))
