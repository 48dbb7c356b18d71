"""Click-driven annotation, the part that needs no GPU (csrc/click.hip's C ABI, ws3d_amd.annotate's CPU fallback, the candidate
order of tools/eval_active.py:202-209 and the detection tail under ANNOTATE_CFG)."""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import annotate_reference as aref  # noqa: E402
from tests import stage2_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_click_prepare_is_exported_bound_and_validates_before_any_hip_call():
    from ws3d_amd import _lib, build
    raw = ctypes.CDLL(build.build())
    hdr = open(os.path.join(ROOT, "include", "ws3d_ops.h")).read()
    assert hasattr(raw, "ws3d_click_prepare") and "ws3d_click_prepare" in _lib.SIGNATURES
    assert re.search(r"WS3D_API int ws3d_click_prepare\(", hdr) and "click.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.ws3d_abi_version() == _lib.ABI_VERSION == 6
    off = (ctypes.c_float * 9)(*([0.0] * 9))
    offp = ctypes.cast(off, ctypes.c_void_p)
    buf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    n = None

    def call(B=1, N=4, K=1, side=5, pts=buf, others=buf):
        return lib.ws3d_click_prepare(B, N, K, side, offp, 0.707, 0.7, 1.5, 1.65, pts, others, n, others, others, others, None)

    assert call(pts=n) == _lib.E_INVALID and b"NULL" in lib.ws3d_last_error()       # null pts with N > 0
    assert call(side=0) == _lib.E_INVALID and b"side" in lib.ws3d_last_error()
    assert call(side=10) == _lib.E_INVALID
    assert call(B=-1) == _lib.E_INVALID and call(N=-1) == _lib.E_INVALID and call(K=-1) == _lib.E_INVALID
    assert call(B=0) == 0 and call(B=0, pts=n, others=n) == 0                       # nothing to do: succeeds without a device


def test_click_scores_on_cpu_tensors_is_gaussian_center_labels():
    from ws3d_amd import annotate, losses, synth
    pts = np.stack([synth.hdl64_cloud(4096, s)[:500] for s in (1, 2)])
    r = np.random.default_rng(0)
    clicks = np.stack([pts[b, r.choice(500, 4, replace=False), :3] for b in range(2)]).astype(np.float32)
    num = [4, 0]
    got = annotate.click_scores(torch.from_numpy(pts), torch.from_numpy(clicks), torch.tensor(num))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 500)
    for b in range(2):
        want = losses.gaussian_center_labels(pts[b, :, :3], clicks[b, :num[b]])[0]
        assert np.array_equal(got[b].numpy(), np.asarray(want, dtype=np.float32)), b
    assert float(got[0].max()) == 1.0 and not got[1].any()          # a point on its click scores 1; no clicks: 0 everywhere
    # num = None: all K clicks
    got = annotate.click_scores(torch.from_numpy(pts[1:]), torch.from_numpy(clicks[1:]))
    assert np.array_equal(got[0].numpy(), np.asarray(losses.gaussian_center_labels(pts[1, :, :3], clicks[1])[0], dtype=np.float32))


def test_candidate_order_is_grid_cell_major_over_whole_click_lists():
    """the reference's loops (i outer, j inner, torch.cat of whole click lists) put click k's grid cell g at slot g * num + k"""
    clicks = np.array([[1.5, 9.0, 20.25], [-7.125, 8.0, 33.5], [12.0, 7.0, 5.75]], dtype=np.float32)
    cand = aref.candidates_np(clicks, 1.65)
    n = clicks.shape[0]
    assert cand.shape == (25 * n, 3) and cand.dtype == np.float32
    for g in range(25):
        for k in range(n):
            want = (clicks[k, 0] + aref.OFFSETS[g // 5], np.float32(1.65), clicks[k, 2] + aref.OFFSETS[g % 5])
            assert tuple(cand[g * n + k]) == want, (g, k)
    from ws3d_amd import annotate
    assert [float(o) for o in annotate.grid_offsets()] == [float(o) for o in aref.OFFSETS]
    padded, cand_num = aref.padded_candidates_np(np.stack([clicks, clicks]), [3, 1])
    assert cand_num.tolist() == [75, 25] and np.array_equal(padded[1, :25, 0], clicks[0, 0] + np.repeat(np.array(aref.OFFSETS), 5))
    assert not padded[1, 25:].any()


def _tail_set():
    """one scene, 2 clicks, 8 candidate slots (slot j belongs to click j % 2).  box_ce is a mean-size box, rcnn_ref = 0 unless said."""
    K = 8
    ce = np.zeros((1, K, 7), dtype=np.float32)
    ce[..., 3:6] = ref.MEAN_SIZE
    ce[..., 1] = -0.75
    rref = np.zeros((1, K, 7), dtype=np.float32)
    cls = np.full((1, K), 2.0, dtype=np.float32)
    iou = np.zeros((1, K), dtype=np.float32)                # (0 is below IOUN.SCORE_THRESH: the unnamed slots drop out)
    center = np.zeros((1, K, 3), dtype=np.float32)
    center[..., 1] = 1.65
    clicks = np.array([[0.0, 0.0, 20.0], [30.0, 0.0, 25.0]], dtype=np.float32)
    for j in range(K):
        center[0, j, 0] = clicks[j % 2, 0] + 0.1 * (j // 2)
        center[0, j, 2] = clicks[j % 2, 2]
    iou[0, 0], iou[0, 2] = 0.6, 0.8         # two candidates of click 0, 0.1 m apart: the one with the higher rcnn_iou survives
    iou[0, 1] = 0.7                         # click 1: h = 1.5 * (1 + 1) = 3.0, outside DEFAULT_CFG's window (1.1, 2.3)
    rref[0, 1, 3] = 1.0
    iou[0, 3] = 0.3                         # exactly on IOUN.SCORE_THRESH: dropped (strict >)
    iou[0, 5], cls[0, 5] = 0.9, -100.0      # fp32 sigmoid(-100) is exactly RCNN.SCORE_THRESH = 0: dropped (strict >)
    return {"box_ce": ce, "rcnn_ref": rref, "rcnn_cls": cls, "rcnn_iou": iou, "center": center, "num": np.array([K], dtype=np.int32)}


def _iou_fn(b):
    n = b.shape[0]
    return torch.tensor([[ref.bev_iou(b[i].numpy(), b[j].numpy()) for j in range(n)] for i in range(n)], dtype=torch.float32)


def test_tail_under_annotate_cfg_keeps_any_size_and_reports_the_click():
    from ws3d_amd import annotate, stage2
    t = {k: torch.from_numpy(v) for k, v in _tail_set().items()}
    assert annotate.ANNOTATE_CFG.rcnn_score_thresh == stage2.DEFAULT_CFG.rcnn_score_thresh == 0.0
    assert annotate.ANNOTATE_CFG.ioun_score_thresh == stage2.DEFAULT_CFG.ioun_score_thresh == 0.3
    assert annotate.ANNOTATE_CFG.nms_iou == stage2.DEFAULT_CFG.nms_iou == 0.01
    sel = stage2.select_boxes(t["box_ce"], t["rcnn_ref"], t["rcnn_cls"], t["rcnn_iou"], t["center"], t["num"], annotate.ANNOTATE_CFG)
    assert sel[1].tolist() == [[True, True, True, False, False, False, False, False]]
    assert float(sel[0][0, 1, 3]) == 3.0
    boxes, scores, count, slot = stage2.detections_loop(*sel, annotate.ANNOTATE_CFG, _iou_fn, return_index=True)
    assert count.tolist() == [2]
    assert slot.tolist() == [[2, 1, -1, -1, -1, -1, -1, -1]]
    assert scores[0, :2].tolist() == [np.float32(0.8), np.float32(0.7)] and not scores[0, 2:].any() and not boxes[0, 2:].any()
    assert torch.equal(boxes[0, :2], sel[0][0, [2, 1]])
    click = torch.where(slot >= 0, slot % 2, slot)          # annotate_batch's mapping: slot % clicks of the scene
    assert click.tolist() == [[0, 1, -1, -1, -1, -1, -1, -1]]
    # the same through detections(); without return_index the three results are unchanged
    out = {k: t[k].reshape(8, -1) for k in ("box_ce", "rcnn_ref", "rcnn_cls", "rcnn_iou")}
    b4 = stage2.detections(out, t["center"], t["num"], annotate.ANNOTATE_CFG, iou_fn=_iou_fn, return_index=True)
    b3 = stage2.detections(out, t["center"], t["num"], annotate.ANNOTATE_CFG, iou_fn=_iou_fn)
    assert len(b3) == 3 and all(torch.equal(x, y) for x, y in zip(b4[:3], b3)) and torch.equal(b4[3], slot)
    # under DEFAULT_CFG's size window the tall box is dropped
    keep = stage2.select_boxes(t["box_ce"], t["rcnn_ref"], t["rcnn_cls"], t["rcnn_iou"], t["center"], t["num"], stage2.DEFAULT_CFG)[1]
    assert keep.tolist() == [[True, False, True, False, False, False, False, False]]


def test_too_many_candidates_raise():
    from ws3d_amd import annotate
    from ws3d_amd._lib import Ws3dError
    with pytest.raises(Ws3dError):
        annotate.annotate_inputs(torch.zeros(1, 8, 4), torch.zeros(1, 16384 // 25 + 1, 3))
