"""GPU checks of click-driven annotation (csrc/click.hip, ws3d_amd.annotate, ws3d_amd.annotate_kitti) against the few host lines of
tools/eval_active.py restated in tests/annotate_reference.py and against ``losses.gaussian_center_labels`` in float64.

Scenes: the ray-cast generator's first N rows for seeds 1, 2, 3; clicks: its 15 car centres moved by a seeded jitter of up to 0.3 m
in x and z.  Several cars stand outside the frustum, so some clicks have an empty cylinder."""
import dataclasses
import os
import sys
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import annotate_reference as aref  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def scenes():
    """pts (3,4096,4) fp32, clicks (3,15,3) fp32, gt boxes (3,15,7)"""
    from ws3d_amd import synth
    pts, clicks, boxes = [], [], []
    for s in SEEDS:
        p, b = synth.hdl64_cloud(4096, s, return_boxes=True)
        c = b[:, :3].astype(np.float32).copy()
        c[:, [0, 2]] += np.random.default_rng(100 + s).uniform(-0.3, 0.3, (c.shape[0], 2)).astype(np.float32)
        pts.append(p); clicks.append(c); boxes.append(b.astype(np.float32))
    return np.stack(pts), np.stack(clicks), np.stack(boxes)


def _cls64(pts, clicks, num):
    """(B,N) float64: gaussian_center_labels' cls, scene by scene"""
    from ws3d_amd import losses
    return np.stack([np.asarray(losses.gaussian_center_labels(pts[b, :, :3], clicks[b, :num[b]])[0], dtype=np.float64) for b in range(pts.shape[0])])


@pytest.fixture(scope="module")
def s2net():
    from ws3d_amd import detect_kitti
    return detect_kitti.load_models()


# ----------------------------------------------------------------------------- 1. score, 2. candidates
def _score_case(scenes, B, N, K, num):
    from ws3d_amd import compat
    pts, clicks, _ = scenes
    pts = pts[:B, :N].copy()
    if K == 15:
        clicks = clicks[:B].copy()
    elif K == 1:
        clicks = clicks[:B, 2:3].copy()
    else:       # K = one more than the kernel's LDS chunk: the car centres again and again, each copy with its own jitter
        assert K == compat.CLICK_LDS_CHUNK + 1
        r = np.random.default_rng(7)
        clicks = np.stack([clicks[b, np.arange(K) % 15] for b in range(B)])
        clicks[:, :, [0, 2]] += r.uniform(-0.3, 0.3, (B, K, 2)).astype(np.float32)
    return pts, clicks.astype(np.float32), ([K] * B if num is None else num)


@pytest.mark.parametrize("B,N,K,num", [(1, 1000, 15, None), (3, 4096, 15, [15, 1, 0]), (2, 1000, 257, None), (1, 64, 1, None)])
def test_score_and_candidates(scenes, B, N, K, num):
    """score: |fp32 - float64 cls| <= 1e-6 (three argument roundings scaled by |a| e^-|a| <= 0.37, expf's last bits and the final
    rounding: under 3e-7 together); a point placed on a click scores exactly 1; a scene without clicks scores exactly 0.
    candidates: bit-equal to the numpy statement, zero padding, exact cand_num."""
    from ws3d_amd import annotate
    pts, clicks, nums = _score_case(scenes, B, N, K, num)
    on = min(5, N - 1)
    if nums[0] > 0:
        pts[0, on, 0], pts[0, on, 1], pts[0, on, 2] = clicks[0, 0, 0], 0.5, clicks[0, 0, 2]       # d = 0.707 * 0.5 < GAUSS_STATUS
    want = _cls64(pts, clicks, nums)
    tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(clicks).cuda()
    tn = None if num is None else torch.tensor(num, dtype=torch.int32).cuda()
    got = annotate.click_scores(tp, tc, tn)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, N)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print("click score: max |fp32 - float64| = %.3g at (B,N,K) = %s" % (err, (B, N, K)))
    assert err <= 1e-6
    if nums[0] > 0:
        assert float(got[0, on]) == 1.0
    for b in range(B):
        if nums[b] == 0:
            assert not got[b].any()
    inp_score, cand, cand_num = annotate._click_prepare(tp, tc, tn, 5, 0.1, 1.65)
    assert torch.equal(inp_score, got)
    want_cand, want_num = aref.padded_candidates_np(clicks, nums, 1.65)
    assert cand_num.dtype == torch.int32 and cand_num.cpu().tolist() == want_num.tolist()
    assert np.array_equal(cand.cpu().numpy(), want_cand)
    for b in range(B):
        assert not cand[b, 25 * nums[b]:].any()


def test_click_prepare_edge_sizes(scenes):
    """K == 0 writes score = 0 and cand_num = 0; N == 0 writes only the candidates; B == 0 is a no-op"""
    from ws3d_amd import annotate
    pts, clicks, _ = scenes
    tp, tc = torch.from_numpy(pts[:2, :300]).cuda(), torch.from_numpy(clicks[:2]).cuda()
    score, cand, cand_num = annotate._click_prepare(tp, tc[:, :0].contiguous(), None, 5, 0.1, 1.65)
    assert not score.any() and tuple(cand.shape) == (2, 0, 3) and cand_num.tolist() == [0, 0]
    score, cand, cand_num = annotate._click_prepare(tp[:, :0].contiguous(), tc, None, 5, 0.1, 1.65)
    assert tuple(score.shape) == (2, 0) and cand_num.tolist() == [375, 375]
    assert np.array_equal(cand.cpu().numpy(), aref.padded_candidates_np(clicks[:2], [15, 15])[0])
    score, cand, cand_num = annotate._click_prepare(tp[:0].contiguous(), tc[:0].contiguous(), None, 5, 0.1, 1.65)
    assert score.numel() == 0 and cand.numel() == 0 and cand_num.numel() == 0


# ----------------------------------------------------------------------------- 3. annotate_inputs
@pytest.mark.parametrize("S", [64, 512])
def test_annotate_inputs_against_the_per_candidate_restatement(scenes, S):
    """count exact (S = 64 truncates: the fullest cylinders hold several hundred points), cur_box_point / cur_box_reflect bit-equal,
    train_mask bit-equal except at points whose float64 score lies within 1e-6 of 0.5 (the fp32 score may fall on the other side);
    such points are at most 1e-3 of a scene -- a condition on the inputs"""
    from ws3d_amd import annotate
    pts, clicks, _ = scenes
    num = [15, 7, 0]
    score64 = _cls64(pts, clicks, num)
    band = np.abs(score64 - 0.5) <= 1e-6
    assert band.mean(axis=1).max() <= 1e-3
    inp = annotate.annotate_inputs(torch.from_numpy(pts).cuda(), torch.from_numpy(clicks).cuda(), torch.tensor(num).cuda(), sampled_pt_num=S)
    cand, cand_num = aref.padded_candidates_np(clicks, num, 1.65)
    assert inp["num"].cpu().tolist() == cand_num.tolist() and np.array_equal(inp["center"].cpu().numpy(), cand)
    assert tuple(inp["cur_box_point"].shape) == (3, 375, S, 3) and tuple(inp["train_mask"].shape) == (3, 375, S, 1)
    assert np.abs(inp["click_score"].cpu().numpy() - score64).max() <= 1e-6
    got = {k: inp[k].cpu().numpy() for k in ("cur_box_point", "cur_box_reflect", "train_mask", "count")}
    empty = truncated = 0
    for b in range(3):
        for j in range(375):
            if j >= cand_num[b]:
                assert got["count"][b, j] == 0 and not got["cur_box_point"][b, j].any() and not got["train_mask"][b, j].any()
                continue
            rows, count, sel = aref.cloud_np(pts[b], score64[b], cand[b, j], S)
            assert got["count"][b, j] == count, (b, j)
            empty += count == 0
            truncated += count > S
            assert np.array_equal(got["cur_box_point"][b, j], rows[:, 0:3]), (b, j)
            assert np.array_equal(got["cur_box_reflect"][b, j], rows[:, 3:4]), (b, j)
            firm = ~band[b][sel] if count else np.ones(S, dtype=bool)
            assert np.array_equal(got["train_mask"][b, j, firm, 0], rows[firm, 4]), (b, j)
    print("annotate_inputs S=%d: %d empty cylinders, %d beyond S" % (S, empty, truncated))
    assert empty > 0 and (truncated > 0 if S == 64 else True)


# ----------------------------------------------------------------------------- 4. annotate_batch
def _check_annotate_batch(s2, pts, clicks, num, cfg, rcnn_batch):
    from ws3d_amd import annotate, iou3d_ops, stage2
    tp, tc, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(clicks).cuda(), torch.tensor(num, dtype=torch.int32).cuda()
    with warnings.catch_warnings(record=True) as caught:        # every synchronising call warns: only the helper's one nonzero may
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            boxes, scores, count, click = annotate.annotate_batch(s2, tp, tc, tn, cfg, rcnn_batch)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in caught if "called a synchronizing" in str(w.message)]
    assert len(syncs) <= 1, syncs
    # the composition, restated: annotate_inputs -> rcnn_forward over the real slots in the same chunks -> detections
    inp = annotate.annotate_inputs(tp, tc, tn, ground_y=cfg.ground_y)
    B, K = inp["center"].shape[0], inp["center"].shape[1]
    real = (torch.arange(K, device="cuda")[None, :] < inp["num"][:, None]).reshape(-1).nonzero().reshape(-1)
    assert real.numel() == 25 * sum(num)
    full = {k: torch.zeros((B * K, w), device="cuda") for k, w in (("rcnn_cls", 1), ("rcnn_iou", 1), ("rcnn_ref", 7), ("box_ce", 7))}
    with torch.no_grad():
        for i0 in range(0, real.numel(), rcnn_batch):
            sel = real[i0:i0 + rcnn_batch]
            res = s2.rcnn_forward({k: inp[k].reshape(B * K, *inp[k].shape[2:])[sel].contiguous() for k in ("cur_box_point", "cur_box_reflect", "train_mask")})
            for k in full:
                full[k][sel] = res[k].reshape(sel.numel(), -1)
    wb, ws, wc, wslot = stage2.detections(full, inp["center"], inp["num"], cfg, return_index=True)
    assert torch.equal(boxes, wb) and torch.equal(scores, ws) and torch.equal(count, wc)
    assert click.dtype == torch.int64 and tuple(click.shape) == (B, K)
    boxes3, scores3, count3 = stage2.detections(full, inp["center"], inp["num"], cfg)      # existing callers: unchanged
    assert torch.equal(boxes3, wb) and torch.equal(scores3, ws) and torch.equal(count3, wc)
    for b in range(B):
        n = int(count[b])
        assert (click[b, n:] == -1).all() and (wslot[b, n:] == -1).all()
        if num[b] == 0:
            assert n == 0
            continue
        assert ((click[b, :n] >= 0) & (click[b, :n] < num[b])).all()
        assert torch.equal(click[b, :n], wslot[b, :n] % num[b])
        # the box at a kept position is the detection of the slot it reports: same score
        assert torch.equal(scores[b, :n], full["rcnn_iou"].reshape(B, K)[b][wslot[b, :n]])
        s = scores[b, :n]
        assert (s[:-1] >= s[1:]).all() and (s > cfg.ioun_score_thresh).all()
        if n > 1:
            iou2d = iou3d_ops.boxes_iou3d_gpu(boxes[b, :n].contiguous(), boxes[b, :n].contiguous())[0]
            iou2d.fill_diagonal_(0)
            assert float(iou2d.max()) < 0.01
    return count.cpu().tolist()


def test_annotate_batch_is_the_composition(scenes, s2net):
    """seeded Stage-2 weights, B = 2, N = 4096, scenes with 15 and 5 clicks, chunks of 200 clouds (the last one ragged): checks the
    composition, not the network.  The seeded IoU head may score every candidate below 0.3, so the same checks run again with
    that threshold removed (survivors guaranteed) on a batch whose second scene has no click."""
    from ws3d_amd import annotate
    pts, clicks, _ = scenes
    counts = _check_annotate_batch(s2net[1], pts[:2], clicks[:2], [15, 5], annotate.ANNOTATE_CFG, 200)
    low = dataclasses.replace(annotate.ANNOTATE_CFG, ioun_score_thresh=-1e9)
    counts_low = _check_annotate_batch(s2net[1], pts[:2], clicks[:2], [15, 0], low, 200)
    print("annotate_batch: kept", counts, "at 0.3;", counts_low, "without the IoU threshold")
    assert counts_low[0] >= 1 and counts_low[1] == 0


# ----------------------------------------------------------------------------- 5. detect_batch after the helper was factored out
def test_detect_batch_equals_the_inlined_loop(scenes, s2net):
    from ws3d_amd import detect_kitti, stage1, stage2
    s1, s2 = s2net
    pts = torch.from_numpy(scenes[0][:2]).cuda()
    cfg = dataclasses.replace(stage1.DEFAULT_CFG, score_thresh=0.1)       # (the seeded Stage-1 heads keep no centre at 0.3)
    rcnn_cfg = dataclasses.replace(stage2.DEFAULT_CFG, ioun_score_thresh=-1e9, size_window=((-1e9, 1e9),) * 3)
    rcnn_batch = 96
    got = detect_kitti.detect_batch(s1, s2, pts, cfg, rcnn_cfg, rcnn_batch)
    with torch.no_grad():       # detect_batch as it stood before the helper existed
        out = s1.rpn_forward({"pts_input": pts})
        inp = stage1.stage2_inputs(out, pts, cfg, sampled_pt_num=cfg.roi_sampled_pts, ground_y=rcnn_cfg.ground_y)
        center, num = inp["center"], inp["num"]
        B, K = center.shape[0], center.shape[1]
        real = (torch.arange(K, device=num.device)[None, :] < num[:, None]).reshape(-1).nonzero().reshape(-1)
        widths = {"rcnn_cls": 1, "rcnn_iou": 1, "rcnn_ref": 7, "box_ce": 7}
        full = {k: torch.zeros((B * K, w), dtype=torch.float32, device=pts.device) for k, w in widths.items()}
        flat = {k: inp[k].reshape(B * K, *inp[k].shape[2:]) for k in ("cur_box_point", "cur_box_reflect", "train_mask")}
        for i0 in range(0, real.numel(), rcnn_batch):
            sel = real[i0:i0 + rcnn_batch]
            res = s2.rcnn_forward({k: v[sel].contiguous() for k, v in flat.items()})
            for k in detect_kitti.OUT_KEYS:
                full[k][sel] = res[k].reshape(sel.numel(), -1)
        want = stage2.detections(full, center, num, rcnn_cfg)
    print("detect_batch: K = %d, %d real slots, kept %s" % (K, real.numel(), got[2].tolist()))
    assert real.numel() > rcnn_batch and int(got[2].sum()) > 0
    assert len(got) == 3 and all(torch.equal(g, w) for g, w in zip(got, want))


# ----------------------------------------------------------------------------- 6. the driver
def test_annotate_kitti_writes_one_file_per_scene(tmp_path, monkeypatch, capsys):
    from ws3d_amd import annotate, annotate_kitti, synth
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, [(7, 20000, 1), (8, 9000, 2)])
    with open(os.path.join(root, "training", "label_2", "000008.txt"), "w") as f:       # scene 8: no Car
        f.write("\n".join(l for l in synth.KITTI_LABEL_TEXT.splitlines() if not l.startswith("Car")) + "\n")
    cars = sum(l.startswith("Car") for l in synth.KITTI_LABEL_TEXT.splitlines())
    out = str(tmp_path / "res")
    monkeypatch.setattr(sys, "argv", ["annotate_kitti", "--root", root, "--split", "val", "--out", out, "--batch", "2"])
    annotate_kitti.main()
    text = capsys.readouterr().out
    assert "2 result files in" in text
    table = [l for l in text.splitlines() if l.startswith("total roi bbox recall")]
    assert len(table) == len(annotate.RECALL_THRESHOLDS) and all("/ %d =" % cars in l for l in table), text
    assert sorted(os.listdir(out)) == ["000007.txt", "000008.txt"] and os.path.getsize(os.path.join(out, "000008.txt")) == 0
    # Stage 2 from a reference-format checkpoint holding the fixture's weights (plain seeded regression layers decode to sizes that
    # fill the image, which the result writer drops), without the IoU threshold: scene 7 gets well-formed rows, scene 8 stays empty
    from tests import stage2_reference as ref
    fx = ref.fixture()
    ckpt = str(tmp_path / "rcnn.pth")
    torch.save({"epoch": 1, "model_state": {"rcnn_net." + k: v for k, v in ref.fixture_state_dict(fx[1], fx[2]).items()}}, ckpt)
    low = dataclasses.replace(annotate.ANNOTATE_CFG, ioun_score_thresh=-1e9)
    files, recalled, total = annotate_kitti.run(root, "val", str(tmp_path / "low"), batch=1, rcnn_ckpt=ckpt, cfg=low)
    assert [os.path.basename(f) for f in files] == ["000007.txt", "000008.txt"] and total == cars and len(recalled) == 9
    rows = [line.split() for line in open(files[0])]
    assert 1 <= len(rows) <= 25 * cars and all(len(r) == 16 and r[0] == "Car" for r in rows)
    assert os.path.getsize(files[1]) == 0
    sc = [float(r[15]) for r in rows]
    assert sc == sorted(sc, reverse=True)
