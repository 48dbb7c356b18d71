"""Stage-2 training without a GPU: the losses' torch route and the independent restatements against the reference's float64 values
(tests/golden/stage2_losses.*, written by tests/golden/make_golden_stage2_train.py), the masked branches, the network's training
switches, the dataset and the schedule."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import stage2_train_reference as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tr.load_cases(GOLDEN)
RCNN_IN = ("rcnn_cls", "rcnn_reg", "pred_boxes3d", "gt_boxes", "cls")
IOUN_IN = ("rcnn_iou", "rcnn_ref", "pred_boxes3d", "refined_box", "gt_boxes", "cls")
GRADS = {"rcnn": ("rcnn_cls", "rcnn_reg"), "ioun": ("rcnn_iou", "rcnn_ref")}


def _inputs(case, names, dtype, grads):
    t = {k: torch.from_numpy(case[k]).to(dtype) for k in names}
    for k in grads:
        t[k].requires_grad_(True)
    return [t[k] for k in names]


def _run(fn, case, phase, dtype, **kw):
    names = RCNN_IN if phase == "rcnn" else IOUN_IN
    args = _inputs(case, names, dtype, GRADS[phase])
    loss, tb = fn(*args, **kw)
    if loss.requires_grad:
        loss.backward()
    grads = {k: (np.zeros(a.shape) if a.grad is None else a.grad.double().numpy()) for k, a in zip(names, args) if k in GRADS[phase]}
    return float(loss.detach()), {k: float(v) for k, v in tb.items()}, grads


def _check(got, case, phase, tol):
    """tol(yardstick, want) -> allowed absolute error"""
    loss, tb, grads = got
    m = case["meta"][phase]
    print(phase, "loss", loss, "want", m["loss"], "yardstick", m["yardstick"]["loss"])
    assert abs(loss - m["loss"]) <= tol(m["yardstick"]["loss"], m["loss"])
    for k, want in m["tb"].items():
        print(" ", k, tb[k], "want", want, "yardstick", m["yardstick"]["tb"][k])
        assert abs(tb[k] - want) <= tol(m["yardstick"]["tb"][k], want), k
    for k, g in grads.items():
        want = case["grad_" + k]
        err = float(np.abs(g - want).max())
        print("  grad", k, "max err", err, "yardstick", m["yardstick"]["grad"][k], "max", float(np.abs(want).max()))
        assert err <= tol(m["yardstick"]["grad"][k], want), k


def _f64_tol(_yardstick, want):
    return 1e-12 * max(float(np.abs(np.asarray(want)).max()), 1e-30) if np.any(want) else 0.0


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
def test_restatement_reproduces_the_reference_in_float64(name, phase):
    fn = tr.rcnn_loss if phase == "rcnn" else tr.ioun_loss
    _check(_run(fn, CASES[name], phase, torch.float64), CASES[name], phase, _f64_tol)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
def test_torch_route_reproduces_the_reference_in_float64(name, phase):
    from ws3d_amd import stage2_losses as sl
    fn = sl.rcnn_loss if phase == "rcnn" else sl.ioun_loss
    got = _run(fn, CASES[name], phase, torch.float64, overlap_fn=tr.oracle_overlap_paired)
    _check(got, CASES[name], phase, _f64_tol)
    m = CASES[name]["meta"]
    assert int(got[1]["fg_sum"]) == m["fg_sum"]
    if phase == "rcnn":
        assert int(got[1]["iou_sum"]) == m["iou_sum"]
        assert set(sl.RCNN_KEYS) <= set(got[1])
    else:
        assert int(got[1]["valid_sum"]) == m["valid_sum"]
        assert set(sl.IOUN_KEYS) <= set(got[1])


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
def test_torch_route_in_fp32_stays_within_four_times_the_yardstick(name, phase):
    from ws3d_amd import stage2_losses as sl
    fn = sl.rcnn_loss if phase == "rcnn" else sl.ioun_loss
    torch.set_num_threads(1)
    got = _run(fn, CASES[name], phase, torch.float32, overlap_fn=tr.oracle_overlap_paired)
    _check(got, CASES[name], phase, lambda y, want: 4.0 * y)


def test_all_background_gives_exact_zeros():
    from ws3d_amd import stage2_losses as sl
    case = CASES["r5_bg"]
    for dtype in (torch.float32, torch.float64):
        loss, tb, grads = _run(sl.rcnn_loss, case, "rcnn", dtype, overlap_fn=tr.oracle_overlap_paired)
        for k in ("rcnn_loss_reg", "rcnn_loss_loc", "rcnn_loss_angle", "rcnn_loss_size", "rcnn_loss_corner", "rcnn_cls_fg", "fg_sum", "iou_sum"):
            assert tb[k] == 0.0, k
        assert not grads["rcnn_reg"].any() and grads["rcnn_cls"].any()
        assert loss == tb["rcnn_loss_cls"] and tb["rcnn_cls_bg"] == 5
        loss, tb, grads = _run(sl.ioun_loss, case, "ioun", dtype, overlap_fn=tr.oracle_overlap_paired)
        assert tb["loss_reg"] == 0.0 and not grads["rcnn_ref"].any() and loss == tb["loss_iou"] > 0


def test_no_iou_pass_turns_the_corner_term_off():
    from ws3d_amd import stage2_losses as sl
    loss, tb, _ = _run(sl.rcnn_loss, CASES["r65_far"], "rcnn", torch.float64, overlap_fn=tr.oracle_overlap_paired)
    assert tb["rcnn_loss_corner"] == 0.0 and tb["iou_sum"] == 0 and tb["fg_sum"] > 0 and tb["rcnn_loss_reg"] > 0


def test_ioun_loss_without_a_gt_box_is_finite():
    """the documented deviation: the reference's mean over an empty selection is NaN, here the IoU term is 0"""
    from ws3d_amd import stage2_losses as sl
    case = dict(CASES["r64"])
    case["gt_boxes"] = np.zeros_like(case["gt_boxes"])
    args = _inputs(case, IOUN_IN, torch.float64, GRADS["ioun"])
    loss, tb = sl.ioun_loss(*args, overlap_fn=tr.oracle_overlap_paired)
    loss.backward()
    assert np.isfinite(float(loss)) and float(tb["loss_iou"]) == 0.0 and float(tb["valid_sum"]) == 0
    assert not args[0].grad.any() and torch.isfinite(args[1].grad).all()
    ref_loss, ref_tb = tr.ioun_loss(*_inputs(case, IOUN_IN, torch.float64, ()))
    assert abs(float(loss) - float(ref_loss)) <= 1e-12 * abs(float(ref_loss))


def test_cpu_tensors_without_an_overlap_function_are_an_error():
    from ws3d_amd import stage2_losses as sl
    from ws3d_amd._lib import Ws3dError
    with pytest.raises(Ws3dError):
        sl.rcnn_loss(*_inputs(CASES["r1_fg"], RCNN_IN, torch.float32, ()))


# --------------------------------------------------------------------------- the network's training switches
@pytest.fixture(scope="module")
def net():
    from ws3d_amd import stage2
    torch.manual_seed(0)
    return stage2.Stage2Net()


def test_freeze_rcnn_tower_freezes_exactly_the_first_tower(net):
    from ws3d_amd import stage2
    prefixes = ("can_", "SA_score_modules.", "IOU_layer.", "ICL_layer.", "ref_layer.")
    kept = net.rcnn_net.freeze_rcnn_tower()
    try:
        for name, p in net.rcnn_net.named_parameters():
            assert p.requires_grad == name.startswith(prefixes), name
        assert sorted(kept) == sorted(n for n, _ in net.rcnn_net.named_parameters() if n.startswith(prefixes))
        assert kept and len(kept) < len(list(net.rcnn_net.parameters()))
        assert all(n.startswith(stage2.IOU_TOWER_PREFIXES) for n in kept)
    finally:
        for p in net.parameters():
            p.requires_grad = True


def test_load_part_ckpt_accepts_a_phase_one_checkpoint(net):
    from ws3d_amd import stage2
    full = {k: v.clone() + 1.0 for k, v in net.state_dict().items()}
    part = {k: v for k, v in full.items() if not k[len("rcnn_net."):].startswith(stage2.IOU_TOWER_PREFIXES)}
    assert 0 < len(part) < len(full)
    fresh = stage2.Stage2Net()
    before = {k: v.clone() for k, v in fresh.state_dict().items()}
    with pytest.raises(RuntimeError):
        fresh.load_part_ckpt(part)
    assert fresh.load_part_ckpt({"model_state": part}, allow_missing_iou=True) == len(part)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, part[k] if k in part else before[k]), k
    broken = dict(part)
    broken.pop("rcnn_net.cls_layer.0.conv.weight")
    with pytest.raises(RuntimeError):
        stage2.Stage2Net().load_part_ckpt(broken, allow_missing_iou=True)


def test_noised_box_applies_the_three_noise_inputs_of_a_stage():
    from ws3d_amd import stage2
    ce = torch.tensor([[0.1, 0.8, -0.2, 1.5, 1.6, 3.9, 0.4], [0.0, 0.7, 0.3, 1.4, 1.7, 4.1, -2.0]])
    assert stage2.noised_box(ce, {}, 0) is ce
    noise = {"iou_trans": torch.tensor([[0.1, -0.2, 0.05], [0.0, 0.0, 0.0]]).view(2, 1, 3, 1).repeat(1, 1, 1, 2),
             "iou_scale": torch.tensor([1.1, 1.0]).view(2, 1, 1, 1).repeat(1, 1, 1, 2), "iou_ry": torch.tensor([0.3, 0.0]).view(2, 1, 1, 1).repeat(1, 1, 1, 2)}
    noise["iou_ry"][0, 0, 0, 1] = -0.5
    got = stage2.noised_box(ce, noise, 0)
    want = ce.clone()
    want[0, 0:3] += torch.tensor([0.1, -0.2, 0.05])
    want[0, 3:6] *= 1.1
    want[0, 6] += 0.3
    assert torch.equal(got, want) and torch.equal(got[1], ce[1])
    assert float(stage2.noised_box(ce, noise, 1)[0, 6]) == float(ce[0, 6] - 0.5)


# --------------------------------------------------------------------------- the dataset, prepare_batch, the schedule
def _records():
    """three hand-made records in gen_box_dataset's format: 700, 300 and 40 points; the second is background"""
    g = np.random.Generator(np.random.PCG64(77))
    recs = []
    for i, n in enumerate((700, 300, 40)):
        fg = i != 1
        pts = np.concatenate([g.uniform(-3, 3, (n, 1)), g.uniform(0.0, 1.7, (n, 1)), g.uniform(-3, 3, (n, 1))], axis=1).astype(np.float32)
        box = np.array([[0.2 * i, 1.65, -0.1, 1.5, 1.6, 3.9, 0.4 + i]], dtype=np.float32)
        recs.append({"instance_id": i, "sample_id": 10 + i, "box_id": 0 if fg else -1, "center": np.zeros((1, 3), dtype=np.float32),
                     "foreground_flag": fg, "gt_boxes": box if fg else np.zeros((1, 7), dtype=np.float32), "cur_box_point": pts,
                     "cur_box_reflect": g.uniform(0, 1, (n, 1)).astype(np.float32), "cur_prob_mask": g.uniform(0, 1, (n, 1)).astype(np.float32),
                     "gt_mask": (g.uniform(0, 1, (n, 1)) < 0.4).astype(np.float32)})
    return recs


SHAPES = {"Rot_y": (4, 4), "noise_scale": (1, 1), "gt_boxes": (1, 8), "ext_noise": (1, 3), "revive_matrix": (2, 4, 4), "cls": (1,),
          "cur_box_point": (512, 4), "cur_box_reflect": (512, 1), "cur_prob_mask": (512, 1), "gt_mask": (512, 1)}


def test_box_dataset_reads_the_pickle_and_shapes_a_sample(tmp_path):
    from ws3d_amd import train_rcnn as t2
    path = tmp_path / "train_boxes.pkl"
    with open(path, "wb") as f:
        pickle.dump(_records(), f)
    for phase in ("rcnn", "ioun"):
        ds = t2.BoxDataset(str(path), "TRAIN", seed=3, phase=phase)
        assert len(ds) == 4 * 3
        for i in range(len(ds)):
            s = ds[i]
            for k, shape in SHAPES.items():
                assert s[k].shape == shape and s[k].dtype == np.float64, (k, s[k].shape)
            assert ("iou_trans" in s) == (phase == "ioun")
            if phase == "ioun":
                assert s["iou_trans"].shape == (1, 3, 1) and s["iou_scale"].shape == (1, 1, 1) and s["iou_ry"].shape == (1, 1, 1)
            assert set(np.unique(s["cur_prob_mask"])) <= {-0.5, 0.5} and set(np.unique(s["gt_mask"])) <= {-0.5, 0.5}
            assert (s["cur_box_point"][:, 3] == 1).all() and s["gt_boxes"][0, 7] == s["cls"][0]
            # Rot_y: a rotation about y plus a translation
            r = s["Rot_y"]
            assert np.allclose(r[:3, :3] @ r[:3, :3].T, np.eye(3), atol=1e-12) and r[1, 1] == 1 and r[0, 0] == r[2, 2] and r[0, 2] == -r[2, 0]
            assert (r[3] == [0, 0, 0, 1]).all()
            assert np.allclose(s["revive_matrix"][0] @ s["revive_matrix"][1], np.eye(4), atol=1e-12)
            if s["cls"][0] == 0:
                assert not s["gt_boxes"].any()
    batch = t2.collate([ds[i] for i in range(5)])
    assert batch["cur_box_point"].shape == (5, 512, 4) and batch["cur_box_point"].dtype == np.float32 and batch["cls"].shape == (5,)
    assert batch["iou_trans"].shape == (5, 1, 3, 1) and batch["gt_boxes"].shape == (5, 1, 8) and batch["revive_matrix"].shape == (5, 2, 4, 4)


def test_box_dataset_eval_mode_is_the_identity_but_for_the_ground_shift_and_padding():
    from ws3d_amd import train_rcnn as t2
    recs = _records()
    ds = t2.BoxDataset(recs, "EVAL", seed=1, phase="ioun")
    assert len(ds) == 3
    for i, rec in enumerate(recs):
        s = ds[i]
        n = rec["cur_box_point"].shape[0]
        take = np.arange(512) % n if n < 512 else np.arange(512)               # wrap-around padding, or the first 512
        want = rec["cur_box_point"].astype(np.float64)[take]
        want[:, 1] -= 1.65
        assert np.array_equal(s["cur_box_point"][:, :3], want)
        assert np.array_equal(s["cur_box_reflect"], rec["cur_box_reflect"].astype(np.float64)[take])
        assert np.array_equal(s["cur_prob_mask"], (rec["cur_prob_mask"][take] > 0.5) - 0.5)
        assert np.array_equal(s["gt_mask"], s["cur_prob_mask"])                 # EVAL: gt_mask = cur_prob_mask
        assert np.array_equal(s["Rot_y"], np.eye(4)) and s["noise_scale"][0, 0] == 1 and (s["ext_noise"] == 1).all()
        assert (s["iou_trans"] == 0).all() and (s["iou_scale"] == 1).all() and (s["iou_ry"] == 0).all()
        box = rec["gt_boxes"].astype(np.float64).reshape(7).copy()
        box[1] -= 1.65
        assert np.array_equal(s["gt_boxes"][0, :7], box * s["cls"][0])


def test_box_dataset_same_seed_same_batch_whatever_the_workers():
    from ws3d_amd import train_rcnn as t2
    recs = _records()
    streams = [t2.batches(t2.BoxDataset(recs, "TRAIN", seed=9, phase="ioun"), 5, workers=w) for w in (0, 0, 3)]
    other = t2.batches(t2.BoxDataset(recs, "TRAIN", seed=10, phase="ioun"), 5)
    for _ in range(3):
        a, b, c = (next(s) for s in streams)
        for k in a:
            same = (lambda x, y: x == y) if isinstance(a[k], list) else np.array_equal
            assert same(a[k], b[k]) and same(a[k], c[k]), k
    assert not np.array_equal(next(other)["cur_box_point"], next(t2.batches(t2.BoxDataset(recs, "TRAIN", seed=9, phase="ioun"), 5))["cur_box_point"])
    for s in streams + [other]:
        s.close()


def test_box_dataset_train_mode_truncates_and_wraps_around():
    """TRAIN: a cloud of 40 points fills 512 slots by repeating its (shuffled, possibly thinned) rows in order"""
    from ws3d_amd import train_rcnn as t2
    ds = t2.BoxDataset(_records(), "TRAIN", seed=4)
    seen = set()
    for i in range(len(ds)):
        for _ in range(6):
            s = ds[i]
            pts = s["cur_box_point"][:, :3]
            uniq = np.unique(pts, axis=0).shape[0]
            seen.add(uniq)
            period = next(p for p in range(1, 513) if np.array_equal(pts[p:], pts[:-p])) if uniq < 512 else 512
            assert period == uniq or uniq == 512, (period, uniq)
    assert 512 in seen and min(seen) <= 40 and (128 in seen or 32 in seen)


def test_prepare_batch_reproduces_the_reference_model_fn():
    """the step fixture's batch through prepare_batch against what the reference's model_fn handed its network: float64 to 1e-12
    relative, fp32 within 4 x the error of the reference's own fp32 run"""
    from ws3d_amd import train_rcnn as t2
    meta, arrays = tr.load_step(GOLDEN)
    batch = tr.step_batch(arrays, "ioun")
    outs = meta["phases"]["rcnn"]["outputs"]
    for dtype in (torch.float64, torch.float32):
        got = t2.prepare_batch(batch, dtype=dtype)
        assert got["cur_box_point"].shape == (6, 512, 3) and got["gt_boxes"].shape == (6, 1, 7) and got["cur_box_point"].dtype == dtype
        for k in ("cur_box_point", "gt_boxes"):
            want = arrays["rcnn/" + k]
            bound = 1e-12 * outs[k]["max_abs"] if dtype == torch.float64 else 4 * outs[k]["yardstick"]
            err = float(np.abs(got[k].double().numpy().reshape(want.shape) - want).max())
            print(dtype, k, "err", err, "bound", bound, "yardstick", outs[k]["yardstick"])
            assert err <= bound, (dtype, k)
        assert torch.equal(got["train_mask"], torch.from_numpy(batch["cur_prob_mask"]).to(dtype)) and got["cls"].shape == (6,)
        assert torch.equal(got["iou_trans"], torch.from_numpy(batch["iou_trans"]).to(dtype))
        assert not got["gt_boxes"][got["cls"] == 0].any()                  # cls 0 leaves a zero box, whatever the noise
    assert not np.array_equal(arrays["rcnn/cur_box_point"], batch["cur_box_point"][..., :3].astype(np.float64))     # the noise is not trivial


def test_prepare_batch_on_the_dataset_s_own_batches():
    from ws3d_amd import train_rcnn as t2
    ds = t2.BoxDataset(_records(), "TRAIN", seed=2, phase="ioun")
    batch = t2.collate([ds[i] for i in range(len(ds))])
    got, wide = t2.prepare_batch(batch), t2.prepare_batch(batch, dtype=torch.float64)
    assert got["cur_box_point"].shape == (12, 512, 3) and got["gt_boxes"].shape == (12, 1, 7) and got["cur_box_point"].dtype == torch.float32
    assert torch.isfinite(got["cur_box_point"]).all() and float((got["cur_box_point"].double() - wide["cur_box_point"]).abs().max()) < 1e-4
    bg = torch.from_numpy(batch["cls"]) == 0
    assert bg.any() and not got["gt_boxes"][bg].any()


def test_step_fixture_is_what_its_generator_promises():
    meta, arrays = tr.load_step(GOLDEN)
    assert set(meta["phases"]) == {"rcnn", "ioun"}
    for ph, m in meta["phases"].items():
        n = len(m["param_names"]) - len(m["no_gradient"])
        assert arrays[ph + "/grad_l2"].shape == (n,) and arrays[ph + "/grad_yardstick"].shape == (n,) and (arrays[ph + "/grad_l2"] > 0).all()
        assert len(m["index_tensors"]) == (6 if ph == "rcnn" else 12) and all(ph + "/" + k in arrays for k in m["index_tensors"])
        assert m["fg_sum"] == 4 and np.isfinite(m["loss"])
    iou = ("can_", "SA_score_modules.", "IOU_layer.", "ICL_layer.", "ref_layer.")
    m = meta["phases"]["ioun"]
    assert all(k[len("rcnn_net."):].startswith(iou) for k in m["trainable"]) and set(m["param_names"]) - set(m["no_gradient"]) == {k for k in m["trainable"] if ".ICL_layer." not in k}      # (ioun_cls feeds no loss)
    assert not any(k[len("rcnn_net."):].startswith(iou) for k in meta["phases"]["rcnn"]["param_names"])


def test_one_cycle_peaks_at_a_fifth_of_the_run():
    from ws3d_amd import train_rcnn as t2
    from ws3d_amd.train_rpn import one_cycle
    cfg = t2.STAGE2_TRAIN
    assert cfg.pct_start == 0.2 and cfg.grad_norm_clip == 1.0 and cfg.lr == 0.002
    total = 1000
    lrs = [one_cycle(i, total, cfg.lr, cfg.moms, cfg.div_factor, cfg.pct_start)[0] for i in range(total)]
    assert int(np.argmax(lrs)) == 200 and lrs[200] == cfg.lr and abs(lrs[0] - cfg.lr / cfg.div_factor) < 1e-12


def test_synthetic_boxes_have_the_dataset_format():
    from ws3d_amd import train_rcnn as t2
    recs = t2.SyntheticBoxes(16, seed=1)
    assert len(recs) == 16 and recs[0]["foreground_flag"] and not recs[1]["foreground_flag"]
    fg = [r for r in recs if r["foreground_flag"]]
    assert 3 <= len(fg) <= 13
    for r in recs:
        assert r["cur_box_point"].shape == (640, 3) and r["gt_boxes"].shape == (1, 7) and r["gt_mask"].shape == (640, 1)
        assert bool(r["gt_boxes"].any()) == r["foreground_flag"]
    r = fg[0]
    assert 0.3 < r["gt_mask"].mean() < 1.0          # most of the cloud lies on the car
    ds = t2.BoxDataset(recs, "TRAIN", seed=0)
    assert ds[0]["cur_box_point"].shape == (512, 4)
