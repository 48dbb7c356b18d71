#!/usr/bin/env python
"""Golden fixture for the Stage-2 training losses: the REFERENCE's own ``get_rcnn_loss`` and ``get_ioun_loss``
(lib/net/train_functions.py:230-516, taken out of ``model_joint_fn_decorator``'s closure) evaluated in float64 on seeded head outputs
and boxes, with the error of the reference's single-thread fp32 evaluation recorded beside every quantity as the yardstick:
``python -B tests/golden/make_golden_stage2_train.py`` -> stage2_losses.{npz,json}.
Runs only in the build container (it imports /root/reference); writes data only.

  * config: weaklyRPN.yaml, weaklyRCNN.yaml, weaklyIOUN.yaml (LOC_XZ_FINE = LOC_Y_BY_BIN = False, NUM_HEAD_BIN = 12)
  * shims: make_golden.install_reference_shims() (``.cuda`` -> identity, ``iou3d_cuda`` from the fp32 oracle in both runs) and
    make_golden_stage2's; ``object_ious_3d_loss`` (logged as rcnn_loss_giou, never added to the loss) is replaced by a zero
  * cases: R = 1 foreground; R = 5 all background; R = 64, 65, 300 mixed; R = 65 with every foreground pair below IoU 0.5.  Each has
    rows with an all-zero gt box (the ioun inputs keep at least one non-zero row).  Predicted boxes are the gt plus seeded jitter, about
    half of the foreground rows pass IoU > 0.5.  Every input is an fp32 value, so the two runs read the same numbers.
  * stored: the inputs; every tb value and the total in float64; the float64 gradients w.r.t. rcnn_cls, rcnn_reg, rcnn_iou, rcnn_ref;
    the fp32 run's absolute error of each
  * a seed is refused unless the fp32 and float64 runs agree on fg_mask, iou_mask and every ry bin label, no paired IoU lies within
    1e-3 of 0.5 and no shift_angle within 1e-4 rad of a bin edge
"""
from __future__ import annotations

import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference"

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402
import make_golden_stage2 as mg2  # noqa: E402
from ws3d_amd.seeded import seeded_state_dict  # noqa: E402

# name, rows, kind
CASES = [("r1_fg", 1, "fg"), ("r5_bg", 5, "bg"), ("r64", 64, "mixed"), ("r65", 65, "mixed"), ("r300", 300, "mixed"), ("r65_far", 65, "far")]
SEEDS = range(40, 60)
MEAN = np.array([1.5, 1.6, 3.9])
RCNN_TB = ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss", "rcnn_loss_loc", "rcnn_loss_angle", "rcnn_loss_size", "rcnn_loss_corner",
           "rcnn_cls_fg", "rcnn_cls_bg")
IOUN_TB = ("ioun_loss_loc", "ioun_loss_siz", "ioun_loss_ang", "loss_iou", "loss_reg", "rcnn_loss_iou")


def make_case(rows, kind, seed):
    """seeded fp32 inputs of both losses for one case"""
    rng = np.random.Generator(np.random.PCG64(7000 + 97 * seed + rows))
    cls = {"fg": np.ones(rows), "bg": np.zeros(rows)}.get(kind)
    if cls is None:
        cls = (rng.uniform(0, 1, rows) < 0.5).astype(np.float64)
        cls[0], cls[1] = 1.0, 0.0
    gt = np.concatenate([rng.uniform(-1.0, 1.0, (rows, 1)), rng.uniform(0.5, 1.0, (rows, 1)), rng.uniform(-1.0, 1.0, (rows, 1)),
                         MEAN * rng.uniform(0.8, 1.25, (rows, 3)), rng.uniform(-np.pi, np.pi, (rows, 1))], axis=1)
    zero_rows = np.flatnonzero(cls == 0)[1::2]          # every second background row carries no gt box
    gt[zero_rows] = 0.0
    scale = rng.uniform(0.0, 1.0, (rows, 1))            # per-row jitter strength: about half of the rows end above IoU 0.5
    pred = gt + scale * np.concatenate([rng.normal(0, 0.6, (rows, 3)), rng.normal(0, 0.2, (rows, 3)), rng.normal(0, 0.4, (rows, 1))], axis=1)
    if kind == "far":
        pred[:, 0] += 1.1
    pred[zero_rows] = MEAN.mean() * rng.uniform(0.5, 1.0, (len(zero_rows), 7))
    rcnn_ref = rng.normal(0, 0.05, (rows, 7))
    refined = np.concatenate([pred[:, :3] + pred[:, 3:6] * rcnn_ref[:, :3], pred[:, 3:6] * (1 + rcnn_ref[:, 3:6]), pred[:, 6:7] + rcnn_ref[:, 6:7]], axis=1)
    data = {"cls": cls, "gt_boxes": gt, "pred_boxes3d": pred, "refined_box": refined, "rcnn_ref": rcnn_ref,
            "rcnn_cls": rng.normal(0, 2.0, (rows,)), "rcnn_reg": rng.normal(0, 0.8, (rows, 52)), "rcnn_iou": rng.uniform(0, 1, (rows,))}
    return {k: v.astype(np.float32) for k, v in data.items()}


_FLOAT = torch.Tensor.float


def set_precision(double: bool):
    """make_golden_stage2's switch, plus ``Tensor.float()`` -> float64 in the float64 run (the losses call ``.float()`` on the labels)"""
    mg2.set_precision(double)
    torch.Tensor.float = (lambda self, *a, **k: _FLOAT(self, *a, **k).double()) if double else _FLOAT


def run_losses(fns, data, double):
    """both reference losses on one case in one precision -> values, gradients and the masks / labels the seed check compares"""
    get_rcnn_loss, get_ioun_loss, iou3d_utils = fns
    set_precision(double)
    try:
        dt = torch.float64 if double else torch.float32
        t = {k: torch.from_numpy(v).to(dt) for k, v in data.items()}
        R = t["cls"].shape[0]
        model = types.SimpleNamespace(rcnn_net=types.SimpleNamespace(cls_loss_func=None))
        out = {}
        # phase rcnn
        cls_out, reg_out = t["rcnn_cls"].clone().requires_grad_(True), t["rcnn_reg"].clone().requires_grad_(True)
        ret = {"rcnn_cls": cls_out.view(R, 1), "rcnn_reg": reg_out, "gt_boxes": t["gt_boxes"].view(R, 1, 7).clone(), "cls": t["cls"].clone(),
               "pred_boxes3d": t["pred_boxes3d"].view(R, 1, 7).clone()}
        tb = {}
        loss = get_rcnn_loss(model, ret, tb, {})
        loss.backward()
        assert loss.dtype == dt
        out["rcnn"] = {"loss": float(loss.item()), "tb": {k: float(tb[k]) for k in RCNN_TB},
                       "grad": {"rcnn_cls": _grad(cls_out), "rcnn_reg": _grad(reg_out)}}
        # phase ioun
        iou_out, ref_out = t["rcnn_iou"].clone().requires_grad_(True), t["rcnn_ref"].clone().requires_grad_(True)
        ret = {"rcnn_iou": iou_out.view(R, 1), "rcnn_ref": ref_out, "gt_boxes": t["gt_boxes"].view(R, 1, 7).clone(), "cls": t["cls"].clone(),
               "pred_boxes3d": t["pred_boxes3d"].view(R, 1, 7).clone(), "refined_box": t["refined_box"].view(R, 1, 7).clone()}
        tb = {}
        loss = get_ioun_loss(model, ret, tb, {}, ret)
        loss.backward()
        assert loss.dtype == dt
        out["ioun"] = {"loss": float(loss.item()), "tb": {k: float(tb[k]) for k in IOUN_TB},
                       "grad": {"rcnn_iou": _grad(iou_out), "rcnn_ref": _grad(ref_out)}}
        # what the seed check compares: the reference's expressions for the masks and labels, in this precision
        with torch.no_grad():
            fg = t["cls"] > 0
            iou3d = torch.diagonal(iou3d_utils.boxes_iou3d_gpu(t["pred_boxes3d"].clone(), t["gt_boxes"].clone())[1])
            iou_ref = torch.diagonal(iou3d_utils.boxes_iou3d_gpu(t["refined_box"].clone(), t["gt_boxes"].clone())[1])
            apc = (2 * np.pi) / 12
            shift = (t["gt_boxes"][:, 6] % (2 * np.pi) + apc / 2) % (2 * np.pi)
            out["check"] = {"fg": fg.numpy().copy(), "iou3d": iou3d.double().numpy().copy(), "iou_mask": (fg & (iou3d > 0.5)).numpy().copy(),
                            "iou_refined": iou_ref.double().numpy().copy(), "shift": shift.double().numpy().copy(),
                            "ry_bin": (shift / apc).floor().long().numpy().copy(), "valid": (t["gt_boxes"].sum(-1) != 0).numpy().copy()}
    finally:
        set_precision(False)
    return out


def _grad(t):
    return np.zeros(tuple(t.shape)) if t.grad is None else t.grad.detach().double().numpy().copy()


def seed_ok(ref, f32):
    a, b = ref["check"], f32["check"]
    fg = a["fg"]
    apc = (2 * np.pi) / 12
    edge = np.abs(a["shift"][fg] / apc - np.round(a["shift"][fg] / apc)) * apc
    return (all(np.array_equal(a[k], b[k]) for k in ("fg", "iou_mask", "ry_bin", "valid"))
            and not (np.abs(a["iou3d"][fg] - 0.5) < 1e-3).any() and not (edge < 1e-4).any())


def reference_losses():
    from lib.config import cfg, cfg_from_file
    for name in ("weaklyRPN.yaml", "weaklyRCNN.yaml", "weaklyIOUN.yaml"):
        cfg_from_file(os.path.join(REF, "tools", "cfgs", name))
    cfg.RCNN.ENABLED = True
    cfg.IOUN.ENABLED = True
    assert not cfg.RCNN.LOC_XZ_FINE and not cfg.RCNN.LOC_Y_BY_BIN and cfg.RCNN.NUM_HEAD_BIN == 12 and cfg.RCNN.LOSS_CLS == 'BinaryCrossEntropy'
    import lib.net.train_functions as tf
    import lib.utils.iou3d.iou3d_utils as iou3d_utils
    model_fn = tf.model_joint_fn_decorator()
    cells = dict(zip(model_fn.__code__.co_freevars, model_fn.__closure__))
    inner = cells["get_rcnn_loss"].cell_contents
    dict(zip(inner.__code__.co_freevars, inner.__closure__))["object_ious_3d_loss"].cell_contents = lambda a, b: torch.zeros(())
    config = {"RCNN.LOC_SCOPE": cfg.RCNN.LOC_SCOPE, "RCNN.LOC_BIN_SIZE": cfg.RCNN.LOC_BIN_SIZE, "RCNN.NUM_HEAD_BIN": cfg.RCNN.NUM_HEAD_BIN,
              "CLS_MEAN_SIZE": [float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0])]}
    return model_fn, (cells["get_rcnn_loss"].cell_contents, cells["get_ioun_loss"].cell_contents, iou3d_utils), config


# --------------------------------------------------------------------------- one whole step per phase
STEP_SEEDS = tuple(range(11, 31))
STEP_CLS = (1.0, 0.0, 1.0, 1.0, 1.0, 0.0)        # per cloud of make_golden_stage2.CLOUDS; the last is the padding cloud
GRAD_SAMPLES = 128
STEP_OUTPUTS = {"rcnn": ("rcnn_cls", "rcnn_reg", "pred_boxes3d"), "ioun": ("rcnn_iou", "rcnn_ref", "pred_boxes3d", "refined_box", "can_xyz")}


def _turn_y(angle, shift=(0.0, 0.0, 0.0)):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, shift[0]], [0, 1, 0, shift[1]], [-s, 0, c, shift[2]], [0, 0, 0, 1]])


def step_batch(seed):
    """the collated batch ``model_fn`` takes (fp32 arrays): the six clouds of the forward fixture's recipe, a seeded box per foreground
    cloud near where the seeded network's boxes fall, and a non-trivial revive_matrix / ext_noise / noise_scale / Rot_y / iou_*"""
    pts = mg2.make_inputs(seed)
    R = pts.shape[0]
    rng = np.random.Generator(np.random.PCG64(8800 + seed))
    cls = np.array(STEP_CLS)
    gt = np.zeros((R, 1, 8))
    revive, rot = np.zeros((R, 2, 4, 4)), np.zeros((R, 4, 4))
    for r in range(R):
        spec = mg2.CLOUDS[r]
        ry = 0.0 if spec is None else spec[0] + rng.uniform(-0.2, 0.2)
        box = np.concatenate((rng.uniform(-0.1, 0.1, 3) + [0, 0.05, 0], MEAN * rng.uniform(0.95, 1.05, 3), [ry], [1.0]))
        gt[r, 0] = box * cls[r]
        revive[r] = np.stack((_turn_y(-ry), _turn_y(ry)))
        rot[r] = _turn_y(rng.uniform(-0.3, 0.3), rng.normal(0, 0.05, 3))
    data = {"cur_box_point": np.concatenate((pts[..., 0:3], np.ones((R, pts.shape[1], 1))), axis=-1), "cur_box_reflect": pts[..., 3:4],
            "cur_prob_mask": pts[..., 4:5], "gt_mask": pts[..., 4:5], "gt_boxes": gt, "cls": cls, "Rot_y": rot,
            "noise_scale": 1.0 + rng.normal(0, 0.02, (R, 1, 1)), "ext_noise": 1.0 + rng.normal(0, 0.02, (R, 1, 3)), "revive_matrix": revive,
            "iou_trans": rng.normal(0, 0.03, (R, 1, 3, 1)), "iou_scale": 1.0 + rng.normal(0, 0.02, (R, 1, 1, 1)), "iou_ry": rng.normal(0, 0.03, (R, 1, 1, 1))}
    for k in ("Rot_y", "noise_scale", "ext_noise", "iou_trans", "iou_scale", "iou_ry"):        # the padding cloud passes through unchanged
        data[k][-1] = np.eye(4) if k == "Rot_y" else (0.0 if k in ("iou_trans", "iou_ry") else 1.0)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in data.items()}


def install_grad_shims():
    """the backward halves of the gather / group shims (scatter-add of the incoming gradient)"""
    p2 = sys.modules["pointnet2_cuda"]

    def _src(idx, c):
        return idx.reshape(idx.shape[0], 1, -1).long().expand(-1, c, -1)

    def gather_points_grad_wrapper(b, c, n, npoints, grad_out, idx, grad_points):
        grad_points.scatter_add_(2, _src(idx, c), grad_out); return 1

    def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points):
        grad_points.scatter_add_(2, _src(idx, c), grad_out.reshape(b, c, -1)); return 1

    p2.gather_points_grad_wrapper, p2.group_points_grad_wrapper = gather_points_grad_wrapper, group_points_grad_wrapper


def run_step(model_fn, phase, seed, batch, double, log):
    """the reference's model_fn on a freshly seeded PointRCNN (its Stage-2 half) in one precision: forward, loss, backward"""
    from lib.config import cfg
    from lib.net.point_rcnn import PointRCNN
    cfg.RPN.ENABLED = False
    cfg.RCNN.ENABLED, cfg.IOUN.ENABLED = phase == "rcnn", phase == "ioun"
    set_precision(double)
    try:
        model = PointRCNN(num_classes=2, use_xyz=True, mode='TRAIN')
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = seeded_state_dict(shapes, seed)
        for k in mg2.SCALED_KEYS:
            if "rcnn_net." + k in sd:
                sd["rcnn_net." + k] = sd["rcnn_net." + k] * mg2.LAST_SCALE
        model.load_state_dict(sd)
        model = (model.double() if double else model).train()
        kept = {}
        hooks = [model.register_forward_pre_hook(lambda mod, args: kept.update(cur_box_point=args[0]["cur_box_point"].detach().clone(),
                                                                               gt_boxes=args[0]["gt_boxes"].detach().clone())),
                 model.register_forward_hook(lambda mod, args, out: kept.update({k: out[k].detach().clone() for k in STEP_OUTPUTS[phase] if k in out}))]
        if phase == "ioun":
            hooks.append(model.rcnn_net.SA_score_modules[0].register_forward_pre_hook(lambda mod, args: kept.update(can_xyz=args[0].detach().clone())))
        log["fps"], log["bq"] = [], []
        data = {k: v.copy() for k, v in batch.items() if phase == "ioun" or not k.startswith("iou_")}
        ret = model_fn(model, data)
        ret.loss.backward()
        for h in hooks:
            h.remove()
        dt = torch.float64 if double else torch.float32
        assert ret.loss.dtype == dt and kept["cur_box_point"].dtype == dt
        res = {"loss": float(ret.loss.item()), "tb": {k: float(v) for k, v in ret.tb_dict.items() if k != "rcnn_loss_giou"},
               "out": {k: v.double().numpy() for k, v in kept.items()},
               "grad": {k: (None if p.grad is None else p.grad.detach().double().numpy()) for k, p in model.named_parameters()},
               "trainable": [k for k, p in model.named_parameters() if p.requires_grad], "fps": list(log["fps"]), "bq": list(log["bq"])}
        with torch.no_grad():       # the masks and labels the seed check compares, from the prepared boxes in this precision
            import lib.utils.iou3d.iou3d_utils as iou3d_utils
            gt, pred = kept["gt_boxes"].view(-1, 7), kept["pred_boxes3d"].view(-1, 7)
            fg = torch.from_numpy(batch["cls"]) > 0
            iou3d = torch.diagonal(iou3d_utils.boxes_iou3d_gpu(pred.clone(), gt.clone())[1])
            apc = (2 * np.pi) / 12
            shift = (gt[:, 6] % (2 * np.pi) + apc / 2) % (2 * np.pi)
            res["check"] = {"fg": fg.numpy().copy(), "iou3d": iou3d.double().numpy().copy(), "iou_mask": (fg & (iou3d > 0.5)).numpy().copy(),
                            "shift": shift.double().numpy().copy(), "ry_bin": (shift / apc).floor().long().numpy().copy(),
                            "valid": (gt.sum(-1) != 0).numpy().copy()}
    finally:
        set_precision(False)
    return res


def step_seed_ok(ref, f32):
    """the issue's refusals (index tensors, masks, labels, thresholds), the same set of parameters with a gradient, and one more: a
    scalar of the fp32 run that lands closer to the float64 value than 2^-24 of it did so by chance -- storing ANY result in fp32
    moves it by up to that much -- and a yardstick made of such a hit could be met by no fp32 computation"""
    same = (len(ref["fps"]) == len(f32["fps"]) and all(np.array_equal(a, b) for a, b in zip(ref["fps"] + ref["bq"], f32["fps"] + f32["bq"])))
    scalars = [(f32["loss"], ref["loss"])] + [(f32["tb"][k], v) for k, v in ref["tb"].items()]
    by_chance = [(a, b) for a, b in scalars if a != b and abs(a - b) < 2.0 ** -24 * abs(b)]
    return (same and seed_ok(ref, f32) and not by_chance
            and [k for k, g in ref["grad"].items() if g is None] == [k for k, g in f32["grad"].items() if g is None])


def main_step(model_fn):
    from tests import train_reference as tr
    log = {"fps": [], "bq": []}
    mg2.install_stage2_shims(log)
    install_grad_shims()
    chosen = None
    for seed in STEP_SEEDS:
        batch = step_batch(seed)
        runs = {ph: (run_step(model_fn, ph, seed, batch, True, log), run_step(model_fn, ph, seed, batch, False, log)) for ph in ("rcnn", "ioun")}
        ok = {ph: step_seed_ok(*runs[ph]) for ph in runs}
        print("step seed", seed, ok, "iou3d", runs["rcnn"][0]["check"]["iou3d"].round(3).tolist())
        if all(ok.values()):
            chosen = (seed, batch, runs)
            break
    assert chosen is not None, "no seed gave a stable step fixture"
    seed, batch, runs = chosen
    arrays = {"batch/" + k: v for k, v in batch.items()}
    meta = {"generator": "tests/golden/make_golden_stage2_train.py", "seed": seed, "last_layer_scale": mg2.LAST_SCALE, "scaled_keys": list(mg2.SCALED_KEYS),
            "fp32_runs": ["1 thread"], "grad_samples": GRAD_SAMPLES, "phases": {}}
    for ph, (ref, f32) in runs.items():
        outs = {}
        for k, v in ref["out"].items():
            if not (ph == "ioun" and k in ("cur_box_point", "gt_boxes")):            # prepare_batch's outputs are the same in both phases
                arrays["%s/%s" % (ph, k)] = v.astype(np.float32) if k == "can_xyz" else v
            outs[k] = {"yardstick": float(np.abs(f32["out"][k] - v).max()), "max_abs": float(np.abs(v).max())}
        if ph == "ioun":
            assert np.array_equal(ref["out"]["cur_box_point"], runs["rcnn"][0]["out"]["cur_box_point"])
            assert np.array_equal(f32["out"]["can_xyz"] == 0, ref["out"]["can_xyz"] == 0)
        names = []
        for kind in ("fps", "bq"):
            for i, a in enumerate(ref[kind]):
                assert a.min() >= 0 and a.max() < 32768
                arrays["%s/%s_%d" % (ph, kind, i)] = a.astype(np.int16)
                names.append("%s_%d" % (kind, i))
        params = list(ref["grad"])
        # gradients as train_step.* keeps them: per parameter the float64 norm, seeded sampled entries, and as the yardstick the
        # relative L2 error of the fp32 run's whole tensor (tests hold every parameter to 4 x the largest of these)
        norms, yard, vals, absent = [], [], [], []
        for k in params:
            g, o = ref["grad"][k], f32["grad"][k]
            if g is None:
                absent.append(k)
                continue
            norms.append(float(np.linalg.norm(g)))
            yard.append(tr.rel_l2(o, g))
            vals.append(g.reshape(-1)[tr.sample_positions(ph + ":" + k, g.size, GRAD_SAMPLES)])
        arrays[ph + "/grad_l2"], arrays[ph + "/grad_yardstick"] = np.array(norms), np.array(yard)
        arrays[ph + "/grad_values"] = np.concatenate(vals).astype(np.float32)
        chk = ref["check"]
        meta["phases"][ph] = {"loss": ref["loss"], "tb": ref["tb"], "outputs": outs, "index_tensors": names, "param_names": params, "no_gradient": absent,
                              "trainable": ref["trainable"], "fg_sum": int(chk["fg"].sum()), "iou_sum": int(chk["iou_mask"].sum()),
                              "yardstick": {"loss": abs(f32["loss"] - ref["loss"]), "tb": {k: abs(f32["tb"][k] - v) for k, v in ref["tb"].items()}}}
        print(ph, "loss", ref["loss"], "yardstick", meta["phases"][ph]["yardstick"]["loss"], "fg", chk["fg"].sum(), "iou>0.5", chk["iou_mask"].sum(),
              "params with gradient", len(norms), "without", len(absent), "grad rel-L2 yardstick median/max", float(np.median(yard)), float(np.max(yard)), "index tensors", len(names),
              "outputs", json.dumps({k: v["yardstick"] for k, v in outs.items()}))
    np.savez_compressed(os.path.join(HERE, "stage2_train_step.npz"), **arrays)
    with open(os.path.join(HERE, "stage2_train_step.json"), "w") as f:
        json.dump(meta, f, indent=0)
    for f in ("stage2_train_step.npz", "stage2_train_step.json"):
        size = os.path.getsize(os.path.join(HERE, f))
        print(f, size, "bytes")
        assert size < 300 * 1024, (f, size)


def main():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.lines, matplotlib.pyplot  # noqa: E401,F401  (train_functions.py imports both; the shims below only fill in what is absent)
    mg.install_reference_shims()
    mg2.install_stage2_shims({"fps": [], "bq": []})
    model_fn, fns, config = reference_losses()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    arrays, meta = {}, {"generator": "tests/golden/make_golden_stage2_train.py", "config": config, "fp32_runs": ["1 thread"], "cases": {}}
    for name, rows, kind in CASES:
        chosen = None
        for seed in SEEDS:
            data = make_case(rows, kind, seed)
            ref, f32 = run_losses(fns, data, True), run_losses(fns, data, False)
            if seed_ok(ref, f32):
                chosen = (seed, data, ref, f32)
                break
            print(name, "seed", seed, "refused")
        assert chosen is not None, name
        seed, data, ref, f32 = chosen
        chk = ref["check"]
        if kind == "far":
            assert not chk["iou_mask"].any() and chk["fg"].any()
        if kind == "mixed":
            share = chk["iou_mask"].sum() / max(chk["fg"].sum(), 1)
            assert 0.25 < share < 0.75, share
            assert (~chk["valid"]).any()
        assert chk["valid"].any()
        for k, v in data.items():
            arrays["%s/%s" % (name, k)] = v
        case = {"rows": rows, "kind": kind, "seed": seed, "fg_sum": int(chk["fg"].sum()), "iou_sum": int(chk["iou_mask"].sum()),
                "valid_sum": int(chk["valid"].sum()), "ry_bin": [int(v) for v in chk["ry_bin"]]}
        for phase in ("rcnn", "ioun"):
            r, f = ref[phase], f32[phase]
            case[phase] = {"loss": r["loss"], "tb": r["tb"],
                           "yardstick": {"loss": abs(f["loss"] - r["loss"]), "tb": {k: abs(f["tb"][k] - v) for k, v in r["tb"].items()},
                                         "grad": {k: float(np.abs(f["grad"][k] - g).max()) for k, g in r["grad"].items()}}}
            for k, g in r["grad"].items():
                arrays["%s/grad_%s" % (name, k)] = g
        arrays["%s/iou3d" % name] = chk["iou3d"]            # the float64 run's paired IoU (pred, gt) and (refined, gt): CPU tests have no overlap kernel
        arrays["%s/iou3d_refined" % name] = chk["iou_refined"]
        meta["cases"][name] = case
        print(name, "seed", seed, "fg", case["fg_sum"], "iou>0.5", case["iou_sum"], "valid", case["valid_sum"],
              "rcnn", ref["rcnn"]["loss"], json.dumps(case["rcnn"]["yardstick"]["tb"]), "ioun", ref["ioun"]["loss"],
              json.dumps(case["ioun"]["yardstick"]["tb"]))
    torch.set_num_threads(threads)
    np.savez_compressed(os.path.join(HERE, "stage2_losses.npz"), **arrays)
    with open(os.path.join(HERE, "stage2_losses.json"), "w") as f:
        json.dump(meta, f, indent=0)
    for f in ("stage2_losses.npz", "stage2_losses.json"):
        size = os.path.getsize(os.path.join(HERE, f))
        print(f, size, "bytes")
        assert size < 300 * 1024, (f, size)
    torch.set_num_threads(1)
    main_step(model_fn)
    torch.set_num_threads(threads)


if __name__ == "__main__":
    main()
