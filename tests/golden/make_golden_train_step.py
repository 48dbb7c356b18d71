#!/usr/bin/env python
"""Golden fixture for ONE Stage-1 training step of the REFERENCE's own network, evaluated in float64, with the error of the
reference's fp32 evaluation of the same step recorded beside it as the yardstick: ``python -B tests/golden/make_golden_train_step.py``
-> train_step.npz + train_step.json.  Runs only in the build container (it imports /root/reference); writes data only.

  * PointRCNN(mode='TRAIN').train() of lib/net/point_rcnn.py with tools/cfgs/weaklyRPN.yaml and RPN.DP_RATIO = 0.0 (config data,
    recorded below: dropout draws from a random stream no other implementation shares), weights from seeded_state_dict(keys, 7)
  * labels from KittiRCNNDataset.generate_gaussian_training_labels, loss from train_functions' model_fn -> get_rpn_loss
  * the CUDA extension is replaced as in make_golden.py; furthest point sampling, ball query and three_nn (indices and squared
    distances) come from the fp32 oracle in BOTH runs, gather / group / interpolate and the three gradient wrappers the
    forward-only shims lack are dtype-generic torch (copies and scatter-adds)
  * float64 run: model.double(), torch.cuda.FloatTensor -> DoubleTensor, Tensor.float() -> round to fp32, then widen (every
    .float() of the reference's step is applied to a label, an input or an integer: the float64 run sees the fp32 values the
    fp32 run sees, which keeps the foreground mask `label > 0` identical where a label underflows in fp32)
  * fp32 run: one, on a single thread (a summation order that does not depend on the machine); of it only ERRORS against the
    float64 run are kept, per quantity.  tests/test_train_step.py bounds the GPU's error by 4 x these.

Recorded from the float64 run: loss, every tb_dict scalar, rpn_cls / rpn_reg at seeded positions, the BatchNorm running
statistics after the step, per parameter tensor the gradient's L2 norm, max-abs, values at seeded positions and 4 seeded +-1
projections; the sha256 of the FPS and ball-query index tensors; per BatchNorm layer the share of pre-activations so close
to 0 that an fp32 evaluation of that layer could put them on the other side of the ReLU.
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
import torch.nn.functional as F  # noqa: E402

import make_golden as mg  # noqa: E402
import oracle  # noqa: E402
from tests import train_reference as tr  # noqa: E402
from ws3d_amd.seeded import seeded_state_dict  # noqa: E402

SEED = 7
CASES = [
    {"name": "two_scenes", "kind": "hdl64", "batch": 2, "n": 16384, "config_id": 71, "cars": 6,
     "logit_samples": 2048, "grad_samples": 128, "stat_samples": None},
    {"name": "no_centres", "kind": "hdl64", "batch": 1, "n": 16384, "config_id": 74, "cars": 0,
     "logit_samples": 512, "grad_samples": 128, "stat_samples": 16},
]
STAT_KINDS = ("running_mean", "running_var")


# --------------------------------------------------------------------------- the extension, dtype-generic + gradients
def install_train_shims(log):
    p2 = sys.modules["pointnet2_cuda"]

    def furthest_point_sampling_wrapper(b, n, m, xyz, temp, idx):
        r = oracle.furthest_point_sample(mg._np(xyz), m)
        log["fps"].append(mg.sha(r.astype(np.int32)))
        idx.copy_(torch.from_numpy(r)); return 1

    def ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx):
        r = oracle.ball_query(radius, nsample, mg._np(xyz), mg._np(new_xyz))
        log["bq"].append([int(n), int(nsample), mg.sha(r.astype(np.int32))])
        idx.copy_(torch.from_numpy(r)); return 1

    def _src(idx, c):
        return idx.reshape(idx.shape[0], 1, -1).long().expand(-1, c, -1)

    def gather_points_wrapper(b, c, n, npoints, points, idx, out):
        out.copy_(torch.gather(points, 2, _src(idx, c))); return 1

    def gather_points_grad_wrapper(b, c, n, npoints, grad_out, idx, grad_points):
        grad_points.scatter_add_(2, _src(idx, c), grad_out); return 1

    def group_points_wrapper(b, c, n, npoints, nsample, points, idx, out):
        out.copy_(torch.gather(points, 2, _src(idx, c)).view(b, c, npoints, nsample)); return 1

    def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points):
        grad_points.scatter_add_(2, _src(idx, c), grad_out.reshape(b, c, -1)); return 1

    def three_nn_wrapper(b, n, m, unknown, known, dist2, idx):
        d2, i = oracle.three_nn_dist2(mg._np(unknown), mg._np(known))
        dist2.copy_(torch.from_numpy(d2)); idx.copy_(torch.from_numpy(i))

    def three_interpolate_wrapper(b, c, m, n, points, idx, weight, out):
        g = torch.gather(points, 2, _src(idx, c)).view(b, c, n, 3)
        out.copy_((g * weight.unsqueeze(1)).sum(-1))

    def three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, grad_points):
        grad_points.scatter_add_(2, _src(idx, c), (grad_out.unsqueeze(-1) * weight.unsqueeze(1)).reshape(b, c, -1))

    for f in (furthest_point_sampling_wrapper, ball_query_wrapper, gather_points_wrapper, gather_points_grad_wrapper, group_points_wrapper,
              group_points_grad_wrapper, three_nn_wrapper, three_interpolate_wrapper, three_interpolate_grad_wrapper):
        setattr(p2, f.__name__, f)


_FLOAT = torch.Tensor.float


def set_precision(double: bool):
    torch.cuda.FloatTensor = torch.DoubleTensor if double else torch.FloatTensor
    torch.Tensor.float = (lambda self, *a, **k: _FLOAT(self, *a, **k).double()) if double else _FLOAT


# --------------------------------------------------------------------------- one step
def run_step(PointRCNN, model_fn, keys, data, double, log, band_probe=None):
    """-> dict of float64 numpy results of one forward + backward of a freshly seeded model"""
    set_precision(double)
    try:
        model = PointRCNN(num_classes=2, use_xyz=True, mode='TRAIN')
        model.load_state_dict(seeded_state_dict({k: tuple(v) for k, v in keys.items()}, SEED))
        model = (model.double() if double else model).train()
        hooks = []
        if band_probe is not None:
            for name, m in model.named_modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    hooks.append(m.register_forward_hook(band_probe(name, m)))
        kept = {}
        hooks.append(model.register_forward_hook(lambda mod, args, out: kept.update(out)))
        log["fps"], log["bq"] = [], []
        ret = model_fn(model, data)
        ret.loss.backward()
        for h in hooks:
            h.remove()
    finally:
        set_precision(False)
    res = {"loss": float(ret.loss.item()), "tb": {k: float(v) for k, v in ret.tb_dict.items()},
           "rpn_cls": kept["rpn_cls"].detach().double().numpy(), "rpn_reg": kept["rpn_reg"].detach().double().numpy(),
           "state": {k: v.detach().double().numpy() for k, v in model.state_dict().items() if not k.endswith("weight") and not k.endswith("bias")},
           "grad": {k: (None if p.grad is None else p.grad.detach().double().numpy()) for k, p in model.named_parameters()},
           "fps": list(log["fps"]), "bq": list(log["bq"])}
    assert kept["rpn_cls"].dtype == (torch.float64 if double else torch.float32)
    return res


def main():
    mg.install_reference_shims()
    log = {"fps": [], "bq": []}
    install_train_shims(log)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from lib.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(REF, "tools", "cfgs", "weaklyRPN.yaml"))
    cfg.RPN.ENABLED = True
    cfg.RPN.DP_RATIO = 0.0
    assert not cfg.RPN.FIXED and cfg.RPN.LOSS_CLS == 'SigmoidFocalLoss' and cfg.RPN.Gaussian_Center
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    from lib.net.point_rcnn import PointRCNN
    import lib.net.train_functions as tf
    model_fn = tf.model_joint_fn_decorator()

    keys = json.load(open(os.path.join(HERE, "stage1_state_dict.json")))["keys"]
    probe = PointRCNN(num_classes=2, use_xyz=True, mode='TRAIN')
    assert list(probe.state_dict().keys()) == list(keys), "DP_RATIO = 0.0 must not change the state_dict layout"
    param_names = [k for k, _ in probe.named_parameters()]
    stat_keys = [k for k in keys if k.endswith(STAT_KINDS)]
    count_keys = [k for k in keys if k.endswith("num_batches_tracked")]
    assert len(param_names) + len(stat_keys) + len(count_keys) == len(keys) == 208

    meta = {"generator": "tests/golden/make_golden_train_step.py", "seed": SEED, "config": {"RPN.DP_RATIO": 0.0, "cfg_file": "tools/cfgs/weaklyRPN.yaml"},
            "oracle_dist_mode": oracle.dist_mode(), "fp32_runs": ["1 thread"],
            "param_names": param_names, "stat_keys": stat_keys, "count_keys": count_keys, "cases": {}}
    arrays = {}
    threads = torch.get_num_threads()
    for case in CASES:
        name = case["name"]
        pc, centres = tr.case_inputs(case)
        B = case["batch"]
        labels = [KittiRCNNDataset.generate_gaussian_training_labels(pc[b, :, :3], centres[b]) for b in range(B)]
        gt = np.zeros((B, max(max(len(c) for c in centres), 1), 3), dtype=np.float32)
        for b in range(B):
            gt[b, :len(centres[b])] = centres[b]
        data = {"pts_input": pc, "gt_centers": gt, "rpn_cls_label": np.stack([np.asarray(l[0], dtype=np.float64) for l in labels]),
                "rpn_reg_label": np.stack([l[1] for l in labels])}

        # the ReLU band: per BatchNorm layer of the float64 run, 4 x the error of the library's fp32 evaluation of that layer on the same
        # input, and the share of float64 pre-activations inside it (tests/test_train_step.py leaves such elements out of the dx check)
        shares = {}

        def band_probe(lname, m):
            def hook(mod, args, out):
                x = args[0].detach()
                y32 = F.batch_norm(x.to(torch.float32), None, None, mod.weight.detach().to(torch.float32),
                                   mod.bias.detach().to(torch.float32), True, 0.0, mod.eps).double()
                band = 4.0 * float((y32 - out.detach()).abs().max())
                shares[lname] = float((out.detach().abs() < band).double().mean())
            return hook

        ref = run_step(PointRCNN, model_fn, keys, data, True, log, band_probe)
        fp32 = []
        for t in (1,):
            torch.set_num_threads(t)
            fp32.append(run_step(PointRCNN, model_fn, keys, data, False, log))
        torch.set_num_threads(threads)
        for r in fp32:
            assert r["fps"] == ref["fps"] and r["bq"] == ref["bq"]
            assert r["tb"]["rpn_fg_sum"] == ref["tb"]["rpn_fg_sum"]
            assert [k for k, g in r["grad"].items() if g is None] == [k for k, g in ref["grad"].items() if g is None]

        worst = lambda f: max(f(r) for r in fp32)           # noqa: E731
        yard = {"loss": worst(lambda r: tr.rel_err(r["loss"], ref["loss"])),
                "tb": {k: worst(lambda r: tr.rel_err(r["tb"][k], v)) for k, v in ref["tb"].items()},
                "rpn_cls": worst(lambda r: tr.max_err(r["rpn_cls"], ref["rpn_cls"])),
                "rpn_reg": worst(lambda r: tr.max_err(r["rpn_reg"], ref["rpn_reg"]))}
        for kind in STAT_KINDS:
            yard[kind] = worst(lambda r: max(tr.max_err(r["state"][k], ref["state"][k]) for k in stat_keys if k.endswith(kind)))
        for k in count_keys:
            assert int(ref["state"][k]) == 1 and all(int(r["state"][k]) == 1 for r in fp32)

        # logits at seeded positions
        for q in ("rpn_cls", "rpn_reg"):
            pos = tr.sample_positions(name + ":" + q, ref[q].size, case["logit_samples"])
            arrays["%s/%s" % (name, q)] = ref[q].reshape(-1)[pos]
        logit_max = {q: float(np.abs(ref[q]).max()) for q in ("rpn_cls", "rpn_reg")}
        # running statistics, concatenated in state_dict order (whole tensors, or seeded positions of each)
        stats = []
        for k in stat_keys:
            v = ref["state"][k].reshape(-1)
            stats.append(v if case["stat_samples"] is None else v[tr.sample_positions(name + ":" + k, v.size, case["stat_samples"])])
        arrays[name + "/running_stats"] = np.concatenate(stats)
        arrays[name + "/running_stats_max"] = np.array([float(np.abs(ref["state"][k]).max()) for k in stat_keys])   # the scale of max_err
        # gradients
        g_l2, g_max, g_yard, g_proj, g_proj_yard, g_val, absent = [], [], [], [], [], [], []
        for k in param_names:
            g = ref["grad"][k]
            if g is None or not np.any(g):
                absent.append(k)
                g = np.zeros(tuple(keys[k]))
            signs = tr.projection_signs(k, g.size)
            l2 = float(np.linalg.norm(g))
            g_l2.append(l2); g_max.append(float(np.abs(g).max()))
            g_proj.append(signs @ g.reshape(-1))
            g_val.append(g.reshape(-1)[tr.sample_positions(name + ":" + k, g.size, case["grad_samples"])].astype(np.float32))
            others = [np.zeros_like(g) if r["grad"][k] is None else r["grad"][k] for r in fp32]
            g_yard.append(max(tr.rel_l2(o, g) for o in others))
            g_proj_yard.append(max(float(np.abs(signs @ o.reshape(-1) - g_proj[-1]).max()) / l2 if l2 > 0 else 0.0 for o in others))
        arrays[name + "/grad_l2"], arrays[name + "/grad_maxabs"] = np.array(g_l2), np.array(g_max)
        arrays[name + "/grad_yardstick"], arrays[name + "/grad_proj"] = np.array(g_yard), np.stack(g_proj)
        arrays[name + "/grad_proj_yardstick"] = np.array(g_proj_yard)
        arrays[name + "/grad_values"] = np.concatenate(g_val)
        meta["cases"][name] = {"case": case, "loss": ref["loss"], "tb": ref["tb"], "yardstick": yard, "logit_max": logit_max, "fps_sha256": ref["fps"],
                               "ball_query_sha256": ref["bq"], "no_gradient": absent,
                               "relu_band_share": {"max": max(shares.values()), "layers": len(shares),
                                                   "worst_layer": max(shares, key=shares.get)},
                               "grad_yardstick_max": float(np.max(g_yard)), "grad_yardstick_median": float(np.median(g_yard))}
        print(name, "loss", ref["loss"], "yardstick", json.dumps(yard), "grad rel-L2 median/max", np.median(g_yard), np.max(g_yard),
              "proj", np.max(g_proj_yard), "band share", max(shares.values()), "no gradient:", absent)
    np.savez_compressed(os.path.join(HERE, "train_step.npz"), **arrays)
    with open(os.path.join(HERE, "train_step.json"), "w") as f:
        json.dump(meta, f, indent=0)
    total = 0
    for f in ("train_step.npz", "train_step.json"):
        total += os.path.getsize(os.path.join(HERE, f))
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
    assert total < 300 * 1024, total


if __name__ == "__main__":
    main()
