#!/usr/bin/env python
"""Golden fixture for the Stage-2 box network: the REFERENCE's own ``RCNNNet`` (lib/net/rcnn_net.py), evaluated in float64 on a
few instance clouds, with the error of the reference's single-thread fp32 evaluation recorded beside every quantity as the
yardstick: ``python -B tests/golden/make_golden_stage2.py`` -> stage2_state_dict.json + stage2_forward.{npz,json}.
Runs only in the build container (it imports /root/reference); writes data only.

  * config: weaklyRPN.yaml, weaklyRCNN.yaml, weaklyIOUN.yaml in that order, then RCNN.ENABLED = IOUN.ENABLED = True
    (tools/eval_auto.py:918-928)
  * shims: make_golden.install_reference_shims() + a stub matplotlib.pyplot, Module.cuda -> identity, Tensor.to(int) -> identity,
    torch.set_default_dtype for the float64 run; furthest point sampling and ball query come from the fp32 oracle in both
    runs (their index tensors are recorded), gather / group are dtype-generic torch
  * weights: seeded_state_dict(keys, SEED), the last layer of reg_layer and of ref_layer.0 scaled by LAST_SCALE (He-normal
    regression outputs would decode to boxes no cloud fits in)
  * clouds: synth.roi_clouds turned and stretched per cloud, lowered to the Stage-2 frame, one blown up so that fewer than 256
    of its points lie inside the 1.2 x box (the IoU tower's sampling then runs into the zeroed duplicates), one all-zero
    padding cloud
  * before anything is written: (a) every FPS / ball-query index tensor of the fp32 run equals the float64 run's, (b) the fp32
    IoU tower gives the same index tensors when box_ce is perturbed by seeded relative +-2^-21 patterns (through the
    reference's own iou_trans / iou_scale / iou_ry inputs).  Another seed is tried when either fails.
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
import oracle  # noqa: E402
from ws3d_amd import synth  # noqa: E402
from ws3d_amd.seeded import seeded_state_dict  # noqa: E402

SEEDS = (11, 12, 13, 14, 15)
LAST_SCALE = 0.05
SCALED_KEYS = ("reg_layer.3.conv.weight", "reg_layer.3.conv.bias", "ref_layer.0.3.conv.weight", "ref_layer.0.3.conv.bias")
NUM_POINT = 512
# per cloud: yaw about y, stretch of (x, y, z); the first and fourth are small enough to lie inside any decoded box, the fifth is the
# blown-up one, the last the padding slot
CLOUDS = [(0.0, (0.3, 0.3, 0.3)), (0.6, (0.9, 1.0, 1.1)), (-1.2, (1.15, 0.9, 0.95)), (2.5, (0.45, 0.5, 0.45)), (0.3, (2.6, 1.5, 2.6)), None]
PERTURBATIONS = 4
OUTPUTS = ("rcnn_cls", "rcnn_reg", "pred_boxes3d", "rcnn_iou", "rcnn_ref", "ioun_cls", "refined_box")


def make_inputs(seed):
    """(R, 512, 5) float32 rows [x, y, z, reflectance, mask]"""
    R = len(CLOUDS)
    rng = np.random.Generator(np.random.PCG64(5000 + seed))
    raw = synth.roi_clouds(R, NUM_POINT, seed).astype(np.float64)
    pts = np.zeros((R, NUM_POINT, 5), dtype=np.float32)
    for r, spec in enumerate(CLOUDS):
        if spec is None:
            continue
        yaw, stretch = spec
        p = raw[r] - np.array([0.0, -1.0, 0.0])
        p = p * np.array(stretch)
        c, s = np.cos(yaw), np.sin(yaw)
        x, z = p[:, 0] * c + p[:, 2] * s, -p[:, 0] * s + p[:, 2] * c
        pts[r, :, 0], pts[r, :, 1], pts[r, :, 2] = x, p[:, 1] - 0.8, z
        pts[r, :, 3] = rng.uniform(0, 1, NUM_POINT)
        pts[r, :, 4] = np.where(rng.uniform(0, 1, NUM_POINT) < 0.5, 0.5, -0.5)
    return pts


def install_stage2_shims(log):
    p2 = sys.modules["pointnet2_cuda"]

    def furthest_point_sampling_wrapper(b, n, m, xyz, temp, idx):
        r = oracle.furthest_point_sample(mg._np(xyz).astype(np.float32), m)
        log["fps"].append(np.asarray(r).astype(np.int32))
        idx.copy_(torch.from_numpy(np.asarray(r))); return 1

    def ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx):
        r = oracle.ball_query(radius, nsample, mg._np(xyz).astype(np.float32), mg._np(new_xyz).astype(np.float32))
        log["bq"].append(np.asarray(r).astype(np.int32))
        idx.copy_(torch.from_numpy(np.asarray(r))); return 1

    def _src(idx, c):
        return idx.reshape(idx.shape[0], 1, -1).long().expand(-1, c, -1)

    def gather_points_wrapper(b, c, n, npoints, points, idx, out):
        out.copy_(torch.gather(points, 2, _src(idx, c))); return 1

    def group_points_wrapper(b, c, n, npoints, nsample, points, idx, out):
        out.copy_(torch.gather(points, 2, _src(idx, c)).view(b, c, npoints, nsample)); return 1

    for f in (furthest_point_sampling_wrapper, ball_query_wrapper, gather_points_wrapper, group_points_wrapper):
        setattr(p2, f.__name__, f)
    plt = types.ModuleType("matplotlib.pyplot")
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = plt
    sys.modules.setdefault("matplotlib", mpl)
    sys.modules.setdefault("matplotlib.pyplot", plt)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    torch.nn.Module.cuda = lambda self, *a, **k: self
    _to = torch.Tensor.to
    torch.Tensor.to = lambda self, *a, **k: self if (len(a) == 1 and isinstance(a[0], int) and not k) else _to(self, *a, **k)


def set_precision(double: bool):
    torch.set_default_dtype(torch.float64 if double else torch.float32)
    torch.cuda.FloatTensor = torch.DoubleTensor if double else torch.FloatTensor


def run(RCNNNet, shapes, seed, pts, double, log, noise=None):
    """one forward of a freshly seeded model -> dict of numpy arrays in the run's precision"""
    set_precision(double)
    try:
        model = RCNNNet(num_classes=2, num_point=NUM_POINT, input_channels=128, use_xyz=True)
        sd = seeded_state_dict(shapes, seed)
        for k in SCALED_KEYS:
            sd[k] = sd[k] * LAST_SCALE
        model.load_state_dict(sd)
        model = (model.double() if double else model).eval()
        dt = torch.float64 if double else torch.float32
        t = torch.from_numpy(pts).to(dt)
        data = {"cur_box_point": t[..., 0:3].contiguous(), "cur_box_reflect": t[..., 3:4].contiguous(), "train_mask": t[..., 4:5].contiguous()}
        if noise is not None:
            data.update({k: torch.from_numpy(v).to(dt) for k, v in noise.items()})
        kept = {}
        h = model.SA_score_modules[0].register_forward_pre_hook(lambda mod, args: kept.update(can_xyz=args[0].detach().clone()))
        log["fps"], log["bq"] = [], []
        with torch.no_grad():
            ret = model(data)
            from lib.utils.bbox_transform import decode_bbox_target_stage_2, box2center_box
            from lib.config import cfg
            reg = ret["rcnn_reg"]
            ce = decode_bbox_target_stage_2(torch.zeros((reg.shape[0], 3)), reg.view(-1, reg.shape[-1]), anchor_size=model.MEAN_SIZE,
                                            loc_scope=cfg.RCNN.LOC_SCOPE, loc_bin_size=cfg.RCNN.LOC_BIN_SIZE, num_head_bin=cfg.RCNN.NUM_HEAD_BIN,
                                            get_xz_fine=False, loc_y_scope=cfg.RCNN.LOC_Y_SCOPE, loc_y_bin_size=cfg.RCNN.LOC_Y_BIN_SIZE,
                                            get_ry_fine=False).view(-1, 1, 7)
            box_ce = box2center_box(ce)
        h.remove()
        assert ret["rcnn_reg"].dtype == dt and kept["can_xyz"].dtype == dt
    finally:
        set_precision(False)
    res = {k: ret[k].detach().numpy().copy() for k in OUTPUTS}
    res["box_ce"] = box_ce.numpy().reshape(-1, 7).copy()
    res["can_xyz"] = kept["can_xyz"].numpy().copy()
    res["fps"], res["bq"] = list(log["fps"]), list(log["bq"])
    return res


def same_indices(a, b, first=0):
    return (len(a["fps"]) == len(b["fps"]) == 6 and len(a["bq"]) == len(b["bq"]) == 6
            and all(np.array_equal(x, y) for x, y in zip(a["fps"][first:], b["fps"][first:]))
            and all(np.array_equal(x, y) for x, y in zip(a["bq"][first:], b["bq"][first:])))


def main():
    mg.install_reference_shims()
    log = {"fps": [], "bq": []}
    install_stage2_shims(log)
    from lib.config import cfg, cfg_from_file
    for name in ("weaklyRPN.yaml", "weaklyRCNN.yaml", "weaklyIOUN.yaml"):
        cfg_from_file(os.path.join(REF, "tools", "cfgs", name))
    cfg.RCNN.ENABLED = True
    cfg.IOUN.ENABLED = True
    from lib.net.rcnn_net import RCNNNet

    probe = RCNNNet(num_classes=2, num_point=NUM_POINT, input_channels=128, use_xyz=True)
    shapes = {k: tuple(v.shape) for k, v in probe.state_dict().items()}
    config = {"RCNN.SA_CONFIG": {k: cfg.RCNN.SA_CONFIG[k] for k in ("NPOINTS", "RADIUS", "NSAMPLE", "MLPS")},
              "IOUN.SA_CONFIG": {k: cfg.IOUN.SA_CONFIG[k] for k in ("NPOINTS", "RADIUS", "NSAMPLE", "MLPS")},
              "RCNN.XYZ_UP_LAYER": cfg.RCNN.XYZ_UP_LAYER, "RCNN.CLS_FC": cfg.RCNN.CLS_FC, "RCNN.REG_FC": cfg.RCNN.REG_FC,
              "IOUN.CLS_FC": cfg.IOUN.CLS_FC, "IOUN.REG_FC": cfg.IOUN.REG_FC,
              "RCNN.USE_BN": cfg.RCNN.USE_BN, "IOUN.USE_BN": cfg.IOUN.USE_BN, "RCNN.DP_RATIO": cfg.RCNN.DP_RATIO, "IOUN.DP_RATIO": cfg.IOUN.DP_RATIO,
              "RCNN.LOC_SCOPE": cfg.RCNN.LOC_SCOPE, "RCNN.LOC_BIN_SIZE": cfg.RCNN.LOC_BIN_SIZE, "RCNN.NUM_HEAD_BIN": cfg.RCNN.NUM_HEAD_BIN,
              "RCNN.LOC_Y_BY_BIN": cfg.RCNN.LOC_Y_BY_BIN, "CLS_MEAN_SIZE": [float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0])],
              "CASCADE": cfg.CASCADE, "ATTENTION": cfg.ATTENTION, "RCNN.SCORE_THRESH": cfg.RCNN.SCORE_THRESH,
              "IOUN.SCORE_THRESH": cfg.IOUN.SCORE_THRESH}
    with open(os.path.join(HERE, "stage2_state_dict.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_stage2.py", "config": config, "keys": {k: list(v) for k, v in shapes.items()}}, f, indent=0)

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    chosen = None
    for seed in SEEDS:
        pts = make_inputs(seed)
        ref = run(RCNNNet, shapes, seed, pts, True, log)
        f32 = run(RCNNNet, shapes, seed, pts, False, log)
        ok_a = same_indices(ref, f32)
        # (b) the fp32 IoU tower under relative +-2^-21 perturbations of box_ce
        ce = f32["box_ce"].astype(np.float64)
        R = ce.shape[0]
        ok_b = True
        for p in range(PERTURBATIONS):
            sign = np.random.Generator(np.random.PCG64(9000 + 10 * seed + p)).choice([-1.0, 1.0], size=(R, 7))
            eps = sign * 2.0 ** -21
            noise = {"iou_trans": (ce[:, 0:3] * eps[:, 0:3]).reshape(R, 1, 3, 1).astype(np.float32),
                     "iou_scale": (1.0 + eps[:, 3:6]).reshape(R, 1, 3, 1).astype(np.float32),
                     "iou_ry": (ce[:, 6:7] * eps[:, 6:7]).reshape(R, 1, 1, 1).astype(np.float32)}
            pert = run(RCNNNet, shapes, seed, pts, False, log, noise)
            ok_b = ok_b and same_indices(f32, pert, first=3)
        inside = (np.abs(ref["can_xyz"]).max(-1) > 0).sum(1)          # points the 1.2 x box keeps (a kept point at the exact origin aside)
        ok_c = bool((inside[:-1] < 256).any() and (inside[:-1] >= 256).any() and not pts[-1].any())
        print("seed", seed, "fp32 == float64 indices:", ok_a, " stable under box_ce perturbation:", ok_b, " points inside:", inside.tolist(), ok_c)
        if ok_a and ok_b and ok_c:
            chosen = (seed, pts, ref, f32)
            break
    torch.set_num_threads(threads)
    assert chosen is not None, "no seed gave a stable fixture"
    seed, pts, ref, f32 = chosen

    arrays = {"pts": pts, "box_ce": ref["box_ce"], "can_xyz": ref["can_xyz"].astype(np.float32)}
    e_ref = {}
    for k in OUTPUTS + ("box_ce", "can_xyz"):
        if k in OUTPUTS:
            arrays[k] = ref[k]
        e_ref[k] = float(np.abs(f32[k].astype(np.float64) - ref[k]).max())
    # the reference's fp32 zero pattern of the canonical cloud equals the float64 run's (else the index tensors would differ)
    assert np.array_equal(f32["can_xyz"] == 0, ref["can_xyz"] == 0)
    names = []
    for tower, base in (("rcnn", 0), ("ioun", 3)):
        for lvl in range(3):
            for kind in ("fps", "bq"):
                a = ref[kind][base + lvl]
                assert a.min() >= 0 and a.max() < 32768
                arrays["%s_%s_%d" % (tower, kind, lvl)] = a.astype(np.int16)
                names.append("%s_%s_%d" % (tower, kind, lvl))
    meta = {"generator": "tests/golden/make_golden_stage2.py", "seed": seed, "last_layer_scale": LAST_SCALE, "scaled_keys": list(SCALED_KEYS),
            "num_point": NUM_POINT, "clouds": [None if c is None else {"yaw": c[0], "stretch": list(c[1])} for c in CLOUDS],
            "oracle_dist_mode": oracle.dist_mode(), "fp32_runs": ["1 thread"], "perturbations": PERTURBATIONS,
            "points_inside_box": [int(v) for v in (np.abs(ref["can_xyz"]).max(-1) > 0).sum(1)],
            "index_tensors": names, "outputs": list(OUTPUTS), "e_ref": e_ref,
            "max_abs": {k: float(np.abs(arrays[k]).max()) for k in OUTPUTS + ("box_ce", "can_xyz")}}
    np.savez_compressed(os.path.join(HERE, "stage2_forward.npz"), **arrays)
    with open(os.path.join(HERE, "stage2_forward.json"), "w") as f:
        json.dump(meta, f, indent=0)
    print("e_ref", json.dumps(e_ref))
    for f in ("stage2_state_dict.json", "stage2_forward.npz", "stage2_forward.json"):
        size = os.path.getsize(os.path.join(HERE, f))
        print(f, size, "bytes")
        assert size < 300 * 1024, (f, size)


if __name__ == "__main__":
    main()
