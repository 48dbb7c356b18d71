"""Two-stage inference over a KITTI directory: ``.bin`` scans in, refined 3-D boxes out as KITTI-format result files.

    python -m ws3d_amd.detect_kitti --root /data/KITTI/object --split val --out results/ [--ckpt stage1.pth] [--rcnn_ckpt stage2.pth] [--eval]

The counterpart of the reference's ``tools/eval_auto.py`` driver, eager, batch by batch:
ingest (``ws3d_amd.kitti_io``) -> ``Stage1Net.rpn_forward`` -> ``stage1.stage2_inputs(sampled_pt_num=512)`` (the instance clouds
around the kept centres) -> ``Stage2Net.rcnn_forward`` over the real slots in chunks of ``rcnn_batch`` clouds -> ``stage2.detections``
-> ``save_kitti_format`` with rcnn_iou as the score.  Weights come from reference checkpoints (``model_state``: ``rpn.*`` keys for
Stage 1, ``rcnn_net.*`` keys for Stage 2, one file may hold both) or, without one, from the seeded initialisation the benchmarks use.
``infer_kitti`` remains the Stage-1-only driver.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import kitti_io, scan_prepare, stage1, stage2

OUT_KEYS = ("rcnn_cls", "rcnn_iou", "rcnn_ref", "box_ce")
CLOUD_ROUTES = ("fixed", "ragged")


def load_stage2(rcnn_ckpt=None, device="cuda:0", rcnn_cfg: stage2.RCNNConfig = stage2.DEFAULT_CFG, num_point: int = 512):
    """Stage 2 alone (``annotate_kitti`` needs no Stage 1): from a reference checkpoint's ``rcnn_net.*`` keys or the seeded initialisation"""
    from .seeded import seeded_state_dict
    s2 = stage2.Stage2Net(mode="TEST", cfg=rcnn_cfg, num_point=num_point).to(torch.device(device)).eval()
    if rcnn_ckpt:
        s2.load_part_ckpt(torch.load(rcnn_ckpt, map_location="cpu"))
    else:
        s2.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in s2.state_dict().items()}, 0))
    return s2


def load_models(ckpt=None, rcnn_ckpt=None, device="cuda:0", cfg: stage1.RPNConfig = stage1.DEFAULT_CFG, rcnn_cfg: stage2.RCNNConfig = stage2.DEFAULT_CFG):
    from .seeded import seeded_state_dict
    dev = torch.device(device)
    s1 = stage1.Stage1Net(mode="TEST", cfg=cfg).to(dev).eval()
    if ckpt:
        state = torch.load(ckpt, map_location="cpu")
        state = state.get("model_state", state)
        s1.load_state_dict({k: v for k, v in state.items() if k.startswith("rpn.")}, strict=True)
    else:
        s1.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in s1.state_dict().items()}, 0))
    return s1, load_stage2(rcnn_ckpt, device, rcnn_cfg, cfg.roi_sampled_pts)


@torch.no_grad()
def rcnn_over_real_slots(s2, inp: dict, rcnn_batch: int = 800) -> dict:
    """``Stage2Net.rcnn_forward`` over the real slots (k < num[b]) of a ``stage2_inputs``-style dict (cur_box_point (B,K,S,3),
    cur_box_reflect, train_mask, center (B,K,3), num (B)) in chunks of ``rcnn_batch`` clouds -> the OUT_KEYS rows for all B K slots,
    zero in the padding: what ``stage2.detections`` reads.  One host synchronisation (the list of real slots).  Shared by
    ``detect_batch`` and ``annotate.annotate_batch``."""
    center, num = inp["center"], inp["num"]
    B, K = center.shape[0], center.shape[1]
    real = (torch.arange(K, device=num.device)[None, :] < num[:, None]).reshape(-1).nonzero().reshape(-1)     # (one synchronisation per batch)
    widths = {"rcnn_cls": 1, "rcnn_iou": 1, "rcnn_ref": 7, "box_ce": 7}
    full = {k: torch.zeros((B * K, w), dtype=torch.float32, device=center.device) for k, w in widths.items()}
    flat = {k: inp[k].reshape(B * K, *inp[k].shape[2:]) for k in ("cur_box_point", "cur_box_reflect", "train_mask")}
    for i0 in range(0, real.numel(), rcnn_batch):
        sel = real[i0:i0 + rcnn_batch]
        res = s2.rcnn_forward({k: v[sel].contiguous() for k, v in flat.items()})
        for k in OUT_KEYS:
            full[k][sel] = res[k].reshape(sel.numel(), -1)
    return full


@torch.no_grad()
def rcnn_over_real_clouds_ragged(s2, inp: dict, rcnn_batch: int = 800) -> dict:
    """``Stage2Net.rcnn_forward_ragged`` over the WHOLE cylinders of a ``stage2_inputs(sampled_pt_num=None)`` dict (cur_box_point
    (T,3), cur_box_reflect, train_mask, offsets (B K + 1), center (B,K,3), num (B)), as tools/eval_auto.py:286-403 feeds
    them: the padding slots k >= num[b] and the empty cylinders (eval_auto.py:339 ``continue``s) are dropped, the others run in
    chunks of at most min(rcnn_batch, 511) clouds -> the OUT_KEYS rows for all B K slots.  A dropped slot holds zeros, with rcnn_cls
    and rcnn_iou at -inf: no threshold of ``stage2.detections`` keeps it.  One host read-back (the sizes)."""
    center = inp["center"]
    B, K = center.shape[0], center.shape[1]
    host = torch.cat((inp["offsets"].reshape(-1).to(torch.int64), inp["num"].reshape(-1).to(torch.int64))).cpu().numpy()
    start, num = host[:B * K + 1], host[B * K + 1:]
    cnt = np.diff(start)
    kept = [s for s in range(B * K) if s % K < num[s // K] and cnt[s] > 0]
    widths = {"rcnn_cls": 1, "rcnn_iou": 1, "rcnn_ref": 7, "box_ce": 7}
    full = {k: torch.zeros((B * K, w), dtype=torch.float32, device=center.device) for k, w in widths.items()}
    dropped = torch.ones(B * K, dtype=torch.bool)
    dropped[torch.as_tensor(kept, dtype=torch.int64)] = False
    dropped = dropped.to(center.device)
    for k in ("rcnn_cls", "rcnn_iou"):
        full[k][dropped] = float("-inf")
    step = max(1, min(int(rcnn_batch), stage2.RAGGED_MAX_CLOUDS))
    for i0 in range(0, len(kept), step):
        slots = kept[i0:i0 + step]
        sizes = [int(cnt[s]) for s in slots]
        r0, r1 = int(start[slots[0]]), int(start[slots[-1] + 1])
        if r1 - r0 == sum(sizes):          # nothing but dropped (empty) slots in between: the chunk is one slice of the packed rows
            rows = slice(r0, r1)
        else:
            rows = torch.from_numpy(np.concatenate([np.arange(start[s], start[s + 1]) for s in slots])).to(center.device)
        sub = {k: inp[k][rows].contiguous() for k in ("cur_box_point", "cur_box_reflect", "train_mask")}
        sub["offsets"] = torch.from_numpy(np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)).to(center.device)
        res = s2.rcnn_forward_ragged(sub, sizes=sizes)
        sel = torch.as_tensor(slots, dtype=torch.int64, device=center.device)
        for k in OUT_KEYS:
            full[k][sel] = res[k].reshape(len(slots), -1)
    return full


@torch.no_grad()
def detect_batch(s1, s2, pts: torch.Tensor, cfg: stage1.RPNConfig = stage1.DEFAULT_CFG, rcnn_cfg: stage2.RCNNConfig = stage2.DEFAULT_CFG,
                 rcnn_batch: int = 800, clouds: str = "fixed"):
    """pts (B,N,4) scenes -> (boxes (B,K,7), scores (B,K), count (B,)): K = the largest number of centres Stage 1 keeps in a scene.
    clouds: "fixed" -- every instance cloud brought to cfg.roi_sampled_pts rows (the reference's training format); "ragged" -- every
    cylinder whole, whatever its size (the reference's evaluation, tools/eval_auto.py:286-403)"""
    if clouds not in CLOUD_ROUTES:
        raise ValueError("clouds must be one of %s, got %r" % (CLOUD_ROUTES, clouds))
    out = s1.rpn_forward({"pts_input": pts})
    if clouds == "ragged":
        inp = stage1.stage2_inputs(out, pts, cfg, sampled_pt_num=None, ground_y=rcnn_cfg.ground_y)
        return stage2.detections(rcnn_over_real_clouds_ragged(s2, inp, rcnn_batch), inp["center"], inp["num"], rcnn_cfg)
    inp = stage1.stage2_inputs(out, pts, cfg, sampled_pt_num=cfg.roi_sampled_pts, ground_y=rcnn_cfg.ground_y)
    return stage2.detections(rcnn_over_real_slots(s2, inp, rcnn_batch), inp["center"], inp["num"], rcnn_cfg)


def run(root: str, split: str, out_dir: str, batch: int = 4, ckpt: str | None = None, rcnn_ckpt: str | None = None, npoints: int = 16384,
        seed: int = 666, device: str = "cuda:0", cfg: stage1.RPNConfig = stage1.DEFAULT_CFG, rcnn_cfg: stage2.RCNNConfig = stage2.DEFAULT_CFG,
        rcnn_batch: int = 800, device_ingest: str = "off", clouds: str = "fixed") -> list:
    """returns the list of result files written (one per scene, possibly empty)"""
    s1, s2 = load_models(ckpt, rcnn_ckpt, device, cfg, rcnn_cfg)
    scenes = kitti_io.KittiScenes(root, split, npoints=npoints, rng=np.random.RandomState(seed))     # eval_auto.py:139 seeds numpy with 666
    dataset = scan_prepare.driver_dataset(scenes, device_ingest)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for i0 in range(0, len(scenes), batch):
        items = [dataset[i] for i in range(i0, min(i0 + batch, len(scenes)))]
        pts = torch.as_tensor(scan_prepare.batch_points(items, device_ingest, npoints, seed, device)).to(torch.device(device))
        boxes, scores, count = (t.cpu().numpy() for t in detect_batch(s1, s2, pts, cfg, rcnn_cfg, rcnn_batch, clouds))
        for j, item in enumerate(items):
            sid, k = int(item["sample_id"]), int(count[j])
            written.append(kitti_io.save_kitti_format(sid, scenes.get_calib(sid), boxes[j, :k], out_dir, scores[j, :k],
                                                      scenes.get_image_shape(sid), "Car"))
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", required=True)
    ap.add_argument("--split", default="val")
    ap.add_argument("--out", required=True)
    ap.add_argument("--ckpt", default=None, help="Stage-1 checkpoint (rpn.* keys)")
    ap.add_argument("--rcnn_ckpt", default=None, help="Stage-2 checkpoint (rcnn_net.* keys)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rcnn_batch", type=int, default=800, help="instance clouds per Stage-2 forward (the reference's Stage-2 batch)")
    ap.add_argument("--npoints", type=int, default=16384)
    ap.add_argument("--device_ingest", default="off", choices=scan_prepare.ROUTES,
                    help="off: the reference's host sampler (default); device: project, filter and sample the raw scans in one HIP call "
                         "(ws3d_amd.scan_prepare, another random stream); host: the same rows computed on the host")
    ap.add_argument("--clouds", default="fixed", choices=CLOUD_ROUTES,
                    help="fixed: every instance cloud cut or repeated to 512 rows (default); ragged: every cylinder whole, as the "
                         "reference evaluates (Stage2Net.rcnn_forward_ragged)")
    ap.add_argument("--eval", action="store_true",
                    help="score the written files against root/training/label_2 and root/ImageSets/<split>.txt (ws3d_amd.kitti_eval)")
    a = ap.parse_args()
    files = run(a.root, a.split, a.out, a.batch, a.ckpt, a.rcnn_ckpt, a.npoints, rcnn_batch=a.rcnn_batch, device_ingest=a.device_ingest, clouds=a.clouds)
    print(f"{len(files)} result files in {a.out}")
    if a.eval:
        from . import kitti_eval
        result, ret = kitti_eval.evaluate(os.path.join(a.root, "training", "label_2"), a.out,
                                          os.path.join(a.root, "ImageSets", a.split + ".txt"), current_class=0)
        print(result, end="")
        for k, v in ret.items():
            print(f"{k}: {v:.4f}")


if __name__ == "__main__":
    main()
