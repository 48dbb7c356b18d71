"""Stage-2 training set from a KITTI directory: the instance clouds around Stage 1's kept centres, labelled and pickled.

    python -m ws3d_amd.gen_box_dataset --root /data/KITTI/object --split train --out DIR [--ckpt x.pth]
                                       [--batch 8] [--score_thresh 0.1] [--with_features]

The counterpart of the reference's ``generate_box_dataset.py``: ingest (``ws3d_amd.kitti_io``) -> Stage-1 forward ->
``stage1.center_proposals`` (:92-140) -> the cylinder of points within 4.0 m of every kept centre in (x, z), shifted to the
centre, cut for the whole batch by ``instance_ops.instance_clouds_ragged`` (replaces the distance matrix and the per-centre
boolean-mask loop, :197-229) -> labelling against the scene's ground-truth cars (:164-183, 232-251; host NumPy,
``label_instance``) -> ``DIR/<split>_boxes.pkl``, a list of dicts with the reference's keys (:294-305).

Deviations: there is no label-noise directory, so the noisy boxes equal the true ones (the two ``|`` terms of :177-180
coincide); a scene without a label file yields records with ``box_id`` -1 instead of nothing (:231).
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import pickle

import numpy as np
import torch

from . import kitti_io, scan_prepare, stage1

FG_DIST, MATCH_DIST, BOX_SCALE, RADIUS = 0.7, 1.5, 1.2, 4.0


def label_instance(center: np.ndarray, cur_box_point: np.ndarray, gt_boxes3d: np.ndarray):
    """One kept centre against the scene's ground-truth boxes (generate_box_dataset.py:164-183, 232-251).
    center (3,), cur_box_point (n,3) already shifted to the centre, gt_boxes3d (G,7) [x, y_bottom, z, h, w, l, ry] ->
    foreground_flag (bool: nearest box by (x, z) distance below 0.7 m), box_id (int: that box's index when below 1.5 m,
    else -1), gt_box (1,7) float32 (the matched box with x, z shifted to the centre, else zeros), gt_mask (n,1) float32
    (membership of the cloud in the matched box with h, w, l x 1.2).  A box's y is its bottom face and the box spans
    y - h ... y, so the larger h grows upwards only, w and l to both sides.  Distances in float32 like the reference's
    device tensors; the membership test is the box's own frame in float64 (the reference triangulates the 8 float32
    corners: equal away from the faces)."""
    center = np.asarray(center, dtype=np.float32).reshape(3)
    pts = np.asarray(cur_box_point, dtype=np.float32).reshape(-1, 3)
    gt = np.asarray(gt_boxes3d, dtype=np.float32).reshape(-1, 7)
    gt_box = np.zeros((1, 7), dtype=np.float32)
    gt_mask = np.zeros((pts.shape[0], 1), dtype=np.float32)
    if gt.shape[0] == 0:
        return False, -1, gt_box, gt_mask
    dx, dz = gt[:, 0] - center[0], gt[:, 2] - center[2]
    dist = np.sqrt(dx * dx + dz * dz)                         # float32, x first (lib/utils/distance.py:3)
    near = int(np.argmin(dist))
    fg = bool(dist[near] < np.float32(FG_DIST))
    if not dist[near] < np.float32(MATCH_DIST):
        return fg, -1, gt_box, gt_mask
    gt_box[0] = gt[near]
    gt_box[0, 0] = gt[near, 0] - center[0]
    gt_box[0, 2] = gt[near, 2] - center[2]
    big = gt_box[0].copy()
    big[3:6] = big[3:6] * np.float32(BOX_SCALE)               # :243-245, in float32
    p = pts.astype(np.float64) - big[0:3].astype(np.float64)
    c, s = np.cos(np.float64(big[6])), np.sin(np.float64(big[6]))
    along_l = p[:, 0] * c - p[:, 2] * s                       # kitti_utils.boxes3d_to_corners3d's rotation, inverted
    along_w = p[:, 0] * s + p[:, 2] * c
    inside = (np.abs(along_l) <= big[5] / 2.0) & (np.abs(along_w) <= big[4] / 2.0) & (p[:, 1] <= 0.0) & (p[:, 1] >= -np.float64(big[3]))
    gt_mask[:, 0] = inside
    return fg, near, gt_box, gt_mask


def run(root: str, split: str, out_dir: str, batch: int = 8, ckpt: str | None = None, score_thresh: float = 0.1,
        with_features: bool = False, npoints: int = 16384, seed: int = 666, device: str = "cuda:0",
        cfg: stage1.RPNConfig = stage1.DEFAULT_CFG, hook=None, device_ingest: str = "off") -> str:
    """writes ``out_dir/<split>_boxes.pkl`` and returns its path.  hook(sample_id, pts_input (N,4), scores (N,)): called once per
    scene with the host copies of what the clouds were cut from."""
    from . import instance_ops
    dev = torch.device(device)
    cfg = dataclasses.replace(cfg, score_thresh=float(score_thresh))
    model = stage1.Stage1Net(mode="TEST", cfg=cfg).to(dev).eval()
    if ckpt:
        state = torch.load(ckpt, map_location="cpu")
        model.load_state_dict(state.get("model_state", state), strict=True)
    else:
        from .seeded import seeded_state_dict
        model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0))
    scenes = kitti_io.KittiScenes(root, split, npoints=npoints, rng=np.random.RandomState(seed))
    dataset = scan_prepare.driver_dataset(scenes, device_ingest)
    database = []
    for i0 in range(0, len(scenes), batch):
        items = [dataset[i] for i in range(i0, min(i0 + batch, len(scenes)))]
        pts = torch.as_tensor(scan_prepare.batch_points(items, device_ingest, npoints, seed, dev)).to(dev)
        B, N = pts.shape[0], pts.shape[1]
        with torch.no_grad():
            out = model.rpn_forward({"pts_input": pts})
            center, _, num = stage1.kept_centres(out, cfg, y=0.0)
            scores = torch.sigmoid(out["rpn_cls"].reshape(B, N))
            feats = None
            if with_features:
                feats = out.get("backbone_features_nlc")
                feats = (out["backbone_features"].transpose(1, 2) if feats is None else feats).contiguous()
            rows, row_feats, offsets, _ = instance_ops.instance_clouds_ragged(pts, scores, center, num, RADIUS, mask_mode=0, features=feats)
        rows, offsets, center, num = rows.cpu().numpy(), offsets.cpu().numpy(), center.cpu().numpy(), num.cpu().numpy()
        row_feats = row_feats.cpu().numpy() if row_feats is not None else None
        K = center.shape[1]
        for b, item in enumerate(items):
            sid = int(item["sample_id"])
            if hook is not None:
                hook(sid, pts[b].cpu().numpy(), scores[b].cpu().numpy())
            label_path = scenes._path("label_2", sid, "txt")
            objs = kitti_io.read_label_file(label_path) if os.path.exists(label_path) else []
            gt = np.array([o.box3d() for o in objs if o.cls_type == "Car"], dtype=np.float32).reshape(-1, 7)
            for k in range(int(num[b])):
                lo, hi = int(offsets[b * K + k]), int(offsets[b * K + k + 1])
                if hi == lo:                                    # :218
                    continue
                if split == "train" and hi - lo <= 5:           # :293
                    continue
                cloud = rows[lo:hi]
                cur_box_point = np.ascontiguousarray(cloud[:, 0:3])
                fg, box_id, gt_box, gt_mask = label_instance(center[b, k], cur_box_point, gt)
                rec = {"instance_id": len(database), "sample_id": sid, "box_id": int(box_id), "center": center[b, k].reshape(1, 3).copy(),
                       "foreground_flag": bool(fg), "gt_boxes": gt_box, "cur_box_point": cur_box_point,
                       "cur_box_reflect": np.ascontiguousarray(cloud[:, 3:4]), "cur_prob_mask": np.ascontiguousarray(cloud[:, 4:5]),
                       "gt_mask": gt_mask}
                if with_features:
                    rec["cur_pts_feature"] = np.ascontiguousarray(row_feats[lo:hi])
                database.append(rec)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "%s_boxes.pkl" % split)
    with open(path, "wb") as f:
        pickle.dump(database, f)
    return path


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--out", required=True)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--score_thresh", type=float, default=0.1)
    ap.add_argument("--with_features", action="store_true")
    ap.add_argument("--npoints", type=int, default=16384)
    ap.add_argument("--device_ingest", default="off", choices=scan_prepare.ROUTES,
                    help="off: the reference's host sampler (default); device: project, filter and sample the raw scans in one HIP call "
                         "(ws3d_amd.scan_prepare, another random stream); host: the same rows computed on the host")
    a = ap.parse_args()
    path = run(a.root, a.split, a.out, a.batch, a.ckpt, a.score_thresh, a.with_features, a.npoints, device_ingest=a.device_ingest)
    with open(path, "rb") as f:
        print(f"{len(pickle.load(f))} instances in {path}")


if __name__ == "__main__":
    main()
