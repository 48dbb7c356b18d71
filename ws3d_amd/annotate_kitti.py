"""Click-driven annotation over a KITTI directory: ``.bin`` scans and one click per ``Car`` in, refined 3-D boxes out as
KITTI-format result files.

    python -m ws3d_amd.annotate_kitti --root /data/KITTI/object --split val --out labels/ [--rcnn_ckpt stage2.pth] [--click_labels SUBDIR] [--batch 4] [--rcnn_batch 800] [--eval]

The counterpart of the reference's ``tools/eval_active.py`` driver.  A scene's clicks are the ``pos`` of the ``Car`` objects in
``root/training/<click_labels or label_2>/`` (the EVAL-mode ``filtrate_objects``: class ``Car`` only, no range filter); scenes come
through ``kitti_io.KittiScenes`` exactly as in ``detect_kitti.run``; ``annotate.annotate_batch`` turns the clicks into boxes, which
are written with ``save_kitti_format`` and rcnn_iou as the score.  A scene without clicks gets an empty file.  The recall of the
``Car`` boxes of ``label_2`` is printed per IoU threshold (eval_active.py:341-365).  No Stage-1 network is loaded; without a
checkpoint Stage 2 runs the seeded initialisation the benchmarks use.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import annotate, kitti_io, scan_prepare, stage2
from .detect_kitti import load_stage2


def car_boxes(label_path: str) -> np.ndarray:
    """(n,7) [x, y, z, h, w, l, ry] of a label file's ``Car`` objects (EVAL-mode filtrate_objects, kitti_rcnn_dataset.py); a missing
    file holds none"""
    if not os.path.exists(label_path):
        return np.zeros((0, 7), dtype=np.float32)
    cars = [o.box3d() for o in kitti_io.read_label_file(label_path) if o.cls_type == "Car"]
    return np.stack(cars).astype(np.float32) if cars else np.zeros((0, 7), dtype=np.float32)


def _pad(rows: list, width: int):
    """ragged list of (n_i, width) arrays -> ((B, max(n), width) zero padded, (B,) int32)"""
    out = np.zeros((len(rows), max([r.shape[0] for r in rows] + [0]), width), dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out, np.array([r.shape[0] for r in rows], dtype=np.int32)


def run(root: str, split: str, out_dir: str, batch: int = 4, rcnn_ckpt: str | None = None, click_labels: str | None = None, npoints: int = 16384,
        seed: int = 666, device: str = "cuda:0", cfg: stage2.RCNNConfig = annotate.ANNOTATE_CFG, rcnn_batch: int = 800,
        device_ingest: str = "off"):
    """returns (the result files written, one per scene and possibly empty; recalled per ``annotate.RECALL_THRESHOLDS``; total ground truths)"""
    dev = torch.device(device)
    s2 = load_stage2(rcnn_ckpt, device, cfg)
    scenes = kitti_io.KittiScenes(root, split, npoints=npoints, rng=np.random.RandomState(seed))     # eval_active.py seeds numpy with 666
    dataset = scan_prepare.driver_dataset(scenes, device_ingest)
    os.makedirs(out_dir, exist_ok=True)
    written, recalled, total = [], [0] * len(annotate.RECALL_THRESHOLDS), 0
    for i0 in range(0, len(scenes), batch):
        items = [dataset[i] for i in range(i0, min(i0 + batch, len(scenes)))]
        ids = [int(item["sample_id"]) for item in items]
        pts = torch.as_tensor(scan_prepare.batch_points(items, device_ingest, npoints, seed, dev)).to(dev)
        clicks, num = _pad([car_boxes(os.path.join(scenes.imageset_dir, click_labels or "label_2", "%06d.txt" % sid))[:, :3] for sid in ids], 3)
        gt, gt_num = _pad([car_boxes(os.path.join(scenes.imageset_dir, "label_2", "%06d.txt" % sid)) for sid in ids], 7)
        boxes, scores, count, _ = annotate.annotate_batch(s2, pts, torch.from_numpy(clicks).to(dev), torch.from_numpy(num).to(dev), cfg, rcnn_batch)
        r, t = annotate.annotation_recall(boxes, count, torch.from_numpy(gt), torch.from_numpy(gt_num))
        recalled, total = [a + b for a, b in zip(recalled, r)], total + t
        boxes, scores, count = boxes.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()
        for j, sid in enumerate(ids):
            k = int(count[j])
            written.append(kitti_io.save_kitti_format(sid, scenes.get_calib(sid), boxes[j, :k], out_dir, scores[j, :k],
                                                      scenes.get_image_shape(sid), "Car"))
    return written, recalled, total


def recall_table(recalled, total: int) -> str:
    lines = ["total roi bbox recall(thresh=%.3f): %d / %d = %f" % (t, r, total, r / max(total, 1))
             for t, r in zip(annotate.RECALL_THRESHOLDS, recalled)]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", required=True)
    ap.add_argument("--split", default="val")
    ap.add_argument("--out", required=True)
    ap.add_argument("--rcnn_ckpt", default=None, help="Stage-2 checkpoint (rcnn_net.* keys)")
    ap.add_argument("--click_labels", default=None, help="sub-directory of root/training whose Car objects give the clicks (default label_2)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rcnn_batch", type=int, default=800, help="instance clouds per Stage-2 forward")
    ap.add_argument("--npoints", type=int, default=16384)
    ap.add_argument("--device_ingest", default="off", choices=scan_prepare.ROUTES,
                    help="off: the reference's host sampler (default); device: project, filter and sample the raw scans in one HIP call "
                         "(ws3d_amd.scan_prepare, another random stream); host: the same rows computed on the host")
    ap.add_argument("--eval", action="store_true",
                    help="score the written files against root/training/label_2 and root/ImageSets/<split>.txt (ws3d_amd.kitti_eval)")
    a = ap.parse_args()
    files, recalled, total = run(a.root, a.split, a.out, a.batch, a.rcnn_ckpt, a.click_labels, a.npoints, rcnn_batch=a.rcnn_batch, device_ingest=a.device_ingest)
    print(f"{len(files)} result files in {a.out}")
    print(recall_table(recalled, total), end="")
    if a.eval:
        from . import kitti_eval
        result, ret = kitti_eval.evaluate(os.path.join(a.root, "training", "label_2"), a.out,
                                          os.path.join(a.root, "ImageSets", a.split + ".txt"), current_class=0)
        print(result, end="")
        for k, v in ret.items():
            print(f"{k}: {v:.4f}")


if __name__ == "__main__":
    main()
