"""The object database of the ground-truth paste augmentation (``gt_paste``): writer, reader and the synthetic stand-in.

    python -m ws3d_amd.gt_database --root R --split train [--label_dir label_2] [--easy_min_points 512] [--mimic_points 100]
                                   --out R/ImageSets/aug_gt_database.pkl

The reference reads ``ImageSets/aug_gt_database.pkl`` (lib/datasets/kitti_rcnn_dataset.py:75-90) but ships NO program that writes
it: the generator is absent from the reference.  The fields below are read off what its reader and its paste touch (:78, :84,
:259-263, :306-314, :360-370) -- a list of one dict per labelled object:

  sample_id         the scan the object comes from (the reader keeps ``sample_id <= last training id``)
  points            (n,3) float32, the scan points inside the object's box; x and z relative to the box centre, y ABSOLUTE (the
                    paste adds the new centre's x and z only)
  intensity         (n,) float32, raw reflectance in [0, 1)
  gt_box3d          (7,) float32 [x, y, z, h, w, l, ry] with x = z = 0
  obj               ``kitti_io.Object3d`` of the label line (pos x = z = 0 like the box)
  presampling_flag  n > easy_min_points: the reader's "easy(pt_num>512)"; the others are its "hard"
  sampled_mask      (n,) bool, all True (the reader indexes points and intensity with it before it thins an easy object)
  mimic_index       (mimic_points,) int32, flagged records only -- OURS, not the reference's: the furthest-point-sampling picks on
                    ``points[sampled_mask]``, computed once here instead of once per draw (see ``gt_paste``)

One record per object that passes the trainer's label filter (``keep_object``: Car / Van inside PC_AREA_SCOPE, like
``KittiCenters._objects``) and holds at least one point.  The crop is ``pts_in_boxes3d`` -- the HIP kernel when a device is
present, its numpy twin ``points_in_boxes_host`` otherwise -- and all flagged objects of a chunk of scans are sampled by ONE
``pn2_ops.furthest_point_sample_ragged`` call (one launch on the device).  Both routes write identical records.
"""
from __future__ import annotations

import argparse
import copy
import pickle
from typing import Iterable, List, Optional

import numpy as np

from . import kitti_io

EASY_MIN_POINTS, MIMIC_POINTS = 512, 100          # kitti_rcnn_dataset.py:89, :311
NEED_HARD, NEED_EASY = 5, 10                      # what one paste draws (AUG_NUM / 3 and 2 AUG_NUM / 3)


def keep_object(obj) -> bool:
    """the TRAIN-mode filtrate_objects of the reference (kitti_rcnn_dataset.py:115-135), as ``KittiCenters._objects`` applies it"""
    (x0, x1), (y0, y1), (z0, z1) = kitti_io.PC_AREA_SCOPE
    return obj.cls_type in ("Car", "Van") and x0 <= obj.pos[0] <= x1 and y0 <= obj.pos[1] <= y1 and z0 <= obj.pos[2] <= z1


def points_in_boxes_host(pts: np.ndarray, boxes3d: np.ndarray) -> np.ndarray:
    """numpy twin of ``ws3d_pts_in_boxes3d`` (csrc/roipool3d.hip make_frame / pt_in_frame; roipool3d_kernel.cu:14-28): pts (N,3),
    boxes3d (M,7) float32 -> (M,N) bool, the same float32 operations in the same order"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    boxes3d = np.ascontiguousarray(boxes3d, dtype=np.float32).reshape(-1, 7)
    out = np.zeros((boxes3d.shape[0], pts.shape[0]), dtype=bool)
    half, ten = np.float32(0.5), np.float32(10.0)
    for i, b in enumerate(boxes3d):
        cy = np.float32(np.float64(b[1]) - np.float64(b[3]) / 2.0)
        cosa, sina = np.float32(np.cos(np.float64(b[6]))), np.float32(np.sin(np.float64(b[6])))
        dx, dy, dz = pts[:, 0] - b[0], pts[:, 1] - cy, pts[:, 2] - b[2]
        x_rot = dx * cosa + dz * (-sina)
        z_rot = dx * sina + dz * cosa
        with np.errstate(invalid="ignore"):
            out[i] = ((np.abs(x_rot) <= b[5] * half) & (np.abs(z_rot) <= b[4] * half) & ~(np.abs(dx) > ten) & ~(np.abs(dy) > b[3] * half)
                      & ~(np.abs(dz) > ten))
    return out


def _crop_masks(pts32: np.ndarray, boxes: np.ndarray, device) -> np.ndarray:
    if device is None:
        return points_in_boxes_host(pts32, boxes)
    import torch
    from . import compat as _C
    flag = _C.pts_in_boxes3d_device(torch.from_numpy(pts32).to(device), torch.from_numpy(boxes).to(device))
    return flag.cpu().numpy() > 0


def _default_device():
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None


def _sample_chunk(records: List[dict], mimic_points: int, device) -> None:
    """mimic_index of every flagged record of the chunk, in one ragged call"""
    import torch
    from . import pn2_ops
    flagged = [r for r in records if r["presampling_flag"]]
    if not flagged:
        return
    clouds = [r["points"][r["sampled_mask"]] for r in flagged]
    xyz = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds, 0), dtype=np.float32))
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32))
    if device is not None:
        xyz, offsets = xyz.to(device), offsets.to(device)
    idx = pn2_ops.furthest_point_sample_ragged(xyz, offsets, mimic_points).cpu().numpy()
    for r, row in zip(flagged, idx):
        r["mimic_index"] = np.ascontiguousarray(row, dtype=np.int32)


def build_gt_database(scenes: Iterable, easy_min_points: int = EASY_MIN_POINTS, mimic_points: int = MIMIC_POINTS, device="auto",
                      chunk: int = 8) -> List[dict]:
    """scenes: iterable of (sample_id, pts_rect (n,3), intensity (n,), objects [Object3d]) -> the list of records (module
    docstring).  device: "auto" (the current HIP device when there is one, else the host), None (host) or a torch device.
    `chunk` scans share one furthest-point-sampling call."""
    if easy_min_points < mimic_points:
        raise ValueError(f"easy_min_points={easy_min_points} < mimic_points={mimic_points}: an easy object must hold the points it is thinned to")
    if device == "auto":
        device = _default_device()
    records, pending, scans = [], [], 0
    for sample_id, pts_rect, intensity, objects in scenes:
        objs = [o for o in objects if keep_object(o)]
        pts32 = np.ascontiguousarray(np.asarray(pts_rect)[:, :3], dtype=np.float32)
        inten = np.asarray(intensity, dtype=np.float32).reshape(-1)
        if objs and pts32.shape[0]:
            boxes = np.stack([o.box3d() for o in objs]).astype(np.float32)
            for o, box, mask in zip(objs, boxes, _crop_masks(pts32, boxes, device)):
                n = int(mask.sum())
                if n == 0:
                    continue
                pts = pts32[mask].copy()
                pts[:, 0] -= box[0]
                pts[:, 2] -= box[2]
                obj = copy.deepcopy(o)
                obj.pos[0] = obj.pos[2] = 0.0
                box = box.copy()
                box[0] = box[2] = 0.0
                pending.append({"sample_id": int(sample_id), "points": pts, "intensity": inten[mask].copy(), "gt_box3d": box, "obj": obj,
                                "presampling_flag": bool(n > easy_min_points), "sampled_mask": np.ones(n, dtype=bool)})
        scans += 1
        if scans % max(chunk, 1) == 0:
            _sample_chunk(pending, mimic_points, device)
            records += pending
            pending = []
    _sample_chunk(pending, mimic_points, device)
    return records + pending


class GtDatabase:
    """what one paste draws from: ``easy`` (presampling_flag) and ``hard`` record lists, every easy record with a ``mimic_index``"""

    def __init__(self, records: Iterable[dict], last_sample_id: Optional[int] = None, mimic_points: int = MIMIC_POINTS):
        records = [r for r in records if last_sample_id is None or int(r["sample_id"]) <= int(last_sample_id)]   # :78
        self.mimic_points = int(mimic_points)
        self.easy = [r for r in records if r["presampling_flag"]]                                                 # :83-87
        self.hard = [r for r in records if not r["presampling_flag"]]
        if len(self.hard) < NEED_HARD or len(self.easy) < NEED_EASY:
            raise ValueError("the ground-truth database is too short to draw from: %d hard and %d easy objects%s, one paste needs %d and %d"
                             % (len(self.hard), len(self.easy), "" if last_sample_id is None else " with sample_id <= %d" % int(last_sample_id),
                                NEED_HARD, NEED_EASY))
        missing = [r for r in self.easy if "mimic_index" not in r or len(r["mimic_index"]) != self.mimic_points]
        for r in missing:             # a pickle made for the reference: sampled here, on the host route
            r["points"] = np.ascontiguousarray(np.asarray(r["points"]).reshape(-1, 3), dtype=np.float32)
            r["sampled_mask"] = np.asarray(r["sampled_mask"], dtype=bool).reshape(-1)
        _sample_chunk(missing, self.mimic_points, None)

    def __len__(self):
        return len(self.easy) + len(self.hard)


class _ForeignObject:
    """stands in for the reference's own ``lib.utils.object3d.Object3d`` when a pickle made for it is read without that package"""


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            if name == "Object3d":
                return _ForeignObject
            raise


def save_gt_database(records: List[dict], path: str) -> None:
    with open(path, "wb") as f:
        pickle.dump(list(records), f, protocol=pickle.HIGHEST_PROTOCOL)


def load_gt_database(path: str, last_sample_id: Optional[int] = None, mimic_points: int = MIMIC_POINTS) -> GtDatabase:
    """read a database file; ``last_sample_id``: the reader's ``sample_id <= last training id`` filter.  Raises ValueError with the
    counts when fewer than 5 hard or 10 easy objects remain."""
    with open(path, "rb") as f:
        records = _Unpickler(f).load()
    return GtDatabase(records, last_sample_id, mimic_points)


# ----------------------------------------------------------------------------- sources
def kitti_scenes(root: str, split: str = "train", label_dir: str = "label_2"):
    """(sample_id, pts_rect, intensity, objects) of every scan of a KITTI object directory that has a label file"""
    import os
    scenes = kitti_io.KittiScenes(root, split)
    for sid in scenes.sample_id_list:
        path = os.path.join(scenes.imageset_dir, label_dir, "%06d.txt" % sid)
        if not os.path.isfile(path):
            continue
        lidar = scenes.get_lidar(sid)
        yield sid, scenes.get_calib(sid).lidar_to_rect(lidar[:, 0:3]), lidar[:, 3], kitti_io.read_label_file(path)


SYNTHETIC_EASY_MIN_POINTS = 128     # ray-cast scenes: about one car in fifty exceeds 512 points, too few to draw 10 easy ones from


def synthetic_scenes(count: int, config_id: int = 8):
    """`count` ray-cast ``synth.hdl64_scan`` scenes with their cars as Object3d labels"""
    from . import synth
    for i in range(count):
        scan, boxes = synth.hdl64_scan(1000 * config_id + i, return_boxes=True)
        objs = [kitti_io.Object3d("Car", 0.0, 0.0, 0.0, np.zeros(4, dtype=np.float32), float(b[3]), float(b[4]), float(b[5]),
                                  b[:3].astype(np.float32), float(b[6])) for b in boxes]
        yield i, scan[:, :3], scan[:, 3], objs


def main():
    ap = argparse.ArgumentParser(description="write the ground-truth paste database of a KITTI object directory")
    ap.add_argument("--root", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--label_dir", default="label_2")
    ap.add_argument("--easy_min_points", type=int, default=EASY_MIN_POINTS)
    ap.add_argument("--mimic_points", type=int, default=MIMIC_POINTS)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    records = build_gt_database(kitti_scenes(a.root, a.split, a.label_dir), a.easy_min_points, a.mimic_points)
    save_gt_database(records, a.out)
    easy = sum(1 for r in records if r["presampling_flag"])
    print("%s: %d objects (easy(pt_num>%d): %d, hard: %d)" % (a.out, len(records), a.easy_min_points, easy, len(records) - easy))


if __name__ == "__main__":
    main()
