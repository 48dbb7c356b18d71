"""KITTI object-detection AP (the official 11-point bbox / bev / 3d / aos table) with the overlaps and the
matching on the GPU: a numba-free drop-in for the reference's ``tools/kitti_object_eval_python``
(``evaluate.evaluate``, ``eval.get_official_eval_result``, ``eval.eval_class``, ``rotate_iou.rotate_iou_gpu_eval``).

    python -m ws3d_amd.kitti_eval --label_dir KITTI/object/training/label_2 --result_dir results/ \\
        --split_file KITTI/ImageSets/val.txt [--current_class Car]

Hot path (csrc/kitti_eval.hip, include/ws3d_ops.h):
  * ``ws3d_kitti_overlaps``: the per-frame (detection x ground truth) overlap blocks of every frame in one
    launch per metric -- the reference builds a cross-frame matrix per group of ~75 frames and reads only
    its diagonal blocks (calculate_iou_partly, eval.py:335-410);
  * ``ws3d_kitti_collect_scores`` / ``ws3d_kitti_count``: compute_statistics_jit (eval.py:155-273), one wave
    per (frame, threshold), and the per-threshold sums of fused_compute_statistics (eval.py:285-333).
Host work is numpy: annotation parsing (``kitti_io.read_label_annos``), clean_data (vectorised), the
threshold list (get_thresholds), the suffix maxima and the 11-point mAP.  There is no CPU fallback.
"""
from __future__ import annotations

import argparse
import io as sysio

import numpy as np

from . import kitti_io

CLASS_NAMES = ["car", "pedestrian", "cyclist"]          # clean_data (eval.py:29-32)
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting"}
N_SAMPLE_PTS = 41


def _torch():
    import torch
    from . import _lib
    return torch, _lib


def _device(device_id: int = 0):
    torch, _lib = _torch()
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.Ws3dError("ws3d_amd.kitti_eval needs a HIP device (no CPU fallback)")
    return torch.device("cuda", device_id)


def _dev(a: np.ndarray, dtype, dev):
    """a device copy; an empty array becomes one zero element, so that every pointer handed to the C ABI is valid"""
    torch, _ = _torch()
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype)).to(dev)


def _ptr(t):
    return t.data_ptr()


def _stream(dev):
    torch, _ = _torch()
    return torch.cuda.current_stream(dev).cuda_stream


# ----------------------------------------------------------------------------- host side
def get_thresholds(scores: np.ndarray, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """the score thresholds at the recall sample points (eval.py:7-25), with its running recall sum"""
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    current_recall = 0
    thresholds = []
    n = len(scores)
    for i in range(n):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < n - 1 else l_recall
        if ((r_recall - current_recall) < (current_recall - l_recall)) and (i < n - 1):
            continue
        thresholds.append(scores[i])
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def _concat(arrays, width=None, dtype=np.float64):
    arrays = list(arrays)
    if not arrays:
        return np.zeros((0,) if width is None else (0, width), dtype)
    return np.concatenate(arrays, 0)


def clean_data(gt: dict, dt: dict, current_class: int, difficulty: int):
    """clean_data (eval.py:28-81) over the concatenated boxes of all frames: ignored_gt, ignored_dt (int32,
    -1 / 0 / 1), the DontCare mask of the ground truths and the number of valid ground truths"""
    cls = CLASS_NAMES[current_class].lower()
    name = gt["name_lower"]
    height = gt["bbox"][:, 3] - gt["bbox"][:, 1]
    valid = np.where(name == cls, 1, np.where(((cls == "pedestrian") & (name == "person_sitting")) |
                                              ((cls == "car") & (name == "van")), 0, -1))
    ignore = ((gt["occluded"] > MAX_OCCLUSION[difficulty]) | (gt["truncated"] > MAX_TRUNCATION[difficulty]) |
              (height <= MIN_HEIGHT[difficulty]))
    ignored_gt = np.where((valid == 1) & ~ignore, 0, np.where((valid == 0) | (ignore & (valid == 1)), 1, -1)).astype(np.int32)
    dt_height = np.abs(dt["bbox"][:, 3] - dt["bbox"][:, 1])
    ignored_dt = np.where(dt_height < MIN_HEIGHT[difficulty], 1, np.where(dt["name_lower"] == cls, 0, -1)).astype(np.int32)
    return int((ignored_gt == 0).sum()), ignored_gt, ignored_dt


def _flatten(annos: list) -> dict:
    """the frames' annotation arrays concatenated, with CSR offsets"""
    n = np.array([len(a["name"]) for a in annos], dtype=np.int64)
    off = np.zeros(len(annos) + 1, dtype=np.int64)
    np.cumsum(n, out=off[1:])
    names = _concat([np.asarray(a["name"]).astype(str) for a in annos], dtype=str)
    return {
        "n": n, "off": off, "name": names, "name_lower": np.char.lower(names),
        "bbox": _concat([np.asarray(a["bbox"], np.float64).reshape(-1, 4) for a in annos], 4),
        "alpha": _concat([np.asarray(a["alpha"], np.float64).reshape(-1) for a in annos]),
        "score": _concat([np.asarray(a["score"], np.float64).reshape(-1) for a in annos]) if all("score" in a for a in annos) else None,
        "occluded": _concat([np.asarray(a["occluded"], np.float64).reshape(-1) for a in annos]),
        "truncated": _concat([np.asarray(a["truncated"], np.float64).reshape(-1) for a in annos]),
        "location": _concat([np.asarray(a["location"], np.float64).reshape(-1, 3) for a in annos], 3),
        "dimensions": _concat([np.asarray(a["dimensions"], np.float64).reshape(-1, 3) for a in annos], 3),
        "rotation_y": _concat([np.asarray(a["rotation_y"], np.float64).reshape(-1) for a in annos]),
    }


def _boxes(fl: dict, metric: int) -> np.ndarray:
    if metric == 0:
        return fl["bbox"]
    if metric == 1:     # calculate_iou_partly (eval.py:360-373): (x, z, l, w, ry)
        return np.concatenate([fl["location"][:, [0, 2]], fl["dimensions"][:, [0, 2]], fl["rotation_y"][:, None]], 1)
    return np.concatenate([fl["location"], fl["dimensions"], fl["rotation_y"][:, None]], 1)


class _Frames:
    """the device side of one (gt_annos, dt_annos) pair: offsets, per-box data and the overlap blocks of each metric"""

    def __init__(self, gt_annos: list, dt_annos: list, device_id: int = 0):
        if len(gt_annos) != len(dt_annos):
            raise ValueError(f"{len(gt_annos)} ground-truth frames but {len(dt_annos)} result frames")
        self.dev = _device(device_id)
        self.frames = len(gt_annos)
        self.gt, self.dt = _flatten(gt_annos), _flatten(dt_annos)
        if self.dt["score"] is None:
            raise ValueError("detections without 'score'")
        pairs = self.gt["n"] * self.dt["n"]
        out_off = np.zeros(self.frames + 1, np.int64)
        np.cumsum(pairs, out=out_off[1:])
        self.max_pairs = int(pairs.max()) if self.frames else 0
        self.max_dt = int(self.dt["n"].max()) if self.frames else 0
        self.total_pairs = int(out_off[-1])
        self.out_off_host = out_off
        self.gt_off = _dev(self.gt["off"], np.int32, self.dev)
        self.dt_off = _dev(self.dt["off"], np.int32, self.dev)
        self.out_off = _dev(out_off, np.int64, self.dev)
        self.dt_score = _dev(self.dt["score"], np.float64, self.dev)
        self.dt_alpha = _dev(self.dt["alpha"], np.float64, self.dev)
        self.gt_alpha = _dev(self.gt["alpha"], np.float64, self.dev)
        self.dt_bbox = _dev(self.dt["bbox"], np.float64, self.dev)
        self.frame_of_gt = np.repeat(np.arange(self.frames), self.gt["n"])
        self._overlaps = {}

    def overlaps(self, metric: int, criterion: int = -1):
        """(total_pairs,) float64 on the device: frame f's (n_dt, n_gt) block at out_off[f]"""
        key = (metric, criterion)
        if key not in self._overlaps:
            torch, _lib = _torch()
            out = torch.empty(max(self.total_pairs, 1), dtype=torch.float64, device=self.dev)
            gtb = _dev(_boxes(self.gt, metric), np.float64, self.dev)
            dtb = _dev(_boxes(self.dt, metric), np.float64, self.dev)
            _lib.check(_lib.load().ws3d_kitti_overlaps(metric, criterion, self.frames, self.max_pairs, _ptr(self.gt_off), _ptr(self.dt_off),
                                                       _ptr(self.out_off), _ptr(dtb), _ptr(gtb), out.data_ptr(), _stream(self.dev)),
                       "ws3d_kitti_overlaps")
            self._overlaps[key] = out
        return self._overlaps[key]

    def blocks(self, metric: int, criterion: int = -1) -> list:
        """the per-frame blocks on the host (the ``overlaps`` list of calculate_iou_partly)"""
        ov = self.overlaps(metric, criterion).cpu().numpy()
        o, g, d = self.out_off_host, self.gt["n"], self.dt["n"]
        return [ov[o[f]:o[f + 1]].reshape(d[f], g[f]) for f in range(self.frames)]

    def prepare(self, current_class: int, difficulty: int):
        num_valid, ignored_gt, ignored_dt = clean_data(self.gt, self.dt, current_class, difficulty)
        dc = self.gt["name"] == "DontCare"
        dc_n = np.bincount(self.frame_of_gt[dc], minlength=self.frames) if self.frames else np.zeros(0, np.int64)
        dc_off = np.zeros(self.frames + 1, np.int64)
        np.cumsum(dc_n, out=dc_off[1:])
        return (num_valid, _dev(ignored_gt, np.int32, self.dev), _dev(ignored_dt, np.int32, self.dev),
                _dev(dc_off, np.int32, self.dev), _dev(self.gt["bbox"][dc].reshape(-1, 4), np.float64, self.dev))

    def collect_scores(self, metric: int, ignored_gt, ignored_dt, min_overlap: float) -> np.ndarray:
        """the thresholds list of the collection pass (eval.py:480-494): matched scores in (frame, gt) order"""
        torch, _lib = _torch()
        n = max(int(self.gt["off"][-1]), 1)
        score = torch.empty(n, dtype=torch.float64, device=self.dev)
        flag = torch.empty(n, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.load().ws3d_kitti_collect_scores(
            self.frames, self.max_dt, _ptr(self.gt_off), _ptr(self.dt_off), _ptr(self.out_off), _ptr(self.overlaps(metric)),
            _ptr(ignored_gt), _ptr(ignored_dt), _ptr(self.dt_score), float(min_overlap), score.data_ptr(), flag.data_ptr(),
            _stream(self.dev)), "ws3d_kitti_collect_scores")
        m = int(self.gt["off"][-1])
        s, f = score[:m].cpu().numpy(), flag[:m].cpu().numpy()
        return s[f == 1]

    def count(self, metric: int, thresholds: np.ndarray, ignored_gt, ignored_dt, dc_off, dc_bbox, min_overlap: float,
              compute_aos: bool) -> np.ndarray:
        """pr (T, 4) = tp, fp, fn, similarity per threshold (fused_compute_statistics over all frames)"""
        torch, _lib = _torch()
        T = len(thresholds)
        if T == 0:
            return np.zeros((0, 4))
        lib = _lib.load()
        th = _dev(np.asarray(thresholds, np.float64), np.float64, self.dev)
        pr = torch.empty((T, 4), dtype=torch.float64, device=self.dev)
        ws = torch.empty(max(int(lib.ws3d_kitti_count_workspace_bytes(self.frames, T)), 16), dtype=torch.uint8, device=self.dev)
        _lib.check(lib.ws3d_kitti_count(
            metric, self.frames, self.max_dt, T, th.data_ptr(), _ptr(self.gt_off), _ptr(self.dt_off), _ptr(dc_off), _ptr(self.out_off),
            _ptr(self.overlaps(metric)), _ptr(ignored_gt), _ptr(ignored_dt), _ptr(self.dt_score), _ptr(self.dt_alpha), _ptr(self.gt_alpha),
            _ptr(self.dt_bbox), _ptr(dc_bbox), float(min_overlap), int(bool(compute_aos)), ws.data_ptr(), ws.numel(), pr.data_ptr(),
            _stream(self.dev)), "ws3d_kitti_count")
        return pr.cpu().numpy()


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=50,
               frames: _Frames | None = None):
    """eval_class (eval.py:443-554): dict of ``recall`` / ``precision`` / ``orientation`` arrays of shape
    [num_class, num_difficulty, num_minoverlap, 41].  ``num_parts`` is accepted for the reference's signature; every
    frame is evaluated in one launch, so any frame count works."""
    fr = frames if frames is not None else _Frames(gt_annos, dt_annos)
    num_minoverlap, num_class, num_difficulty = len(min_overlaps), len(current_classes), len(difficultys)
    precision = np.zeros([num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS])
    recall = np.zeros([num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS])
    aos = np.zeros([num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS])
    for m, current_class in enumerate(current_classes):
        for l, difficulty in enumerate(difficultys):
            num_valid, ignored_gt, ignored_dt, dc_off, dc_bbox = fr.prepare(current_class, difficulty)
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                thresholds = np.array(get_thresholds(fr.collect_scores(metric, ignored_gt, ignored_dt, min_overlap), num_valid))
                pr = fr.count(metric, thresholds, ignored_gt, ignored_dt, dc_off, dc_bbox, min_overlap, compute_aos)
                T = len(thresholds)
                with np.errstate(divide="ignore", invalid="ignore"):
                    recall[m, l, k, :T] = pr[:, 0] / (pr[:, 0] + pr[:, 2])
                    precision[m, l, k, :T] = pr[:, 0] / (pr[:, 0] + pr[:, 1])
                    if compute_aos:
                        aos[m, l, k, :T] = pr[:, 3] / (pr[:, 0] + pr[:, 1])
                for arr in ((precision, recall, aos) if compute_aos else (precision, recall)):
                    row = arr[m, l, k]
                    row[:T] = np.maximum.accumulate(row[::-1])[::-1][:T]     # np.max(row[i:]) for i < T
    return {"recall": recall, "precision": precision, "orientation": aos}


def get_mAP(prec):
    """11-point AP (eval.py:557-561)"""
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def print_str(value, *arg, sstream=None):
    if sstream is None:
        sstream = sysio.StringIO()
    sstream.truncate(0)
    sstream.seek(0)
    print(value, *arg, file=sstream)
    return sstream.getvalue()


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False):
    """do_eval (eval.py:572-591): the three metrics over the same frames (offsets and box data uploaded once)"""
    difficultys = [0, 1, 2]
    fr = _Frames(gt_annos, dt_annos)
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 0, min_overlaps, compute_aos, frames=fr)
    mAP_bbox = get_mAP(ret["precision"])
    mAP_aos = get_mAP(ret["orientation"]) if compute_aos else None
    mAP_bev = get_mAP(eval_class(gt_annos, dt_annos, current_classes, difficultys, 1, min_overlaps, frames=fr)["precision"])
    mAP_3d = get_mAP(eval_class(gt_annos, dt_annos, current_classes, difficultys, 2, min_overlaps, frames=fr)["precision"])
    return mAP_bbox, mAP_bev, mAP_3d, mAP_aos


def get_official_eval_result(gt_annos, dt_annos, current_classes):
    """the official AP table (eval.py:614-684): same string, same ``ret_dict`` keys"""
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25], [0.5, 0.25, 0.25, 0.5, 0.25]])
    min_overlaps = np.stack([overlap_0_7, overlap_0_5], axis=0)  # [2, 3, 5]
    name_to_class = {v: n for n, v in CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = min_overlaps[:, :, current_classes]
    result = ""
    compute_aos = False     # alpha is valid unless the first non-empty frame's first detection says -10
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            if anno["alpha"][0] != -10:
                compute_aos = True
            break
    mAPbbox, mAPbev, mAP3d, mAPaos = do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos)
    ret_dict = {}
    for j, curcls in enumerate(current_classes):
        for i in range(min_overlaps.shape[0]):
            result += print_str((f"{CLASS_TO_NAME[curcls]} " "AP@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])))
            result += print_str(f"bbox AP:{mAPbbox[j, 0, i]:.4f}, {mAPbbox[j, 1, i]:.4f}, {mAPbbox[j, 2, i]:.4f}")
            result += print_str(f"bev  AP:{mAPbev[j, 0, i]:.4f}, {mAPbev[j, 1, i]:.4f}, {mAPbev[j, 2, i]:.4f}")
            result += print_str(f"3d   AP:{mAP3d[j, 0, i]:.4f}, {mAP3d[j, 1, i]:.4f}, {mAP3d[j, 2, i]:.4f}")
            if compute_aos:
                result += print_str(f"aos  AP:{mAPaos[j, 0, i]:.2f}, {mAPaos[j, 1, i]:.2f}, {mAPaos[j, 2, i]:.2f}")
    for metric, arr in (("3d", mAP3d), ("bev", mAPbev), ("image", mAPbbox)):
        for d, diff in enumerate(("easy", "moderate", "hard")):
            ret_dict[f"Car_{metric}_{diff}"] = arr[0, d, 0]
    return result, ret_dict


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """rotated-box overlap (rotate_iou.py:291-329): boxes (N, 5), query_boxes (K, 5) as (x, z, l, w, ry) -> (N, K) float32,
    devRotateIoUEval(query_box, box, criterion) per pair, criterion -1 / 0 / 1 / 2.  One launch of ws3d_kitti_overlaps."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    query_boxes = np.asarray(query_boxes, dtype=np.float32).reshape(-1, 5)
    N, K = boxes.shape[0], query_boxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.float32)
    torch, _lib = _torch()
    dev = _device(device_id)
    out = torch.empty(N * K, dtype=torch.float64, device=dev)
    b, q = _dev(boxes, np.float64, dev), _dev(query_boxes, np.float64, dev)
    gt_off = _dev(np.array([0, K]), np.int32, dev)
    dt_off = _dev(np.array([0, N]), np.int32, dev)
    out_off = _dev(np.array([0, N * K]), np.int64, dev)
    _lib.check(_lib.load().ws3d_kitti_overlaps(1, int(criterion), 1, N * K, gt_off.data_ptr(), dt_off.data_ptr(), out_off.data_ptr(),
                                               b.data_ptr(), q.data_ptr(), out.data_ptr(), _stream(dev)), "ws3d_kitti_overlaps")
    return out.cpu().numpy().astype(np.float32).reshape(N, K)


def filter_annos_low_score(image_annos, thresh):
    """kitti_common.filter_annos_low_score (kitti_common.py:190-201): keep detections with score >= thresh"""
    out = []
    for anno in image_annos:
        keep = [i for i, s in enumerate(anno["score"]) if s >= thresh]
        out.append({k: v[keep] for k, v in anno.items()})
    return out


def _read_imageset_file(path):
    with open(path) as f:
        return [int(line) for line in f.readlines() if line.strip()]


def evaluate(label_path, result_path, label_split_file, current_class=0, coco=False, score_thresh=-1):
    """evaluate.evaluate (evaluate.py:14-29): (result_str, ret_dict) of the result files in ``result_path`` against the
    labels of the split's ids"""
    if coco:
        raise NotImplementedError("COCO-style AP (get_coco_eval_result) is not provided by ws3d_amd.kitti_eval")
    dt_annos = kitti_io.read_label_annos(result_path)
    if score_thresh > 0:
        dt_annos = filter_annos_low_score(dt_annos, score_thresh)
    gt_annos = kitti_io.read_label_annos(label_path, _read_imageset_file(label_split_file))
    return get_official_eval_result(gt_annos, dt_annos, current_class)


def _class_arg(v: str):
    parts = [p for p in v.split(",") if p]
    vals = [int(p) if p.lstrip("-").isdigit() else p for p in parts]
    return vals if len(vals) > 1 else vals[0]


def main(argv=None):
    ap = argparse.ArgumentParser(description="KITTI object-detection AP (official 11-point table) on the GPU")
    ap.add_argument("--label_dir", required=True, help="directory of %%06d.txt label files (training/label_2)")
    ap.add_argument("--result_dir", required=True, help="directory of %%06d.txt result files")
    ap.add_argument("--split_file", required=True, help="ImageSets/<split>.txt: the ids to evaluate")
    ap.add_argument("--current_class", type=_class_arg, default=0, help="Car / Pedestrian / Cyclist or 0 / 1 / 2; comma-separated for several")
    ap.add_argument("--score_thresh", type=float, default=-1)
    a = ap.parse_args(argv)
    result, _ = evaluate(a.label_dir, a.result_dir, a.split_file, a.current_class, score_thresh=a.score_thresh)
    print(result, end="")


if __name__ == "__main__":
    main()
