"""Click-driven annotation: a person's BEV clicks on object centres in, refined 3-D boxes out -- what WS3D's trained Stage-2
network is for.  Counterpart of the reference's ``tools/eval_active.py`` for a padded batch of scenes:

    clicks -> ``click_scores`` (click_gaussian_mask, eval_active.py:187, 656-675) and the 5 x 5 grid of jittered candidates per
    click (eval_active.py:198-209), one call of csrc/click.hip -> ``instance_ops.instance_clouds`` around every candidate ->
    ``Stage2Net.rcnn_forward`` over the real candidates in chunks -> ``stage2.detections`` under ``ANNOTATE_CFG`` (the two score
    thresholds and the 0.01 BEV sweep of eval_active.py:324, 463, 486-499; no size window) -> per scene the kept boxes and the
    click each came from.

No Stage-1 network takes part.  ``annotate_kitti`` is the directory driver.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import losses, stage2
from ._lib import Ws3dError

ANNOTATE_CFG = dataclasses.replace(stage2.DEFAULT_CFG, size_window=((-float("inf"), float("inf")),) * 3)
MAX_CANDIDATES = 16384      # stage2.detections sorts a scene's candidates through compat.topk_sorted
RECALL_THRESHOLDS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)       # eval_active.py's thresh_list


def grid_offsets(side: int = 5, step: float = 0.1) -> list:
    """the jitter grid's steps as the fp32 values torch adds in ``sample[:, 0] += 0.1 * i`` (eval_active.py:203-207): the Python
    float step * (m - side // 2) rounded to fp32"""
    return [np.float32(step * (m - side // 2)) for m in range(side)]


def _prep(pts, clicks, num):
    if pts.dim() != 3 or pts.shape[2] != 4 or clicks.dim() != 3 or clicks.shape[0] != pts.shape[0] or clicks.shape[2] != 3:
        raise Ws3dError(f"annotate: pts (B,N,4) and clicks (B,K,3) expected, got {tuple(pts.shape)} {tuple(clicks.shape)}")
    pts = pts.float().contiguous()
    clicks = clicks.to(pts.device).float().contiguous()
    if num is not None:
        num = num.to(device=pts.device, dtype=torch.int32).contiguous()
    return pts, clicks, num


def _click_prepare(pts, clicks, num, side, step, centre_y):
    from . import compat as _C
    B, N, K = pts.shape[0], pts.shape[1], clicks.shape[1]
    score = torch.empty((B, N), dtype=torch.float32, device=pts.device)
    cand = torch.empty((B, side * side * K, 3), dtype=torch.float32, device=pts.device)
    cand_num = torch.empty((B,), dtype=torch.int32, device=pts.device)
    _C.click_prepare(pts, clicks, num, grid_offsets(side, step), losses.GAUSS_HEIGHT, losses.GAUSS_STATUS, losses.GAUSS_COV, centre_y,
                     score, cand, cand_num)
    return score, cand, cand_num


def click_scores(pts: torch.Tensor, clicks: torch.Tensor, num: torch.Tensor | None = None) -> torch.Tensor:
    """pts (B,N,4), clicks (B,K,3) (y is not read), num (B) clicks per scene (None: all K) -> score (B,N) fp32 in [0,1]: the
    Gaussian of a point's distance to the nearest click, ``losses.gaussian_center_labels``' cls (click_gaussian_mask,
    eval_active.py:656-675), 0 everywhere in a scene without clicks.  GPU tensors: csrc/click.hip in fp32; CPU tensors:
    ``gaussian_center_labels`` itself, scene by scene."""
    pts, clicks, num = _prep(pts, clicks, num)
    if pts.is_cuda:
        return _click_prepare(pts, clicks, num, 1, 0.0, 0.0)[0]
    out = torch.empty(pts.shape[:2], dtype=torch.float32)
    for b in range(pts.shape[0]):
        k = clicks.shape[1] if num is None else min(max(int(num[b]), 0), clicks.shape[1])
        out[b] = torch.from_numpy(np.asarray(losses.gaussian_center_labels(pts[b, :, :3].numpy(), clicks[b, :k].numpy())[0], dtype=np.float32))
    return out


def annotate_inputs(pts: torch.Tensor, clicks: torch.Tensor, num: torch.Tensor | None = None, radius: float = 4.0, sampled_pt_num: int = 512,
                    ground_y: float = 1.65, side: int = 5, step: float = 0.1) -> dict:
    """The Stage-2 inputs of every jittered candidate of every click (eval_active.py:187-272) for a batch, in two kernel calls and
    without a host synchronisation.  pts (B,N,4), clicks (B,K,3), num (B) clicks per scene (None: all K).  Returns the dict
    ``stage1.stage2_inputs`` returns, under the names ``rcnn_forward`` reads, for Kc = side*side*K candidate slots per scene:
      cur_box_point (B,Kc,S,3), cur_box_reflect (B,Kc,S,1), train_mask (B,Kc,S,1) = (click_score > 0.5) - 0.5, count (B,Kc) int32
      members per cylinder (not capped), center (B,Kc,3) with y = ground_y, num (B) int32 = side*side*num clicks, and click_score (B,N).
    Candidate slot j of a scene with n clicks is grid cell g = j // n (x offset g // side, z offset g % side) of click j % n: the
    reference's order, whole click lists concatenated.

    The reference first drops the points farther than 4 m from every candidate (eval_active.py:212-217); that removes no member of
    any cylinder and keeps scene order, so the cut alone reproduces it.  Like ``detect_kitti``, this route feeds the first
    ``sampled_pt_num`` members of a cylinder, repeated cyclically, where the reference feeds all of them."""
    from . import instance_ops
    pts, clicks, num = _prep(pts, clicks, num)
    if side * side * clicks.shape[1] > MAX_CANDIDATES:
        raise Ws3dError(f"annotate: {side * side} x {clicks.shape[1]} candidates per scene exceed the {MAX_CANDIDATES} the detection tail sorts")
    score, cand, cand_num = _click_prepare(pts, clicks, num, side, step, ground_y)
    rows, _, count = instance_ops.instance_clouds(pts, score, cand, cand_num, radius, sampled_pt_num, mask_mode=1, mask_thresh=0.5)
    return {'cur_box_point': rows[..., 0:3], 'cur_box_reflect': rows[..., 3:4], 'train_mask': rows[..., 4:5], 'count': count,
            'center': cand, 'num': cand_num, 'click_score': score}


@torch.no_grad()
def annotate_batch(s2, pts: torch.Tensor, clicks: torch.Tensor, num: torch.Tensor | None = None, cfg: stage2.RCNNConfig = ANNOTATE_CFG,
                   rcnn_batch: int = 800, sampled_pt_num: int = 512, side: int = 5, step: float = 0.1):
    """s2: a ``Stage2Net`` in eval mode; pts (B,N,4); clicks (B,K,3); num (B) clicks per scene (None: all K) ->
    boxes (B,Kc,7), scores (B,Kc) = rcnn_iou descending, count (B,), click (B,Kc) int64: the index of the click every kept box came
    from, -1 in the padding; Kc = side*side*K.  One host synchronisation (the list of real candidates, ``rcnn_over_real_slots``)."""
    from .detect_kitti import rcnn_over_real_slots
    B, Kc = pts.shape[0], side * side * clicks.shape[1]
    if B == 0 or Kc == 0:
        dev = pts.device
        return (torch.zeros((B, Kc, 7), device=dev), torch.zeros((B, Kc), device=dev), torch.zeros((B,), dtype=torch.int64, device=dev),
                torch.full((B, Kc), -1, dtype=torch.int64, device=dev))
    inp = annotate_inputs(pts, clicks, num, sampled_pt_num=sampled_pt_num, ground_y=cfg.ground_y, side=side, step=step)
    boxes, scores, count, slot = stage2.detections(rcnn_over_real_slots(s2, inp, rcnn_batch), inp['center'], inp['num'], cfg, return_index=True)
    clicks_per_scene = (inp['num'] // (side * side)).to(torch.int64).clamp(min=1)[:, None]
    return boxes, scores, count, torch.where(slot >= 0, slot % clicks_per_scene, slot)


def annotation_recall(boxes: torch.Tensor, count: torch.Tensor, gt_boxes: torch.Tensor, gt_num: torch.Tensor, thresholds=RECALL_THRESHOLDS):
    """boxes (B,K,7) with count (B) real rows per scene, gt_boxes (B,G,7) with gt_num (B) -> (recalled: one int per threshold, the
    ground truths whose largest 3-D IoU against the scene's boxes exceeds it; total ground truths).  eval_active.py:341-365, scene
    by scene on the host with ``iou3d_ops.boxes_iou3d_gpu``."""
    from . import iou3d_ops
    recalled, total = [0] * len(thresholds), 0
    for b in range(boxes.shape[0]):
        n, g = int(count[b]), int(gt_num[b])
        total += g
        if n == 0 or g == 0:
            continue
        best = iou3d_ops.boxes_iou3d_gpu(boxes[b, :n].float().contiguous(), gt_boxes[b, :g].to(boxes.device).float().contiguous())[1].max(dim=0)[0]
        for i, t in enumerate(thresholds):
            recalled[i] += int((best > t).sum())
    return recalled, total
