"""Float64 restatements of the Stage-2 training losses for the tests: written from the reference's text
(lib/net/train_functions.py:230-516, lib/utils/loss_utils.py:151-338, lib/utils/kitti_utils.py:104-147,
lib/utils/iou3d/iou3d_utils.py:21-56) in the reference's order -- selections and host branches, not masks -- with none of the
package's code.  The rotated BEV overlap comes from the fp32 CPU oracle, as in the fixture's generator."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MEAN_SIZE = np.array([1.5, 1.6, 3.9], dtype=np.float32)     # cfg.CLS_MEAN_SIZE[0], a float32 array in the reference
LOC_SCOPE, LOC_BIN_SIZE, NUM_HEAD_BIN = 1.5, 0.5, 12


def oracle_overlap_paired(bev_a, bev_b):
    """(n,5), (n,5) -> (n,) overlap areas: the diagonal of the oracle's N x N matrix (fp32 inside)"""
    import oracle
    a, b = bev_a.detach().cpu().numpy(), bev_b.detach().cpu().numpy()
    return torch.from_numpy(np.diagonal(oracle.boxes_overlap_bev(a, b)).copy())


def boxes3d_to_bev(boxes3d):
    """(n,7) [x, y, z, h, w, l, ry] -> (n,5): the box's footprint in the x-z plane as two opposite corners before rotation, and ry"""
    x, z, half_w, half_l = boxes3d[:, 0], boxes3d[:, 2], boxes3d[:, 4] / 2, boxes3d[:, 5] / 2
    return torch.stack((x - half_l, z - half_w, x + half_l, z + half_w, boxes3d[:, 6]), dim=1)


def iou3d_diagonal(boxes_a, boxes_b, overlap_paired=oracle_overlap_paired):
    """the diagonal of boxes_iou3d_gpu (iou3d_utils.py:21-56)"""
    if boxes_a.shape[0] == 0:
        return boxes_a.new_zeros((0,))
    overlaps_bev = overlap_paired(boxes3d_to_bev(boxes_a), boxes3d_to_bev(boxes_b)).to(boxes_a.dtype)
    a_min, a_max = boxes_a[:, 1] - boxes_a[:, 3], boxes_a[:, 1]
    b_min, b_max = boxes_b[:, 1] - boxes_b[:, 3], boxes_b[:, 1]
    overlaps_h = torch.clamp(torch.min(a_max, b_max) - torch.max(a_min, b_min), min=0)
    overlaps_3d = overlaps_bev * overlaps_h
    vol_a = boxes_a[:, 3] * boxes_a[:, 4] * boxes_a[:, 5]
    vol_b = boxes_b[:, 3] * boxes_b[:, 4] * boxes_b[:, 5]
    return overlaps_3d / torch.clamp(vol_a + vol_b - overlaps_3d, min=1e-7)


# signs of a corner's offset from the box's bottom-face centre along the box's own l and w axes; corners 0-3 on the bottom face, 4-7 above
CORNER_L = (+1, +1, -1, -1, +1, +1, -1, -1)
CORNER_W = (+1, -1, -1, +1, +1, -1, -1, +1)
CORNER_UP = (0, 0, 0, 0, 1, 1, 1, 1)


def corners3d(boxes3d):
    """(n,7) [x, y_bottom, z, h, w, l, ry] -> (n,8,3): the eight corners in the order of the reference's boxes3d_to_corners3d_torch
    (camera frame: y points down, the box spans y - h .. y; ry turns the l axis from +x towards -z)"""
    out = []
    cos, sin = torch.cos(boxes3d[:, 6]), torch.sin(boxes3d[:, 6])
    for sl, sw, up in zip(CORNER_L, CORNER_W, CORNER_UP):
        along_l, along_w = sl * boxes3d[:, 5] / 2, sw * boxes3d[:, 4] / 2
        out.append(torch.stack((boxes3d[:, 0] + (cos * along_l + sin * along_w), boxes3d[:, 1] - up * boxes3d[:, 3],
                                boxes3d[:, 2] + (-sin * along_l + cos * along_w)), dim=1))
    return torch.stack(out, dim=1)


def rcnn_reg_loss(pred_reg, reg_label):
    """get_rcnn_reg_loss with get_xz_fine = get_y_by_bin = get_ry_fine = False"""
    nb = int((LOC_SCOPE + 1e-3) / LOC_BIN_SIZE) * 2
    x_res_l, z_res_l, start = nb * 2, nb * 3, nb * 4
    loc_loss = 0
    loc_loss = loc_loss + F.smooth_l1_loss(pred_reg[:, x_res_l:x_res_l + 1].sum(dim=1), reg_label[:, 0] / LOC_SCOPE)
    loc_loss = loc_loss + F.smooth_l1_loss(pred_reg[:, z_res_l:z_res_l + 1].sum(dim=1), reg_label[:, 2] / LOC_SCOPE)
    loc_loss = loc_loss + F.mse_loss(pred_reg[:, start:start + 1].sum(dim=1), reg_label[:, 1])
    start += 1
    angle_per_class = (2 * np.pi) / NUM_HEAD_BIN
    heading = reg_label[:, 6] % (2 * np.pi)
    shift = (heading + angle_per_class / 2) % (2 * np.pi)
    bin_label = (shift / angle_per_class).floor().long()
    res_norm = (shift - (bin_label.to(shift.dtype) * angle_per_class + angle_per_class / 2)) / (angle_per_class / 2)
    onehot = torch.zeros((bin_label.shape[0], NUM_HEAD_BIN), dtype=pred_reg.dtype)
    onehot.scatter_(1, bin_label.view(-1, 1), 1)
    loss_bin = F.cross_entropy(pred_reg[:, start:start + NUM_HEAD_BIN], bin_label)
    loss_res = F.smooth_l1_loss((pred_reg[:, start + NUM_HEAD_BIN:start + 2 * NUM_HEAD_BIN] * onehot).sum(dim=1), res_norm)
    start += 2 * NUM_HEAD_BIN
    anchor = torch.from_numpy(MEAN_SIZE).to(pred_reg.dtype)
    size_loss = F.smooth_l1_loss(pred_reg[:, start:start + 3], (reg_label[:, 3:6] - anchor) / anchor)
    return loc_loss, loss_bin + loss_res, size_loss


def rcnn_loss(rcnn_cls, rcnn_reg, pred_boxes3d, gt_boxes, cls, overlap_paired=oracle_overlap_paired):
    """get_rcnn_loss -> (loss, tb of floats)"""
    zero = torch.zeros((), dtype=rcnn_reg.dtype)
    fg_mask = cls > 0
    loss_loc = loss_angle = loss_size = loss_reg = corner = zero
    if int(fg_mask.sum()) != 0:
        loss_loc, loss_angle, loss_size = rcnn_reg_loss(rcnn_reg[fg_mask], gt_boxes[fg_mask])
        iou3d = iou3d_diagonal(pred_boxes3d[fg_mask], gt_boxes[fg_mask], overlap_paired).detach()
        iou_mask = iou3d > 0.5
        if int(iou_mask.sum()) != 0:
            gt_f = gt_boxes[fg_mask][iou_mask].clone()
            pred_corner = corners3d(pred_boxes3d[fg_mask][iou_mask])
            gt_corner = corners3d(gt_f)
            gt_f[:, 6] += np.pi
            flip_corner = corners3d(gt_f)
            dist = torch.min(torch.norm(pred_corner - gt_corner, dim=-1), torch.norm(pred_corner - flip_corner, dim=-1))
            corner = F.smooth_l1_loss(dist, torch.zeros_like(dist))
        loss_loc, loss_size, corner = loss_loc * 20, loss_size * 300, corner * 10
        loss_reg = loss_loc + loss_angle + loss_size
    per_row = F.binary_cross_entropy(torch.sigmoid(rcnn_cls.view(-1)), cls, reduction='none')
    valid = (cls >= 0).to(per_row.dtype)
    loss_cls = (per_row * valid).sum() / torch.clamp(valid.sum(), min=1.0)
    loss = loss_cls + loss_reg + corner
    tb = {"rcnn_loss_cls": loss_cls, "rcnn_loss_reg": loss_reg, "rcnn_loss": loss, "rcnn_loss_loc": loss_loc, "rcnn_loss_angle": loss_angle,
          "rcnn_loss_size": loss_size, "rcnn_loss_corner": corner, "rcnn_cls_fg": (cls > 0).sum(), "rcnn_cls_bg": (cls == 0).sum()}
    return loss, {k: float(v.detach()) for k, v in tb.items()}


def ioun_loss(rcnn_iou, rcnn_ref, pred_boxes3d, refined_box, gt_boxes, cls, overlap_paired=oracle_overlap_paired):
    """get_ioun_loss -> (loss, tb of floats); with no non-zero gt box the IoU term is 0 (the reference: NaN)"""
    zero = torch.zeros((), dtype=rcnn_ref.dtype)
    fg_mask = cls > 0
    loss_loc = loss_siz = loss_ang = zero
    if int(fg_mask.sum()) != 0:
        ref, gt, pred = rcnn_ref[fg_mask], gt_boxes[fg_mask], pred_boxes3d[fg_mask]
        loss_loc = F.smooth_l1_loss(ref[:, :3], (gt[:, :3] - pred[:, :3]) / pred[:, 3:6]) * 300
        loss_siz = F.smooth_l1_loss(ref[:, 3:6], (gt[:, 3:6] - pred[:, 3:6]) / pred[:, 3:6]) * 300
        loss_ang = F.smooth_l1_loss(ref[:, 6], gt[:, 6] % np.pi - pred[:, 6] % np.pi) * 20
    loss_reg = loss_loc + loss_siz + loss_ang
    valid = gt_boxes.sum(-1) != 0
    loss_iou = zero
    if int(valid.sum()) != 0:
        label = iou3d_diagonal(refined_box[valid], gt_boxes[valid], overlap_paired).detach().pow(2)
        loss_iou = F.mse_loss(rcnn_iou.view(-1)[valid], label) * 100
    loss = loss_iou + loss_reg
    tb = {"ioun_loss_loc": loss_loc, "ioun_loss_siz": loss_siz, "ioun_loss_ang": loss_ang, "loss_iou": loss_iou, "loss_reg": loss_reg,
          "rcnn_loss_iou": loss}
    return loss, {k: float(v.detach()) for k, v in tb.items()}


# --------------------------------------------------------------------------- fixture access shared by the CPU and GPU tests
def load_cases(golden_dir):
    """-> {case: {'meta': ..., array name: numpy array}} of tests/golden/stage2_losses.*"""
    import json
    import os
    meta = json.load(open(os.path.join(golden_dir, "stage2_losses.json")))
    arrays = np.load(os.path.join(golden_dir, "stage2_losses.npz"))
    cases = {}
    for name, m in meta["cases"].items():
        cases[name] = {"meta": m}
        cases[name].update({k.split("/", 1)[1]: arrays[k] for k in arrays.files if k.startswith(name + "/")})
    return cases


def bound(yardstick, want):
    """the GPU tests' bound: 4 x the fixture's fp32 yardstick, or four fp32 roundings of the largest magnitude in the tensor"""
    return max(4.0 * yardstick, 2.0 ** -22 * float(np.abs(np.asarray(want, dtype=np.float64)).max()))



def load_step(golden_dir):
    """-> (meta, arrays) of tests/golden/stage2_train_step.*: one whole training step per phase, the reference's model_fn in float64"""
    import json
    import os
    return json.load(open(os.path.join(golden_dir, "stage2_train_step.json"))), dict(np.load(os.path.join(golden_dir, "stage2_train_step.npz")))


def step_batch(arrays, phase):
    """the collated batch the fixture's step started from (the iou_* inputs only in phase ioun)"""
    return {k[len("batch/"):]: v for k, v in arrays.items() if k.startswith("batch/") and (phase == "ioun" or not k.startswith("batch/iou_"))}
