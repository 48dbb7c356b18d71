"""Stage-2 training losses: ``rcnn_loss`` (phase 1, the RCNN tower) and ``ioun_loss`` (phase 2, the IoU tower).

Counterpart of ``get_rcnn_loss`` / ``get_ioun_loss`` (lib/net/train_functions.py:230-516) and ``get_rcnn_reg_loss``
(lib/utils/loss_utils.py:151-338) for tools/cfgs/weaklyRCNN.yaml / weaklyIOUN.yaml.  Two routes to the same numbers:

  * ``rcnn_loss_torch`` / ``ioun_loss_torch``: a plain-torch restatement, device-agnostic and dtype-generic (CPU, float64).  The
    reference branches on the host on ``fg_sum`` and ``iou_sum``; here every selection is a mask and every mean is
    ``sum / clamp(count, min=1)``, so an empty selection gives an exact 0 and nothing is read back.  It is the fallback and what the
    kernels are tested against.
  * on the GPU in fp32, for the bin layout ``stage2.supported`` describes (x / z / y by offset, ``get_ry_fine = False``), one launch
    per loss: ``ws3d_stage2_rcnn_loss`` / ``ws3d_stage2_ioun_loss`` (csrc/stage2_loss.hip) compute every component, the counts and the
    gradient of the total w.r.t. the head outputs; the autograd backward only scales the saved gradients.  ``FUSED_LOSSES = False``
    forces the torch route.  ``cascade != 1``, ``attention`` and ``use_bn`` are outside what the kernels were written for: such a
    configuration takes the torch route.

The 3-D IoU of row i's box against row i's gt box is ``iou3d_ops.boxes_iou3d_paired`` -- the reference computes the N x N matrix
three times per step and keeps the diagonal.  Without a GPU there is no rotated overlap in this package: pass ``overlap_fn``
(BEV boxes (n,5), (n,5) -> paired overlap areas (n,)).

What is differentiable: ``rcnn_cls`` and ``rcnn_reg`` (rcnn), ``rcnn_iou`` and ``rcnn_ref`` (ioun).  The boxes are constants: the
reference decodes ``pred_boxes3d`` from detached outputs, so the corner term has a value and no gradient, and the IoU label is
detached.  Both functions return ``(loss, tb)``; ``tb`` holds the reference's ``tb_dict`` keys as 0-dim device tensors, to be read in
one go with ``losses.resolve_scalars``.  ``rcnn_loss_giou`` is logged by the reference and never added to its loss; it is not built.

Two deviations: with no row holding a non-zero gt box, the reference's "range MSE" is the mean over an empty selection, NaN; here
that term is 0.  And its rows are those whose gt box has ANY non-zero entry, not those whose entries do not sum to zero: the same rows
unless a box cancels to exactly zero, where the sum would depend on the summation order.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .stage2 import DEFAULT_CFG, RCNNConfig

FUSED_LOSSES = True     # GPU + fp32 + the default bin layout: one HIP launch per loss; clear to force the torch restatement

RCNN_KEYS = ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss", "rcnn_loss_loc", "rcnn_loss_angle", "rcnn_loss_size", "rcnn_loss_corner",
             "rcnn_cls_fg", "rcnn_cls_bg")
IOUN_KEYS = ("ioun_loss_loc", "ioun_loss_siz", "ioun_loss_ang", "loss_iou", "loss_reg", "rcnn_loss_iou")


def fused_supported(cfg: RCNNConfig) -> bool:
    """the configurations the fused kernels cover"""
    return not (cfg.loc_y_by_bin or cfg.use_bn or cfg.attention or cfg.cascade != 1)


# --------------------------------------------------------------------------- helpers of the torch route
def boxes3d_to_bev(boxes3d):
    """(n,7) -> (n,5) [x1, y1, x2, y2, ry] (kitti_utils.py:134-147)"""
    half_l, half_w = boxes3d[:, 5] / 2, boxes3d[:, 4] / 2
    cu, cv = boxes3d[:, 0], boxes3d[:, 2]
    return torch.stack((cu - half_l, cv - half_w, cu + half_l, cv + half_w, boxes3d[:, 6]), dim=1)


def paired_iou3d(boxes_a, boxes_b, overlap_fn=None, full_matrix=False):
    """(n,7), (n,7) -> iou3d (n,) of pair i.  overlap_fn None: the HIP kernel (fp32 GPU tensors; ``full_matrix`` takes the reference's
    route instead, the N x N matrix and its diagonal -- for timing).  With overlap_fn: the expressions of
    ``iou3d_ops.boxes_iou3d_gpu`` on the paired overlap, in the boxes' dtype."""
    if overlap_fn is None:
        from . import iou3d_ops
        if full_matrix:
            return torch.diagonal(iou3d_ops.boxes_iou3d_gpu(boxes_a.contiguous(), boxes_b.contiguous())[1]).contiguous()
        return iou3d_ops.boxes_iou3d_paired(boxes_a, boxes_b)[1]
    overlap = overlap_fn(boxes3d_to_bev(boxes_a), boxes3d_to_bev(boxes_b)).to(boxes_a)
    a_min, a_max = boxes_a[:, 1] - boxes_a[:, 3], boxes_a[:, 1]
    b_min, b_max = boxes_b[:, 1] - boxes_b[:, 3], boxes_b[:, 1]
    overlaps_h = torch.clamp(torch.min(a_max, b_max) - torch.max(a_min, b_min), min=0)
    overlaps_3d = overlap * overlaps_h
    vol_a = boxes_a[:, 3] * boxes_a[:, 4] * boxes_a[:, 5]
    vol_b = boxes_b[:, 3] * boxes_b[:, 4] * boxes_b[:, 5]
    return overlaps_3d / torch.clamp(vol_a + vol_b - overlaps_3d, min=1e-7)


def boxes3d_to_corners3d(boxes3d):
    """(n,7) [x, y, z, h, w, l, ry] -> (n,8,3) (kitti_utils.py:104-131)"""
    h, w, l, ry = boxes3d[:, 3:4], boxes3d[:, 4:5], boxes3d[:, 5:6], boxes3d[:, 6:7]
    zeros = torch.zeros_like(h)
    x_c = torch.cat([l / 2., l / 2., -l / 2., -l / 2., l / 2., l / 2., -l / 2., -l / 2.], dim=1)
    y_c = torch.cat([zeros, zeros, zeros, zeros, -h, -h, -h, -h], dim=1)
    z_c = torch.cat([w / 2., -w / 2., -w / 2., w / 2., w / 2., -w / 2., -w / 2., w / 2.], dim=1)
    cosa, sina = torch.cos(ry), torch.sin(ry)
    x = cosa * x_c + sina * z_c + boxes3d[:, 0:1]
    y = y_c + boxes3d[:, 1:2]
    z = -sina * x_c + cosa * z_c + boxes3d[:, 2:3]
    return torch.stack((x, y, z), dim=2)


def _masked_mean(values, mask, per_row=1):
    """sum of `values` over the rows of `mask` / (max(rows, 1) * per_row): the mean over the selection, an exact 0 when it is empty.
    The sum runs in float64 whatever the dtype (a few thousand terms): the masked sum visits the rows in another order than the
    reference's mean over the selected rows, and in fp32 that alone would cost a last-place unit of the result."""
    m = mask if values.dim() == 1 else mask.unsqueeze(1)
    count = torch.clamp(mask.sum(dtype=torch.float64), min=1.0)
    return (torch.where(m, values, torch.zeros_like(values)).sum(dtype=torch.float64) / (count * per_row)).to(values.dtype)


def _bin_residual(shift, bin_size, bins):
    """bin label (clamped into the row: masked rows may hold anything) and the in-bin residual normalised by half a bin"""
    label = (shift / bin_size).floor().long()
    res = (shift - (label.to(shift.dtype) * bin_size + bin_size / 2)) / (bin_size / 2)
    return torch.clamp(label, 0, bins - 1), res


def _picked(block, label):
    return torch.gather(block, 1, label.view(-1, 1)).squeeze(1)


# --------------------------------------------------------------------------- the torch route
def rcnn_loss_torch(rcnn_cls, rcnn_reg, pred_boxes3d, gt_boxes, cls, cfg: RCNNConfig = DEFAULT_CFG, overlap_fn=None, full_matrix=False):
    """``get_rcnn_loss`` with masks; see the module docstring.  -> (loss, tb of 0-dim tensors)"""
    dt = rcnn_reg.dtype
    R = rcnn_reg.shape[0]
    logits, reg = rcnn_cls.reshape(-1), rcnn_reg.reshape(R, -1)
    gt, pred = gt_boxes.detach().reshape(R, 7).to(dt), pred_boxes3d.detach().reshape(R, 7).to(dt)
    label = cls.detach().reshape(-1).to(dt)
    fg = label > 0
    nb = int((cfg.loc_scope + 1e-3) / cfg.loc_bin_size) * 2
    ny = int((cfg.loc_y_scope + 1e-3) / cfg.loc_y_bin_size) * 2
    hb = cfg.num_head_bin
    anchor = torch.from_numpy(np.asarray(cfg.cls_mean_size, dtype=np.float32)).to(reg)       # cfg.CLS_MEAN_SIZE is a float32 array

    # get_rcnn_reg_loss, LOC_XZ_FINE = False (loss_utils.py:213-224)
    loss_x = _masked_mean(F.smooth_l1_loss(reg[:, 2 * nb], gt[:, 0] / cfg.loc_scope, reduction='none'), fg)
    loss_z = _masked_mean(F.smooth_l1_loss(reg[:, 3 * nb], gt[:, 2] / cfg.loc_scope, reduction='none'), fg)
    start = 4 * nb
    if cfg.loc_y_by_bin:        # :228-247
        y_shift = torch.clamp(gt[:, 1] + cfg.loc_y_scope, 0, cfg.loc_y_scope * 2 - 1e-3)
        y_label = torch.clamp((y_shift / cfg.loc_y_bin_size).floor().long(), 0, ny - 1)
        y_res = (y_shift - (y_label.to(dt) * cfg.loc_y_bin_size + cfg.loc_y_bin_size / 2)) / cfg.loc_y_bin_size
        loss_y = (_masked_mean(F.cross_entropy(reg[:, start:start + ny], y_label, reduction='none'), fg)
                  + _masked_mean(F.smooth_l1_loss(_picked(reg[:, start + ny:start + 2 * ny], y_label), y_res, reduction='none'), fg))
        start += 2 * ny
    else:                       # :249-256
        loss_y = _masked_mean((reg[:, start] - gt[:, 1]) ** 2, fg)
        start += 1
    loss_loc = (loss_x + loss_z) + loss_y
    # heading, get_ry_fine = False (:294-310)
    apc = (2 * np.pi) / hb
    shift = (gt[:, 6] % (2 * np.pi) + apc / 2) % (2 * np.pi)
    ry_label, ry_res = _bin_residual(shift, apc, hb)
    loss_angle = (_masked_mean(F.cross_entropy(reg[:, start:start + hb], ry_label, reduction='none'), fg)
                  + _masked_mean(F.smooth_l1_loss(_picked(reg[:, start + hb:start + 2 * hb], ry_label), ry_res, reduction='none'), fg))
    start += 2 * hb
    loss_size = _masked_mean(F.smooth_l1_loss(reg[:, start:start + 3], (gt[:, 3:6] - anchor) / anchor, reduction='none'), fg, per_row=3)

    # the corner term over the foreground rows whose box overlaps its gt box by more than 0.5 (train_functions.py:258-273)
    iou3d = paired_iou3d(pred, gt, overlap_fn, full_matrix)
    iou_mask = fg & (iou3d > 0.5)
    pred_corner, gt_corner = boxes3d_to_corners3d(pred), boxes3d_to_corners3d(gt)
    flipped = torch.cat((gt[:, :6], gt[:, 6:7] + np.pi), dim=1)
    dist = torch.min(torch.norm(pred_corner - gt_corner, dim=-1), torch.norm(pred_corner - boxes3d_to_corners3d(flipped), dim=-1))
    corner = _masked_mean(F.smooth_l1_loss(dist, torch.zeros_like(dist), reduction='none'), iou_mask, per_row=8)

    loss_loc, loss_size, corner = loss_loc * 20, loss_size * 300, corner * 10
    loss_reg = loss_loc + loss_angle + loss_size
    # classification (:321-327): the library's binary_cross_entropy (each log clamped at -100), gradient through the sigmoid
    valid = label >= 0
    per_row = F.binary_cross_entropy(torch.sigmoid(logits), torch.where(valid, label, torch.zeros_like(label)), reduction='none')
    loss_cls = _masked_mean(per_row, valid)
    loss = loss_cls + loss_reg + corner
    tb = {"rcnn_loss_cls": loss_cls, "rcnn_loss_reg": loss_reg, "rcnn_loss": loss, "rcnn_loss_loc": loss_loc, "rcnn_loss_angle": loss_angle,
          "rcnn_loss_size": loss_size, "rcnn_loss_corner": corner, "rcnn_cls_fg": fg.sum(), "rcnn_cls_bg": (label == 0).sum(),
          "fg_sum": fg.sum(), "iou_sum": iou_mask.sum()}
    return loss, {k: v.detach() for k, v in tb.items()}


def ioun_loss_torch(rcnn_iou, rcnn_ref, pred_boxes3d, refined_box, gt_boxes, cls, cfg: RCNNConfig = DEFAULT_CFG, overlap_fn=None,
                    full_matrix=False):
    """``get_ioun_loss`` with masks; see the module docstring.  -> (loss, tb of 0-dim tensors)"""
    dt = rcnn_ref.dtype
    R = rcnn_ref.shape[0]
    iou_out, ref = rcnn_iou.reshape(-1), rcnn_ref.reshape(R, 7)
    gt, pred, refined = (t.detach().reshape(R, 7).to(dt) for t in (gt_boxes, pred_boxes3d, refined_box))
    fg = cls.detach().reshape(-1) > 0
    zero = torch.zeros((), dtype=dt, device=ref.device)

    def target(t):      # rows outside the selection may hold anything (a zero-size box divides by zero): their target is 0
        return torch.where(fg.view(-1, *([1] * (t.dim() - 1))), t, zero)

    loss_loc = _masked_mean(F.smooth_l1_loss(ref[:, :3], target((gt[:, :3] - pred[:, :3]) / pred[:, 3:6]), reduction='none'), fg, per_row=3) * 300
    loss_siz = _masked_mean(F.smooth_l1_loss(ref[:, 3:6], target((gt[:, 3:6] - pred[:, 3:6]) / pred[:, 3:6]), reduction='none'), fg, per_row=3) * 300
    loss_ang = _masked_mean(F.smooth_l1_loss(ref[:, 6], target(gt[:, 6] % np.pi - pred[:, 6] % np.pi), reduction='none'), fg) * 20
    loss_reg = loss_loc + loss_siz + loss_ang
    # "range MSE" (:488-491) over the rows with a non-zero gt box
    valid = (gt != 0).any(dim=-1)        # the reference: gt.sum(-1) != 0 -- the same rows unless a box's entries cancel to exactly zero
    iou_label = torch.where(valid, paired_iou3d(refined, gt, overlap_fn, full_matrix).pow(2), zero)
    loss_iou = _masked_mean((iou_out - iou_label) ** 2, valid) * 100
    loss = loss_iou + loss_reg
    tb = {"ioun_loss_loc": loss_loc, "ioun_loss_siz": loss_siz, "ioun_loss_ang": loss_ang, "loss_iou": loss_iou, "loss_reg": loss_reg,
          "rcnn_loss_iou": loss, "fg_sum": fg.sum(), "valid_sum": valid.sum()}
    return loss, {k: v.detach() for k, v in tb.items()}


# --------------------------------------------------------------------------- the fused route
class _RcnnLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rcnn_cls, rcnn_reg, pred_boxes3d, gt_boxes, cls, cfg):
        from . import compat as _C
        vals, counts, g_cls, g_reg = _C.stage2_rcnn_loss(rcnn_cls.contiguous(), rcnn_reg.contiguous(), pred_boxes3d.contiguous(), gt_boxes.contiguous(),
                                                         cls.contiguous(), cfg.loc_scope, cfg.loc_bin_size, cfg.num_head_bin, cfg.cls_mean_size)
        ctx.save_for_backward(g_cls, g_reg)
        ctx.mark_non_differentiable(vals, counts)
        return vals[6].clone(), vals, counts

    @staticmethod
    def backward(ctx, grad_loss, _vals, _counts):
        g_cls, g_reg = ctx.saved_tensors
        return grad_loss * g_cls, grad_loss * g_reg, None, None, None, None


class _IounLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rcnn_iou, rcnn_ref, pred_boxes3d, refined_box, gt_boxes, cls):
        from . import compat as _C
        vals, counts, g_iou, g_ref = _C.stage2_ioun_loss(rcnn_iou.contiguous(), rcnn_ref.contiguous(), pred_boxes3d.contiguous(), refined_box.contiguous(),
                                                         gt_boxes.contiguous(), cls.contiguous())
        ctx.save_for_backward(g_iou, g_ref)
        ctx.mark_non_differentiable(vals, counts)
        return vals[5].clone(), vals, counts

    @staticmethod
    def backward(ctx, grad_loss, _vals, _counts):
        g_iou, g_ref = ctx.saved_tensors
        return grad_loss * g_iou, grad_loss * g_ref, None, None, None, None


def _fused(cfg, *tensors):
    return FUSED_LOSSES and fused_supported(cfg) and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def rcnn_loss(rcnn_cls, rcnn_reg, pred_boxes3d, gt_boxes, cls, cfg: RCNNConfig = DEFAULT_CFG, overlap_fn=None):
    """rcnn_cls (R,) or (R,1), rcnn_reg (R,52), pred_boxes3d (R,7) or (R,1,7), gt_boxes likewise, cls (R,) -> (loss, tb):
    ``rcnn_loss = cls + (20 loc + angle + 300 size) + 10 corner``.  tb: RCNN_KEYS (+ ``fg_sum``, ``iou_sum``), 0-dim device tensors."""
    R = rcnn_reg.shape[0]
    args = (rcnn_cls.reshape(-1), rcnn_reg.reshape(R, -1), pred_boxes3d.detach().reshape(R, 7), gt_boxes.detach().reshape(R, 7), cls.detach().reshape(-1))
    if overlap_fn is not None or not _fused(cfg, *args):
        return rcnn_loss_torch(*args, cfg=cfg, overlap_fn=overlap_fn)
    loss, vals, counts = _RcnnLossFn.apply(*args, cfg)
    tb = {"rcnn_loss_cls": vals[0], "rcnn_loss_reg": vals[5], "rcnn_loss": vals[6], "rcnn_loss_loc": vals[1], "rcnn_loss_angle": vals[2],
          "rcnn_loss_size": vals[3], "rcnn_loss_corner": vals[4], "rcnn_cls_fg": counts[0], "rcnn_cls_bg": counts[3], "fg_sum": counts[0],
          "iou_sum": counts[1]}
    return loss, tb


def ioun_loss(rcnn_iou, rcnn_ref, pred_boxes3d, refined_box, gt_boxes, cls, cfg: RCNNConfig = DEFAULT_CFG, overlap_fn=None):
    """rcnn_iou (R,) or (R,1), rcnn_ref (R,7), pred_boxes3d / refined_box / gt_boxes (R,7) or (R,1,7), cls (R,) -> (loss, tb):
    ``rcnn_loss_iou = 100 mse(iou) + 300 loc + 300 size + 20 angle``.  tb: IOUN_KEYS (+ ``fg_sum``, ``valid_sum``), 0-dim device tensors."""
    R = rcnn_ref.shape[0]
    args = (rcnn_iou.reshape(-1), rcnn_ref.reshape(R, 7), pred_boxes3d.detach().reshape(R, 7), refined_box.detach().reshape(R, 7),
            gt_boxes.detach().reshape(R, 7), cls.detach().reshape(-1))
    if overlap_fn is not None or not _fused(cfg, *args):
        return ioun_loss_torch(*args, cfg=cfg, overlap_fn=overlap_fn)
    loss, vals, counts = _IounLossFn.apply(*args)
    tb = {"ioun_loss_loc": vals[0], "ioun_loss_siz": vals[1], "ioun_loss_ang": vals[2], "loss_iou": vals[3], "loss_reg": vals[4],
          "rcnn_loss_iou": vals[5], "fg_sum": counts[0], "valid_sum": counts[1]}
    return loss, tb
