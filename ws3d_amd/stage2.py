"""Stage-2 box network of WS3D on the MI355X ops: instance clouds in, refined 3-D boxes out.

Counterpart of lib/net/rcnn_net.py:16-399 (``RCNNNet``: the RCNN tower and the IoU-net cascade that refines the tower's box),
lib/net/point_rcnn.py's ``rcnn_forward`` and the detection tail of tools/eval_auto.py:397-444, 572-612, for the configuration
tools/cfgs/weaklyRPN.yaml + weaklyRCNN.yaml + weaklyIOUN.yaml with RCNN.ENABLED = IOUN.ENABLED = True (eval_auto.py:918-928).
``RCNNNet.state_dict()`` has the reference's keys and shapes (135 keys, the never-called ``input_tansformer`` included), so a
reference ``rcnn_ckpt`` loads key for key.  The EasyDict/YAML tree is the frozen dataclass ``RCNNConfig``.

Two routes through the network:
  * the module route: SharedMLP / PointnetSAModule / Conv1d blocks and the torch functions below, any configuration;
  * in eval mode on the GPU, when ``supported(model)`` holds and ``CHANNELS_LAST_FASTPATH`` is set, the channels-last route
    ``fast_forward``: per tower ``ws3d_stage2_embed`` (canonical transform + xyz_up + feature_up + merge_down of a 64-point tile
    in one kernel on the fp32 matrix cores, csrc/stage2.hip), the three grouped levels through ``fastpath.sa_forward`` (FPS, ball
    query, compact pairs, P = feats . W_f as one row GEMM, then ``ws3d_pgather_gemm3_compact`` or, where that entry returns
    WS3D_E_UNSUPPORTED, ``ws3d_pgather_gemm2_compact`` + ``ws3d_gemm_pool_compact``: ``sa_forward`` reads the return code at every
    call, nothing is latched per model), the GroupAll level and the heads as row GEMMs; ``ws3d_stage2_boxes`` between the towers.
Training: ``towers='rcnn'`` is phase 1 (the reference with IOUN.ENABLED = False), ``freeze_rcnn_tower`` + the optional inputs
iou_trans / iou_scale / iou_ry (noise on the box the IoU tower is given, rcnn_net.py:325-335) are phase 2; the losses are in
``stage2_losses``, the driver is ``train_rcnn``.  Training runs the module route (the channels-last route keeps nothing for backward).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from . import nn_blocks as pt_utils
from .pn2_modules import PointnetSAModule


@dataclass(frozen=True)
class RCNNConfig:
    """the effective values of weaklyRPN.yaml, weaklyRCNN.yaml, weaklyIOUN.yaml on top of lib/config.py (the IoU-net's
    SA_CONFIG, CLS_FC, REG_FC, USE_BN and DP_RATIO equal the RCNN's)"""
    npoints: tuple = (256, 128, 32, None)
    radius: tuple = (0.2, 0.4, 1.0, 100)
    nsample: tuple = (16, 32, 64, 64)
    mlps: tuple = ((128, 128, 128), (128, 128, 128), (128, 128, 256), (256, 256, 512))
    xyz_up_layer: tuple = (128, 128)
    cls_fc: tuple = (256, 256)
    reg_fc: tuple = (256, 256)
    use_bn: bool = False
    dp_ratio: float = 0.0
    loc_scope: float = 1.5
    loc_bin_size: float = 0.5
    num_head_bin: int = 12
    loc_y_by_bin: bool = False
    loc_y_scope: float = 0.5
    loc_y_bin_size: float = 0.25
    cls_mean_size: tuple = (1.5, 1.6, 3.9)      # h, w, l
    cascade: int = 1
    attention: bool = False
    rcnn_score_thresh: float = 0.0
    ioun_score_thresh: float = 0.3
    size_window: tuple = ((1.1, 2.3), (1.2, 2.1), (2.1, 5.1))       # h, w, l (eval_auto.py:433-436)
    nms_iou: float = 0.01                                           # eval_auto.py:606
    ground_y: float = 1.65                                          # eval_auto.py:403
    extend_factor: float = 1.2                                      # rcnn_net.py:346

    @property
    def reg_channel(self) -> int:
        per_loc_bin_num = int(self.loc_scope / self.loc_bin_size) * 2
        loc_y_bin_num = int(self.loc_y_scope / self.loc_y_bin_size) * 2
        return per_loc_bin_num * 4 + self.num_head_bin * 2 + 3 + (loc_y_bin_num * 2 if self.loc_y_by_bin else 1)


DEFAULT_CFG = RCNNConfig()
IOU_TOWER_PREFIXES = ("can_xyz_up_layer.", "can_feature_up_layer.", "can_merge_down_layer.", "SA_score_modules.", "ATT_score_modules.",
                      "IOU_layer.", "ICL_layer.", "ref_layer.")      # what the reference creates after it freezes the rest (rcnn_net.py:126-196)

# eval-mode GPU inference runs the channels-last route ``fast_forward`` (same weights and operators, (R,P,C) feature rows, the
# tower fronts and the box decode on csrc/stage2.hip); clear to force the module route
CHANNELS_LAST_FASTPATH = True
MODULE_ROUTE_MAX_CLOUDS = 96      # the module route in eval mode on the GPU runs larger batches in slices of this many clouds (96 x 512 channels < 65536)


# --------------------------------------------------------------------------- lib/utils/bbox_transform.py as plain torch
def decode_bbox_target_stage_2(roi_box3d, pred_reg, loc_scope, loc_bin_size, num_head_bin, anchor_size, get_xz_fine=True,
                               get_y_by_bin=False, loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False):
    """roi_box3d (N,3+), pred_reg (N,C) -> (N,7) [x, y, z, h, w, l, ry] (bbox_transform.py:64-179, same operation order; the bin
    indices go through ``.float()`` as there, so bin * angle_per_class is an fp32 product whatever pred_reg's dtype)"""
    anchor_size = torch.as_tensor(anchor_size, dtype=pred_reg.dtype, device=pred_reg.device)
    nb = int(loc_scope / loc_bin_size) * 2
    ny = int(loc_y_scope / loc_y_bin_size) * 2
    x_res_l, z_res_l = nb * 2, nb * 3
    start = nb * 4
    if get_xz_fine:
        x_bin = torch.argmax(pred_reg[:, 0:nb], dim=1)
        z_bin = torch.argmax(pred_reg[:, nb:2 * nb], dim=1)
        pos_x = x_bin.float() * loc_bin_size + loc_bin_size / 2 - loc_scope
        pos_z = z_bin.float() * loc_bin_size + loc_bin_size / 2 - loc_scope
        pos_x = pos_x + torch.gather(pred_reg[:, x_res_l:x_res_l + nb], 1, x_bin.unsqueeze(1)).squeeze(1) * loc_bin_size
        pos_z = pos_z + torch.gather(pred_reg[:, z_res_l:z_res_l + nb], 1, z_bin.unsqueeze(1)).squeeze(1) * loc_bin_size
    else:
        pos_x = pred_reg[:, x_res_l] * loc_scope
        pos_z = pred_reg[:, z_res_l] * loc_scope
    if get_y_by_bin:
        y_bin = torch.argmax(pred_reg[:, start:start + ny], dim=1)
        y_res = torch.gather(pred_reg[:, start + ny:start + 2 * ny], 1, y_bin.unsqueeze(1)).squeeze(1) * loc_y_bin_size
        pos_y = y_bin.float() * loc_y_bin_size + loc_y_bin_size / 2 - loc_y_scope + y_res
        start += 2 * ny
    else:
        pos_y = pred_reg[:, start]
        start += 1
    ry_bin = torch.argmax(pred_reg[:, start:start + num_head_bin], dim=1)
    ry_res_norm = torch.gather(pred_reg[:, start + num_head_bin:start + 2 * num_head_bin], 1, ry_bin.unsqueeze(1)).squeeze(1)
    if get_ry_fine:
        angle_per_class = np.pi / num_head_bin
        ry = (ry_bin.float() * angle_per_class + angle_per_class / 2) + ry_res_norm * (angle_per_class / 2)
    else:
        angle_per_class = (2 * np.pi) / num_head_bin
        ry = (ry_bin.float() * angle_per_class + ry_res_norm * (angle_per_class / 2)) % (2 * np.pi)
        ry = torch.where(ry > np.pi, ry - 2 * np.pi, ry)
    start += 2 * num_head_bin
    assert (start + 3) - pred_reg.shape[1] < 3
    hwl = pred_reg[:, start:start + 3] * anchor_size + anchor_size
    return torch.cat(((pos_x + roi_box3d[:, 0]).view(-1, 1), pos_y.view(-1, 1), (pos_z + roi_box3d[:, 2]).view(-1, 1), hwl, ry.view(-1, 1)), dim=1)


def center_box2box(pred_boxes3d_ce):
    """(..., 7) rows with y at the box's middle -> y at its bottom face, ry in [0, 2 pi) (bbox_transform.py:286-290)"""
    out = pred_boxes3d_ce.clone()
    out[..., 1] = out[..., 1] + out[..., 3] / 2
    out[..., 6] = out[..., 6] % (np.pi * 2)
    return out


def box2center_box(pred_boxes3d):
    """the inverse shift of y; ry is returned as it came (bbox_transform.py:292-296: the reference wraps the ry of its ARGUMENT
    in place, after the clone it returns was taken -- an argument nobody reads again)"""
    out = pred_boxes3d.clone()
    out[..., 1] = out[..., 1] - out[..., 3] / 2
    return out


def refine_box(pred_boxes3d, rcnn_ref):
    """(N,7) boxes, (N,7) refinements -> (N,7) (bbox_transform.py:298-303)"""
    return torch.cat((pred_boxes3d[:, :3] + pred_boxes3d[:, 3:6] * rcnn_ref[:, :3], pred_boxes3d[:, 3:6] * (1 + rcnn_ref[:, 3:6]),
                      (pred_boxes3d[:, 6] + rcnn_ref[:, 6]).unsqueeze(1)), dim=1)


def canonical_points(xyz, box_ce, extend=1.2):
    """xyz (R,P,3), box_ce (R,7) [x, y, z, h, w, l, ry] -> the points in the box's frame, in half extents (rcnn_net.py:337-351):
    centre subtracted, turned by -ry about y, x / y / z divided by l/2, h/2, w/2; a point whose largest |coordinate| exceeds
    `extend` becomes (0, 0, 0)"""
    b = box_ce.unsqueeze(1)
    x, y, z = xyz[..., 0] - b[..., 0], xyz[..., 1] - b[..., 1], xyz[..., 2] - b[..., 2]
    a = -b[..., 6]
    c, s = torch.cos(a), torch.sin(a)
    cx = (x * c + z * s) / (b[..., 5] / 2)
    cy = y / (b[..., 3] / 2)
    cz = (x * (-s) + z * c) / (b[..., 4] / 2)
    can = torch.stack((cx, cy, cz), dim=-1)
    out = can.abs().amax(dim=-1, keepdim=True) > extend
    return torch.where(out, torch.zeros_like(can), can)


def noised_box(pred_ce, input_data, stage):
    """the training noise on the box cascade stage `stage` is given (rcnn_net.py:325-335): centre += iou_trans (R,1,3,C), sizes *=
    iou_scale (R,1,1,C), ry += iou_ry (R,1,1,C); the box itself when the keys are absent"""
    if 'iou_trans' not in input_data:
        return pred_ce
    R = pred_ce.shape[0]
    trans, scale, ry = (input_data[k][..., stage].to(pred_ce) for k in ('iou_trans', 'iou_scale', 'iou_ry'))
    return torch.cat((pred_ce[:, 0:3] + trans.reshape(R, 3), pred_ce[:, 3:6] * scale.reshape(R, -1), pred_ce[:, 6:7] + ry.reshape(R, 1)), dim=1).contiguous()


def supported(model: "RCNNNet") -> bool:
    """what the channels-last route covers: no BatchNorm, no attention, one cascade stage, the 128-wide embedding of
    ws3d_stage2_embed, the bin layout of ws3d_stage2_boxes, three grouped levels + one GroupAll level per tower"""
    c = model.cfg
    levels = [sa.npoint is not None for sa in model.SA_modules]
    return (not c.use_bn and not c.attention and c.cascade == 1 and tuple(c.xyz_up_layer) == (128, 128) and not c.loc_y_by_bin
            and c.reg_channel == int(c.loc_scope / c.loc_bin_size) * 8 + 2 * c.num_head_bin + 4
            and levels == [True] * (len(levels) - 1) + [False] and all(m[0].use_xyz for m in (sa.groupers for sa in model.SA_modules))
            and all(b.conv.out_channels % 4 == 0 for sa in list(model.SA_modules) + list(model.SA_score_modules) for mlp in sa.mlps for b in mlp))


# --------------------------------------------------------------------------- the network
class Transformer(nn.Module):
    """lib/net/transformer.py:13-61: built by the reference's RCNNNet and never called; here for its state_dict keys"""

    def __init__(self, num_points=2000, K=3):
        super().__init__()
        self.K, self.N = K, num_points
        self.identity = torch.eye(K).float().view(-1)        # a plain attribute, not a key
        self.block1 = nn.Sequential(nn.Conv1d(K, 64, 1), nn.BatchNorm1d(64), nn.ReLU())
        self.block2 = nn.Sequential(nn.Conv1d(64, 128, 1), nn.BatchNorm1d(128), nn.ReLU())
        self.block3 = nn.Sequential(nn.Conv1d(128, 1024, 1), nn.BatchNorm1d(1024), nn.ReLU())
        self.mlp = nn.Sequential(nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(),
                                 nn.Linear(256, K * K))


def _head(pre, fc_dims, out_channels, bn, dp_ratio):
    layers = []
    for width in fc_dims:
        layers.append(pt_utils.Conv1d(pre, width, bn=bn))
        pre = width
    layers.append(pt_utils.Conv1d(pre, out_channels, activation=None))
    if dp_ratio >= 0:
        layers.insert(1, nn.Dropout(dp_ratio))
    return nn.Sequential(*layers)


class RCNNNet(nn.Module):
    """lib/net/rcnn_net.py:16-399 with cfg.RCNN.USE_RPN_FEATURES, cfg.RCNN.ROI_SAMPLE_JIT and cfg.IOUN.ENABLED set"""

    def __init__(self, num_classes=2, num_point=512, input_channels=128, use_xyz=True, cfg: RCNNConfig = DEFAULT_CFG):
        super().__init__()
        self.cfg = cfg
        self.rcnn_input_channel = 5
        bn = cfg.use_bn
        c_out = cfg.xyz_up_layer[-1]

        def sa_tower(mods, atts, act):
            channel_in = input_channels
            for k in range(len(cfg.npoints)):
                if cfg.attention:
                    atts.append(pt_utils.SharedMLP([channel_in], bn=bn, activation=act))
                mlps = [channel_in] + list(cfg.mlps[k])
                npoint = cfg.npoints[k] if cfg.npoints[k] not in (-1, None) else None
                mods.append(PointnetSAModule(npoint=npoint, radius=cfg.radius[k], nsample=cfg.nsample[k], mlp=mlps, use_xyz=use_xyz, bn=bn))
                channel_in = mlps[-1]
            return channel_in

        self.SA_modules = nn.ModuleList()
        self.ATT_modules = nn.ModuleList()
        self.input_tansformer = Transformer(num_point, 3)
        self.xyz_up_layer = pt_utils.SharedMLP([3] + list(cfg.xyz_up_layer), bn=bn)
        self.feature_up_layer = pt_utils.SharedMLP([self.rcnn_input_channel - 3] + list(cfg.xyz_up_layer), bn=bn)
        self.merge_down_layer = pt_utils.SharedMLP([c_out * 2, c_out], bn=bn)
        channel_in = sa_tower(self.SA_modules, self.ATT_modules, nn.ReLU(inplace=True))
        self.cls_layer = _head(channel_in, cfg.cls_fc, 1 if num_classes == 2 else num_classes, bn, cfg.dp_ratio)
        self.reg_layer = _head(channel_in, cfg.reg_fc, cfg.reg_channel, bn, cfg.dp_ratio)

        self.cascade = cfg.cascade
        self.can_xyz_up_layer = nn.ModuleList()
        self.can_feature_up_layer = nn.ModuleList()
        self.can_merge_down_layer = nn.ModuleList()
        self.SA_score_modules = nn.ModuleList()
        self.ATT_score_modules = nn.ModuleList()
        self.IOU_layer = nn.ModuleList()
        self.ICL_layer = nn.ModuleList()
        self.ref_layer = nn.ModuleList()
        for _ in range(self.cascade):
            self.can_xyz_up_layer.append(pt_utils.SharedMLP([3] + list(cfg.xyz_up_layer), bn=bn))
            self.can_feature_up_layer.append(pt_utils.SharedMLP([2] + list(cfg.xyz_up_layer), bn=bn))
            self.can_merge_down_layer.append(pt_utils.SharedMLP([c_out * 2, c_out], bn=bn))
            iou_channel_in = sa_tower(self.SA_score_modules, self.ATT_score_modules, nn.ELU(inplace=True))
            self.IOU_layer.append(_head(iou_channel_in, cfg.cls_fc, 1, bn, cfg.dp_ratio))
            self.ICL_layer.append(_head(iou_channel_in, cfg.cls_fc, 1, bn, cfg.dp_ratio))
            self.ref_layer.append(_head(iou_channel_in, cfg.reg_fc, 7, bn, cfg.dp_ratio))
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layer[-1].conv.weight, mean=0, std=0.001)

    # ---- a tower's front: (R,P,3) coordinates [in the box's frame], (R,P,2) reflectance + mask -> xyz (R,P,3), features (R,128,P)
    def _front(self, xyz, raw_features, box_ce, up_xyz, up_feat, merge, pts_feature):
        if box_ce is not None:
            xyz = canonical_points(xyz, box_ce.view(-1, 7), self.cfg.extend_factor)
        uper_xyz = up_xyz(xyz.transpose(1, 2).unsqueeze(3))
        if pts_feature is not None:
            uper_feature = pts_feature.transpose(1, 2).unsqueeze(3)
        else:
            uper_feature = up_feat(raw_features.transpose(1, 2).unsqueeze(3))
        merged = merge(torch.cat((uper_xyz, uper_feature), dim=1))
        return xyz.contiguous(), merged.squeeze(3)

    def _tower(self, xyz, features, sa_modules, att_modules, trace):
        l_xyz, l_features = [xyz], [features]
        for i, sa in enumerate(sa_modules):
            if self.cfg.attention:
                f = l_features[i]
                context = att_modules[i](f.unsqueeze(3)).squeeze(3)
                attention = torch.softmax(torch.bmm(f.transpose(1, 2), f) / math.sqrt(float(f.shape[1])), dim=1)
                l_features[i] = torch.bmm(context, attention) + f
            li_xyz, li_features = sa(l_xyz[i], l_features[i])
            _trace_level(trace, sa, l_xyz[i], li_xyz)
            l_xyz.append(li_xyz)
            l_features.append(li_features)
        return l_features[-1]

    def freeze_rcnn_tower(self):
        """phase 2: ``requires_grad = False`` on everything the reference creates before its IoU modules (rcnn_net.py:126-128);
        -> the names of the parameters that stay trainable"""
        kept = []
        for name, p in self.named_parameters():
            p.requires_grad = name.startswith(IOU_TOWER_PREFIXES)
            if p.requires_grad:
                kept.append(name)
        return kept

    def forward(self, input_data, box_ce=None, trace=None, towers='both'):
        """input_data: cur_box_point (R,P,3), cur_box_reflect (R,P,1), train_mask (R,P,1) [, cur_pts_feature (R,P,128)]
        [, iou_trans (R,1,3,C), iou_scale (R,1,1,C), iou_ry (R,1,1,C): ``noised_box``; pred_boxes3d and refined_box follow the noised box].
        box_ce: optional (R,7) boxes for the IoU tower instead of the RCNN tower's own (teacher forcing; tests).
        trace: optional list; receives per grouped level of both towers a dict with the level's sampling (``_trace_level``).
        towers: 'both', or 'rcnn' = the RCNN tower alone (IOUN.ENABLED = False): rcnn_cls, rcnn_reg and pred_boxes3d (R,1,7) = the
        decoded box itself, y at the bottom face (rcnn_net.py:307).
        -> rcnn_cls (R,1), rcnn_reg (R,52), pred_boxes3d (R,1,7), rcnn_iou (R,1), rcnn_ref (R,7), ioun_cls (R,1),
        refined_box (R,1,7), box_ce (R,7), canonical_xyz (R,P,3), plus the input dict."""
        xyz = input_data['cur_box_point']
        pts_feature = input_data.get('cur_pts_feature')
        if (CHANNELS_LAST_FASTPATH and not self.training and xyz.is_cuda and xyz.dtype == torch.float32 and pts_feature is None):
            ok = self.__dict__.get("_fastpath_ok")
            if ok is None:
                ok = self.__dict__["_fastpath_ok"] = supported(self)
            if ok:
                return fast_forward(self, input_data, box_ce, trace, towers)
        if towers not in ('both', 'rcnn'):
            raise ValueError("towers must be 'both' or 'rcnn', got %r" % (towers,))
        if not self.training and xyz.is_cuda and xyz.shape[0] > MODULE_ROUTE_MAX_CLOUDS and trace is None:
            # eval on the GPU: the channels-first epilogue kernels behind Conv1d / SharedMLP take up to 65535 (cloud, channel) rows per launch
            parts = []
            for i0 in range(0, xyz.shape[0], MODULE_ROUTE_MAX_CLOUDS):
                sl = slice(i0, i0 + MODULE_ROUTE_MAX_CLOUDS)
                parts.append(self.forward({k: (v[sl] if torch.is_tensor(v) and v.shape[:1] == xyz.shape[:1] else v) for k, v in input_data.items()},
                                          None if box_ce is None else box_ce[sl], None, towers))
            ret = {k: torch.cat([p_[k] for p_ in parts], dim=0) for k in parts[0] if k not in input_data}
            ret.update(input_data)
            return ret
        raw_features = torch.cat((input_data['cur_box_reflect'], input_data['train_mask']), dim=-1)
        c = self.cfg
        with torch.set_grad_enabled(self.training):
            x0, f0 = self._front(xyz, raw_features, None, self.xyz_up_layer, self.feature_up_layer, self.merge_down_layer, pts_feature)
            top = self._tower(x0, f0, self.SA_modules, self.ATT_modules, trace)
            rcnn_cls = self.cls_layer(top).transpose(1, 2).contiguous().squeeze(dim=1)
            rcnn_reg = self.reg_layer(top).transpose(1, 2).contiguous().squeeze(dim=1)
            R = rcnn_reg.shape[0]
            decoded = None
            if towers == 'rcnn' and rcnn_reg.is_cuda and rcnn_reg.dtype == torch.float32 and not c.loc_y_by_bin:
                # phase 1: the box the loss reads comes from ws3d_stage2_boxes, the same bits on both routes
                from . import compat as _C
                decoded, _ = _C.stage2_boxes(rcnn_reg.detach().contiguous(), c.loc_scope, c.loc_bin_size, c.num_head_bin, c.cls_mean_size)
            elif box_ce is None or towers == 'rcnn':
                mean_size = torch.from_numpy(np.asarray(c.cls_mean_size, dtype=np.float32)).to(rcnn_reg)
                decoded = decode_bbox_target_stage_2(
                    torch.zeros((R, 3), dtype=rcnn_reg.dtype, device=rcnn_reg.device), rcnn_reg.detach().view(R, -1), anchor_size=mean_size,
                    loc_scope=c.loc_scope, loc_bin_size=c.loc_bin_size, num_head_bin=c.num_head_bin, get_xz_fine=False,
                    loc_y_scope=c.loc_y_scope, loc_y_bin_size=c.loc_y_bin_size, get_ry_fine=False)
            ret = {'rcnn_cls': rcnn_cls, 'rcnn_reg': rcnn_reg}
            if towers == 'rcnn':
                ret['pred_boxes3d'] = decoded.view(R, 1, 7)
                ret.update(input_data)
                return ret
            pred_ce = box_ce.view(R, 7) if box_ce is not None else box2center_box(decoded)
            n_sa = len(self.SA_score_modules) // self.cascade
            rcnn_ref = None
            for s in range(self.cascade):
                if s != 0:
                    pred_ce = refine_box(pred_ce, rcnn_ref.view(R, 7))
                pred_ce = noised_box(pred_ce, input_data, s)
                # (the reference feeds the IoU tower the raw reflectance + mask, never cur_pts_feature: rcnn_net.py:357)
                xc, fc = self._front(xyz, raw_features, pred_ce, self.can_xyz_up_layer[s], self.can_feature_up_layer[s], self.can_merge_down_layer[s], None)
                top = self._tower(xc, fc, self.SA_score_modules[s * n_sa:(s + 1) * n_sa], self.ATT_score_modules[s * n_sa:(s + 1) * n_sa], trace)
                rcnn_iou = self.IOU_layer[s](top).transpose(1, 2).contiguous().squeeze(dim=1)
                rcnn_ref = self.ref_layer[s](top).transpose(1, 2).contiguous().squeeze(dim=1)
                ioun_cls = self.ICL_layer[s](top).transpose(1, 2).contiguous().squeeze(dim=1)
                pred_boxes3d = center_box2box(pred_ce)
                refined_box = refine_box(pred_boxes3d, rcnn_ref.view(R, 7))
                ret.update({'rcnn_iou': rcnn_iou, 'rcnn_ref': rcnn_ref, 'ioun_cls': ioun_cls, 'pred_boxes3d': pred_boxes3d.view(R, 1, 7),
                            'refined_box': refined_box.view(R, 1, 7), 'box_ce': pred_ce, 'canonical_xyz': xc})
        ret.update(input_data)
        return ret


def _trace_level(trace, sa, xyz, new_xyz):
    """tests: append {'new_xyz': the centres the level used, 'fps': furthest_point_sample(xyz, npoint), 'bq': ball_query(...)} -- the
    index tensors come from the stand-alone kernels on the level's input (the routes themselves run fused forms that keep no lists);
    new_xyz == xyz[fps] ties the two together.  GroupAll levels are skipped."""
    if trace is None or sa.npoint is None:
        return
    from . import pn2_ops
    g = sa.groupers[0]
    trace.append({'new_xyz': new_xyz, 'fps': pn2_ops.furthest_point_sample(xyz.contiguous(), sa.npoint),
                  'bq': pn2_ops.ball_query(g.radius, g.nsample, xyz.contiguous(), new_xyz.contiguous())})


# --------------------------------------------------------------------------- the channels-last route
def _front_rows(model, pts5, box_ce, up_xyz, up_feat, merge):
    """ws3d_stage2_embed with the five layers' W^T, cached per weight set -> xyz (R,P,3), feats (R,P,128)"""
    from . import compat as _C
    layers = [up_xyz.layer0, up_xyz.layer1, up_feat.layer0, up_feat.layer1, merge.layer0]
    key = tuple((t.data_ptr(), t._version) for l in layers for t in (l.conv.weight, l.conv.bias))
    cache = model.__dict__.setdefault("_front_packs", {})
    hit = cache.get(id(up_xyz))
    if hit is None or hit[0] != key:
        with torch.no_grad():       # W^T: row = input channel (the k of the kernel's K loops), 128 output columns
            packed = [t for l in layers for t in (l.conv.weight.reshape(l.conv.weight.shape[0], -1).t().contiguous(), l.conv.bias.contiguous())]
        hit = cache[id(up_xyz)] = (key, packed)
    xyz_out, feat = _C.stage2_embed(pts5, box_ce, *hit[1], extend=model.cfg.extend_factor)
    return xyz_out, feat.view(pts5.shape[0], pts5.shape[1], -1)


def _tower_rows(xyz, feats, sa_modules, trace, first_level=0):
    """the set-abstraction levels of a tower over channels-last rows -> (R, 512); first_level: the position of sa_modules[0] in the
    tower (the ragged route runs level 0 itself and hands over the levels behind it)"""
    from . import compat as _C, fastpath as fp
    for level, sa in enumerate(sa_modules, first_level):
        if sa.npoint is not None:
            new_xyz, new_feats = fp.sa_forward(sa, xyz, feats, level=level)
            _trace_level(trace, sa, xyz, new_xyz)
            xyz, feats = new_xyz, new_feats
            continue
        # GroupAll: the whole (small) cloud is the one group, UNCENTRED coordinates in front of the features (pointnet2_utils.py:280-284)
        R, n = xyz.shape[0], xyz.shape[1]
        blocks = fp._blocks(sa.mlps[0])
        y = torch.cat((xyz, feats), dim=2).view(R * n, -1)
        for blk in blocks[:-1]:
            y = fp._layer(y, blk)
        wt, bias, relu = fp._row_weights(blocks[-1])
        out = torch.empty((R, wt.size(1)), dtype=torch.float32, device=xyz.device)
        if not (fp.FUSED_GEMM_POOL and _C.gemm_pool(y, wt, bias, relu, n, out, 0)):
            _C.rowmax_rows(fp._layer(y, blocks[-1]), n, out, 0)
        return out
    raise ValueError("a tower must end in a GroupAll level")


def _head_rows(rows, seq):
    from . import fastpath as fp
    for blk in fp._blocks(seq):
        rows = fp._layer(rows, blk)
    return rows


@torch.no_grad()
def fast_forward(model: RCNNNet, input_data, box_ce=None, trace=None, towers='both'):
    """``RCNNNet.forward`` over channels-last rows for an eval-mode model that ``supported`` accepts; same dict.  Padding slots
    (all-zero clouds) run through like any cloud."""
    from . import compat as _C
    c = model.cfg
    pts5 = torch.cat((input_data['cur_box_point'], input_data['cur_box_reflect'], input_data['train_mask']), dim=-1).contiguous()
    R = pts5.shape[0]
    x0, f0 = _front_rows(model, pts5, None, model.xyz_up_layer, model.feature_up_layer, model.merge_down_layer)
    top = _tower_rows(x0, f0, model.SA_modules, trace)
    rcnn_cls, rcnn_reg = _head_rows(top, model.cls_layer), _head_rows(top, model.reg_layer)
    if towers == 'rcnn':
        decoded, _ = _C.stage2_boxes(rcnn_reg, c.loc_scope, c.loc_bin_size, c.num_head_bin, c.cls_mean_size)
        ret = {'rcnn_cls': rcnn_cls, 'rcnn_reg': rcnn_reg, 'pred_boxes3d': decoded.view(R, 1, 7)}
        ret.update(input_data)
        return ret
    if box_ce is not None:
        pred_ce = box_ce.view(R, 7).contiguous()
    else:
        _, pred_ce = _C.stage2_boxes(rcnn_reg, c.loc_scope, c.loc_bin_size, c.num_head_bin, c.cls_mean_size)
    pred_ce = noised_box(pred_ce, input_data, 0)
    xc, fc = _front_rows(model, pts5, pred_ce, model.can_xyz_up_layer[0], model.can_feature_up_layer[0], model.can_merge_down_layer[0])
    top = _tower_rows(xc, fc, model.SA_score_modules, trace)
    rcnn_iou, rcnn_ref, ioun_cls = _head_rows(top, model.IOU_layer[0]), _head_rows(top, model.ref_layer[0]), _head_rows(top, model.ICL_layer[0])
    pred_boxes3d = center_box2box(pred_ce)
    refined_box = refine_box(pred_boxes3d, rcnn_ref)
    ret = {'rcnn_cls': rcnn_cls, 'rcnn_reg': rcnn_reg, 'rcnn_iou': rcnn_iou, 'rcnn_ref': rcnn_ref, 'ioun_cls': ioun_cls,
           'pred_boxes3d': pred_boxes3d.view(R, 1, 7), 'refined_box': refined_box.view(R, 1, 7), 'box_ce': pred_ce, 'canonical_xyz': xc}
    ret.update(input_data)
    return ret


# --------------------------------------------------------------------------- the channels-last route on WHOLE clouds of different sizes
RAGGED_MAX_CLOUDS = 511       # per call of the ragged route: the consumer kernels take rows // 64 <= 65535 (128 centres x 64 samples a cloud)


def ragged_max_clouds(model: RCNNNet) -> int:
    """the clouds one pass of the ragged route takes: level 1's C * npoint * nsample list entries / 64 must fit the consumer kernels'
    16-bit grid, and never more than RAGGED_MAX_CLOUDS"""
    sa = model.SA_modules[0]
    return max(1, min(RAGGED_MAX_CLOUDS, (65535 * 64) // (sa.npoint * sa.groupers[0].nsample)))


def _sa_level_ragged(sa, xyz, feats, offsets, sizes, trace):
    """The first set-abstraction level over packed rows: xyz (T,3), feats (T,C), cloud i = rows offsets[i] .. offsets[i+1] ->
    new_xyz (Cn,m,3), new_feats (Cn,m,O).  The geometry comes from csrc/stage2_ragged.hip (sampling with gather, ball query with
    lists that index the packed array); the SharedMLP and the pool run through the consumer kernels of ``fastpath.sa_forward`` with
    the packed batch as ONE scene of T points and Cn * m centres."""
    from . import compat as _C, fastpath as fp, pn2_ops
    g, blocks = sa.groupers[0], fp._blocks(sa.mlps[0])
    Cn, T, m, ns = len(sizes), xyz.shape[0], sa.npoint, g.nsample
    idx, new_xyz = pn2_ops.furthest_point_sample_gather_ragged(xyz, offsets, m, sizes=sizes)
    nbr = pn2_ops.ball_query_ragged(g.radius, ns, xyz, offsets, new_xyz, sizes=sizes, global_rows=True)
    if trace is not None:
        trace.append({'new_xyz': new_xyz, 'fps': idx, 'bq': nbr - offsets[:-1].view(Cn, 1, 1)})
    x1, c1, n1, f1 = xyz.view(1, T, 3), new_xyz.view(1, Cn * m, 3), nbr.view(1, Cn * m, ns), feats.view(1, T, -1)
    wt1, b1, r1 = fp._row_weights_xyz_last(blocks[0])
    o1 = blocks[0].conv.out_channels
    y, rest = None, blocks[1:-1]
    if len(blocks) >= 3:
        # layer 1 is linear in the grouped row: its feature part is one product over the packed points, the lists gather it
        pmat, offs, w1xs = fp._per_point_l1(sa, f1, [nbr])
        if o1 <= 128:
            wt2, b2, r2 = fp._row_weights(blocks[1])
            y = _C.pgather_gemm2(pmat, offs[0], o1, x1, c1, n1, w1xs[0], b1, r1, wt2, b2, r2)
            rest = blocks[2:-1]
        if y is None:
            y = _C.pgather_rows(pmat, offs[0], o1, x1, c1, n1, w1xs[0], b1, r1)
            rest = blocks[1:-1]
    if y is None:
        y = _C.gather_gemm(f1, x1, c1, n1, wt1, b1, r1)
        rest = blocks[1:-1]
    if y is None:
        raise RuntimeError("no consumer kernel took the ragged level (%d rows, %d -> %d channels)" % (n1.numel(), feats.shape[1], o1))
    for blk in rest:
        y = fp._layer(y, blk)
    wt, bias, relu = fp._row_weights(blocks[-1])
    out = torch.empty((Cn * m, wt.size(1)), dtype=torch.float32, device=xyz.device)
    if not (fp.FUSED_GEMM_POOL and _C.gemm_pool(y, wt, bias, relu, ns, out, 0)):
        _C.rowmax_rows(fp._layer(y, blocks[-1]), ns, out, 0)
    return new_xyz, out.view(Cn, m, -1)


@torch.no_grad()
def fast_forward_ragged(model: RCNNNet, input_data, sizes, box_ce=None, trace=None, towers='both'):
    """``fast_forward`` for Cn whole clouds of different sizes packed into (T,.) rows (``Stage2Net.rcnn_forward_ragged`` states the
    inputs): the tower fronts per row, level 1 of each tower through ``_sa_level_ragged``, everything behind it on the fixed-size
    (Cn, npoint, .) tensors as in ``fast_forward``.  At most ``ragged_max_clouds(model)`` clouds."""
    from . import compat as _C
    c = model.cfg
    offsets = input_data['offsets'].to(torch.int32).contiguous()
    pts5 = torch.cat((input_data['cur_box_point'], input_data['cur_box_reflect'], input_data['train_mask']), dim=-1).contiguous()
    T, R = pts5.shape[0], len(sizes)

    def tower(rows5, up_xyz, up_feat, merge, sa_modules):
        x, f = _front_rows(model, rows5.view(1, T, 5), None, up_xyz, up_feat, merge)
        nx, nf = _sa_level_ragged(sa_modules[0], x.view(T, 3), f.view(T, -1), offsets, sizes, trace)
        return x.view(T, 3), _tower_rows(nx, nf, sa_modules[1:], trace, first_level=1)

    _, top = tower(pts5, model.xyz_up_layer, model.feature_up_layer, model.merge_down_layer, model.SA_modules)
    rcnn_cls, rcnn_reg = _head_rows(top, model.cls_layer), _head_rows(top, model.reg_layer)
    if towers == 'rcnn':
        decoded, _ = _C.stage2_boxes(rcnn_reg, c.loc_scope, c.loc_bin_size, c.num_head_bin, c.cls_mean_size)
        ret = {'rcnn_cls': rcnn_cls, 'rcnn_reg': rcnn_reg, 'pred_boxes3d': decoded.view(R, 1, 7)}
        ret.update(input_data)
        return ret
    if box_ce is not None:
        pred_ce = box_ce.view(R, 7).contiguous()
    else:
        _, pred_ce = _C.stage2_boxes(rcnn_reg, c.loc_scope, c.loc_bin_size, c.num_head_bin, c.cls_mean_size)
    can5 = _C.stage2_canonical_ragged(pts5, offsets, sizes, pred_ce, c.extend_factor)
    xc, top = tower(can5, model.can_xyz_up_layer[0], model.can_feature_up_layer[0], model.can_merge_down_layer[0], model.SA_score_modules)
    rcnn_iou, rcnn_ref, ioun_cls = _head_rows(top, model.IOU_layer[0]), _head_rows(top, model.ref_layer[0]), _head_rows(top, model.ICL_layer[0])
    pred_boxes3d = center_box2box(pred_ce)
    refined_box = refine_box(pred_boxes3d, rcnn_ref)
    ret = {'rcnn_cls': rcnn_cls, 'rcnn_reg': rcnn_reg, 'rcnn_iou': rcnn_iou, 'rcnn_ref': rcnn_ref, 'ioun_cls': ioun_cls,
           'pred_boxes3d': pred_boxes3d.view(R, 1, 7), 'refined_box': refined_box.view(R, 1, 7), 'box_ce': pred_ce, 'canonical_xyz': xc}
    ret.update(input_data)
    return ret


RAGGED_KEYS = ('cur_box_point', 'cur_box_reflect', 'train_mask')


def _cat_ragged(parts, input_data):
    """the dicts of consecutive groups of clouds -> one: per-cloud rows concatenated, canonical_xyz as packed (T,3) rows"""
    ret = {}
    for k in parts[0]:
        if k not in input_data:
            ret[k] = torch.cat([p[k].reshape(-1, 3) if k == 'canonical_xyz' else p[k] for p in parts], dim=0)
    ret.update(input_data)
    return ret


class Stage2Net(nn.Module):
    """``PointRCNN`` restricted to its Stage-2 half (lib/net/point_rcnn.py): attribute ``rcnn_net`` keeps the checkpoint prefix"""

    def __init__(self, num_classes=2, use_xyz=True, mode='TEST', cfg: RCNNConfig = DEFAULT_CFG, num_point=512, input_channels=128):
        super().__init__()
        self.mode = mode
        self.cfg = cfg
        self.rcnn_net = RCNNNet(num_classes=num_classes, num_point=num_point, input_channels=input_channels, use_xyz=use_xyz, cfg=cfg)

    def load_part_ckpt(self, state: dict, allow_missing_iou: bool = False) -> int:
        """load the ``rcnn_net.*`` entries of a reference checkpoint (the whole dict or its ``model_state``); other prefixes
        (``rpn.*``) are ignored, the way tools/train_utils' load_part_ckpt ignores keys the model lacks.  Every key of this model
        must be there -- except, with allow_missing_iou, the IoU tower's (``IOU_TOWER_PREFIXES``): a phase-1 reference checkpoint,
        written with IOUN.ENABLED = False, has none of them, and they keep their initialisation.  -> number of tensors loaded"""
        state = state.get("model_state", state)
        own = {k: v for k, v in state.items() if k.startswith("rcnn_net.")}
        if not allow_missing_iou:
            self.load_state_dict(own, strict=True)
            return len(own)
        result = self.load_state_dict(own, strict=False)
        bad = [k for k in result.missing_keys if not k[len("rcnn_net."):].startswith(IOU_TOWER_PREFIXES)]
        if bad or result.unexpected_keys:
            raise RuntimeError("load_part_ckpt: missing keys outside the IoU tower %s, unexpected keys %s" % (bad, list(result.unexpected_keys)))
        return len(own)

    def rcnn_forward(self, input_data, towers='both'):
        """(R,P,.) inputs, or (B,K,P,.) as ``stage1.stage2_inputs`` returns them (flattened to R = B K; outputs come back (R, ...))"""
        pts = input_data['cur_box_point']
        if pts.dim() == 4:
            flat = dict(input_data)
            for k in ('cur_box_point', 'cur_box_reflect', 'train_mask', 'cur_pts_feature'):
                if k in flat:
                    flat[k] = flat[k].reshape(-1, *flat[k].shape[2:])
            out = self.rcnn_net(flat, towers=towers)
            for k in ('cur_box_point', 'cur_box_reflect', 'train_mask', 'cur_pts_feature'):
                if k in input_data:
                    out[k] = input_data[k]
            return out
        return self.rcnn_net(input_data, towers=towers)

    forward = rcnn_forward

    def rcnn_forward_ragged(self, input_data, towers='both', box_ce=None, trace=None, sizes=None):
        """Stage 2 on WHOLE instance clouds, the form tools/eval_auto.py:286-403 evaluates in (every cylinder as it is, one cloud per
        ``rcnn_forward`` call there).  input_data: cur_box_point (T,3), cur_box_reflect (T,1), train_mask (T,1) packed rows and
        offsets (C+1): cloud i owns rows offsets[i] .. offsets[i+1] -- the slice of ``stage1.stage2_inputs(sampled_pt_num=None)`` for
        the non-empty clouds.  sizes: the C sizes on the host when the caller has them (else offsets is read back once).
        -> ``rcnn_forward``'s dict with R = C; canonical_xyz is (T,3).  box_ce (C,7) and trace as in ``RCNNNet.forward``; a trace
        entry holds (C, npoint[, nsample]) tensors, indices local to each cloud.  An empty cloud raises ValueError.
        An eval-mode model that ``supported`` accepts, on CUDA fp32 tensors with CHANNELS_LAST_FASTPATH set, takes
        ``fast_forward_ragged`` (a few dozen launches per ``ragged_max_clouds`` clouds); everything else runs the reference's own form,
        ``self.rcnn_net`` on (1, n_i, .) inputs cloud by cloud."""
        xyz, offsets = input_data['cur_box_point'], input_data['offsets']
        if towers not in ('both', 'rcnn'):
            raise ValueError("towers must be 'both' or 'rcnn', got %r" % (towers,))
        if xyz.dim() != 2 or xyz.shape[1] != 3 or offsets.dim() != 1 or offsets.numel() < 1:
            raise ValueError("cur_box_point (T,3) and offsets (C+1,) expected, got %s %s" % (tuple(xyz.shape), tuple(offsets.shape)))
        if sizes is None:
            sizes = (offsets[1:] - offsets[:-1]).tolist()
        sizes = [int(s) for s in sizes]
        if len(sizes) != offsets.numel() - 1 or sum(sizes) != xyz.shape[0]:
            raise ValueError("%d clouds that add up to %d rows expected, got sizes that add up to %d" % (offsets.numel() - 1, xyz.shape[0], sum(sizes)))
        if any(s < 1 for s in sizes):
            raise ValueError("cloud %d is empty: callers filter empty clouds out" % [i for i, s in enumerate(sizes) if s < 1][0])
        net = self.rcnn_net
        fast = (CHANNELS_LAST_FASTPATH and not net.training and xyz.is_cuda and xyz.dtype == torch.float32 and 'cur_pts_feature' not in input_data
                and len(sizes) > 0)
        if fast:
            ok = net.__dict__.get("_fastpath_ok")
            if ok is None:
                ok = net.__dict__["_fastpath_ok"] = supported(net)
            fast = ok
        starts = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        step = ragged_max_clouds(net) if fast else 1
        parts, traces = [], []
        for i0 in range(0, len(sizes), step):
            i1 = min(i0 + step, len(sizes))
            r0, r1 = int(starts[i0]), int(starts[i1])
            tr = [] if trace is not None else None
            ce = None if box_ce is None else box_ce[i0:i1]
            if fast:
                sub = {k: input_data[k][r0:r1] for k in RAGGED_KEYS}
                sub['offsets'] = offsets if step >= len(sizes) else (offsets[i0:i1 + 1] - offsets[i0])
                parts.append(fast_forward_ragged(net, sub, sizes[i0:i1], ce, tr, towers))
            else:
                sub = {k: input_data[k][r0:r1].unsqueeze(0) for k in RAGGED_KEYS}
                parts.append(net(sub, box_ce=ce, trace=tr, towers=towers))
            traces.append(tr)
            for k in RAGGED_KEYS + ('offsets',):
                parts[-1].pop(k, None)
        if not parts:
            raise ValueError("no cloud")
        if trace is not None:
            for lvl in range(len(traces[0])):
                trace.append({k: torch.cat([t[lvl][k] for t in traces], dim=0) for k in traces[0][lvl]})
        return _cat_ragged(parts, input_data)


# --------------------------------------------------------------------------- the detection tail
def select_boxes(box_ce, rcnn_ref, rcnn_cls, rcnn_iou, center, num, cfg: RCNNConfig = DEFAULT_CFG):
    """the element-wise part of ``detections`` in torch (the restatement ws3d_stage2_select is tested against):
    box_ce (B,K,7), rcnn_ref (B,K,7), rcnn_cls (B,K), rcnn_iou (B,K), center (B,K,3), num (B,) ->
    boxes (B,K,7) in the scene's frame, keep (B,K) bool, key (B,K): rcnn_iou where kept, -1e30 elsewhere"""
    B, K = rcnn_cls.shape
    box = refine_box(center_box2box(box_ce.reshape(-1, 7)), rcnn_ref.reshape(-1, 7)).view(B, K, 7)
    ry = box[..., 6] % (np.pi * 2)
    ry = torch.where(ry > np.pi, ry - np.pi * 2, ry)
    box = torch.stack((box[..., 0] + center[..., 0], box[..., 1] + cfg.ground_y, box[..., 2] + center[..., 2], box[..., 3], box[..., 4], box[..., 5], ry), dim=-1)
    keep = (torch.sigmoid(rcnn_cls) > cfg.rcnn_score_thresh) & (rcnn_iou > cfg.ioun_score_thresh)
    for c, (lo, hi) in zip((3, 4, 5), cfg.size_window):
        keep = keep & (box[..., c] > lo) & (box[..., c] < hi)
    keep = keep & (torch.arange(K, device=num.device)[None, :] < num[:, None])
    return box, keep, torch.where(keep, rcnn_iou, torch.full_like(rcnn_iou, -1e30))


@torch.no_grad()
def detections(out: dict, center: torch.Tensor, num: torch.Tensor, cfg: RCNNConfig = DEFAULT_CFG, iou_fn=None, return_index: bool = False):
    """tools/eval_auto.py:397-444, 572-612 for a batch.  out: ``rcnn_forward``'s dict for R = B K clouds, center (B,K,3) the
    kept centres, num (B,) how many of the K slots of a scene are real.  Refined box with ry in (-pi, pi], shifted to the scene's
    frame; kept where sigmoid(rcnn_cls) > RCNN.SCORE_THRESH, rcnn_iou > IOUN.SCORE_THRESH (the raw value), the size window and
    k < num[b]; sorted by rcnn_iou descending; greedy keep while the largest BEV IoU against the kept boxes is < 0.01.
    -> boxes (B,K,7), scores (B,K) = rcnn_iou, count (B,), zero padded.  No host synchronisation on the GPU.
    return_index: a fourth result, index (B,K) int64: the slot k of ``center`` every kept box came from, -1 in the padding.
    iou_fn: forces the scene-by-scene host loop ``detections_loop`` with that BEV IoU (CPU tensors have no other route)."""
    B, K = center.shape[0], center.shape[1]
    cls, iou = out['rcnn_cls'].reshape(B, K).contiguous(), out['rcnn_iou'].reshape(B, K).contiguous()
    ce = out['box_ce'] if 'box_ce' in out else box2center_box_from_pred(out['pred_boxes3d'])
    ce, ref = ce.reshape(B, K, 7).contiguous(), out['rcnn_ref'].reshape(B, K, 7).contiguous()
    num = num.to(torch.int32)
    if cls.is_cuda and iou_fn is None:
        from . import compat as _C
        box, keep, key = _C.stage2_select(ce, ref, cls, iou, center.contiguous(), num.contiguous(), cfg.rcnn_score_thresh, cfg.ioun_score_thresh,
                                          cfg.size_window, cfg.ground_y)
        sc, order = _C.topk_sorted(key, K, spread=False)
        flagged = keep.to(torch.int32).sum(dim=1)
        box_sorted, bev = _C.gather_boxes_bev(box, order)
        # the kernel suppresses a pair whose IoU is ABOVE its threshold; the reference keeps a box while IoU < 0.01 (compared in fp32)
        thresh = float(np.nextafter(np.float32(cfg.nms_iou), np.float32(0)))
        kept_idx, kept_num = _C.nms_device_batched(bev, thresh, False)
        # survivors are listed in ascending sorted position and the flagged boxes sort first: the real ones are a prefix
        real = (torch.arange(kept_idx.shape[1], device=kept_idx.device)[None, :] < kept_num[:, None]) & (kept_idx < flagged[:, None])
        boxes, scores, count, _ = _C.select_proposals(box_sorted, sc, kept_idx, real.sum(dim=1).to(torch.int32), K)
        if not return_index:
            return boxes, scores, count
        # kept_idx holds sorted positions (only its first kept_num entries are written), order the slot at every sorted position
        slot = order.gather(1, kept_idx[:, :K].clamp(0, max(K - 1, 0))) if K else order
        pad = torch.arange(K, device=slot.device)[None, :] >= count[:, None]
        return boxes, scores, count, slot.masked_fill(pad, -1)
    return detections_loop(*select_boxes(ce, ref, cls, iou, center, num, cfg), cfg, iou_fn, return_index)


def box2center_box_from_pred(pred_boxes3d):
    """the box_ce a forward dict without one was computed from (pred_boxes3d = center_box2box(box_ce)); ry only modulo 2 pi"""
    return box2center_box(pred_boxes3d.reshape(-1, 7))


def detections_loop(box, keep, key, cfg: RCNNConfig = DEFAULT_CFG, iou_fn=None, return_index: bool = False):
    """the sort and the greedy sweep of ``detections`` scene by scene on the host, one synchronisation per scene, as the reference
    runs them.  iou_fn: (n,7) boxes -> (n,n) BEV IoU; default: the rotated-overlap kernel behind ``iou3d_ops.boxes_iou3d_gpu``,
    which needs the boxes on the GPU (there is no CPU overlap in this package).  return_index: also index (B,K) int64, the slot
    of ``box`` every kept box came from, -1 in the padding."""
    if iou_fn is None:
        from . import iou3d_ops
        iou_fn = lambda b: iou3d_ops.boxes_iou3d_gpu(b, b)[0]       # noqa: E731
    B, K = keep.shape
    boxes = torch.zeros((B, K, 7), dtype=box.dtype, device=box.device)
    scores = torch.zeros((B, K), dtype=box.dtype, device=box.device)
    count = torch.zeros((B,), dtype=torch.int64, device=box.device)
    index = torch.full((B, K), -1, dtype=torch.int64, device=box.device)
    for b in range(B):
        sel = box[b][keep[b]]
        s = key[b][keep[b]]
        if sel.shape[0] == 0:
            continue
        order = torch.argsort(-s, stable=True)
        sel, s = sel[order], s[order]
        slot = keep[b].nonzero().reshape(-1)[order]
        kept = [0]
        if sel.shape[0] > 1:
            iou2d = iou_fn(sel).cpu()
            for i in range(1, sel.shape[0]):
                if float(iou2d[kept, i].max()) < np.float32(cfg.nms_iou):
                    kept.append(i)
        n = len(kept)
        boxes[b, :n], scores[b, :n], count[b], index[b, :n] = sel[kept], s[kept], n, slot[kept]
    return (boxes, scores, count, index) if return_index else (boxes, scores, count)
