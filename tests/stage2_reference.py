"""Test infrastructure for Stage 2: float64 torch restatements of the tower front (embed), the canonical transform, the box decode
and the detection tail, restated from what lib/net/rcnn_net.py, lib/utils/bbox_transform.py and tools/eval_auto.py compute (tensor
ops and loops in the reference's order, none of the package's code), plus the fixture loaders.  Used by tests/test_stage2.py (CPU)
and tests/test_gpu_stage2.py."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from tests import exact_overlap

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEAN_SIZE = np.asarray([1.5, 1.6, 3.9], dtype=np.float32)       # cfg.CLS_MEAN_SIZE[0] as the reference holds it: fp32
OUTPUTS = ("rcnn_cls", "rcnn_reg", "pred_boxes3d", "rcnn_iou", "rcnn_ref", "ioun_cls", "refined_box")
INDEX_NAMES = [("%s_%s_%d" % (t, "fps", l), "%s_%s_%d" % (t, "bq", l)) for t in ("rcnn", "ioun") for l in range(3)]


def fixture():
    """-> (arrays of stage2_forward.npz, meta of stage2_forward.json, {key: shape} of stage2_state_dict.json)"""
    arrays = dict(np.load(os.path.join(GOLDEN, "stage2_forward.npz")))
    meta = json.load(open(os.path.join(GOLDEN, "stage2_forward.json")))
    keys = json.load(open(os.path.join(GOLDEN, "stage2_state_dict.json")))["keys"]
    return arrays, meta, keys


def fixture_state_dict(meta, keys):
    """the weights the fixture was generated with: seeded, the two last regression layers scaled"""
    from ws3d_amd.seeded import seeded_state_dict
    sd = seeded_state_dict({k: tuple(v) for k, v in keys.items()}, meta["seed"])
    for k in meta["scaled_keys"]:
        sd[k] = sd[k] * meta["last_layer_scale"]
    return sd


def fixture_inputs(arrays, device="cpu", dtype=torch.float32):
    t = torch.from_numpy(arrays["pts"]).to(device=device, dtype=dtype)
    return {"cur_box_point": t[..., 0:3].contiguous(), "cur_box_reflect": t[..., 3:4].contiguous(), "train_mask": t[..., 4:5].contiguous()}


# --------------------------------------------------------------------------- rcnn_net.py:232-239, 337-351
def canonical_ref(xyz, box_ce, extend=1.2):
    """xyz (R,P,3), box_ce (R,7) float64 -> canonical xyz (R,P,3)"""
    xyz = xyz.clone()
    ce = box_ce.view(-1, 1, 7)
    xyz[:, :, 0] = xyz[:, :, 0] - ce[:, :, 0]
    xyz[:, :, 1] = xyz[:, :, 1] - ce[:, :, 1]
    xyz[:, :, 2] = xyz[:, :, 2] - ce[:, :, 2]
    ry = -ce[:, :, 6]
    rot = torch.zeros((xyz.shape[0], 3, 3), dtype=xyz.dtype)
    rot[:, 0, 0] = torch.cos(ry[:, 0])
    rot[:, 0, 2] = torch.sin(ry[:, 0])
    rot[:, 1, 1] = 1
    rot[:, 2, 0] = -torch.sin(ry[:, 0])
    rot[:, 2, 2] = torch.cos(ry[:, 0])
    can = torch.einsum('ijk,ikl->ijl', xyz, rot.permute(0, 2, 1))
    can[:, :, 0] = can[:, :, 0] / (ce[:, :, 5] / 2)
    can[:, :, 1] = can[:, :, 1] / (ce[:, :, 3] / 2)
    can[:, :, 2] = can[:, :, 2] / (ce[:, :, 4] / 2)
    mask = torch.max(torch.abs(can), dim=-1)[0] > extend
    can[mask] = 0.0
    return can


def embed_ref(pts, box_ce, w, extend=1.2):
    """pts (R,P,5), box_ce (R,7) or None, w = [wx0 (128,3), bx0, wx1 (128,128), bx1, wf0 (128,2), bf0, wf1, bf1, wm (128,256), bm] (conv
    layout: out x in), everything float64 -> (xyz (R,P,3), feat (R*P,128)) (rcnn_net.py:253-267 / 355-365)"""
    wx0, bx0, wx1, bx1, wf0, bf0, wf1, bf1, wm, bm = w
    xyz = pts[..., 0:3] if box_ce is None else canonical_ref(pts[..., 0:3], box_ce, extend)
    rows = xyz.reshape(-1, 3)
    raw = pts[..., 3:5].reshape(-1, 2)
    ux = torch.relu(torch.relu(rows @ wx0.t() + bx0) @ wx1.t() + bx1)
    uf = torch.relu(torch.relu(raw @ wf0.t() + bf0) @ wf1.t() + bf1)
    return xyz, torch.relu(torch.cat((ux, uf), dim=1) @ wm.t() + bm)


# --------------------------------------------------------------------------- bbox_transform.py:64-179 as rcnn_net.py:294-302 calls it
def decode_ref(pred_reg, loc_scope=1.5, loc_bin_size=0.5, num_head_bin=12, anchor_size=MEAN_SIZE):
    anchor = torch.from_numpy(np.asarray(anchor_size)).to(pred_reg.dtype)
    per_loc_bin_num = int(loc_scope / loc_bin_size) * 2
    x_res_l, z_res_l = per_loc_bin_num * 2, per_loc_bin_num * 3
    start_offset = per_loc_bin_num * 4
    pos_x = pred_reg[:, x_res_l] * loc_scope
    pos_z = pred_reg[:, z_res_l] * loc_scope
    pos_y = pred_reg[:, start_offset]
    start_offset += 1
    ry_bin_l, ry_bin_r = start_offset, start_offset + num_head_bin
    ry_res_l, ry_res_r = ry_bin_r, ry_bin_r + num_head_bin
    ry_bin = torch.argmax(pred_reg[:, ry_bin_l:ry_bin_r], dim=1)
    ry_res_norm = torch.gather(pred_reg[:, ry_res_l:ry_res_r], dim=1, index=ry_bin.unsqueeze(dim=1)).squeeze(dim=1)
    angle_per_class = (2 * np.pi) / num_head_bin
    ry_res = ry_res_norm * (angle_per_class / 2)
    ry = (ry_bin.float() * angle_per_class + ry_res) % (2 * np.pi)
    ry[ry > np.pi] -= 2 * np.pi
    size_res_l, size_res_r = ry_res_r, ry_res_r + 3
    assert size_res_r == pred_reg.shape[1]
    hwl = pred_reg[:, size_res_l:size_res_r] * anchor + anchor
    return torch.cat((pos_x.view(-1, 1), pos_y.view(-1, 1), pos_z.view(-1, 1), hwl, ry.view(-1, 1)), dim=1), ry_bin


def box2center_box_ref(pred_boxes3d):
    ce = pred_boxes3d.clone()
    ce[:, 1] -= ce[:, 3] / 2
    return ce


def center_box2box_ref(ce):
    box = ce.clone()
    box[:, 1] += box[:, 3] / 2
    box[:, 6] = box[:, 6] % (np.pi * 2)
    return box


def refine_box_ref(pred_boxes3d, rcnn_ref):
    out = pred_boxes3d.clone()
    out[:, :3] = pred_boxes3d[:, :3] + (pred_boxes3d[:, 3:6] * rcnn_ref[:, :3])
    out[:, 3:6] = pred_boxes3d[:, 3:6] * (1 + rcnn_ref[:, 3:6])
    out[:, 6] = pred_boxes3d[:, 6] + rcnn_ref[:, 6]
    return out


# --------------------------------------------------------------------------- tools/eval_auto.py:397-444, 572-612
def bev_iou(a, b) -> float:
    """float64 BEV IoU of two boxes (x, y, z, h, w, l, ry): iou3d_utils.boxes_iou3d_gpu's iou2d on the exact overlap"""
    ov = exact_overlap.overlap_bev(a, b)
    return ov / max(float(a[4]) * float(a[5]) + float(b[4]) * float(b[5]) - ov, 1e-7)


def select_ref(box_ce, rcnn_ref, rcnn_cls, rcnn_iou, center, num, rcnn_thresh=0.0, ioun_thresh=0.3, ground_y=1.65, dtype=torch.float32):
    """slot by slot, the way the reference's loop over a scene's centres builds box_list / raw_score_list / iou_score_list
    (eval_auto.py:397-410) and filters them (:420-436), in `dtype` tensors compared against python scalars as the reference compares
    them (fp32: its own precision) -> boxes (B,K,7) numpy of that dtype, keep (B,K) bool"""
    B, K = rcnn_cls.shape
    boxes = torch.zeros((B, K, 7), dtype=dtype)
    keep = np.zeros((B, K), dtype=bool)
    for b in range(B):
        for k in range(K):
            ce = torch.as_tensor(box_ce[b, k]).to(dtype).view(1, 7)
            box = refine_box_ref(center_box2box_ref(ce), torch.as_tensor(rcnn_ref[b, k]).to(dtype).view(1, 7)).view(1, 1, 7)
            box[:, :, 6] = box[:, :, 6] % (np.pi * 2)
            if box[:, :, 6] > np.pi:
                box[:, :, 6] -= np.pi * 2
            box[:, :, 0] += float(center[b, k, 0])
            box[:, :, 2] += float(center[b, k, 2])
            box[:, :, 1] += ground_y
            boxes[b, k] = box.view(7)
            score = torch.sigmoid(torch.as_tensor(rcnn_cls[b, k]).to(dtype))
            q = torch.as_tensor(rcnn_iou[b, k]).to(dtype)
            h, w, l = box[0, 0, 3], box[0, 0, 4], box[0, 0, 5]
            ok = (score > rcnn_thresh) & (q > ioun_thresh)
            ok = ok & (h > 1.1) & (h < 2.3) & (w > 1.2) & (w < 2.1) & (l > 2.1) & (l < 5.1)
            keep[b, k] = bool(ok) and k < int(num[b])
    return boxes.numpy(), keep


def detections_ref(boxes, keep, rcnn_iou, iou_fn=bev_iou):
    """the sort and the greedy loop of eval_auto.py:597-609 per scene -> list of (kept slot indices in output order)"""
    out = []
    for b in range(boxes.shape[0]):
        slots = [k for k in range(boxes.shape[1]) if keep[b, k]]
        slots.sort(key=lambda k: -float(rcnn_iou[b, k]))        # (stable: equal scores keep slot order)
        if len(slots) > 1:
            keep_id = [0]
            for i in range(1, len(slots)):
                if max(iou_fn(boxes[b, slots[j]], boxes[b, slots[i]]) for j in keep_id) < 0.01:
                    keep_id.append(i)
            slots = [slots[i] for i in keep_id]
        out.append(slots)
    return out


def hand_built_set():
    """detections on two scenes of 8 slots: a score exactly on each threshold, a size on the window's edge, a padding slot,
    two overlapping boxes (the weaker is suppressed), two far apart.  box_ce is the centre form of a mean-size box; rcnn_ref = 0 but
    where a size is pushed to an edge.  -> dict of float32 numpy arrays"""
    B, K = 2, 8
    ce = np.zeros((B, K, 7), dtype=np.float32)
    ce[..., 3:6] = MEAN_SIZE
    ce[..., 1] = -0.75
    ref = np.zeros((B, K, 7), dtype=np.float32)
    cls = np.full((B, K), 2.0, dtype=np.float32)
    iou = np.zeros((B, K), dtype=np.float32)
    center = np.zeros((B, K, 3), dtype=np.float32)
    center[..., 1] = 1.65
    for b in range(B):
        center[b, :, 0] = 10.0 * np.arange(K)            # far apart unless moved below
        center[b, :, 2] = 20.0 + b
    iou[0] = [0.9, 0.3, 0.5, 0.8, 0.7, 0.95, 0.6, 0.99]
    #   slot 1: rcnn_iou exactly on IOUN.SCORE_THRESH -> dropped (strict >)
    ce[0, 2, 6] = 3.5                                       # slot 2: ry beyond pi -> wrapped into (-pi, pi]
    center[0, 4, 0], center[0, 4, 2] = center[0, 3, 0] + 0.5, center[0, 3, 2] + 0.2      # slot 4 overlaps slot 3 (0.8 > 0.7): suppressed
    ce[0, 4, 6] = 0.4
    ref[0, 5, 3] = np.float32(2.3 / 1.5 - 1.0)             # slot 5: h lands on (or a rounding beside) the window's upper edge 2.3
    cls[0, 6] = -100.0                                     # slot 6: fp32 sigmoid(cls) is exactly RCNN.SCORE_THRESH = 0 -> dropped (strict >)
    #   slot 7: behind num[0] = 7 -> a padding slot, dropped although it has the best score
    iou[1] = [0.4, 0.41, 0.2, 0.0, 0.0, 0.0, 0.0, 0.0]
    center[1, 1, 0], center[1, 1, 2] = center[1, 0, 0] + 1.0, center[1, 0, 2]            # slot 1 (better score) overlaps slot 0
    ref[1, 1, 0:3] = [0.1, -0.05, 0.02]
    ref[1, 1, 6] = -0.3
    num = np.asarray([7, 3], dtype=np.int32)
    return {"box_ce": ce, "rcnn_ref": ref, "rcnn_cls": cls, "rcnn_iou": iou, "center": center, "num": num}


# --------------------------------------------------------------------------- the parity pin on the GPU
def fixture_model(meta, keys, device="cuda"):
    from ws3d_amd import stage2
    net = stage2.Stage2Net()
    net.rcnn_net.load_state_dict(fixture_state_dict(meta, keys), strict=True)
    return net.to(device).eval()


def parity_run(net, arrays, fast: bool, teacher: bool):
    """one forward of the fixture's clouds on the GPU by the module route (fast = False) or the channels-last route, the IoU tower fed
    the fixture's float64 box_ce rounded to fp32 (teacher) or the RCNN tower's own -> (errors against the float64 run per quantity,
    {index tensor name: equal?}, {'new_xyz': every level's centres equal xyz[fps]?}, the output dict)"""
    from ws3d_amd import stage2
    data = fixture_inputs(arrays, "cuda")
    box_ce = torch.from_numpy(arrays["box_ce"]).float().cuda() if teacher else None
    trace = []
    old = stage2.CHANNELS_LAST_FASTPATH
    stage2.CHANNELS_LAST_FASTPATH = fast
    try:
        with torch.no_grad():
            out = net.rcnn_net(data, box_ce=box_ce, trace=trace)
    finally:
        stage2.CHANNELS_LAST_FASTPATH = old
    err = {k: float(np.abs(out[k].double().cpu().numpy().reshape(arrays[k].shape) - arrays[k]).max()) for k in OUTPUTS}
    err["box_ce"] = float(np.abs(out["box_ce"].double().cpu().numpy() - arrays["box_ce"]).max())
    can = out["canonical_xyz"].cpu().numpy()
    err["can_xyz"] = float(np.abs(can.astype(np.float64) - arrays["can_xyz"].astype(np.float64)).max())
    same = {"can_xyz_zero_pattern": bool(np.array_equal(can == 0, arrays["can_xyz"] == 0))}
    assert len(trace) == len(INDEX_NAMES)
    centres_ok = True
    xyz_levels = [data["cur_box_point"], out["canonical_xyz"]]
    for i, ((fps_name, bq_name), lvl) in enumerate(zip(INDEX_NAMES, trace)):
        same[fps_name] = bool(np.array_equal(lvl["fps"].cpu().numpy(), arrays[fps_name].astype(np.int32)))
        same[bq_name] = bool(np.array_equal(lvl["bq"].cpu().numpy(), arrays[bq_name].astype(np.int32)))
        src = xyz_levels[i // 3] if i % 3 == 0 else trace[i - 1]["new_xyz"]
        picked = torch.gather(src, 1, lvl["fps"].long().unsqueeze(-1).expand(-1, -1, 3))
        centres_ok = centres_ok and bool(torch.equal(picked, lvl["new_xyz"]))
    same["new_xyz_is_xyz_at_fps"] = centres_ok
    return err, same, out
