"""Stage-2 instance clouds: the cylinder of scene points around every kept centre, cut on the device for a whole batch
(csrc/instance_clouds.hip).  Counterpart of the per-centre Python loops of generate_box_dataset.py:197-229 and
tools/eval_auto.py:286-292, 323-372, and of the pad-to-512 rule of lib/datasets/kitti_boxplace_dataset.py:327-337."""
from __future__ import annotations

import torch

from . import compat as _C


def _prep(pts_input, scores, centres, num, features):
    B, N = pts_input.shape[0], pts_input.shape[1]
    pts = pts_input.float().contiguous()
    score = scores.reshape(B, N).float().contiguous()
    cen = centres.float().contiguous()
    if num is not None:
        num = num.to(torch.int32).contiguous()
    feats = features.float().contiguous() if features is not None else None
    return pts, score, cen, num, feats


def instance_clouds(pts_input, scores, centres, num=None, radius=4.0, sampled_pt_num=512, mask_mode=0, mask_thresh=0.5,
                    features=None, return_idx=False):
    """pts_input (B,N,4) x, y, z, reflectance; scores (B,N) or (B,N,1) sigmoid of rpn_cls; centres (B,K,3); num (B) valid
    centre slots per scene (None: all K); features (B,N,C) channels-last, C % 4 == 0.
    -> cloud (B,K,S,5) rows (x - cx, y - cy, z - cz, reflectance, m), cloud_feats (B,K,S,C) | None, count (B,K) int32 =
    the true number of points with sqrt(dx^2 + dz^2) < radius [, pts_idx (B,K,S) int32].  m = score (mask_mode 0,
    generate_box_dataset.py:222) or (score > mask_thresh) - 0.5 (mask_mode 1, tools/eval_auto.py:345, 367).  The first
    min(count, S) members in scene order, repeated cyclically up to S rows (kitti_boxplace_dataset.py:327-337); an empty
    cylinder and every slot >= num[b] give zero rows.  One launch, no host synchronisation, no pre-zeroing."""
    pts, score, cen, num, feats = _prep(pts_input, scores, centres, num, features)
    B, K, S = pts.shape[0], cen.shape[1], int(sampled_pt_num)
    dev = pts.device
    cloud = torch.empty((B, K, S, 5), dtype=torch.float32, device=dev)
    cloud_feats = torch.empty((B, K, S, feats.shape[2]), dtype=torch.float32, device=dev) if feats is not None else None
    count = torch.empty((B, K), dtype=torch.int32, device=dev)
    pts_idx = torch.empty((B, K, S), dtype=torch.int32, device=dev) if return_idx else None
    _C.instance_clouds_forward(pts, score, feats, cen, num, radius, mask_mode, mask_thresh, cloud, cloud_feats, count, pts_idx)
    return (cloud, cloud_feats, count) + ((pts_idx,) if return_idx else ())


def instance_clouds_ragged(pts_input, scores, centres, num=None, radius=4.0, mask_mode=0, mask_thresh=0.5, features=None,
                           return_idx=False):
    """Same inputs -> rows (total,5), row_feats (total,C) | None, offsets (B*K+1) int64, count (B,K) int32 [, row_idx
    (total) int32]: centre (b, k)'s members are rows offsets[b*K + k] : offsets[b*K + k + 1], all of them, in scene order --
    what generate_box_dataset.py:220-229 stores and tools/eval_auto.py:341-372 feeds.  Two launches and ONE host
    synchronisation (the total number of rows sizes the outputs)."""
    pts, score, cen, num, feats = _prep(pts_input, scores, centres, num, features)
    B, K = pts.shape[0], cen.shape[1]
    dev = pts.device
    count = torch.zeros((B, K), dtype=torch.int32, device=dev)
    _C.instance_clouds_count(pts, cen, num, radius, count)
    offsets = torch.zeros(B * K + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
    total = int(offsets[-1])
    rows = torch.empty((total, 5), dtype=torch.float32, device=dev)
    row_feats = torch.empty((total, feats.shape[2]), dtype=torch.float32, device=dev) if feats is not None else None
    row_idx = torch.empty((total,), dtype=torch.int32, device=dev) if return_idx else None
    if total:
        _C.instance_clouds_emit(pts, score, feats, cen, num, radius, mask_mode, mask_thresh, offsets, rows, row_feats, row_idx)
    return (rows, row_feats, offsets, count) + ((row_idx,) if return_idx else ())
