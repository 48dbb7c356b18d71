"""Ground-truth paste augmentation of one training scene, on the host: the reference's ``apply_gt_aug_to_one_scene`` and
``aug_gt_dict`` (lib/datasets/kitti_rcnn_dataset.py:257-371; GT_AUG_ENABLED / GT_AUG_APPLY_PROB of tools/cfgs/weaklyRPN.yaml).

Up to 15 database objects (``gt_database.GtDatabase``) are pasted into a scene before it is filtered and sub-sampled: 5 hard ones
(few points) and 5 easy ones thinned to ``mimic_points`` by furthest point sampling -- the "mimic hard" objects -- at 35-70 m, and
5 easy ones pasted whole at 3-35 m, all on the arc 45-135 degrees in front of the sensor.  The draws come in the reference's order:

  1. ``pyrng.sample(hard, 5)``, 2. ``pyrng.sample(easy, 10)``, 3. per object the draws of ``losses.scene_augmentation`` (rotation
  about y, scaling, x flip of the object about ITS OWN centre: its points are stored centre-relative in x and z),
  4. ``rng.uniform(pi/4, 3pi/4, 15)``, 5. ``rng.uniform(35, 70, 10)``, 6. ``rng.uniform(3, 35, 5)``.

What the reference's lines do, kept here:
  * candidate i is dropped when it lies within 6.0 m (x, z) of an ORIGINAL centre or of ANY earlier candidate, dropped ones included;
  * objects 10-14 have their easy flag cleared, so only objects 5-9 -- where kept -- are thinned;
  * scene points within 3.6 m (x, z; ``>`` keeps) of any kept centre are removed, the rest keep their order;
  * kept objects are appended in candidate order; an object's y is never moved (the database stores it absolute).
Where it departs:
  * no kept candidate: the reference dies on an empty ``np.min``; here the scene comes back unchanged (so does a scene without
    original centres and a first candidate, which has nothing to collide with);
  * ``mimic="stored"`` (the default) takes the thinned subset from the database (``mimic_index``, sampled once from the un-augmented
    object when the database was built) instead of sampling the augmented object on every draw.  The three augmentations are
    similarities, so in exact arithmetic the picks are the same; in float32 a near-tie may fall the other way, which is the one
    place the pasted points can differ from the reference's in bits.  ``mimic="draw"`` samples per draw like the reference
    (``fps_host``, the CPU route of ``pn2_ops.furthest_point_sample_ragged``) and reproduces it bit for bit.
Nothing here touches the device: it runs inside the forked loader processes.
"""
from __future__ import annotations

import numpy as np

from . import _lib, fps_host, losses

AUG_NUM = 15                      # kitti_rcnn_dataset.py:21
SPARSE_DISTANCE = 6.0             # GT_DATABASE_SPARSE_DISTANCE, :20
CLEAR_DISTANCE = 3.6              # :342


def _bev_distance(centre, pts_xz):
    """distance_2_numpy (lib/utils/distance.py:5) of one centre (x, z) to points (N,2): float64 like the reference's broadcast"""
    return np.sqrt((centre[0] - pts_xz[:, 0]) ** 2 + (centre[1] - pts_xz[:, 1]) ** 2)


def plan_paste(pts_rect, gt_centres, db, rng, pyrng, mimic: str = "stored"):
    """the draws and decisions of one paste -> (keep (N,) bool over the scene points | None when nothing is pasted,
    [object points (n_i,3) float32 at their new place], [object intensities (n_i,)], extra_centres (K,3) float32)"""
    if mimic not in ("stored", "draw"):
        raise ValueError("mimic must be 'stored' or 'draw'")
    third = AUG_NUM // 3
    picked = pyrng.sample(db.hard, third) + pyrng.sample(db.easy, 2 * third)
    obj_pts, obj_box = [], []
    for rec in picked:                                                       # aug_gt_dict: every object, kept or not, draws
        p, b, _ = losses.scene_augmentation(rec["points"].reshape(-1, 3), rec["gt_box3d"].reshape(-1, 7), rng)
        obj_pts.append(p)
        obj_box.append(b.reshape(-1))
    thin = [bool(rec["presampling_flag"]) and i < 2 * third for i, rec in enumerate(picked)]
    theta = rng.uniform(0.25 * np.pi, 0.75 * np.pi, AUG_NUM)
    depth = np.concatenate((rng.uniform(35.0, 70.0, 2 * third), rng.uniform(3, 35.0, third)))
    centre = np.zeros((AUG_NUM, 3))
    centre[:, 0] = np.cos(theta) * depth
    centre[:, 2] = np.sin(theta) * depth

    originals = np.asarray(gt_centres)
    originals = originals.reshape(-1, originals.shape[-1] if originals.ndim == 2 else 3)[:, :3]
    rivals = np.concatenate((originals, centre), axis=0)[:, [0, 2]]        # float64
    k0 = originals.shape[0]
    kept = [i for i in range(AUG_NUM)
            if i + k0 == 0 or np.min(_bev_distance(centre[i, [0, 2]], rivals[:i + k0])) > SPARSE_DISTANCE]
    if not kept:
        return None, [], [], np.zeros((0, 3), dtype=np.float32)

    out_pts, out_int, extra = [], [], []
    for i in kept:
        rec, p, inten = picked[i], obj_pts[i], np.asarray(picked[i]["intensity"]).reshape(-1)
        if thin[i]:
            mask = rec["sampled_mask"]
            p, inten = p[mask], inten[mask]
            if mimic == "stored":
                sel = rec["mimic_index"]
            else:
                sel = fps_host.furthest_point_sample(np.ascontiguousarray(p, dtype=np.float32), db.mimic_points, _lib.DIST_MODE)
            p, inten = p[sel], inten[sel]
        p = np.array(p, dtype=np.float32, copy=True)
        # float32 sums with the centre rounded to float32 first (what the reference's in-place '+=' of a float64 scalar computes
        # under the value-based casting of its numpy); y stays
        p[:, 0] = p[:, 0] + np.float32(centre[i, 0])
        p[:, 2] = p[:, 2] + np.float32(centre[i, 2])
        box = obj_box[i].astype(np.float32)
        box[0], box[2] = centre[i, 0], centre[i, 2]
        out_pts.append(p)
        out_int.append(np.asarray(inten).reshape(-1))
        extra.append(box[:3])
    xz = np.asarray(pts_rect)[:, [0, 2]]
    nearest = np.full(xz.shape[0], np.inf)
    for i in kept:
        nearest = np.minimum(nearest, _bev_distance(centre[i, [0, 2]], xz))
    return nearest > CLEAR_DISTANCE, out_pts, out_int, np.stack(extra).astype(np.float32)


def paste_scene(pts_rect, intensity, gt_centres, db, rng, pyrng, mimic: str = "stored"):
    """pts_rect (N,3), intensity (N,) raw in [0,1), gt_centres (K,>=3) of the scene's own objects, db a ``GtDatabase``, rng a
    ``numpy.random``-like stream (rand / uniform), pyrng a ``random.Random``-like one (sample) ->
    (pts_rect (N',3), intensity (N',), extra_centres (K',3) float32): the cleared scene followed by the pasted objects, and the
    centres to append to the scene's labels (x, z the new place, y the object's own)."""
    keep, obj_pts, obj_int, extra = plan_paste(pts_rect, gt_centres, db, rng, pyrng, mimic)
    if keep is None:
        return pts_rect, intensity, extra
    pts = np.concatenate([np.asarray(pts_rect)[keep]] + obj_pts, axis=0)
    inten = np.concatenate([np.asarray(intensity).reshape(-1)[keep]] + obj_int, axis=0)
    return pts, inten, extra
