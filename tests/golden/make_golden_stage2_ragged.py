#!/usr/bin/env python
"""Golden fixture for Stage 2 on WHOLE instance clouds: the REFERENCE's own ``RCNNNet`` called ONCE PER CLOUD on (1, n_i, .) inputs,
as tools/eval_auto.py:388 calls it, in float64 and in single-thread fp32:
``python -B tests/golden/make_golden_stage2_ragged.py`` -> stage2_ragged.{npz,json}.
Runs only in the build container (it imports /root/reference); writes data only.

Shims, weight recipe (the seed and the scaled last layers of stage2_forward.json: the same model) and ``run`` are
make_golden_stage2.py's; furthest point sampling and ball query come from the fp32 oracle in both runs and are logged.
  * clouds of SIZES = 1, 37, 127, 128, 129, 513, 1100, 1500 points: both sides of level 1's npoint and of the 512 rows of the fixed
    route.  The last two are real cylinders: 4 m in (x, z) around cars of ``synth.hdl64_cloud(16384, scene)`` scenes (the first
    cars whose cylinders hold enough points), x and z shifted to the car, y lowered by 1.65, cut to size in scene order; most of their
    points lie outside the 1.2 x box and are zeroed in the IoU tower.  The others follow make_golden_stage2.make_inputs, cut to size.
  * before anything is written, per cloud: (a) every index tensor of the fp32 run equals the float64 run's, (b) the fp32 IoU tower
    gives the same index tensors under seeded relative +-2^-21 perturbations of box_ce.  Another input seed is tried when a cloud fails.
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402
import make_golden_stage2 as ms  # noqa: E402
import oracle  # noqa: E402
from ws3d_amd import synth  # noqa: E402

SIZES = (1, 37, 127, 128, 129, 513, 1100, 1500)
CYLINDERS = (6, 7)                     # positions in SIZES of the real cylinders
INPUT_SEEDS = (21, 22, 23, 24, 25, 26)
SCENE = 3000                           # synth.hdl64_cloud(16384, SCENE + 10 * input seed + 0 .. 7)
RADIUS, GROUND_Y = 4.0, 1.65
# yaw, stretch of the recipe clouds (make_golden_stage2.CLOUDS' kind): small ones inside any decoded box, one larger than it
RECIPES = ((0.0, (0.3, 0.3, 0.3)), (0.6, (0.9, 1.0, 1.1)), (-1.2, (1.15, 0.9, 0.95)), (2.5, (0.45, 0.5, 0.45)), (0.3, (0.5, 0.6, 0.5)),
           (1.1, (1.0, 0.9, 1.0)))


def recipe_cloud(n, slot, seed):
    """make_golden_stage2.make_inputs' rows for one cloud of n points"""
    rng = np.random.Generator(np.random.PCG64(5000 + 100 * seed + slot))
    raw = synth.roi_clouds(1, max(n, 2), 100 * seed + slot)[0][:n].astype(np.float64)
    yaw, stretch = RECIPES[slot]
    p = (raw - np.array([0.0, -1.0, 0.0])) * np.array(stretch)
    c, s = np.cos(yaw), np.sin(yaw)
    pts = np.zeros((n, 5), dtype=np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = p[:, 0] * c + p[:, 2] * s, p[:, 1] - 0.8, -p[:, 0] * s + p[:, 2] * c
    pts[:, 3] = rng.uniform(0, 1, n)
    pts[:, 4] = np.where(rng.uniform(0, 1, n) < 0.5, 0.5, -0.5)
    return pts


def cylinders(seed, sizes):
    """one 4 m cylinder per entry of `sizes`: the scenes SCENE + 10 seed + 0 .. 7 are walked car by car and the first car whose
    cylinder holds at least the wanted number of points gives its first rows, in scene order: [x - cx, y - 1.65, z - cz,
    intensity - 0.5, +0.5 within 2 m of the car / -0.5 beyond] -> (clouds, [(scene, car)]) or None"""
    out, where, want = [], [], list(sizes)
    for j in range(8):
        pc, boxes = synth.hdl64_cloud(16384, SCENE + 10 * seed + j, return_boxes=True)
        d2 = (pc[:, None, 0] - boxes[None, :, 0]) ** 2 + (pc[:, None, 2] - boxes[None, :, 2]) ** 2
        for k in range(boxes.shape[0]):
            if not want:
                break
            rows = np.nonzero(d2[:, k] < RADIUS * RADIUS)[0]
            if rows.size < want[0]:
                continue
            rows = rows[:want.pop(0)]
            p = np.zeros((rows.size, 5), dtype=np.float32)
            p[:, 0], p[:, 1], p[:, 2] = pc[rows, 0] - boxes[k, 0], pc[rows, 1] - np.float32(GROUND_Y), pc[rows, 2] - boxes[k, 2]
            p[:, 3] = pc[rows, 3]
            p[:, 4] = np.where(d2[rows, k] < 4.0, 0.5, -0.5)
            out.append(p)
            where.append((SCENE + 10 * seed + j, k))
        if not want:
            return out, where
    return None


def make_clouds(seed):
    cyl = cylinders(seed, [SIZES[i] for i in CYLINDERS])
    if cyl is None:
        return None
    cyl, where = cyl
    make_clouds.where = where
    clouds, slot = [], 0
    for i, n in enumerate(SIZES):
        if i in CYLINDERS:
            clouds.append(cyl[CYLINDERS.index(i)])
        else:
            clouds.append(recipe_cloud(n, slot, seed))
            slot += 1
    return clouds


def main():
    mg.install_reference_shims()
    log = {"fps": [], "bq": []}
    ms.install_stage2_shims(log)
    from lib.config import cfg, cfg_from_file
    for name in ("weaklyRPN.yaml", "weaklyRCNN.yaml", "weaklyIOUN.yaml"):
        cfg_from_file(os.path.join(ms.REF, "tools", "cfgs", name))
    cfg.RCNN.ENABLED = True
    cfg.IOUN.ENABLED = True
    from lib.net.rcnn_net import RCNNNet

    fixed = json.load(open(os.path.join(HERE, "stage2_forward.json")))
    wseed = fixed["seed"]
    assert fixed["last_layer_scale"] == ms.LAST_SCALE and tuple(fixed["scaled_keys"]) == ms.SCALED_KEYS
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(HERE, "stage2_state_dict.json")))["keys"].items()}

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    chosen = None
    for seed in INPUT_SEEDS:
        clouds = make_clouds(seed)
        if clouds is None:
            print("input seed", seed, ": the scene's cylinders are too small")
            continue
        refs, f32s, ok = [], [], True
        for i, pts in enumerate(clouds):
            ref = ms.run(RCNNNet, shapes, wseed, pts[None], True, log)
            f32 = ms.run(RCNNNet, shapes, wseed, pts[None], False, log)
            ok_a = ms.same_indices(ref, f32) and np.array_equal(f32["can_xyz"] == 0, ref["can_xyz"] == 0)
            ce = f32["box_ce"].astype(np.float64)
            ok_b = True
            for p in range(ms.PERTURBATIONS):
                sign = np.random.Generator(np.random.PCG64(9000 + 1000 * seed + 10 * i + p)).choice([-1.0, 1.0], size=(1, 7))
                eps = sign * 2.0 ** -21
                noise = {"iou_trans": (ce[:, 0:3] * eps[:, 0:3]).reshape(1, 1, 3, 1).astype(np.float32),
                         "iou_scale": (1.0 + eps[:, 3:6]).reshape(1, 1, 3, 1).astype(np.float32),
                         "iou_ry": (ce[:, 6:7] * eps[:, 6:7]).reshape(1, 1, 1, 1).astype(np.float32)}
                ok_b = ok_b and ms.same_indices(f32, ms.run(RCNNNet, shapes, wseed, pts[None], False, log, noise), first=3)
            inside = int((np.abs(ref["can_xyz"][0]).max(-1) > 0).sum())
            print("input seed", seed, "cloud", i, "of", pts.shape[0], "points: fp32 == float64 indices:", ok_a, " stable under box_ce perturbation:",
                  ok_b, " points inside the 1.2 x box:", inside)
            ok = ok and ok_a and ok_b
            if i in CYLINDERS:
                ok = ok and inside < pts.shape[0] // 2          # most of a real cylinder is zeroed
            if not ok:
                break
            refs.append(ref)
            f32s.append(f32)
        if ok:
            chosen = (seed, clouds, refs, f32s)
            break
    torch.set_num_threads(threads)
    assert chosen is not None, "no input seed gave a stable fixture"
    seed, clouds, refs, f32s = chosen

    offsets = np.concatenate(([0], np.cumsum([c.shape[0] for c in clouds]))).astype(np.int32)
    arrays = {"pts": np.concatenate(clouds), "offsets": offsets, "box_ce": np.concatenate([r["box_ce"] for r in refs]),
              "can_xyz": np.concatenate([r["can_xyz"][0] for r in refs]).astype(np.float32)}
    e_ref = {}
    for k in ms.OUTPUTS + ("box_ce", "can_xyz"):
        if k in ms.OUTPUTS:
            arrays[k] = np.concatenate([r[k] for r in refs])
        e_ref[k] = float(max(np.abs(f[k].astype(np.float64) - r[k]).max() for f, r in zip(f32s, refs)))
    names = []
    for tower, base in (("rcnn", 0), ("ioun", 3)):
        for lvl in range(3):
            for kind in ("fps", "bq"):
                a = np.concatenate([r[kind][base + lvl] for r in refs])
                assert a.min() >= 0 and a.max() < 32768
                arrays["%s_%s_%d" % (tower, kind, lvl)] = a.astype(np.int16)
                names.append("%s_%s_%d" % (tower, kind, lvl))
    meta = {"generator": "tests/golden/make_golden_stage2_ragged.py", "seed": wseed, "input_seed": seed,
            "cylinder_scene_and_car": [list(map(int, w)) for w in make_clouds.where],
            "sizes": list(SIZES), "cylinders": list(CYLINDERS), "last_layer_scale": ms.LAST_SCALE, "scaled_keys": list(ms.SCALED_KEYS),
            "oracle_dist_mode": oracle.dist_mode(), "fp32_runs": ["1 thread"], "perturbations": ms.PERTURBATIONS,
            "points_inside_box": [int((np.abs(r["can_xyz"][0]).max(-1) > 0).sum()) for r in refs],
            "index_tensors": names, "outputs": list(ms.OUTPUTS), "e_ref": e_ref,
            "max_abs": {k: float(np.abs(arrays[k]).max()) for k in ms.OUTPUTS + ("box_ce", "can_xyz")}}
    np.savez_compressed(os.path.join(HERE, "stage2_ragged.npz"), **arrays)
    with open(os.path.join(HERE, "stage2_ragged.json"), "w") as f:
        json.dump(meta, f, indent=0)
    print("e_ref", json.dumps(e_ref))
    for f in ("stage2_ragged.npz", "stage2_ragged.json"):
        size = os.path.getsize(os.path.join(HERE, f))
        print(f, size, "bytes")
        assert size < 300 * 1024, (f, size)


if __name__ == "__main__":
    main()
