"""ws3d_amd.gen_box_dataset: the labelling against a restatement of generate_box_dataset.py:164-183, 232-251 (CPU), and the
driver on a synthetic KITTI tree (GPU)."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ----------------------------------------------------------------------------- the reference's lines, restated
def ref_corners3d(boxes3d):
    """lib/utils/kitti_utils.py:66-101 boxes3d_to_corners3d(rotate=True): float32 corners, bottom face (y) first, top at y - h"""
    n = boxes3d.shape[0]
    h, w, l = boxes3d[:, 3], boxes3d[:, 4], boxes3d[:, 5]
    x_c = np.array([l / 2., l / 2., -l / 2., -l / 2., l / 2., l / 2., -l / 2., -l / 2.], dtype=np.float32).T
    z_c = np.array([w / 2., -w / 2., -w / 2., w / 2., w / 2., -w / 2., -w / 2., w / 2.], dtype=np.float32).T
    y_c = np.zeros((n, 8), dtype=np.float32)
    y_c[:, 4:8] = -h.reshape(n, 1).repeat(4, axis=1)
    ry = boxes3d[:, 6]
    zeros, ones = np.zeros(ry.size, dtype=np.float32), np.ones(ry.size, dtype=np.float32)
    rot = np.transpose(np.array([[np.cos(ry), zeros, -np.sin(ry)], [zeros, ones, zeros], [np.sin(ry), zeros, np.cos(ry)]]), (2, 0, 1))
    r = np.matmul(np.concatenate((x_c.reshape(-1, 8, 1), y_c.reshape(-1, 8, 1), z_c.reshape(-1, 8, 1)), axis=2), rot)
    out = r + boxes3d[:, None, 0:3]
    return out.astype(np.float32)


def ref_label(center, cur_box_point, gt_boxes3d_cam, delaunay):
    """generate_box_dataset.py:164-183 (val split: the noisy boxes play no part) and :232-251 for one centre"""
    dist2 = lambda a, b: np.sqrt(np.sum((a[None, :] - b[:, None]) ** 2, axis=2))   # noqa: E731  lib/utils/distance.py:5
    box_id, fg_flag, gt_box = -1, False, np.zeros(7)
    gt_mask = np.zeros((cur_box_point.shape[0], 1))
    if gt_boxes3d_cam.shape[0] == 0:
        return fg_flag, box_id, gt_box.reshape(1, 7), gt_mask
    d = dist2(gt_boxes3d_cam[:, [0, 2]], center.reshape(1, 3)[:, [0, 2]])           # (1, G)
    index = np.argmin(d, axis=-1)
    foreground_flag = np.min(d, axis=-1) < np.float32(0.7)        # (torch compares a float32 tensor with the scalar in float32)
    foreground_flag_g = np.min(d, axis=-1) < np.float32(1.5)
    if foreground_flag[0]:
        fg_flag = True
    if foreground_flag_g[0]:
        box_id = index[0]
        gt_box = gt_boxes3d_cam[box_id].copy().reshape(7)
        gt_box[0] = gt_box[0] - center[0]
        gt_box[2] = gt_box[2] - center[2]
        gt_box[3] = gt_box[3] * 1.2
        gt_box[4] = gt_box[4] * 1.2
        gt_box[5] = gt_box[5] * 1.2
        corners = ref_corners3d(gt_box.reshape(-1, 7))
        gt_mask = (delaunay(corners.reshape(-1, 3)).find_simplex(cur_box_point) >= 0).reshape(-1, 1)      # kitti_utils.in_hull :163-177
        gt_box = gt_boxes3d_cam[box_id].copy().reshape(7)
        gt_box[0] = gt_box[0] - center[0]
        gt_box[2] = gt_box[2] - center[2]
    return fg_flag, int(box_id), gt_box.reshape(1, 7), gt_mask


def face_distance(points, gt_box_rel):
    """distance of every point to the nearest face PLANE of the box enlarged by 1.2 (float64, the box's own frame)"""
    b = gt_box_rel.astype(np.float32).copy()
    b[3:6] = b[3:6] * np.float32(1.2)
    p = points.astype(np.float64) - b[0:3].astype(np.float64)
    c, s = np.cos(np.float64(b[6])), np.sin(np.float64(b[6]))
    al, aw = p[:, 0] * c - p[:, 2] * s, p[:, 0] * s + p[:, 2] * c
    return np.minimum.reduce([np.abs(np.abs(al) - b[5] / 2.0), np.abs(np.abs(aw) - b[4] / 2.0), np.abs(p[:, 1]), np.abs(p[:, 1] + np.float64(b[3]))])


def test_labelling_matches_reference_restatement():
    """flags, box_id and gt_boxes equal; gt_mask equal on every point farther than 1e-4 m from a face of the enlarged box.  The
    exclusion is capped: it may leave out at most 1 % of the points (a 2e-4 m shell around a car-sized box's ~60 m^2 surface is
    about 0.01 % of the cylinder's volume)."""
    spatial = pytest.importorskip("scipy.spatial")        # present on the CPU machine: this test runs there
    from ws3d_amd import gen_box_dataset
    rng = np.random.default_rng(2024)
    seen = {"fg": 0, "match_only": 0, "none": 0, "no_gt": 0, "inside": 0}
    total = excluded = 0
    headings = np.concatenate((np.linspace(-np.pi, np.pi, 33), rng.uniform(-np.pi, np.pi, 87)))       # the full circle
    for trial, ry in enumerate(headings):
        center = np.array([rng.uniform(-30, 30), 0.0, rng.uniform(5, 60)], dtype=np.float32)
        n = int(rng.integers(6, 1500))
        r, phi = 4.0 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        cloud = np.stack((r * np.cos(phi), rng.uniform(-1.5, 2.2, n), r * np.sin(phi)), axis=1).astype(np.float32)   # shifted to the centre
        G = 0 if trial % 17 == 16 else int(rng.integers(1, 5))
        gt = np.zeros((G, 7), dtype=np.float32)
        for g in range(G):
            off = rng.uniform(0, 3.0) if g == 0 else rng.uniform(2.0, 20.0)       # box 0: inside / between / beyond 0.7 m and 1.5 m
            a = rng.uniform(0, 2 * np.pi)
            gt[g] = (center[0] + off * np.cos(a), rng.uniform(1.4, 1.9), center[2] + off * np.sin(a), rng.uniform(1.3, 1.9), rng.uniform(1.4, 1.9),
                     rng.uniform(3.2, 4.6), ry if g == 0 else rng.uniform(-np.pi, np.pi))
        gt = gt[rng.permutation(G)]
        fg, box_id, gt_box, gt_mask = gen_box_dataset.label_instance(center, cloud, gt)
        rfg, rid, rbox, rmask = ref_label(center, cloud, gt, spatial.Delaunay)
        assert isinstance(fg, bool) and isinstance(box_id, int) and fg == rfg and box_id == rid, trial
        assert gt_box.dtype == np.float32 and gt_box.shape == (1, 7) and gt_mask.dtype == np.float32 and gt_mask.shape == (n, 1)
        np.testing.assert_array_equal(gt_box, rbox.astype(np.float32))
        total += n
        if box_id >= 0:
            far = face_distance(cloud, gt_box[0]) > 1e-4
            excluded += int((~far).sum())
            np.testing.assert_array_equal(gt_mask[far, 0] > 0, rmask[far, 0] > 0)
            seen["inside"] += int(gt_mask.sum())
            seen["fg" if fg else "match_only"] += 1
        else:
            assert not gt_mask.any() and not gt_box.any() and not fg
            seen["no_gt" if G == 0 else "none"] += 1
    assert excluded <= 0.01 * total, (excluded, total)
    assert all(v > 0 for v in seen.values()), seen


def test_enlarged_box_grows_upwards_only():
    """a box's y is its bottom face and it spans y - h ... y: the 1.2 x h reaches higher (smaller y), not below the bottom"""
    from ws3d_amd import gen_box_dataset
    gt = np.array([[10.0, 1.6, 20.0, 1.5, 1.6, 4.0, 0.3]], dtype=np.float32)
    center = np.array([10.0, 0.0, 20.0], dtype=np.float32)
    pts = np.array([[0, 1.61, 0], [0, 1.59, 0], [0, 1.6 - 1.79, 0], [0, 1.6 - 1.81, 0], [2.39 * np.cos(0.3), 1.0, -2.39 * np.sin(0.3)],
                    [2.41 * np.cos(0.3), 1.0, -2.41 * np.sin(0.3)], [0.95 * np.sin(0.3), 1.0, 0.95 * np.cos(0.3)], [0.97 * np.sin(0.3), 1.0, 0.97 * np.cos(0.3)]],
                   dtype=np.float32)
    fg, box_id, gt_box, gt_mask = gen_box_dataset.label_instance(center, pts, gt)
    assert fg and box_id == 0
    np.testing.assert_array_equal(gt_box, np.array([[0.0, 1.6, 0.0, 1.5, 1.6, 4.0, 0.3]], dtype=np.float32))
    np.testing.assert_array_equal(gt_mask[:, 0], [0, 1, 1, 0, 1, 0, 1, 0])


# ----------------------------------------------------------------------------- GPU: the driver
KEYS = {"instance_id", "sample_id", "box_id", "center", "foreground_flag", "gt_boxes", "cur_box_point", "cur_box_reflect", "cur_prob_mask",
        "gt_mask"}


@pytest.mark.gpu
def test_driver_writes_reference_shaped_records(tmp_path):
    from ws3d_amd import gen_box_dataset, synth
    with open(os.path.join(HERE, "golden", "kitti_ingest.json")) as f:
        scenes = [tuple(s) for s in json.load(f)["scenes"]]
    root, out = str(tmp_path / "kitti"), str(tmp_path / "boxes")
    synth.write_kitti_tree(root, scenes)
    seen = {}
    # score_thresh: the CLI's default 0.1 first, lower values only if that keeps no centre.  Needed on the seeded weights: 0.1 itself
    # (13228 records from the two scenes: the untrained heads score thousands of points above it).
    for thresh in (0.1, 0.01, 0.001):
        seen.clear()
        path = gen_box_dataset.run(root, "val", out, batch=2, score_thresh=thresh, with_features=True,
                                   hook=lambda sid, pts, sc: seen.__setitem__(sid, (pts, sc)))
        with open(path, "rb") as f:
            data = pickle.load(f)
        if data:
            break
    print("score_thresh needed:", thresh, "records:", len(data))
    assert os.path.basename(path) == "val_boxes.pkl" and len(data) >= 1, thresh
    assert sorted(seen) == [s[0] for s in scenes]
    # loads without ws3d_amd importable types
    code = "import pickle, sys; d = pickle.load(open(sys.argv[1], 'rb')); assert 'ws3d_amd' not in sys.modules and 'torch' not in sys.modules; print(len(d))"
    r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and int(r.stdout) == len(data), r.stderr
    assert [d["instance_id"] for d in data] == list(range(len(data)))
    for d in data:
        assert set(d) == KEYS | {"cur_pts_feature"}
        n = d["cur_box_point"].shape[0]
        assert n > 0 and type(d["instance_id"]) is int and type(d["sample_id"]) is int and type(d["box_id"]) is int and type(d["foreground_flag"]) is bool
        shapes = {"center": (1, 3), "gt_boxes": (1, 7), "cur_box_point": (n, 3), "cur_box_reflect": (n, 1), "cur_prob_mask": (n, 1), "gt_mask": (n, 1),
                  "cur_pts_feature": (n, 128)}
        for k, shp in shapes.items():
            assert type(d[k]) is np.ndarray and d[k].dtype == np.float32 and d[k].shape == shp, (k, d[k].dtype, d[k].shape)
        # recomputation from the record's own centre and the scene the clouds were cut from (generate_box_dataset.py:200, 216-227)
        pts, sc = seen[d["sample_id"]]
        c = d["center"].reshape(3)
        assert c[1] == 0.0
        dx, dz = c[0] - pts[:, 0], c[2] - pts[:, 2]
        flag = np.sqrt(dx * dx + dz * dz) < np.float32(4.0)
        np.testing.assert_array_equal(d["cur_box_point"], pts[flag, :3] - c.reshape(1, 3))
        np.testing.assert_array_equal(d["cur_box_reflect"], pts[flag, 3:4])
        np.testing.assert_array_equal(d["cur_prob_mask"], sc[flag].reshape(-1, 1))
        fg, box_id, gt_box, gt_mask = gen_box_dataset.label_instance(c, d["cur_box_point"], np.array(
            [[-0.65, 1.71, 46.70, 1.65, 1.67, 3.64, -1.59], [-16.53, 2.39, 58.49, 1.67, 1.87, 3.69, 1.57]], dtype=np.float32))   # synth.KITTI_LABEL_TEXT's cars
        assert (fg, box_id) == (d["foreground_flag"], d["box_id"])
        np.testing.assert_array_equal(gt_box, d["gt_boxes"])
        np.testing.assert_array_equal(gt_mask, d["gt_mask"])
