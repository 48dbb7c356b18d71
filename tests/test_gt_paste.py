"""The ground-truth paste augmentation on the host: ``gt_paste.paste_scene`` against a restatement of the reference's
``aug_gt_dict`` / ``apply_gt_aug_to_one_scene`` (lib/datasets/kitti_rcnn_dataset.py:257-371) written out below in this file's own
words, the database writer / reader (``gt_database``) on the host route, and the untouched default of the training datasets."""
import copy
import random

import numpy as np
import pytest

from ws3d_amd import gt_database as gdb
from ws3d_amd import gt_paste, kitti_io, losses

MIMIC, EASY_MIN = 100, 128
CAR_POINTS = (10, 40, 90, 150, 200, 260, 300)       # three hard and four easy objects per scan at EASY_MIN


# ----------------------------------------------------------------------------- a small labelled world
def _scan(seed):
    """(pts_rect (n,3) float32, intensity (n,), [Object3d]): a road sheet and seven cars filled with points"""
    rng = np.random.default_rng(seed)
    road = np.stack([rng.uniform(-40, 40, 3000), 1.6 + rng.normal(0, 0.02, 3000), rng.uniform(0, 70, 3000)], 1)
    pts, objs = [road], []
    for j, n in enumerate(CAR_POINTS):
        x, z = -30.0 + 10.0 * j + rng.uniform(-1, 1), rng.uniform(8, 60)
        h, w, l, ry = rng.uniform(1.4, 1.7), rng.uniform(1.5, 1.8), rng.uniform(3.4, 4.4), rng.uniform(-np.pi, np.pi)
        u, v, t = rng.uniform(-0.47, 0.47, n) * l, rng.uniform(-0.47, 0.47, n) * w, rng.uniform(0.03, 0.97, n) * h
        pts.append(np.stack([x + u * np.cos(ry) + v * np.sin(ry), 1.6 - t, z - u * np.sin(ry) + v * np.cos(ry)], 1))
        objs.append(kitti_io.Object3d("Van" if j == 2 else "Car", 0.0, 0.0, 0.0, np.zeros(4, np.float32), h, w, l,
                                      np.array([x, 1.6, z], np.float32), ry))
    objs.append(kitti_io.Object3d("Pedestrian", 0.0, 0.0, 0.0, np.zeros(4, np.float32), 1.7, 0.6, 0.6, np.array([0, 1.6, 20], np.float32), 0.0))
    objs.append(kitti_io.Object3d("Car", 0.0, 0.0, 0.0, np.zeros(4, np.float32), 1.5, 1.6, 4.0, np.array([0, 1.6, 90], np.float32), 0.0))  # out of scope
    pts = np.concatenate(pts).astype(np.float32)
    return pts, rng.uniform(0, 1, pts.shape[0]).astype(np.float32), objs


@pytest.fixture(scope="module")
def world():
    return [(sid, *_scan(sid)) for sid in (3, 11, 15, 20)]


@pytest.fixture(scope="module")
def records(world):
    recs = gdb.build_gt_database(world, easy_min_points=EASY_MIN, mimic_points=MIMIC, device=None, chunk=2)
    for r in recs:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)          # shared by every test below: nothing may write into the database
    return recs


@pytest.fixture(scope="module")
def db(records):
    return gdb.GtDatabase(records, mimic_points=MIMIC)


# ----------------------------------------------------------------------------- the reference's paste, restated
def _restated_object_draw(points, box):
    """data_augmentation (:223-255) as aug_gt_dict calls it: rotation and scaling always, flip with probability one half"""
    on = 1 - np.random.rand(3)
    if on[0] < 1.0:
        a = np.random.uniform(-np.pi / 18.0, np.pi / 18.0)
        turn = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        points[:, [0, 2]] = np.dot(points[:, [0, 2]], np.transpose(turn))
        box[:, [0, 2]] = np.dot(box[:, [0, 2]], np.transpose(turn))
    if on[1] < 1.0:
        s = np.random.uniform(0.95, 1.05)
        points = points * s
        box[:, 0:6] = box[:, 0:6] * s
    if on[2] < 0.5:
        points[:, 0] = -points[:, 0]
        box[:, 0] = -box[:, 0]
    return points, box


def _pair_distance(a, b):
    return np.sqrt(np.sum((a[None, :] - b[:, None]) ** 2, axis=2))


def _restated_paste(oracle, pts_rect, intensity, own_centres, easy, hard):
    """:266-371 with the global ``random`` / ``numpy.random`` streams.  -> (pts, intensity, extra centres, kept candidate ids) or None
    where the reference itself stops (no candidate survives: its np.min over no centres raises)"""
    total = 15
    chosen = copy.deepcopy(random.sample(hard, total // 3))
    chosen += copy.deepcopy(random.sample(easy, total // 3 * 2))
    for g in chosen:
        g["points"], box = _restated_object_draw(g["points"].reshape(-1, 3), g["gt_box3d"].reshape(-1, 7))
        g["gt_box3d"] = box.reshape(-1)
    for i in range(total // 3 * 2, total):
        chosen[i]["presampling_flag"] = False
    angle = np.random.uniform(0.25 * np.pi, 0.75 * np.pi, total)
    rng_far, rng_near = np.random.uniform(35., 70., total // 3 * 2), np.random.uniform(3, 35., total // 3)
    reach = np.concatenate((rng_far, rng_near))
    spot = np.zeros((total, 3))
    spot[:, 0], spot[:, 2] = np.cos(angle) * reach, np.sin(angle) * reach
    everyone = np.concatenate((own_centres, spot), axis=0)
    table = _pair_distance(everyone[:, [0, 2]], spot[:, [0, 2]])
    own = own_centres.shape[0]
    survivors = [i for i in range(total) if np.min(table[i, :i + own]) > 6.0]
    if not survivors:
        return None
    chosen, spot = [chosen[i] for i in survivors], spot[survivors]
    for g in chosen:
        if not g["presampling_flag"]:
            continue
        g["points"], g["intensity"] = g["points"][g["sampled_mask"]], g["intensity"][g["sampled_mask"]]
        pick = oracle.furthest_point_sample(np.ascontiguousarray(g["points"], np.float32)[None], MIMIC)[0]
        g["points"], g["intensity"] = g["points"][pick], g["intensity"][pick]
    free = np.min(_pair_distance(spot[:, [0, 2]], pts_rect[:, [0, 2]]), axis=-1) > 3.6
    pts_rect, intensity, boxes = pts_rect[free], intensity[free], np.zeros((0, 7))
    for g, c in zip(chosen, spot):
        # the reference's in-place '+=' of a float64 scalar into float32 points: a float32 sum with the scalar rounded first
        g["points"][:, 0] += np.float32(c[0])
        g["points"][:, 2] += np.float32(c[2])
        g["gt_box3d"][0], g["gt_box3d"][2] = c[0], c[2]
        pts_rect = np.concatenate((pts_rect, g["points"]), axis=0)
        intensity = np.concatenate((intensity, g["intensity"].reshape(-1)), axis=0)
        boxes = np.concatenate((boxes, g["gt_box3d"].reshape(-1, 7)), axis=0)
    return pts_rect, intensity, boxes[:, :3], survivors


def _grid(step):
    xs, zs = np.arange(-52.0, 52.1, step), np.arange(0.0, 72.1, step)
    return np.stack([np.repeat(xs, zs.size), np.full(xs.size * zs.size, 1.6), np.tile(zs, xs.size)], 1).astype(np.float32)


def _own_centres(world, k):
    return np.array([o.pos for o in world[k][3] if gdb.keep_object(o)], dtype=np.float32)


SCENES = {"plain": 0, "other_scan": 2, "crowded": 1, "full": 1}


@pytest.mark.parametrize("name", list(SCENES))
def test_draw_mode_reproduces_the_restated_reference(oracle, world, db, name):
    _, pts, inten, _ = world[SCENES[name]]
    own = {"crowded": _grid(13.0), "full": _grid(8.0)}.get(name, _own_centres(world, SCENES[name]))
    seed = 100 + len(name)
    random.seed(seed); np.random.seed(seed)
    want = _restated_paste(oracle, pts.copy(), inten.copy(), own, db.easy, db.hard)
    after = (random.random(), np.random.rand())
    random.seed(seed); np.random.seed(seed)
    got_pts, got_int, got_extra = gt_paste.paste_scene(pts, inten, own, db, np.random, random, mimic="draw")
    assert (random.random(), np.random.rand()) == after            # the same number of draws from both streams
    if name == "full":
        assert want is None
        assert got_pts is pts and got_int is inten and got_extra.shape == (0, 3)
        return
    w_pts, w_int, w_extra, survivors = want
    assert {"plain": len(survivors) >= 6, "other_scan": len(survivors) >= 6, "crowded": 1 <= len(survivors) <= 7}[name], survivors
    assert got_pts.dtype == w_pts.dtype == np.float32 and np.array_equal(got_pts, w_pts)
    assert np.array_equal(got_int, w_int) and got_int.shape == (got_pts.shape[0],)
    assert got_extra.dtype == np.float32 and np.array_equal(got_extra, w_extra.astype(np.float32))
    assert np.array_equal(got_extra.astype(np.float64), w_extra)         # the reference's float64 table holds float32 values


class _NoObjectAugmentation:
    """a numpy-like stream whose rand() draws are 0: ``1 - rand(3)`` then enables none of rotation / scaling / flip"""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def rand(self, *shape):
        return np.zeros(shape) if shape else 0.0

    def uniform(self, *a):
        return self.rs.uniform(*a)


def test_stored_picks_equal_drawn_picks_without_object_augmentation(world, db):
    _, pts, inten, _ = world[0]
    own = _own_centres(world, 0)
    out = [gt_paste.paste_scene(pts, inten, own, db, _NoObjectAugmentation(5), random.Random(5), mimic=mode) for mode in ("stored", "draw")]
    assert out[0][2].shape[0] >= 6
    for a, b in zip(*out):
        assert np.array_equal(a, b)


class _Scripted:
    """a stream that hands out prepared uniform() arrays (angles, far ranges, near ranges) and never augments an object"""

    def __init__(self, xz):
        xz = np.asarray(xz, dtype=np.float64)
        self.queue = [np.arctan2(xz[:, 1], xz[:, 0]), np.hypot(xz[:10, 0], xz[:10, 1]), np.hypot(xz[10:, 0], xz[10:, 1])]

    def rand(self, *shape):
        return np.zeros(shape)

    def uniform(self, lo, hi, size):
        out = self.queue.pop(0)
        assert out.shape == (size,)
        return out


def test_collision_clearing_and_thinning_rules(world, db):
    _, pts, inten, _ = world[0]
    own = np.array([[0.0, 1.6, 40.0]], dtype=np.float32)
    # candidate 0 sits 4 m from the scene's own centre: dropped.  Candidate 1 is 9 m from that centre but 5 m from the DROPPED
    # candidate 0: dropped too (the reference's table holds every earlier candidate).  The rest stand 9 m apart on two rows.
    xz = [(4.0, 40.0), (9.0, 40.0)] + [(-36.0 + 9.0 * j, 55.0) for j in range(8)] + [(-18.0 + 9.0 * j, 20.0) for j in range(5)]
    picks = random.Random(9)
    chosen = picks.sample(db.hard, 5) + picks.sample(db.easy, 10)
    keep, obj_pts, obj_int, extra = gt_paste.plan_paste(pts, own, db, _Scripted(xz), random.Random(9))
    kept = list(range(2, 15))
    assert np.allclose(extra[:, [0, 2]], np.array(xz)[kept], atol=1e-4) and extra.shape == (13, 3)
    assert [p.shape[0] for p in obj_pts] == [chosen[i]["points"].shape[0] if (i < 5 or i >= 10) else MIMIC for i in kept]
    assert all(chosen[i]["points"].shape[0] > EASY_MIN for i in range(5, 15))           # 10..14: easy objects, pasted whole
    assert all(p.shape[0] == q.shape[0] for p, q in zip(obj_pts, obj_int))
    # clearing: '>' keeps -- no surviving scene point within 3.6 m (x, z) of a kept centre, and nothing else was removed
    d = np.sqrt(((pts[:, None, [0, 2]].astype(np.float64) - np.array(xz)[kept][None]) ** 2).sum(-1)).min(1)
    assert np.array_equal(keep, d > 3.6) and 0 < (~keep).sum() < keep.size
    out_pts, out_int, _ = gt_paste.paste_scene(pts, inten, own, db, _Scripted(xz), random.Random(9))
    assert np.array_equal(out_pts[:keep.sum()], pts[keep]) and np.array_equal(out_int[:keep.sum()], inten[keep])     # stable compaction
    assert np.array_equal(out_pts[keep.sum():], np.concatenate(obj_pts))                                            # appended in order
    # an object's y is never moved: the pasted heights are the stored ones
    first = chosen[2]
    assert np.array_equal(obj_pts[0][:, 1], first["points"][:, 1]) and np.array_equal(extra[0, 1], first["gt_box3d"][1])


def test_scene_without_own_centres_and_bad_mode(world, db):
    _, pts, inten, _ = world[0]
    out = gt_paste.paste_scene(pts, inten, np.zeros((0, 3), np.float32), db, np.random.RandomState(1), random.Random(1))
    assert out[2].shape[0] >= 1 and out[0].shape[0] == out[1].shape[0]
    with pytest.raises(ValueError):
        gt_paste.paste_scene(pts, inten, np.zeros((0, 3), np.float32), db, np.random.RandomState(1), random.Random(1), mimic="fresh")


# ----------------------------------------------------------------------------- the database
def test_host_crop_matches_the_oracle(oracle, world):
    _, pts, _, objs = world[0]
    boxes = np.stack([o.box3d() for o in objs])
    assert np.array_equal(gdb.points_in_boxes_host(pts, boxes), oracle.pts_in_boxes3d(pts, boxes) > 0)


def test_database_records_and_round_trip(oracle, world, records, tmp_path):
    assert len(records) == 4 * len(CAR_POINTS)                     # the pedestrian and the out-of-scope car are not in it
    by_scan = {sid: [r for r in records if r["sample_id"] == sid] for sid in (3, 11, 15, 20)}
    for sid, pts, inten, objs in world:
        for r, o in zip(by_scan[sid], [o for o in objs if gdb.keep_object(o)]):
            n = r["points"].shape[0]
            assert set(r) - {"mimic_index"} == {"sample_id", "points", "intensity", "gt_box3d", "obj", "presampling_flag", "sampled_mask"}
            assert r["points"].dtype == np.float32 and r["points"].shape == (n, 3) and r["intensity"].shape == (n,)
            assert r["gt_box3d"].dtype == np.float32 and r["gt_box3d"].shape == (7,) and r["gt_box3d"][0] == 0 == r["gt_box3d"][2]
            assert np.array_equal(r["gt_box3d"][[1, 3, 4, 5, 6]], o.box3d()[[1, 3, 4, 5, 6]])
            assert isinstance(r["obj"], kitti_io.Object3d) and r["obj"].pos[0] == 0 == r["obj"].pos[2] and o.pos[0] != 0   # a copy
            assert r["sampled_mask"].dtype == bool and r["sampled_mask"].all() and r["sampled_mask"].shape == (n,)
            assert isinstance(r["presampling_flag"], bool) and r["presampling_flag"] == (n > EASY_MIN)
            inside = oracle.pts_in_boxes3d(pts, o.box3d()[None])[0] > 0
            assert n == inside.sum() >= 10 and np.array_equal(r["intensity"], inten[inside])
            assert np.array_equal(r["points"][:, 1], pts[inside][:, 1])                                              # y absolute
            assert np.array_equal(r["points"][:, [0, 2]], pts[inside][:, [0, 2]] - o.box3d()[[0, 2]])                # x, z relative
            if r["presampling_flag"]:
                assert r["mimic_index"].dtype == np.int32
                assert np.array_equal(r["mimic_index"], oracle.furthest_point_sample(r["points"][None], MIMIC)[0])
            else:
                assert "mimic_index" not in r
    path = str(tmp_path / "aug_gt_database.pkl")
    gdb.save_gt_database(records, path)
    full = gdb.load_gt_database(path)
    assert (len(full.easy), len(full.hard), full.mimic_points) == (16, 12, MIMIC)
    part = gdb.load_gt_database(path, last_sample_id=15)
    assert (len(part.easy), len(part.hard)) == (12, 9) and all(r["sample_id"] <= 15 for r in part.easy + part.hard)
    assert np.array_equal(part.easy[0]["points"], by_scan[3][3]["points"])
    with pytest.raises(ValueError, match="too short.*3 hard and 4 easy.*sample_id <= 3"):
        gdb.load_gt_database(path, last_sample_id=3)
    # a pickle made for the reference carries no mimic_index: it is sampled on load
    bare = [{k: v for k, v in r.items() if k != "mimic_index"} for r in records]
    gdb.save_gt_database(bare, path)
    again = gdb.load_gt_database(path)
    assert all(np.array_equal(a["mimic_index"], b["mimic_index"]) for a, b in zip(again.easy, full.easy))
    with pytest.raises(ValueError):
        gdb.build_gt_database(world, easy_min_points=50, mimic_points=100, device=None)


# ----------------------------------------------------------------------------- the datasets
def test_default_is_untouched_and_the_paste_reaches_the_labels(db, tmp_path):
    from ws3d_amd import synth, train_rpn
    # SyntheticCenters without a database: the scene and labels of the generators, and no draw from the stream
    rs = np.random.RandomState(4)
    item = train_rpn.SyntheticCenters(2, npoints=2048, rng=rs)[1]
    pc = synth.lidar_cloud(2048, 8001)
    centres = synth.random_boxes3d(15, 8001 * 7919 + 13)[:, :3].astype(np.float32)
    cls, reg = losses.gaussian_center_labels(pc[:, :3], centres)
    assert np.array_equal(item["pts_input"], pc) and np.array_equal(item["gt_centers"], centres)
    assert np.array_equal(item["rpn_cls_label"], cls.astype(np.float32)) and np.array_equal(item["rpn_reg_label"], reg)
    assert rs.rand() == np.random.RandomState(4).rand()
    pasted = train_rpn.SyntheticCenters(2, npoints=2048, rng=np.random.RandomState(4), gt_database=db)[1]
    assert pasted["pts_input"].shape == (2048, 4) and pasted["pts_input"].dtype == np.float32
    assert pasted["gt_centers"].shape[0] > 15 and np.array_equal(pasted["gt_centers"][:15], centres)
    assert pasted["rpn_cls_label"].shape == (2048,) and -0.5 <= pasted["pts_input"][:, 3].min() and pasted["pts_input"][:, 3].max() < 0.5
    # KittiCenters / rpn_input_from_scan
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, [(7, 20000, 1), (8, 9000, 2)])
    plain = train_rpn.KittiCenters(root, "val", npoints=4096, rng=np.random.RandomState(6))
    scenes = plain.scenes
    want = kitti_io.rpn_input_from_scan(scenes.get_lidar(7), scenes.get_calib(7), scenes.get_image_shape(7), 4096, True, np.random.RandomState(6))
    same = kitti_io.rpn_input_from_scan(scenes.get_lidar(7), scenes.get_calib(7), scenes.get_image_shape(7), 4096, True, np.random.RandomState(6),
                                        paste=None)
    got = plain[0]
    own = np.array([o.pos for o in plain._objects(7)], dtype=np.float32).reshape(-1, 3)
    assert np.array_equal(want, same) and np.array_equal(got["pts_input"], want.astype(np.float32)) and np.array_equal(got["gt_centers"], own)
    cls, reg = losses.gaussian_center_labels(want[:, :3], own)
    assert np.array_equal(got["rpn_cls_label"], cls.astype(np.float32)) and np.array_equal(got["rpn_reg_label"], reg)
    aug = train_rpn.KittiCenters(root, "val", npoints=4096, rng=np.random.RandomState(6), gt_database=db)[0]
    assert aug["pts_input"].shape == (4096, 4) and aug["gt_centers"].shape[0] > own.shape[0]
    assert np.array_equal(aug["gt_centers"][:own.shape[0]], own) and aug["rpn_cls_label"].shape == (4096,)
    none = train_rpn.KittiCenters(root, "val", npoints=4096, rng=np.random.RandomState(6), gt_database=db, gt_aug_prob=0.0)[0]
    assert np.array_equal(none["gt_centers"], own)          # the draw happened, the paste did not
