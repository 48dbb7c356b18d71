"""CPU checks of scan preparation (ws3d_amd/scan_prepare.py, csrc/scan_prepare.hip): the host restatement of the contract against
``kitti_io`` on the golden tree, the sampler's selection and order rules on a class vector, statuses, and the C entry's argument
validation (no GPU: everything refused here is refused before any HIP call)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from ws3d_amd import kitti_io, scan_prepare as sp, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS4 = 4.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    with open(os.path.join(HERE, "golden", "kitti_ingest.json")) as f:
        fx = json.load(f)
    root = str(tmp_path_factory.mktemp("kitti"))
    synth.write_kitti_tree(root, [tuple(s) for s in fx["scenes"]])
    return kitti_io.KittiScenes(root, "val")


@pytest.fixture(scope="module")
def raw_items(tree):
    return [tree.raw_item(i) for i in range(len(tree))]


def test_raw_item_reads_files_and_samples_nothing(tree, raw_items):
    it = raw_items[0]
    assert set(it) == {"sample_id", "pts_lidar", "calib", "img_shape"} and it["sample_id"] == 7
    assert it["pts_lidar"].shape == (60000, 4) and it["img_shape"] == (375, 1242, 3) and isinstance(it["calib"], kitti_io.Calibration)
    np.testing.assert_array_equal(it["pts_lidar"], tree.get_lidar(7))


def _sums64(raw, tables):
    """float64 values of the contract's sums and, for each, the sum of the absolute values of its terms expanded down to the inputs
    (what bounds the rounding error of ANY fp32 evaluation order of that sum by 4 * 2^-24 * S: one rounding per product, one per addition)"""
    T, P = tables[:12].reshape(4, 3).astype(np.float64), tables[12:].reshape(3, 4).astype(np.float64)
    p = raw[:, :3].astype(np.float64)
    r = p @ T[:3] + T[3]
    Sr = np.abs(p) @ np.abs(T[:3]) + np.abs(T[3])
    h = r @ P[:, :3].T + P[:, 3]
    Sh = Sr @ np.abs(P[:, :3]).T + np.abs(P[:, 3])
    return r, Sr, h, Sh


def _boundary_slack(raw, tables, img_shape, scope):
    """per point: the smallest |float64 distance to a mask boundary| / (4 * 2^-24 * S of the sum that is compared there); below 1 the
    fp32 result may fall on either side.  The image tests are taken in their homogeneous form h_0 - W r_2 (r_2 > 0 where it matters)."""
    r, Sr, h, Sh = _sums64(raw, tables)
    H, W = float(img_shape[0]), float(img_shape[1])
    P23 = float(tables[12 + 11])
    ratios = [np.abs(h[:, 0]) / (EPS4 * Sh[:, 0]), np.abs(h[:, 0] - W * r[:, 2]) / (EPS4 * (Sh[:, 0] + W * Sr[:, 2])),
              np.abs(h[:, 1]) / (EPS4 * Sh[:, 1]), np.abs(h[:, 1] - H * r[:, 2]) / (EPS4 * (Sh[:, 1] + H * Sr[:, 2])),
              np.abs(h[:, 2] - P23) / (EPS4 * (Sh[:, 2] + abs(P23))), np.abs(h[:, 2] - P23 - 40.0) / (EPS4 * (Sh[:, 2] + abs(P23)))]
    for j, (lo, hi) in enumerate(scope):
        ratios += [np.abs(r[:, j] - lo) / (EPS4 * Sr[:, j]), np.abs(r[:, j] - hi) / (EPS4 * Sr[:, j])]
    return np.min(np.stack(ratios), axis=0)


def test_masks_and_coordinates_agree_with_kitti_io(raw_items):
    """the restatement's valid set and near / far split equal kitti_io's (BLAS sums in its own order) except where a point lies within
    the rounding bound of a boundary, for at most 0.1 % of the points; coordinates within 4 * 2^-24 * sum|terms| of lidar_to_rect"""
    for it in raw_items:
        raw, calib, shape = it["pts_lidar"], it["calib"], it["img_shape"]
        tables = sp.calib_tables(calib)
        cls, rect = sp.classify(raw, tables, shape)
        order = np.argsort(-raw[:, 2])                                  # rpn_input_from_scan's first line
        srt = raw[order]
        ref_rect = calib.lidar_to_rect(srt[:, 0:3])
        ref_img, ref_depth = calib.rect_to_img(ref_rect)
        keep = kitti_io.valid_point_mask(ref_rect, ref_img, ref_depth, shape)
        full = kitti_io.rpn_input_from_scan(raw, calib, shape, random_select=False)
        np.testing.assert_array_equal(full, np.concatenate((ref_rect[keep], (srt[keep, 3] - 0.5).reshape(-1, 1)), axis=1))
        ref_cls = np.zeros(len(raw), dtype=np.uint8)
        ref_cls[order] = np.where(keep, np.where(ref_depth < 40.0, sp.NEAR, sp.FAR), sp.INVALID)
        differ = np.flatnonzero(ref_cls != cls)
        print("scene %d: %d of %d classes differ" % (it["sample_id"], len(differ), len(raw)))
        assert len(differ) <= len(raw) // 1000
        assert (_boundary_slack(raw[differ], tables, shape, kitti_io.PC_AREA_SCOPE) < 1.0).all()
        ref_raw_order = np.empty_like(ref_rect)
        ref_raw_order[order] = ref_rect
        _, Sr, _, _ = _sums64(raw, tables)
        err = np.abs(rect.astype(np.float64) - ref_raw_order.astype(np.float64))
        print("scene %d: %.1f %% of the rows bit-equal, largest difference %.2e" %
              (it["sample_id"], 100.0 * (rect == ref_raw_order).all(axis=1).mean(), err.max()))
        assert (err <= EPS4 * Sr).all()


# ----------------------------------------------------------------------------- the sampler on a class vector
def _class_vector():
    """300 points: 48 invalid, 192 near, 60 far, shuffled.  V = 252 so that at npoints = 1000 the tiled list (reps = 4, 1008 entries)
    loses 8 entries: under a correct uniform draw a point loses 3 of its 4 copies with probability ~ 4 (8/1008)^3 = 2e-6, 5e-4 over
    the 252 points and below 1 % over the 16 seeds used -- small enough for 'between reps - 2 and reps' to be asserted of every draw
    (at V = 260, 40 dropped entries, one draw in 17 would break it)."""
    cls = np.array([sp.INVALID] * 48 + [sp.NEAR] * 192 + [sp.FAR] * 60, dtype=np.uint8)
    return cls[np.random.Generator(np.random.PCG64(5)).permutation(300)]


def _lexicographic(cls, npoints, seed, key, key_bits):
    """the selection and order rules spelled with Python tuples"""
    n = len(cls)
    valid = [i for i in range(n) if cls[i] != sp.INVALID]
    far = [i for i in range(n) if cls[i] == sp.FAR]
    if len(valid) > npoints:
        cand, k, kept = [i for i in range(n) if cls[i] == sp.NEAR], npoints - len(far), list(far)
    else:
        reps = -(-npoints // len(valid))
        cand, k, kept = [r * n + i for r in range(reps) for i in valid], npoints, []
    sel, _ = sp.entry_keys(np.array(cand, dtype=np.uint64), seed, key, key_bits)
    kept += [e for _, e in sorted(zip(sel.tolist(), cand))[:k]]
    _, order = sp.entry_keys(np.array(kept, dtype=np.uint64), seed, key, key_bits)
    return [e for _, e in sorted(zip(order.tolist(), kept))]


@pytest.mark.parametrize("key_bits", [32, 4])
def test_subsample_keeps_far_points_and_draws_near_ones_uniformly(key_bits):
    cls = _class_vector()
    near, far = np.flatnonzero(cls == sp.NEAR), np.flatnonzero(cls == sp.FAR)
    hits = np.zeros(300, dtype=np.int64)
    seeds = 512
    for seed in range(seeds):
        e, status = sp.sample_entries(cls, 100, seed, 42, key_bits)
        assert status == sp.OK and len(e) == 100 == len(set(e.tolist())) and (e < 300).all()
        assert set(far.tolist()) <= set(e.tolist()) and (cls[e.astype(np.int64)] != sp.INVALID).all()
        hits[e.astype(np.int64)] += 1
        if seed < 8:
            assert e.tolist() == _lexicographic(cls, 100, seed, 42, key_bits)
    p = (100 - len(far)) / len(near)
    z = (hits[near] - seeds * p) / np.sqrt(seeds * p * (1 - p))
    print("key_bits %d: inclusion counts of the near points, largest |z| = %.2f" % (key_bits, np.abs(z).max()))
    assert np.abs(z).max() < 5.0


@pytest.mark.parametrize("key_bits", [32, 4])
def test_tiling_draws_every_valid_point_about_reps_times(key_bits):
    cls = _class_vector()
    valid = np.flatnonzero(cls != sp.INVALID)
    reps = -(-1000 // len(valid))
    for seed in range(16):
        e, status = sp.sample_entries(cls, 1000, seed, 7, key_bits)
        assert status == sp.OK and len(e) == 1000 == len(set(e.tolist()))
        count = np.bincount((e % np.uint64(300)).astype(np.int64), minlength=300)
        assert count[cls == sp.INVALID].sum() == 0 and count.sum() == 1000
        assert (count[valid] >= reps - 2).all() and (count[valid] <= reps).all()
        if seed < 4:
            assert e.tolist() == _lexicographic(cls, 1000, seed, 7, key_bits)
    e, status = sp.sample_entries(cls, len(valid), 3, 7, key_bits)         # V == npoints: a permutation of the valid points
    assert status == sp.OK and sorted(e.tolist()) == valid.tolist()
    assert e.tolist() != valid.tolist() and e.tolist() == _lexicographic(cls, len(valid), 3, 7, key_bits)


def test_ties_exist_at_four_key_bits_and_keys_follow_splitmix64():
    sel, order = sp.entry_keys(np.arange(300, dtype=np.uint64), 1, 2, 4)
    assert sel.max() < 16 and order.max() < 16 and len(set(sel.tolist())) <= 16
    # splitmix64's published first outputs for the state 0 (the generator adds the golden ratio before mixing)
    assert int(sp.splitmix64(0)[0]) == 0xE220A8397B1DCDAF and int(sp.splitmix64(0x9E3779B97F4A7C15)[0]) == 0x6E789E6AA1B965F4
    base = int(sp.splitmix64((666 + sp.GOLDEN * 7) % 2 ** 64)[0])
    h = int(sp.splitmix64((base + 12345) % 2 ** 64)[0])
    sel32, ord32 = sp.entry_keys(np.array([12345], dtype=np.uint64), 666, 7, 32)
    assert (int(sel32[0]), int(ord32[0])) == (h >> 32, h & 0xffffffff)
    sel5, ord5 = sp.entry_keys(np.array([12345], dtype=np.uint64), 666, 7, 5)
    assert (int(sel5[0]), int(ord5[0])) == ((h >> 32) >> 27, (h & 0xffffffff) >> 27)
    # a negative scene key is its two's complement
    a = sp.entry_keys(np.arange(4, dtype=np.uint64), 1, -1, 32)[0]
    b = sp.entry_keys(np.arange(4, dtype=np.uint64), 1, 2 ** 64 - 1, 32)[0]
    np.testing.assert_array_equal(a, b)


# ----------------------------------------------------------------------------- whole scenes
def _small_scenes(raw_items):
    calib, shape = raw_items[0]["calib"], raw_items[0]["img_shape"]
    scans = [synth.velodyne_scan(n, 20 + k) for k, n in enumerate((3000, 700, 1500))]
    return scans, [calib] * 3, [shape] * 3


def test_rows_do_not_depend_on_the_batch_layout(raw_items):
    scans, calibs, shapes = _small_scenes(raw_items)
    keys = [11, 12, 13]
    whole = sp.prepare_scans_host(scans, calibs, shapes, keys, npoints=600, seed=9)
    assert whole["status"].tolist() == [0, 0, 0] and whole["pts_input"].shape == (3, 600, 4) and whole["pts_input"].dtype == np.float32
    assert whole["valid_count"][0] > 600 >= whole["valid_count"][1]            # both branches of the rule are in play
    for b in range(3):
        alone = sp.prepare_scans_host(scans[b:b + 1], calibs[:1], shapes[:1], keys[b:b + 1], npoints=600, seed=9)
        for k in whole:
            np.testing.assert_array_equal(alone[k][0], whole[k][b], err_msg=k)
    rev = sp.prepare_scans_host(scans[::-1], calibs, shapes, keys[::-1], npoints=600, seed=9)
    for k in whole:
        np.testing.assert_array_equal(rev[k][::-1], whole[k], err_msg=k)
    other_seed = sp.prepare_scans_host(scans, calibs, shapes, keys, npoints=600, seed=10)
    other_key = sp.prepare_scans_host(scans, calibs, shapes, [21, 22, 23], npoints=600, seed=9)
    for b in range(3):
        assert not np.array_equal(other_seed["src_index"][b], whole["src_index"][b])
        assert not np.array_equal(other_key["src_index"][b], whole["src_index"][b])


def test_statuses_wrapper_errors_and_source_indices(raw_items):
    scans, calibs, shapes = _small_scenes(raw_items)
    behind = scans[1].copy()
    behind[:, 0] = -behind[:, 0]                                             # every point behind the camera
    scans = [scans[0], behind, scans[2], np.zeros((0, 4), dtype=np.float32)]
    calibs, shapes, keys = calibs + calibs[:1], shapes + shapes[:1], [1, 2, 3, 4]
    res = sp.prepare_scans_host(scans, calibs, shapes, keys, npoints=600)
    assert res["status"].tolist() == [0, 1, 0, 1] and res["valid_count"][1] == 0 == res["valid_count"][3]
    assert not res["pts_input"][1].any() and (res["src_index"][1] == -1).all() and not res["pts_input"][3].any()
    for b in (0, 2):
        src = res["src_index"][b]
        assert src.min() >= 0 and src.max() < len(scans[b])
        rect, _, _, _ = sp.project(scans[b][src], sp.calib_tables(calibs[b]))
        np.testing.assert_array_equal(res["pts_input"][b, :, :3], rect)
        np.testing.assert_array_equal(res["pts_input"][b, :, 3], scans[b][src, 3] - np.float32(0.5))
        cls, _ = sp.classify(scans[b], sp.calib_tables(calibs[b]), shapes[b])
        assert (cls[src] != sp.INVALID).all()
    # more far points than rows: status 2, the other scenes as before; the wrapper raises, also on its host route
    cls0, _ = sp.classify(scans[0], sp.calib_tables(calibs[0]), shapes[0])
    F = int((cls0 == sp.FAR).sum())
    assert F > 2
    few = sp.prepare_scans_host(scans, calibs, shapes, keys, npoints=F - 1)
    assert few["status"][0] == 2 and not few["pts_input"][0].any() and few["status"][1] == 1
    ok = sp.prepare_scans_host(scans[2:3], calibs[:1], shapes[:1], keys[2:3], npoints=F - 1)
    np.testing.assert_array_equal(few["pts_input"][2], ok["pts_input"][0])
    with pytest.raises(ValueError, match="beyond 40 m"):
        sp.prepare_scans(scans, calibs, shapes, keys, npoints=F - 1, device="cpu")
    got = sp.prepare_scans(scans, calibs, shapes, keys, npoints=F - 1, device="cpu", check=False)
    assert got["status"].tolist() == few["status"].tolist()
    exact = sp.prepare_scans(scans, calibs, shapes, keys, npoints=F, device="cpu")          # npoints == F: no near point is kept
    assert exact["status"][0] == 0 and (cls0[exact["src_index"][0].numpy()] == sp.FAR).all()
    with pytest.raises(ValueError):
        sp.prepare_scans(scans, calibs, shapes, keys, npoints=0, device="cpu")
    with pytest.raises(ValueError):
        sp.prepare_scans(scans, calibs, shapes, keys, key_bits=33, device="cpu")


def test_nan_point_is_invalid_and_scope_none_keeps_more(raw_items):
    scans, calibs, shapes = _small_scenes(raw_items)
    raw = scans[0].copy()
    cls, _ = sp.classify(raw, sp.calib_tables(calibs[0]), shapes[0])
    i = int(np.flatnonzero(cls != sp.INVALID)[0])
    raw[i, 1] = np.nan
    cls_nan, _ = sp.classify(raw, sp.calib_tables(calibs[0]), shapes[0])
    assert cls_nan[i] == sp.INVALID and (np.delete(cls_nan, i) == np.delete(cls, i)).all()
    open_cls, _ = sp.classify(scans[0], sp.calib_tables(calibs[0]), shapes[0], area_scope=None)
    assert (open_cls != sp.INVALID).sum() > (cls != sp.INVALID).sum() and ((open_cls != sp.INVALID) >= (cls != sp.INVALID)).all()


def test_driver_helpers(tree):
    with pytest.raises(ValueError):
        sp.driver_dataset(tree, "gpu")
    assert sp.driver_dataset(tree, "off") is tree
    rawds = sp.driver_dataset(tree, "host")
    assert len(rawds) == 2 and "pts_lidar" in rawds[1]
    from ws3d_amd import loader
    (items,) = list(loader.item_batches(rawds, [[0, 1]], workers=2))            # loader processes only read files
    assert [it["sample_id"] for it in items] == [7, 8] and items[0]["pts_lidar"].shape == (60000, 4) and "pts_input" not in items[0]
    pts = sp.batch_points([rawds[1]], "host", 16384, 666, "cpu")
    ref = sp.prepare_scans_host([rawds[1]["pts_lidar"]], [rawds[1]["calib"]], [rawds[1]["img_shape"]], [8])
    np.testing.assert_array_equal(pts.numpy(), ref["pts_input"])
    assert ref["valid_count"][0] < 16384                                       # the 9000-point scene is tiled


# ----------------------------------------------------------------------------- the C entry
@pytest.fixture(scope="module")
def lib():
    from ws3d_amd import _lib, build
    build.build()
    return _lib.load()


def test_entries_are_declared_exported_and_bound(lib):
    from ws3d_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ws3d_ops.h")).read()
    assert "scan_prepare.hip" in build.SOURCES
    for name in ("ws3d_scan_prepare_limit", "ws3d_scan_prepare_workspace_bytes", "ws3d_scan_prepare"):
        assert re.search(r"WS3D_API\s+[\w\s\*]+?\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 6 == lib.ws3d_abi_version()
    assert lib.ws3d_scan_prepare_limit() >= 16384
    assert lib.ws3d_scan_prepare_workspace_bytes(0, 0) == 0
    assert lib.ws3d_scan_prepare_workspace_bytes(2, 1000) >= 1000
    assert lib.ws3d_scan_prepare_workspace_bytes(4, 100000) > lib.ws3d_scan_prepare_workspace_bytes(2, 1000)


def _aligned(nbytes):
    buf = np.zeros(nbytes + 64, dtype=np.uint8)
    at = (-buf.ctypes.data) % 64
    return buf, buf.ctypes.data + at


def test_invalid_arguments_are_refused_before_any_hip_call(lib):
    from ws3d_amd import _lib
    keep, p = _aligned(1 << 16)
    scope = (ctypes.c_float * 6)(-40, 40, -3, 3, 0, 70.4)
    need = lib.ws3d_scan_prepare_workspace_bytes(1, 100)
    names = ("offsets", "raw", "calib", "img_hw", "scene_key", "pts_input", "src_index", "valid_count", "status", "workspace")

    def call(scenes=1, total=100, max_n=100, npoints=16, key_bits=32, ws_bytes=need, scope=scope, **ptr):
        a = {k: ptr.get(k, p) for k in names}
        return lib.ws3d_scan_prepare(scenes, a["offsets"], total, max_n, a["raw"], a["calib"], a["img_hw"], scope, npoints, 666, a["scene_key"],
                                     key_bits, a["pts_input"], a["src_index"], a["valid_count"], a["status"], a["workspace"], ws_bytes, None)

    assert call(npoints=0) == _lib.E_INVALID and b"invalid" in lib.ws3d_last_error()
    assert call(npoints=-5) == _lib.E_INVALID
    assert call(key_bits=0) == _lib.E_INVALID and call(key_bits=33) == _lib.E_INVALID and call(key_bits=-1) == _lib.E_INVALID
    assert call(scenes=-1) == _lib.E_INVALID and call(total=-1) == _lib.E_INVALID and call(max_n=-1) == _lib.E_INVALID
    for name in names:
        assert call(**{name: None}) == _lib.E_INVALID, name
    assert call(ws_bytes=need - 1) == _lib.E_INVALID and call(ws_bytes=0) == _lib.E_INVALID
    assert call(raw=p + 4) == _lib.E_INVALID and call(pts_input=p + 8) == _lib.E_INVALID          # 16-byte alignment
    assert call(npoints=lib.ws3d_scan_prepare_limit() + 1, ws_bytes=1 << 30) == _lib.E_UNSUPPORTED
    assert call(npoints=16384, max_n=1 << 20, total=1 << 20, ws_bytes=1 << 30) == _lib.E_UNSUPPORTED   # entry numbers would pass 2^32
    # no scene: nothing to do, whatever else is passed
    assert call(scenes=0, ws_bytes=0, scope=None, **{name: None for name in names}) == 0
    del keep
