"""ws3d_scan_prepare on the device against its host restatement (ws3d_amd.scan_prepare.prepare_scans_host): every output bit-equal
on ragged batches, on the boundaries of the selection rule, with ties forced, and through the drivers."""
import os

import numpy as np
import pytest
import torch

from ws3d_amd import kitti_io, scan_prepare as sp, synth

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1023, 1025, 3000, 40000)
KEYS = ("pts_input", "src_index", "valid_count", "status")


@pytest.fixture(scope="module")
def cam(tmp_path_factory):
    """calibration and image size of the synthetic KITTI tree"""
    root = str(tmp_path_factory.mktemp("cam"))
    synth.write_kitti_tree(root, [(1, 8, 1)])
    ds = kitti_io.KittiScenes(root, "val")
    return ds.get_calib(1), ds.get_image_shape(1)


@pytest.fixture(scope="module")
def batch():
    """the ragged call: every size of SIZES (seed 3: the 40 000-point scan has V = 23 056, F = 7 073), a scan entirely behind the
    camera between valid ones, and a NaN coordinate in a point that would be valid"""
    scans = [synth.velodyne_scan(n, 3) for n in SIZES]
    behind = synth.velodyne_scan(500, 4)
    behind[:, 0] = -behind[:, 0]
    scans.insert(6, behind)
    scans[8] = scans[8].copy()
    scans[8][5:40, 2] = np.nan                   # (3000 points: some of these 35 are valid without the NaN)
    return scans, [100 + i for i in range(len(scans))]


_host_cache = {}


def host_ref(cam, batch, npoints, key_bits=32, scope=kitti_io.PC_AREA_SCOPE):
    key = (npoints, key_bits, scope is None)
    if key not in _host_cache:
        scans, keys = batch
        res = sp.prepare_scans_host(scans, [cam[0]] * len(scans), [cam[1]] * len(scans), keys, npoints, 666, scope, key_bits)
        for v in res.values():
            v.setflags(write=False)
        _host_cache[key] = res
    return _host_cache[key]


def on_device(cam, scans, keys, npoints, key_bits=32, scope=kitti_io.PC_AREA_SCOPE, seed=666):
    res = sp.prepare_scans(scans, [cam[0]] * len(scans), [cam[1]] * len(scans), keys, npoints, seed, scope, key_bits, device="cuda:0", check=False)
    assert all(res[k].is_cuda for k in KEYS)
    return {k: res[k].cpu().numpy() for k in KEYS}


def assert_same(got, want, rows=slice(None)):
    for k in KEYS:
        a, b = got[k][rows], want[k][rows]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=k)


def test_kernel_takes_the_production_size():
    from ws3d_amd import _lib
    assert _lib.load().ws3d_scan_prepare_limit() >= 16384


@pytest.mark.parametrize("npoints", [16, 100, 16384])
def test_ragged_batch_is_bit_equal_to_the_host_restatement(cam, batch, npoints):
    scans, keys = batch
    want = host_ref(cam, batch, npoints)
    got = on_device(cam, scans, keys, npoints)
    print("npoints %d: V %s status %s" % (npoints, want["valid_count"].tolist(), want["status"].tolist()))
    assert_same(got, want)
    assert want["status"][0] == 1 and want["status"][6] == 1 and want["valid_count"][6] == 0          # empty scan, scan behind the camera
    if npoints == 16384:
        assert want["status"].tolist() == [1, 1, 0, 0, 0, 0, 1, 0, 0, 0] and want["valid_count"][9] == 23056      # subsample path at 16384
        assert (got["src_index"][9] >= 0).all() and len(set(got["src_index"][9].tolist())) == 16384
    nan_rows = np.flatnonzero(np.isnan(scans[8]).any(axis=1))
    assert not np.isin(got["src_index"][8], nan_rows).any() and not np.isnan(got["pts_input"]).any()


def _boundary_cases():
    return [(s, name) for s in (4, 8) for name in ("V", "V+1", "V-1", "F", "F-1")]


@pytest.mark.parametrize("scene,which", _boundary_cases())
def test_boundaries_of_the_selection_rule(cam, batch, scene, which):
    """npoints set from one scene's own V and F (the 65- and the 3000-point scan): V (a permutation), V + 1 (tiled twice), V - 1 (one near
    point dropped), F (no near point kept), F - 1 (status 2 for that scene, the others as when run alone)"""
    scans, keys = batch
    pick = [3, 4, 6, 8, 5]                                     # a short call around the two scenes
    sub, sub_keys = [scans[i] for i in pick], [keys[i] for i in pick]
    cls, _ = sp.classify(scans[scene], sp.calib_tables(cam[0]), cam[1])
    V, F = int((cls != sp.INVALID).sum()), int((cls == sp.FAR).sum())
    assert V > F > 1
    npoints = {"V": V, "V+1": V + 1, "V-1": V - 1, "F": F, "F-1": F - 1}[which]
    want = sp.prepare_scans_host(sub, [cam[0]] * len(sub), [cam[1]] * len(sub), sub_keys, npoints)
    got = on_device(cam, sub, sub_keys, npoints)
    assert_same(got, want)
    at = pick.index(scene)
    assert got["valid_count"][at] == V and got["status"][at] == (2 if which == "F-1" else 0)
    if which == "V":
        assert sorted(got["src_index"][at].tolist()) == np.flatnonzero(cls != sp.INVALID).tolist()
    if which == "F":
        assert sorted(got["src_index"][at].tolist()) == np.flatnonzero(cls == sp.FAR).tolist()
    if which == "F-1":
        assert not got["pts_input"][at].any() and (got["src_index"][at] == -1).all()
        other = 0 if at != 0 else 1
        alone = on_device(cam, sub[other:other + 1], sub_keys[other:other + 1], npoints)
        for k in KEYS:
            np.testing.assert_array_equal(alone[k][0], got[k][other], err_msg=k)
        with pytest.raises(ValueError, match="beyond 40 m"):
            sp.prepare_scans(sub, [cam[0]] * len(sub), [cam[1]] * len(sub), sub_keys, npoints, device="cuda:0")


@pytest.mark.parametrize("key_bits,npoints", [(4, 100), (4, 16384), (1, 100), (1, 16384)])
def test_ties_on_the_cut_and_in_the_order(cam, batch, key_bits, npoints):
    scans, keys = batch
    assert_same(on_device(cam, scans, keys, npoints, key_bits), host_ref(cam, batch, npoints, key_bits))


def test_reversed_batch_other_seed_and_no_scope(cam, batch):
    scans, keys = batch
    want = host_ref(cam, batch, 16384)
    rev = on_device(cam, scans[::-1], keys[::-1], 16384)
    for k in KEYS:
        np.testing.assert_array_equal(rev[k][::-1], want[k], err_msg=k)
    other = on_device(cam, scans, keys, 16384, seed=667)
    assert not np.array_equal(other["src_index"][9], want["src_index"][9])
    open_want = host_ref(cam, batch, 16384, scope=None)
    assert open_want["valid_count"][9] > want["valid_count"][9]
    assert_same(on_device(cam, scans, keys, 16384, scope=None), open_want)


# ----------------------------------------------------------------------------- drivers
TREE = [(7, 60000, 1), (8, 9000, 2), (11, 30000, 3)]


def _read(files):
    return [open(f, "rb").read() for f in files]


def test_infer_kitti_routes(tmp_path):
    """device and host ingest write byte-identical result files (the same rows go in); 'off' is the driver as it was.  (Two batches in
    flight instead of four: every slot of the pipeline is primed per run, and the short last batch is reached either way.)"""
    from ws3d_amd import infer_kitti
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, TREE)
    names = ["000007.txt", "000008.txt", "000011.txt"]
    dev = infer_kitti.run(root, "val", str(tmp_path / "dev"), batch=2, depth=2, device_ingest="device")
    host = infer_kitti.run(root, "val", str(tmp_path / "host"), batch=2, depth=2, device_ingest="host")
    assert [os.path.basename(f) for f in dev] == names == [os.path.basename(f) for f in host]
    assert _read(dev) == _read(host) and sum(len(t) for t in _read(dev)) > 0
    off = infer_kitti.run(root, "val", str(tmp_path / "off"), batch=2, depth=2, device_ingest="off")
    assert [os.path.basename(f) for f in off] == names
    for f in off + dev:
        objs = kitti_io.read_label_file(f)
        assert len(objs) <= 100
        for o in objs:
            assert o.cls_type == "Car" and np.isfinite(o.box3d()).all() and 0.0 <= o.box2d[0] <= o.box2d[2] <= 1241.0
    with pytest.raises(ValueError):
        infer_kitti.run(root, "val", str(tmp_path / "bad"), batch=2, device_ingest="gpu")


def test_detect_kitti_device_and_host_ingest_write_the_same_files(tmp_path):
    """the two-stage driver with Stage 2 from the fixture's weights and the IoU threshold lowered, as in its own test (the plain seeded
    heads write empty files): boxes come out, and the same ones on both routes"""
    import dataclasses
    from tests import stage2_reference as ref
    from ws3d_amd import detect_kitti, stage1, stage2
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, TREE[:2])
    fx = ref.fixture()
    ckpt = str(tmp_path / "rcnn.pth")
    torch.save({"epoch": 1, "model_state": {"rcnn_net." + k: v for k, v in ref.fixture_state_dict(fx[1], fx[2]).items()}}, ckpt)
    kw = dict(batch=2, rcnn_ckpt=ckpt, cfg=dataclasses.replace(stage1.DEFAULT_CFG, score_thresh=0.1),
              rcnn_cfg=dataclasses.replace(stage2.DEFAULT_CFG, ioun_score_thresh=-1e9))
    dev = detect_kitti.run(root, "val", str(tmp_path / "dev"), device_ingest="device", **kw)
    host = detect_kitti.run(root, "val", str(tmp_path / "host"), device_ingest="host", **kw)
    assert [os.path.basename(f) for f in dev] == ["000007.txt", "000008.txt"] == [os.path.basename(f) for f in host]
    lines = sum(t.count(b"\n") for t in _read(dev))
    print("detect_kitti: %d result lines" % lines)
    assert lines > 0 and _read(dev) == _read(host)
