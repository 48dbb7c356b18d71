"""The ground-truth database built on the device (crop by ``ws3d_pts_in_boxes3d``, all easy objects of a chunk of scans through one
``ws3d_furthest_point_sampling_ragged`` launch) against the host build, and training steps on pasted scenes on both label routes."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def builds():
    from ws3d_amd import gt_database as gdb
    scenes = list(gdb.synthetic_scenes(8))
    kw = dict(easy_min_points=gdb.SYNTHETIC_EASY_MIN_POINTS, chunk=3)            # three chunks: 3 + 3 + 2 scans
    return gdb.build_gt_database(scenes, device=torch.device("cuda:0"), **kw), gdb.build_gt_database(scenes, device=None, **kw)


def test_device_and_host_builds_are_identical(builds):
    dev, host = builds
    assert len(dev) == len(host) > 0
    easy = sum(r["presampling_flag"] for r in dev)
    assert easy >= 10 and len(dev) - easy >= 5              # enough to draw from (train_rpn --gt_aug synthetic relies on it)
    for a, b in zip(dev, host):
        assert set(a) == set(b)
        for key in a:
            if key == "obj":
                assert a[key].cls_type == b[key].cls_type and np.array_equal(a[key].box3d(), b[key].box3d())
            elif isinstance(a[key], np.ndarray):
                assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (a["sample_id"], key)
            else:
                assert a[key] == b[key], (a["sample_id"], key)
    assert all(r["mimic_index"].shape == (100,) and len(set(r["mimic_index"].tolist())) == 100 for r in dev if r["presampling_flag"])


@pytest.mark.parametrize("device_targets", [False, True])
def test_training_steps_on_pasted_scenes(builds, device_targets):
    from ws3d_amd import gt_database as gdb, stage1, train_rpn
    db = gdb.GtDatabase(builds[0])
    cfg = stage1.RPNConfig(num_points=4096, npoints=(1024, 256, 64, 16))
    tcfg = train_rpn.TrainConfig()
    plain = train_rpn.SyntheticCenters(2, npoints=4096, config_id=31, labels=not device_targets)
    ds = train_rpn.SyntheticCenters(2, npoints=4096, config_id=31, labels=not device_targets, rng=np.random.RandomState(7), gt_database=db)
    torch.manual_seed(5)
    model = stage1.Stage1Net(mode="TRAIN", cfg=cfg).cuda().train()
    opt = train_rpn.AdamOneCycle(model.parameters(), 100, tcfg)
    collate = train_rpn._collate_centers if device_targets else train_rpn._collate
    for it in range(3):
        items = [ds[i] for i in range(2)]
        assert all(s["pts_input"].shape == (4096, 4) and s["gt_centers"].shape[0] > plain[i]["gt_centers"].shape[0] for i, s in enumerate(items))
        tb = train_rpn.train_step(model, opt, collate(items), it, cfg, tcfg, torch.device("cuda"), fused_loss=device_targets)
        assert math.isfinite(float(tb["loss"])) and math.isfinite(float(tb["grad_norm"])) and int(tb["rpn_fg_sum"]) > 0
