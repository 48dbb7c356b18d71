"""GPU checks of Stage 2 on whole instance clouds (csrc/stage2_ragged.hip, stage2.Stage2Net.rcnn_forward_ragged): the three
kernels against the C oracle / the per-cloud kernels on every cloud alone (exact); the network -- ragged route and per-cloud loop,
teacher-forced and free-running -- against the float64 run of the REFERENCE's own RCNNNet on every cloud alone
(tests/golden/stage2_ragged.*) and, for equal sizes, against tests/golden/stage2_forward.*; chunking; the driver.  Bounds: 4 x the
error of the reference's single-thread fp32 run of the same quantity against float64 (the rule of tests/test_gpu_stage2.py)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import stage2_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 37, 63, 64, 65, 127, 128, 129, 1000, 4096, 4097]      # both sides of m = 128, of a wave, of the on-chip limit
HALF_SAME, ALL_SAME, ORIGIN = 9, 4, 8                                 # clouds (by position in SIZES) with special content


def _packed(clouds):
    sizes = [c.shape[0] for c in clouds]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return np.concatenate(clouds).astype(np.float32), offsets, sizes


@pytest.fixture(scope="module")
def clouds():
    """car-sized clouds of SIZES points; one with half its points identical (the IoU tower's zeroed pattern, zeros in front and
    scattered), one of identical points only, one with most points at the origin"""
    from ws3d_amd import synth
    cs = [synth.roi_clouds(1, n, 300 + j)[0].copy() for j, n in enumerate(SIZES)]
    g = np.random.Generator(np.random.PCG64(11))
    cs[HALF_SAME][g.permutation(SIZES[HALF_SAME])[:SIZES[HALF_SAME] // 2]] = 0.0
    cs[ALL_SAME][:] = cs[ALL_SAME][0]
    cs[ORIGIN][g.permutation(SIZES[ORIGIN])[:100]] = 0.0
    return cs


@pytest.fixture(scope="module")
def fps_expected(oracle, clouds):
    """the oracle's picks per cloud alone, m = 128 (its first 32 are the m = 32 picks: the selection is greedy); computed once"""
    return np.stack([oracle.furthest_point_sample(c[None], 128)[0] for c in clouds])


# ------------------------------------------------------------------------------------------------ canonical transform
def test_canonical_ragged_then_embed_is_bit_equal_to_embed_per_cloud():
    """sizes (1, 63, 64, 65, 200): the 64-row tiles of the embed kernel straddle clouds; the second-to-last box is so small that every
    point of its cloud is zeroed"""
    from ws3d_amd import compat as C
    from tests.test_gpu_stage2 import _embed_weights
    sizes = [1, 63, 64, 65, 200]
    g = torch.Generator().manual_seed(5)
    T = sum(sizes)
    pts = torch.cat((torch.randn(T, 3, generator=g) * torch.tensor([1.5, 0.6, 0.8]), torch.rand(T, 1, generator=g),
                     (torch.rand(T, 1, generator=g) < 0.5).float() - 0.5), dim=-1)
    box = torch.cat((torch.randn(5, 3, generator=g) * 0.2, torch.tensor([1.5, 1.6, 3.9]) * (1 + 0.1 * torch.randn(5, 3, generator=g)),
                     torch.rand(5, 1, generator=g) * 6.0 - 3.0), dim=1)
    box[3, 0:3] = torch.tensor([40.0, 0.0, 0.0])
    box[3, 3:6] = 1e-3
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32).cuda()
    packed = [(t.t().contiguous() if t.dim() == 2 else t).cuda() for t in _embed_weights(7)]
    pts_d, box_d = pts.cuda(), box.cuda()
    can = C.stage2_canonical_ragged(pts_d, offsets, sizes, box_d)
    assert can.shape == (T, 5) and torch.equal(can[:, 3:], pts_d[:, 3:])
    xyz_r, feat_r = C.stage2_embed(can.view(1, T, 5), None, *packed)
    assert torch.equal(xyz_r.view(T, 3), can[:, :3])
    o = 0
    for i, n in enumerate(sizes):
        xyz_i, feat_i = C.stage2_embed(pts_d[o:o + n].view(1, n, 5).contiguous(), box_d[i:i + 1].contiguous(), *packed)
        assert torch.equal(xyz_i.view(n, 3), xyz_r.view(T, 3)[o:o + n]), i
        assert torch.equal(feat_i, feat_r[o:o + n]), i
        o += n
    z = xyz_r.view(T, 3)
    assert not z[128:193].any() and z[193:].any() and z[:128].any()


# ------------------------------------------------------------------------------------------------ sampling + gather
@pytest.mark.parametrize("m", [128, 32])
def test_fps_ragged_gather_matches_the_oracle_per_cloud(clouds, fps_expected, m):
    from ws3d_amd import pn2_ops
    xyz, offsets, sizes = _packed(clouds)
    xyz_d = torch.from_numpy(xyz).cuda()
    idx, new_xyz = pn2_ops.furthest_point_sample_gather_ragged(xyz_d, torch.from_numpy(offsets).cuda(), m, sizes=sizes)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (len(sizes), m) and tuple(new_xyz.shape) == (len(sizes), m, 3)
    got = idx.cpu().numpy()
    bad = [SIZES[i] for i in range(len(sizes)) if not np.array_equal(got[i], fps_expected[i, :m])]
    assert not bad, "clouds of %s points differ from the oracle" % bad
    # a cloud smaller than m: its distinct points first, then index 0; the all-identical cloud: index 0 throughout
    assert len(set(got[2][:37].tolist())) == min(m, 37) and not got[2][37:].any() and not got[ALL_SAME].any()
    rows = torch.from_numpy(offsets[:-1].astype(np.int64)).cuda()[:, None] + idx.long()
    assert torch.equal(new_xyz, xyz_d[rows])
    # the same answer without the host sizes (offsets read back once)
    idx2, new2 = pn2_ops.furthest_point_sample_gather_ragged(xyz_d, torch.from_numpy(offsets).cuda(), m)
    assert torch.equal(idx2, idx) and torch.equal(new2, new_xyz)


def test_fps_ragged_entries_validate_before_any_launch(clouds):
    """the existing entry still refuses n_i < m; the new one refuses an empty cloud; neither touches idx"""
    from ws3d_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    xyz = torch.from_numpy(clouds[5][:60].copy()).to(dev)
    for entry, sizes, m, want in (("old", [50, 10], 16, _lib.E_INVALID), ("new", [40, 0, 20], 4, _lib.E_INVALID), ("new", [50, 10], 16, 0)):
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
        idx = torch.full((len(sizes), m), -7, dtype=torch.int32, device=dev)
        new_xyz = torch.full((len(sizes), m, 3), -7.0, device=dev)
        host = (ctypes.c_int32 * len(sizes))(*sizes)
        if entry == "old":
            rc = lib.ws3d_furthest_point_sampling_ragged(len(sizes), offsets.data_ptr(), ctypes.cast(host, ctypes.c_void_p), m, xyz.data_ptr(),
                                                         idx.data_ptr(), None)
        else:
            rc = lib.ws3d_furthest_point_sampling_ragged_gather(len(sizes), offsets.data_ptr(), ctypes.cast(host, ctypes.c_void_p), m, xyz.data_ptr(),
                                                                idx.data_ptr(), new_xyz.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == want, (entry, sizes)
        if want:
            assert b"invalid" in lib.ws3d_last_error() and bool((idx == -7).all()) and bool((new_xyz == -7).all())
        else:
            assert bool((idx >= 0).all()) and bool((idx[1] < 10).all())


# ------------------------------------------------------------------------------------------------ ball query
@pytest.mark.parametrize("radius,nsample", [(0.2, 64), (0.4, 16)])
def test_ball_query_ragged_matches_the_oracle_per_cloud(oracle, clouds, fps_expected, radius, nsample):
    """centres = the sampled points (m = 128: clouds below 128 points repeat point 0), the last centre of every cloud moved 50 m away
    (a row without a hit).  Clouds are scaled so that the lists run from over-full to the centre alone: 0.25 x (dense: more than
    nsample hits), 1 x, 6 x (sparse: a centre sees only itself)"""
    from ws3d_amd import pn2_ops
    scale = [0.25, 1.0, 6.0]
    cs = [c * np.float32(scale[i % 3]) for i, c in enumerate(clouds)]
    xyz, offsets, sizes = _packed(cs)
    m = 128
    centres = np.stack([c[fps_expected[i]] for i, c in enumerate(cs)]).astype(np.float32)
    centres[:, m - 1] += np.float32(50.0)
    want = np.stack([oracle.ball_query(radius, nsample, c[None], centres[i][None])[0] for i, c in enumerate(cs)])
    counts = np.stack([(((c[None, :, :] - centres[i][:, None, :]).astype(np.float64) ** 2).sum(-1) < radius * radius).sum(1) for i, c in enumerate(cs)])
    assert (counts[:, :m - 1] > nsample).any() and (counts[:, :m - 1] == 1).any() and ((counts > 1) & (counts < nsample)).any()
    assert not counts[:, m - 1].any() and not want[:, m - 1].any()
    assert (counts[ORIGIN] > nsample).any()                # most of that cloud sits on one point: a centre there fills at once
    xyz_d, off_d, new_d = torch.from_numpy(xyz).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(centres).cuda()
    local = pn2_ops.ball_query_ragged(radius, nsample, xyz_d, off_d, new_d, sizes=sizes)
    glob = pn2_ops.ball_query_ragged(radius, nsample, xyz_d, off_d, new_d, sizes=sizes, global_rows=True)
    torch.cuda.synchronize()
    assert local.dtype == torch.int32 and tuple(local.shape) == (len(sizes), m, nsample)
    got = local.cpu().numpy()
    bad = [SIZES[i] for i in range(len(sizes)) if not np.array_equal(got[i], want[i])]
    assert not bad, "clouds of %s points differ from the oracle" % bad
    assert np.array_equal(glob.cpu().numpy(), want + offsets[:-1, None, None])


def test_ball_query_ragged_tile_tail_and_limits(oracle, clouds):
    """m = 21 is no multiple of the 16 centres of a workgroup; nsample above 64 is refused"""
    from ws3d_amd import _lib, pn2_ops
    cs = [clouds[3], clouds[9], clouds[0]]
    xyz, offsets, sizes = _packed(cs)
    centres = np.stack([np.resize(c, (21, 3)) for c in cs]).astype(np.float32)
    want = np.stack([oracle.ball_query(0.5, 7, c[None], centres[i][None])[0] for i, c in enumerate(cs)])
    got = pn2_ops.ball_query_ragged(0.5, 7, torch.from_numpy(xyz).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(centres).cuda())
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(_lib.Ws3dError, match="rc=%d" % _lib.E_UNSUPPORTED):
        pn2_ops.ball_query_ragged(0.5, 65, torch.from_numpy(xyz).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(centres).cuda())


# ------------------------------------------------------------------------------------------------ the network
def _load_ragged_fixture():
    import json
    import os
    arrays = dict(np.load(os.path.join(ref.GOLDEN, "stage2_ragged.npz")))
    meta = json.load(open(os.path.join(ref.GOLDEN, "stage2_ragged.json")))
    keys = json.load(open(os.path.join(ref.GOLDEN, "stage2_state_dict.json")))["keys"]
    return arrays, meta, keys


@pytest.fixture(scope="module")
def rfx():
    return _load_ragged_fixture()


@pytest.fixture(scope="module")
def net(rfx):
    return ref.fixture_model(rfx[1], rfx[2])          # (the weights of stage2_forward.*: same seed, same scaled layers)


def _packed_inputs(pts, offsets, device="cuda"):
    t = torch.from_numpy(np.ascontiguousarray(pts)).to(device)
    return {"cur_box_point": t[:, 0:3].contiguous(), "cur_box_reflect": t[:, 3:4].contiguous(), "train_mask": t[:, 4:5].contiguous(),
            "offsets": torch.from_numpy(np.asarray(offsets)).to(device)}


def _ragged_parity(net, arrays, pts, offsets, fast, teacher, monkeypatch, expect_chunks=1):
    """one ``rcnn_forward_ragged`` over packed clouds against a fixture's float64 arrays -> (errors per quantity, {name: equal?})"""
    from ws3d_amd import stage2
    calls = []
    real = stage2.fast_forward_ragged
    monkeypatch.setattr(stage2, "fast_forward_ragged", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    monkeypatch.setattr(stage2, "CHANNELS_LAST_FASTPATH", fast)
    data = _packed_inputs(pts, offsets)
    C = len(offsets) - 1
    box_ce = torch.from_numpy(arrays["box_ce"]).float().cuda() if teacher else None
    trace = []
    with torch.no_grad():
        out = net.rcnn_forward_ragged(data, box_ce=box_ce, trace=trace)
    torch.cuda.synchronize()
    assert len(calls) == (expect_chunks if fast else 0)
    err = {k: float(np.abs(out[k].double().cpu().numpy().reshape(arrays[k].shape) - arrays[k]).max()) for k in ref.OUTPUTS}
    err["box_ce"] = float(np.abs(out["box_ce"].double().cpu().numpy() - arrays["box_ce"]).max())
    can = out["canonical_xyz"].cpu().numpy()
    want_can = arrays["can_xyz"].reshape(-1, 3)
    assert can.shape == want_can.shape and out["rcnn_reg"].shape == (C, 52) and out["refined_box"].shape == (C, 1, 7)
    err["can_xyz"] = float(np.abs(can.astype(np.float64) - want_can.astype(np.float64)).max())
    same = {"can_xyz_zero_pattern": bool(np.array_equal(can == 0, want_can == 0))}
    assert len(trace) == len(ref.INDEX_NAMES)
    for (fps_name, bq_name), lvl in zip(ref.INDEX_NAMES, trace):
        same[fps_name] = bool(np.array_equal(lvl["fps"].cpu().numpy(), arrays[fps_name].astype(np.int32)))
        same[bq_name] = bool(np.array_equal(lvl["bq"].cpu().numpy(), arrays[bq_name].astype(np.int32)))
    return err, same, out


def _assert_within(tag, err, same, meta):
    for k in sorted(err):
        print("%-34s %-13s err %.3g  bound %.3g  (e_ref %.3g, max|.| %.3g)" % (tag, k, err[k], 4 * meta["e_ref"][k], meta["e_ref"][k], meta["max_abs"][k]))
    assert all(same.values()), {k: v for k, v in same.items() if not v}
    bad = {k: (v, 4 * meta["e_ref"][k]) for k, v in err.items() if not v <= 4 * meta["e_ref"][k]}
    assert not bad, bad


@pytest.mark.parametrize("fast", [True, False], ids=["ragged_route", "per_cloud_loop"])
@pytest.mark.parametrize("teacher", [True, False], ids=["teacher_forced", "free_running"])
def test_network_matches_the_reference_per_cloud_float64_run(rfx, net, fast, teacher, monkeypatch):
    """clouds of 1 .. 1500 points, two of them real cylinders: every index tensor of both towers and the canonical zero pattern exact,
    all outputs within 4 x e_ref of the reference's float64 run on each cloud alone"""
    a, meta, _ = rfx
    assert np.diff(a["offsets"]).tolist() == meta["sizes"]
    err, same, _ = _ragged_parity(net, a, a["pts"], a["offsets"], fast, teacher, monkeypatch)
    _assert_within("%s %s" % ("ragged_route" if fast else "per_cloud_loop", "teacher_forced" if teacher else "free_running"), err, same, meta)


@pytest.mark.parametrize("teacher", [True, False], ids=["teacher_forced", "free_running"])
def test_equal_sizes_match_the_fixed_size_fixture(net, teacher, monkeypatch):
    """the six 512-point clouds of stage2_forward.* (the sparse one and the all-zero padding cloud included) through the ragged route"""
    a, meta, _ = ref.fixture()
    R, P = a["pts"].shape[0], a["pts"].shape[1]
    err, same, _ = _ragged_parity(net, a, a["pts"].reshape(R * P, 5), np.arange(R + 1, dtype=np.int32) * P, True, teacher, monkeypatch)
    _assert_within("equal sizes %s" % ("teacher_forced" if teacher else "free_running"), err, same, meta)


def test_chunks_of_three_clouds(rfx, net, monkeypatch):
    """the ragged route in passes of 3 + 3 + 2 clouds, and the driver's rcnn_batch = 3 over the same clouds as one scene of 8 slots"""
    from ws3d_amd import detect_kitti, stage2
    a, meta, _ = rfx
    monkeypatch.setattr(stage2, "RAGGED_MAX_CLOUDS", 3)
    err, same, _ = _ragged_parity(net, a, a["pts"], a["offsets"], True, False, monkeypatch, expect_chunks=3)
    _assert_within("chunks of 3", err, same, meta)
    monkeypatch.undo()
    inp = _packed_inputs(a["pts"], a["offsets"].astype(np.int64))
    inp.update({"center": torch.zeros((1, 8, 3), device="cuda"), "num": torch.tensor([8], dtype=torch.int32, device="cuda")})
    full = detect_kitti.rcnn_over_real_clouds_ragged(net, inp, rcnn_batch=3)
    errs = {k: float(np.abs(full[k].double().cpu().numpy().reshape(a[k].shape) - a[k]).max()) for k in detect_kitti.OUT_KEYS}
    print("driver, rcnn_batch 3:", {k: "%.3g (bound %.3g)" % (v, 4 * meta["e_ref"][k]) for k, v in errs.items()})
    assert all(v <= 4 * meta["e_ref"][k] for k, v in errs.items()), errs


def test_driver_ragged_clouds_on_the_synthetic_kitti_tree(rfx, net, tmp_path):
    """``run(clouds="ragged")`` writes one file per scene; the per-slot rows of ``rcnn_over_real_clouds_ragged`` equal ``rcnn_forward`` on
    each cylinder alone (the reference's form) within 4 x e_ref, dropped slots are never kept; the default route is untouched"""
    import dataclasses
    import json
    import os
    from ws3d_amd import detect_kitti, kitti_io, scan_prepare, stage1, stage2, synth
    meta = rfx[1]
    with open(os.path.join(ref.GOLDEN, "kitti_ingest.json")) as f:
        scenes = [tuple(s) for s in json.load(f)["scenes"]]
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, scenes)
    cfg1 = dataclasses.replace(stage1.DEFAULT_CFG, score_thresh=0.1)          # (the seeded Stage-1 heads keep nothing at 0.3)
    cfg2 = dataclasses.replace(stage2.DEFAULT_CFG, ioun_score_thresh=-1e9)
    ckpt = str(tmp_path / "rcnn.pth")
    torch.save({"epoch": 1, "model_state": {"rcnn_net." + k: v for k, v in ref.fixture_state_dict(meta, rfx[2]).items()}}, ckpt)
    files = detect_kitti.run(root, "val", str(tmp_path / "ragged"), batch=2, rcnn_ckpt=ckpt, cfg=cfg1, rcnn_cfg=cfg2, clouds="ragged")
    assert [os.path.basename(f) for f in files] == ["%06d.txt" % s[0] for s in scenes]
    rows = [line.split() for f in files for line in open(f)]
    assert rows and all(len(r) == 16 and r[0] == "Car" for r in rows)

    s1, _ = detect_kitti.load_models(None, ckpt, "cuda:0", cfg1, cfg2)
    ks = kitti_io.KittiScenes(root, "val", npoints=16384, rng=np.random.RandomState(666))
    dataset = scan_prepare.driver_dataset(ks, "off")
    items = [dataset[i] for i in range(2)]
    pts = torch.as_tensor(scan_prepare.batch_points(items, "off", 16384, 666, "cuda:0")).to("cuda:0")
    with torch.no_grad():
        out = s1.rpn_forward({"pts_input": pts})
        inp = stage1.stage2_inputs(out, pts, cfg1, sampled_pt_num=None, ground_y=cfg2.ground_y)
        full = detect_kitti.rcnn_over_real_clouds_ragged(net, inp)
        B, K = inp["center"].shape[:2]
        off, num = inp["offsets"].cpu().numpy(), inp["num"].cpu().numpy()
        cnt = np.diff(off)
        kept = [s for s in range(B * K) if s % K < num[s // K] and cnt[s] > 0]
        dropped = sorted(set(range(B * K)) - set(kept))
        print("driver: %d slots, %d kept, sizes %d .. %d (median %d), %d above 512" % (B * K, len(kept), cnt[kept].min(), cnt[kept].max(),
                                                                                         int(np.median(cnt[kept])), int((cnt[kept] > 512).sum())))
        sample = kept[::max(1, len(kept) // 24)][:24]
        worst = {k: 0.0 for k in detect_kitti.OUT_KEYS}
        for s in sample:
            one = net.rcnn_forward({k: inp[k][off[s]:off[s + 1]].unsqueeze(0).contiguous() for k in ("cur_box_point", "cur_box_reflect", "train_mask")})
            for k in detect_kitti.OUT_KEYS:
                worst[k] = max(worst[k], float((one[k].reshape(-1) - full[k][s]).abs().max()))
        print("ragged rows vs rcnn_forward per cloud:", {k: "%.3g (bound %.3g)" % (v, 4 * meta["e_ref"][k]) for k, v in worst.items()})
        assert all(v <= 4 * meta["e_ref"][k] for k, v in worst.items()), worst
        boxes, scores, count, index = stage2.detections(full, inp["center"], inp["num"], cfg2, return_index=True)
        chosen = set((b * K + int(k)) for b in range(B) for k in index[b].tolist() if k >= 0)
        assert chosen and not chosen & set(dropped)
        # the default route: what detect_batch computed before the switch existed
        got = detect_kitti.detect_batch(s1, net, pts, cfg1, cfg2)
        fixed = stage1.stage2_inputs(out, pts, cfg1, sampled_pt_num=cfg1.roi_sampled_pts, ground_y=cfg2.ground_y)
        want = stage2.detections(detect_kitti.rcnn_over_real_slots(net, fixed, 800), fixed["center"], fixed["num"], cfg2)
        explicit = detect_kitti.detect_batch(s1, net, pts, cfg1, cfg2, clouds="fixed")
        assert all(torch.equal(g, w) and torch.equal(g, e) for g, w, e in zip(got, want, explicit))
