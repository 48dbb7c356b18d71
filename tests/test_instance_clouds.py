"""Stage-2 instance clouds (csrc/instance_clouds.hip, ws3d_amd.instance_ops, stage1.stage2_inputs).

CPU part: the C ABI (symbols, argument errors, zero-sized calls) and the kernels' resources.  GPU part: the fixed and the
ragged form against the reference's few lines of selection (generate_box_dataset.py:197-229, tools/eval_auto.py:286-292,
323-372, kitti_boxplace_dataset.py:327-337) restated here in torch / NumPy.  Every comparison is assert_array_equal: each
output is a copy or one correctly rounded subtraction."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ws3d_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws3d_instance_clouds", "ws3d_instance_clouds_count", "ws3d_instance_clouds_emit")


# ----------------------------------------------------------------------------- CPU: ABI
def test_new_entries_are_exported_and_bound():
    from ws3d_amd import _lib, build
    raw = ctypes.CDLL(build.build())
    hdr = open(os.path.join(ROOT, "include", "ws3d_ops.h")).read()
    for name in NEW:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"WS3D_API int %s\(" % name, hdr), name
    assert _lib.load().ws3d_abi_version() == 6
    assert "instance_clouds.hip" in build.SOURCES


def test_new_entries_reject_bad_arguments_and_accept_empty_calls():
    from ws3d_amd import _lib
    lib = _lib.load()
    n = None

    def fixed(B=1, N=16, K=2, C=0, S=8, radius=4.0, mode=0, ptrs=(n,) * 9):
        return lib.ws3d_instance_clouds(B, N, K, C, S, radius, mode, 0.5, *ptrs, None)

    def count(B=1, N=16, K=2, radius=4.0):
        return lib.ws3d_instance_clouds_count(B, N, K, radius, n, n, n, n, None)

    def emit(B=1, N=16, K=2, C=0, radius=4.0, mode=0):
        return lib.ws3d_instance_clouds_emit(B, N, K, C, radius, mode, 0.5, n, n, n, n, n, n, n, n, n, None)

    bad = [fixed(B=-1), fixed(N=-1), fixed(K=-1), fixed(C=-4), fixed(C=6), fixed(S=0), fixed(S=-3), fixed(radius=0.0), fixed(radius=-1.0),
           fixed(radius=float("inf")), fixed(radius=float("nan")), fixed(mode=2), fixed(mode=-1), fixed(),      # fixed(): required pointers NULL
           count(B=-1), count(N=-2), count(K=-1), count(radius=0.0), count(radius=float("nan")), count(),
           emit(B=-1), emit(N=-1), emit(K=-1), emit(C=2), emit(radius=float("inf")), emit(radius=-2.0), emit(mode=3), emit()]
    for i, rc in enumerate(bad):
        assert rc != 0, i
    assert fixed(S=0) == _lib.E_INVALID and b"invalid" in lib.ws3d_last_error()
    assert fixed() == _lib.E_INVALID and b"NULL" in lib.ws3d_last_error()
    assert emit(C=2) == _lib.E_INVALID and b"multiple of 4" in lib.ws3d_last_error()
    # nothing to do: succeeds without a device
    assert fixed(B=0) == 0 and fixed(K=0) == 0
    assert count(B=0) == 0 and count(K=0) == 0 and count(N=0) == 0
    assert emit(B=0) == 0 and emit(K=0) == 0 and emit(N=0) == 0


def test_cpu_tensors_raise():
    from ws3d_amd import instance_ops
    from ws3d_amd._lib import Ws3dError
    with pytest.raises(Ws3dError):
        instance_ops.instance_clouds(torch.zeros(1, 8, 4), torch.zeros(1, 8), torch.zeros(1, 2, 3), sampled_pt_num=4)


# ----------------------------------------------------------------------------- CPU: resources
def test_instance_cloud_kernels_have_no_spills_and_no_scratch(tmp_path):
    from ws3d_amd import build
    src = os.path.join(ROOT, "ws3d_amd", "csrc", "instance_clouds.hip")
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "instance_clouds.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    report = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
        if m and name:
            report[name][m.group(1).strip()] = m.group(2)
    kernels = [k for k in report if "instance_clouds" in k and "kernel" in k]
    assert len(kernels) == 3 and len(report) == 3, sorted(report)
    for k, v in report.items():
        assert v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0", (k, v)
        assert v["ScratchSize [bytes/lane]"] == "0", (k, v)


# ----------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ref_flags(pts, centres):
    """lib/utils/distance.py:3 distance_2(centres_xz, points_xz) < radius is applied by the caller: (N, K) distances of one scene,
    on the device, exactly as generate_box_dataset.py:200 / eval_auto.py:324 compute them"""
    a, b = centres[:, [0, 2]], pts[:, [0, 2]]
    return torch.sqrt(torch.sum((a[None, :] - b[:, None]) ** 2, dim=2))


def ref_members(pts, centres, num, radius):
    """per scene and centre slot: the member point indices in scene order (boolean-mask order); empty for slots >= num[b]"""
    B, K = centres.shape[0], centres.shape[1]
    members = []
    for b in range(B):
        flag = host(ref_flags(pts[b], centres[b]) < radius)                # (N, K)
        members.append([np.flatnonzero(flag[:, k]) if k < num[b] else np.zeros(0, dtype=np.int64) for k in range(K)])
    return members


def ref_rows(pts_b, score_b, centre, idx, mask_mode, thresh=0.5):
    """generate_box_dataset.py:220-227 (mask_mode 0) / eval_auto.py:341-345, 367 (mask_mode 1) for one centre, NumPy float32"""
    xyz = pts_b[idx, :3] - centre.reshape(1, 3)
    refl = pts_b[idx, 3:4]
    s = score_b[idx].reshape(-1, 1)
    m = s if mask_mode == 0 else (s > np.float32(thresh)).astype(np.float32) - np.float32(0.5)
    return np.concatenate((xyz, refl, m), axis=1).astype(np.float32)


def cyclic(idx, S):
    """kitti_boxplace_dataset.py:327-337: the first S rows, shorter clouds repeated cyclically"""
    t = min(len(idx), S)
    return idx[:t][np.arange(S) % t]


def make_case(kind, B, N, K, seed, C=0):
    pc = synth.make_batch(kind, B, N, seed)
    rng = np.random.default_rng(seed)
    score = rng.uniform(0, 1, (B, N)).astype(np.float32)
    feats = rng.standard_normal((B, N, C)).astype(np.float32) if C else None
    centres = np.zeros((B, K, 3), dtype=np.float32)
    for b in range(B):
        pick = rng.integers(0, N, K)
        centres[b, :, 0] = pc[b, pick, 0] + rng.normal(0, 1.0, K).astype(np.float32)
        centres[b, :, 2] = pc[b, pick, 2] + rng.normal(0, 1.0, K).astype(np.float32)
    return pc, score, feats, centres


def check_fixed(pc, score, feats, centres, num, S, mask_mode, members, radius=4.0):
    from ws3d_amd import instance_ops
    B, K = centres.shape[0], centres.shape[1]
    cloud, cfeat, count, pidx = instance_ops.instance_clouds(
        dev(pc), dev(score), dev(centres), None if num is None else dev(np.asarray(num, dtype=np.int32)), radius=radius, sampled_pt_num=S,
        mask_mode=mask_mode, features=None if feats is None else dev(feats), return_idx=True)
    assert tuple(cloud.shape) == (B, K, S, 5) and count.dtype == torch.int32 and pidx.dtype == torch.int32
    cloud, count, pidx = host(cloud), host(count), host(pidx)
    cfeat = host(cfeat) if feats is not None else None
    exp_cloud = np.zeros((B, K, S, 5), dtype=np.float32)
    exp_idx = np.zeros((B, K, S), dtype=np.int32)
    exp_count = np.zeros((B, K), dtype=np.int32)
    exp_feat = np.zeros((B, K, S, feats.shape[2]), dtype=np.float32) if feats is not None else None
    for b in range(B):
        for k in range(K):
            idx = members[b][k]
            exp_count[b, k] = len(idx)
            if len(idx) == 0:
                continue
            sel = cyclic(idx, S)
            exp_idx[b, k] = sel
            exp_cloud[b, k] = ref_rows(pc[b], score[b], centres[b, k], sel, mask_mode)
            if feats is not None:
                exp_feat[b, k] = feats[b][sel]
    np.testing.assert_array_equal(count, exp_count)
    np.testing.assert_array_equal(pidx, exp_idx)
    np.testing.assert_array_equal(cloud, exp_cloud)
    if feats is not None:
        np.testing.assert_array_equal(cfeat, exp_feat)
    return count


@gpu
@pytest.mark.parametrize("S", [512, 100])
@pytest.mark.parametrize("C", [0, 128])
@pytest.mark.parametrize("kind", ["hdl64", "lidar"])
def test_fixed_form_matches_reference_selection(kind, C, S):
    B, N, K = 3, 16384, 200
    pc, score, feats, centres = make_case(kind, B, N, K, 77, C)
    centres[0, 5, 0] = 1000.0                                        # an empty cylinder
    num = (K, K - 7, 0)
    for cy in (0.0, 1.65):
        centres[:, :, 1] = cy
        members = ref_members(dev(pc), dev(centres), num, 4.0)
        for mask_mode in (0, 1):
            count = check_fixed(pc, score, feats, centres, num, S, mask_mode, members)
    live = count[0]
    assert (live > S).any() and ((live > 0) & (live < S)).any() and live[5] == 0   # the test's own coverage
    assert num[1] < K and num[2] == 0 and (count[1, num[1]:] == 0).all() and (count[2] == 0).all()


@gpu
@pytest.mark.parametrize("C", [0, 128])
@pytest.mark.parametrize("kind", ["hdl64", "lidar"])
def test_ragged_form_matches_reference_selection(kind, C):
    from ws3d_amd import instance_ops
    B, N, K = 3, 16384, 200
    pc, score, feats, centres = make_case(kind, B, N, K, 77, C)
    centres[0, 5, 0] = 1000.0
    centres[:, :, 1] = 1.65
    num = np.array((K, K - 7, 0), dtype=np.int32)
    members = ref_members(dev(pc), dev(centres), num, 4.0)
    fixed_count = host(instance_ops.instance_clouds(dev(pc), dev(score), dev(centres), dev(num), sampled_pt_num=64)[2])
    for mask_mode in (0, 1):
        rows, rfeat, offsets, count, ridx = instance_ops.instance_clouds_ragged(
            dev(pc), dev(score), dev(centres), dev(num), mask_mode=mask_mode, features=None if feats is None else dev(feats), return_idx=True)
        assert offsets.dtype == torch.int64 and tuple(offsets.shape) == (B * K + 1,) and ridx.dtype == torch.int32
        count, offsets = host(count), host(offsets)
        np.testing.assert_array_equal(count, fixed_count)
        np.testing.assert_array_equal(offsets, np.concatenate(([0], np.cumsum(count.reshape(-1).astype(np.int64)))))
        exp_idx = np.concatenate([members[b][k] for b in range(B) for k in range(K)])
        exp_rows = np.concatenate([ref_rows(pc[b], score[b], centres[b, k], members[b][k], mask_mode) for b in range(B) for k in range(K)])
        assert rows.shape[0] == offsets[-1] == len(exp_idx) > 0
        np.testing.assert_array_equal(host(ridx), exp_idx.astype(np.int32))
        np.testing.assert_array_equal(host(rows), exp_rows)
        if feats is not None:
            exp_feat = np.concatenate([feats[b][members[b][k]] for b in range(B) for k in range(K)])
            np.testing.assert_array_equal(host(rfeat), exp_feat)
        else:
            assert rfeat is None


@gpu
@pytest.mark.parametrize("N,K", [(1, 3), (63, 65), (3000, 1), (3000, 65)])
def test_edges_sizes_not_multiples_of_64(N, K):
    from ws3d_amd import instance_ops
    B = 2
    pc, score, feats, centres = make_case("lidar", B, N, K, 5, 8)
    members = ref_members(dev(pc), dev(centres), (K, K), 4.0)
    for S in (16, 512):
        check_fixed(pc, score, feats, centres, None, S, 1, members)
    rows, rfeat, offsets, count, ridx = instance_ops.instance_clouds_ragged(dev(pc), dev(score), dev(centres), features=dev(feats), return_idx=True)
    exp_idx = np.concatenate([members[b][k] for b in range(B) for k in range(K)])
    np.testing.assert_array_equal(host(ridx), exp_idx.astype(np.int32))
    np.testing.assert_array_equal(host(rows), np.concatenate([ref_rows(pc[b], score[b], centres[b, k], members[b][k], 0)
                                                              for b in range(B) for k in range(K)]))
    np.testing.assert_array_equal(host(rfeat), np.concatenate([feats[b][members[b][k]] for b in range(B) for k in range(K)]))


@gpu
def test_edges_nan_points_identical_centres_poisoned_outputs():
    from ws3d_amd import compat, instance_ops
    B, N, K, S, C = 2, 3000, 20, 128, 8
    pc, score, feats, centres = make_case("lidar", B, N, K, 9, C)
    pc[0, 10:40, 0] = np.nan                         # NaN coordinates: those points belong to no cloud
    pc[1, 100:120, 2] = np.nan
    centres[0, 7] = centres[0, 3]                    # two identical centres
    centres[1, 2, 0] = 1000.0                        # an empty cylinder
    num = np.array((K, K - 3), dtype=np.int32)
    members = ref_members(dev(pc), dev(centres), num, 4.0)
    allm = np.concatenate([m for mb in members for m in mb])
    assert len(allm) and not np.isnan(pc[0][np.concatenate(members[0])][:, [0, 2]]).any() and not np.isin(np.arange(10, 40), np.concatenate(members[0])).any()
    check_fixed(pc, score, feats, centres, num, S, 0, members)
    # every element is written: NaN-poisoned outputs come back clean
    cloud = torch.full((B, K, S, 5), float("nan"), device="cuda")
    cfeat = torch.full((B, K, S, C), float("nan"), device="cuda")
    count = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    pidx = torch.full((B, K, S), -7, dtype=torch.int32, device="cuda")
    pc_ok = np.nan_to_num(pc, nan=500.0)
    compat.instance_clouds_forward(dev(pc_ok), dev(score), dev(feats), dev(centres), dev(num), 4.0, 1, 0.5, cloud, cfeat, count, pidx)
    assert not torch.isnan(cloud).any() and not torch.isnan(cfeat).any() and (count >= 0).all() and (pidx >= 0).all()
    np.testing.assert_array_equal(host(cloud[0, 7]), host(cloud[0, 3]))
    np.testing.assert_array_equal(host(cfeat[0, 7]), host(cfeat[0, 3]))
    assert int(count[0, 3]) > 0 and int(count[1, 2]) == 0 and not cloud[1, 2].any() and not cloud[1, K - 3:].any() and not cfeat[1, K - 3:].any()
    # the ragged form drops the NaN points too
    rows, _, offsets, rcount, ridx = instance_ops.instance_clouds_ragged(dev(pc), dev(score), dev(centres), dev(num), return_idx=True)
    np.testing.assert_array_equal(host(ridx), allm.astype(np.int32))


@gpu
def test_fixed_form_under_graph_capture():
    from ws3d_amd import instance_ops
    B, N, K, S, C = 2, 3000, 33, 64, 8
    pc, score, feats, centres = make_case("lidar", B, N, K, 11, C)
    num = np.array((K, 5), dtype=np.int32)
    st = [dev(pc), dev(score), dev(centres), dev(num), dev(feats)]

    def call():
        return instance_ops.instance_clouds(st[0], st[1], st[2], st[3], sampled_pt_num=S, mask_mode=1, features=st[4], return_idx=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = call()
    pc2, score2, feats2, centres2 = make_case("lidar", B, N, K, 12, C)      # fresh inputs
    for t, a in zip(st, (pc2, score2, centres2, np.array((7, K), dtype=np.int32), feats2)):
        t.copy_(dev(a))
    g.replay()
    torch.cuda.synchronize()
    got = [host(o) for o in outs]
    eager = [host(o) for o in call()]
    for a, b in zip(got, eager):
        np.testing.assert_array_equal(a, b)
    assert got[2][0, 7:].max() == 0 and got[2].max() > 0


@gpu
@pytest.mark.parametrize("S", [None, 512, 32])
def test_stage2_inputs_match_eval_auto_restated(S):
    """stage1.stage2_inputs == tools/eval_auto.py:286-292, 323-372 restated literally (any-centre prefilter, y -= 1.65, per-centre
    mask, (score > 0.5) - 0.5), centres from center_proposals on the seeded random heads of
    test_gpu_parity.py::test_center_proposal_stage_matches_reference_loop, two scenes"""
    from ws3d_amd import stage1
    rng = np.random.default_rng(3)
    B, N, C = 2, 3000, 8
    pc = synth.make_batch("lidar", B, N, 77)
    pts_input = dev(pc)
    out = {"backbone_xyz": dev(pc[:, :, :3].copy()),
           "rpn_reg": dev(rng.standard_normal((B, N, 40)).astype(np.float32)),
           "rpn_cls": dev(rng.normal(-0.5, 1.5, (B, N, 1)).astype(np.float32)),
           "backbone_features": dev(rng.standard_normal((B, C, N)).astype(np.float32))}
    res = stage1.stage2_inputs(out, pts_input, sampled_pt_num=S, with_features=True)
    K = res["center"].shape[1]
    num = host(res["num"])
    assert res["num"].dtype == torch.int32 and tuple(res["count"].shape) == (B, K) and tuple(res["center_score"].shape) == (B, K)
    dist2 = lambda a, b: torch.sqrt(torch.sum((a[None, :] - b[:, None]) ** 2, dim=2))   # noqa: E731  lib/utils/distance.py:3
    for b in range(B):
        one = {k: v[b] for k, v in out.items() if k != "backbone_features"}
        ctr, norm, _ = stage1.center_proposals(one)
        assert ctr.shape[0] == num[b] > 10
        np.testing.assert_array_equal(host(res["center"][b, :num[b], [0, 2]]), host(ctr[:, [0, 2]]))
        assert (host(res["center"][b, :, 1]) == np.float32(1.65)).all()
        np.testing.assert_array_equal(host(res["center_score"][b, :num[b]]), host(norm))
        # ---- eval_auto.py:286-292
        inputs = pts_input[b].clone()
        feats = out["backbone_features"][b].t().clone()
        rcnn_input_scores = torch.sigmoid(out["rpn_cls"][b]).view(-1)
        rpn_center = ctr[:, [0, 2]]
        point_center_distance = dist2(rpn_center, inputs[:, [0, 2]])
        cur_proposal_points_index = torch.min(point_center_distance, dim=-1)[0] < 4.0
        inputs = inputs[cur_proposal_points_index]
        feats = feats[cur_proposal_points_index]
        rcnn_input_scores = rcnn_input_scores.view(-1)[cur_proposal_points_index]
        # ---- eval_auto.py:323-372
        inputs[:, 1] -= 1.65
        point_center_distance = dist2(rpn_center[:, :], inputs[:, [0, 2]])
        for c in range(rpn_center.shape[0]):
            cur_input = inputs.clone()
            cur_input_score = rcnn_input_scores.clone()
            cur_center_points_index = (point_center_distance[:, c] < 4.0).view(-1)
            n = int(cur_center_points_index.long().sum())
            assert int(res["count"][b, c]) == n
            if n == 0:
                continue
            cur_center_points_xyz = cur_input[cur_center_points_index, :3]
            cur_center_points_xyz[:, 0] -= rpn_center[c, 0]
            cur_center_points_xyz[:, 2] -= rpn_center[c, 1]
            cur_center_points_r = cur_input[cur_center_points_index, 3].view(-1, 1)
            cur_center_points_mask = (cur_input_score[cur_center_points_index] > 0.5).view(-1, 1).float()
            cur_center_points_mask = cur_center_points_mask.float() - 0.5
            cur_feat = feats[cur_center_points_index]
            if S is None:
                lo, hi = int(res["offsets"][b * K + c]), int(res["offsets"][b * K + c + 1])
                got = [res[k][lo:hi] for k in ("cur_box_point", "cur_box_reflect", "train_mask", "cur_pts_feature")]
                sel = np.arange(n)
            else:
                got = [res[k][b, c] for k in ("cur_box_point", "cur_box_reflect", "train_mask", "cur_pts_feature")]
                sel = cyclic(np.arange(n), S)
            for g, e in zip(got, (cur_center_points_xyz, cur_center_points_r, cur_center_points_mask, cur_feat)):
                np.testing.assert_array_equal(host(g), host(e)[sel])
        if S is not None:
            assert not res["cur_box_point"][b, num[b]:].any() and not res["train_mask"][b, num[b]:].any()
    if S == 32:
        assert int(res["count"].max()) > 32          # the truncating branch ran
