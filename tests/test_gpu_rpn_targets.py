"""The Stage-1 targets and loss from the device (csrc/rpn_targets.hip): ``ws3d_rpn_center_labels`` against
``losses.gaussian_center_labels``, ``ws3d_rpn_loss`` against ``losses.rpn_loss`` run on the CPU in float64 on the same fp32 inputs and
against the reference's own model_fn (tests/golden/train_losses.json), and one training step on both loss routes."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = 2.0 ** -22, 1e-37      # one fp32 rounding of a float64 result, doubled; the absolute term covers fp32 underflow only
CONFIGS = {"default": (4.0, 0.8), "fine": (3.0, 0.5)}


# --------------------------------------------------------------------------- labels
def _label_batch(n):
    """three synth scenes with 70, 0 and 1 centres (70 = more than one LDS chunk of 64, the empty scene in the middle).  The scene with
    the lone centre has points placed on the denormal ring (16.0 .. 18.6 m in 0.05 m steps: labels from ~1e-32 through the fp32
    denormals to an exact 0) and across the `close` edge (3.99 .. 4.01 m), at height 0 so that the planar distance is the distance."""
    from ws3d_amd import synth
    rng = np.random.default_rng(n)
    counts = np.array([70, 0, 1], dtype=np.int32)
    pts = np.stack([synth.lidar_cloud(n, 500 + n + b) for b in range(3)]).astype(np.float32)
    centres = rng.uniform(-30, 30, (3, 70, 3)).astype(np.float32)          # padding that would change every label if it were read
    centres[0, :, [0, 2]] = pts[0, rng.integers(0, n, 70)][:, [0, 2]].T + rng.normal(0, 1.5, (2, 70)).astype(np.float32)
    lone = np.array([3.25, 1.0, 31.5], dtype=np.float32)
    centres[2, 0] = lone
    radii = np.concatenate([np.arange(16.0, 18.6001, 0.05), np.arange(3.99, 4.0101, 0.002)])
    assert radii.size == 53 + 11 <= n
    ang = rng.uniform(0, 2 * np.pi, radii.size)
    pts[2, :radii.size, 0] = (lone[0] + radii * np.cos(ang)).astype(np.float32)
    pts[2, :radii.size, 1] = 0.0
    pts[2, :radii.size, 2] = (lone[2] + radii * np.sin(ang)).astype(np.float32)
    return pts, centres, counts, radii.size


@pytest.mark.parametrize("n", [70, 1000, 4096])
def test_center_labels_match_numpy(n):
    from ws3d_amd import compat as _C, losses
    pts, centres, counts, placed = _label_batch(n)
    want = [losses.gaussian_center_labels(pts[b, :, :3], centres[b, :counts[b]]) for b in range(3)]
    want_cls = np.stack([np.asarray(w[0]).astype(np.float32) for w in want])
    want_reg = np.stack([w[1] for w in want])
    d_pts, d_centres, d_counts = (torch.from_numpy(a).cuda() for a in (pts, centres, counts))
    cls, reg = losses.center_labels_batch(d_pts, d_centres, d_counts)
    out = (torch.full((3, n), 7.0, device="cuda"), torch.full((3, n, 3), 7.0, device="cuda"))
    _C.rpn_center_labels(d_pts, d_centres, d_counts, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[0], cls) and torch.equal(out[1], reg)
    cls, reg = cls.cpu().numpy(), reg.cpu().numpy()
    tiny = np.finfo(np.float32).tiny
    ring = want_cls[2, :placed]
    print("n", n, "fg", int((want_cls > 0).sum()), "denormal labels", int(((want_cls > 0) & (want_cls < tiny)).sum()), "close", int((want_reg[..., 0] != 0).sum()),
          "ring: normal / denormal / zero", int((ring >= tiny).sum()), int(((ring > 0) & (ring < tiny)).sum()), int((ring == 0).sum()))
    # the placed points do what they were placed for
    assert ((ring > 0) & (ring < tiny)).sum() >= 5 and (ring == 0).sum() >= 2 and (ring >= tiny).sum() >= 10
    edge = want_reg[2, placed - 11:placed]
    assert (edge[:, [0, 2]] != 0).any(axis=1).sum() in range(2, 10)             # both sides of d < 4
    assert not want_cls[1].any() and not want_reg[1].any() and (want_reg[0, :, 0] != 0).any()
    assert np.array_equal(reg.view(np.int32), want_reg.view(np.int32))          # bit-identical, the sign of a zero included
    assert np.array_equal(cls > 0, want_cls > 0)
    ulps = np.abs(cls.view(np.int32).astype(np.int64) - want_cls.view(np.int32).astype(np.int64))       # labels are >= 0: the bits are ordered
    print("cls_label: max distance in fp32 units", int(ulps.max()), "elements that differ", int((ulps != 0).sum()))
    assert ulps.max() <= 1


# --------------------------------------------------------------------------- loss
def _loss_inputs(rows, config, kind, seed=0):
    """fp32 numpy inputs of one case.  kinds: 'mixed' (about a third foreground, labels from denormal to 1), 'no_centres' (every label 0),
    'all_fg' (every row foreground), 'last_block' (the only foreground rows are the last 40: in the ragged tail where there is one).
    Logits include +-30 and +-100; offsets reach +-3.9 (both clamp ends at loc_scope 3.0) and most foreground rows have offset 0."""
    loc_scope, bin_size = CONFIGS[config]
    bins = int((loc_scope + 1e-3) / bin_size) * 2
    rng = np.random.default_rng(1000 * rows + 10 * sorted(CONFIGS).index(config) + seed)
    soft = np.exp(-rng.uniform(0, 110, rows)).astype(np.float32)                # down to the fp32 denormals (e^-104 = 6.8e-46 rounds to one)
    soft[rng.random(rows) < 0.1] = 1.0
    if kind == "mixed":
        label = np.where(rng.random(rows) < 0.35, soft, 0).astype(np.float32)
    elif kind == "no_centres":
        label = np.zeros(rows, dtype=np.float32)
    elif kind == "all_fg":
        label = np.maximum(soft, np.float32(1e-45))
    else:
        label = np.zeros(rows, dtype=np.float32)
        label[-40:] = np.maximum(soft[-40:], np.float32(1e-45))
    offsets = np.where(rng.random((rows, 3)) < 0.4, rng.uniform(-3.9, 3.9, (rows, 3)), 0).astype(np.float32)
    offsets[:, 1] = 0
    offsets[-3:, 0], offsets[-3:, 2] = (3.9, -3.9, 0.0), (-3.9, 3.9, 3.9)
    logits = rng.normal(-2.0, 3.0, rows).astype(np.float32)
    special = np.array([30, -30, 100, -100, 0.0, 30, -30, 100, -100], dtype=np.float32)
    logits[:9] = special                    # on whatever labels the head of the case holds ...
    logits[-9:] = special                   # ... and on its tail (foreground rows in every kind but 'no_centres')
    reg = rng.normal(0, 2.0, (rows, 4 * bins)).astype(np.float32)
    return logits, reg, label, offsets, loc_scope, bin_size


_REFERENCE = {}


def _reference(rows, config, kind):
    """losses.rpn_loss on the CPU in float64 on the fp32 inputs, computed once per case: (inputs, loss, tb, parts, grad_cls, grad_reg)"""
    key = (rows, config, kind)
    if key not in _REFERENCE:
        from ws3d_amd import losses
        logits, reg, label, offsets, loc_scope, bin_size = _loss_inputs(rows, config, kind)
        t_cls = torch.from_numpy(logits).double().reshape(1, rows, 1).requires_grad_(True)
        t_reg = torch.from_numpy(reg).double().reshape(1, rows, -1).requires_grad_(True)
        d_label, d_off = torch.from_numpy(label).double().reshape(1, rows), torch.from_numpy(offsets).double().reshape(1, rows, 3)
        loss, tb = losses.rpn_loss(t_cls, t_reg, d_label, d_off, loc_scope, bin_size)
        loss.backward()
        fg = label > 0
        parts = dict.fromkeys(("loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res"), 0.0)
        if fg.any():
            parts = losses.rpn_reg_loss(t_reg.detach()[0][torch.from_numpy(fg)], d_off[0][torch.from_numpy(fg)], loc_scope, bin_size)[1]
        g_reg = np.zeros((rows, reg.shape[1])) if t_reg.grad is None else t_reg.grad.numpy().reshape(rows, -1)
        _REFERENCE[key] = ((logits, reg, label, offsets, loc_scope, bin_size), loss.item(), tb, parts, t_cls.grad.numpy().reshape(-1), g_reg)
    return _REFERENCE[key]


def _close(got, want):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    err = np.abs(got - want)
    normal = np.abs(want) >= np.finfo(np.float32).tiny          # (below: fp32 denormals and underflow, the absolute term's ground)
    worst = float((err[normal] / np.abs(want[normal])).max()) if normal.any() else 0.0
    return bool((err <= ATOL + RTOL * np.abs(want)).all()), worst


@pytest.mark.parametrize("kind", ["mixed", "no_centres", "all_fg", "last_block"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("rows", [70, 2 * 1000, 2 * 4096])
def test_fused_loss_matches_the_float64_run(rows, config, kind):
    from ws3d_amd import compat as _C, losses
    (logits, reg, label, offsets, loc_scope, bin_size), want_loss, want_tb, want_parts, want_gcls, want_greg = _reference(rows, config, kind)
    t_cls = torch.from_numpy(logits).cuda().reshape(1, rows, 1).requires_grad_(True)
    t_reg = torch.from_numpy(reg).cuda().reshape(1, rows, -1).requires_grad_(True)
    d_label, d_off = torch.from_numpy(label).cuda().reshape(1, rows), torch.from_numpy(offsets).cuda().reshape(1, rows, 3)
    loss, tb = losses.rpn_loss_fused(t_cls, t_reg, d_label, d_off, loc_scope, bin_size)
    assert type(loss.grad_fn).__name__.startswith("_RpnLossFn") and all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 for v in tb.values())
    loss.backward()
    vals = _C.rpn_loss(t_cls.detach().reshape(rows), t_reg.detach().reshape(rows, -1), d_label.reshape(rows), d_off.reshape(rows, 3), loc_scope, bin_size)[0]
    torch.cuda.synchronize()
    fg_sum = int(tb["rpn_fg_sum"])
    got = losses.resolve_scalars(dict(tb))
    bad = []

    def check(name, g, w):
        ok, worst = _close(g, w)
        print("%5d %-8s %-11s %-18s worst relative error among fp32-normal values %.3g (bound %.3g)" % (rows, config, kind, name, worst, RTOL))
        if not ok:
            bad.append((name, worst))

    check("loss", float(loss.detach()), want_loss)
    for k in ("rpn_loss", "rpn_loss_cls", "rpn_loss_reg", "rpn_loss_cls_pos", "rpn_loss_cls_neg"):
        check(k, got[k], want_tb[k])
    for i, k in enumerate(("loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res")):
        check(k, float(vals[5 + i]), want_parts[k])
    check("grad_cls", t_cls.grad.cpu().numpy().reshape(-1), want_gcls)
    check("grad_reg", t_reg.grad.cpu().numpy().reshape(rows, -1), want_greg)
    assert not bad, bad
    assert fg_sum == want_tb["rpn_fg_sum"] == int((label > 0).sum()) and float(loss.detach()) == got["rpn_loss"]
    if kind == "no_centres":
        assert got["rpn_loss_reg"] == 0.0 and not t_reg.grad.any()
    if kind == "all_fg":
        assert fg_sum == rows
    if kind == "last_block":
        assert fg_sum == min(rows, 40) and not t_reg.grad[0, :max(rows - 40, 0)].any()


@pytest.mark.parametrize("rows", [70, 2 * 1000, 2 * 4096])
def test_repeated_calls_on_one_workspace_and_into_views_are_bit_identical(rows):
    from ws3d_amd import _lib, compat as _C
    logits, reg, label, offsets, loc_scope, bin_size = _loss_inputs(rows, "default", "mixed")
    args = [torch.from_numpy(a).cuda() for a in (logits, reg, label, offsets)]
    width = reg.shape[1]
    first = _C.rpn_loss(*args, loc_scope, bin_size)
    ws = torch.empty((_lib.load().ws3d_rpn_loss_workspace_bytes(rows) + 64,), dtype=torch.uint8, device="cuda")
    slab = torch.full((16 + 4 + rows + 4 + rows * width + 8,), float("nan"), device="cuda")          # views into one buffer, 16-byte aligned
    views = (slab[0:9], torch.empty((1,), dtype=torch.int32, device="cuda"), slab[16:16 + rows], slab[16 + rows + (-rows) % 4:][:rows * width].view(rows, width))
    runs = []
    for _ in range(3):
        out = _C.rpn_loss(*args, loc_scope, bin_size, out=views, workspace=ws)
        assert all(o.data_ptr() == v.data_ptr() for o, v in zip(out, views))
        runs.append([o.clone() for o in out])
        other = _C.rpn_loss(*[a[:rows // 2].contiguous() for a in args], loc_scope, bin_size, workspace=ws)      # another problem through the same workspace
    torch.cuda.synchronize()
    assert not torch.equal(other[0], first[0])
    for run in runs:
        assert all(torch.equal(a, b) for a, b in zip(run, first))
    assert bool(torch.isnan(slab[9:16]).all()) and bool(torch.isnan(slab[-8:]).all())           # nothing written beside the views


def test_no_rows_gives_zeros():
    from ws3d_amd import compat as _C
    e = [torch.zeros(s, device="cuda") for s in ((0,), (0, 40), (0,), (0, 3))]
    vals, counts, g_cls, g_reg = _C.rpn_loss(*e, 4.0, 0.8)
    assert not vals.any() and int(counts[0]) == 0 and g_cls.shape == (0,) and g_reg.shape == (0, 40)


@pytest.mark.parametrize("name", ["two_scenes", "no_centres"])
def test_fused_route_matches_the_reference_model_fn(name):
    """the cases of tests/golden/train_losses.json (the reference's label generator and model_fn), labels and loss both from the device,
    at the tolerances tests/test_train.py holds the host route to"""
    from tests.test_train import _inputs
    from ws3d_amd import losses
    with open(os.path.join(HERE, "golden", "train_losses.json")) as f:
        ref = json.load(f)["cases"][name]
    pc, centres, rpn_cls, rpn_reg = _inputs(ref["case"])
    B, cars = pc.shape[0], ref["case"]["cars"]
    padded = np.full((B, max(cars, 1), 3), 5.0, dtype=np.float32)
    for b in range(B):
        padded[b, :cars] = centres[b]
    cls_label, reg_label = losses.center_labels_batch(torch.from_numpy(pc).cuda(), torch.from_numpy(padded).cuda(),
                                                      torch.full((B,), cars, dtype=torch.int32, device="cuda"))
    flat = cls_label.cpu().numpy().reshape(-1)
    want = np.asarray(ref["cls_label"]["val"], dtype=np.float64).astype(np.float32)
    assert np.abs(flat[np.array(ref["cls_label"]["pos"])].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 1
    assert int((flat > 0).sum()) == int(ref["tb"]["rpn_fg_sum"])       # (the fixture's cls_label.fg counts the float64 labels: no underflow there)
    assert hashlib.sha256(np.ascontiguousarray(reg_label.cpu().numpy()).tobytes()).hexdigest() == ref["reg_label"]["sha256"]

    t_cls = torch.from_numpy(rpn_cls).cuda().requires_grad_(True)
    t_reg = torch.from_numpy(rpn_reg).cuda().requires_grad_(True)
    loss, tb = losses.rpn_loss_fused(t_cls, t_reg, cls_label, reg_label, loc_scope=4.0, loc_bin_size=0.8)
    loss.backward()
    tb = losses.resolve_scalars(dict(tb))
    assert loss.item() == pytest.approx(ref["loss"], rel=1e-6)
    for k, v in ref["tb"].items():
        assert tb[k] == pytest.approx(v, rel=2e-6, abs=1e-7), k
    g = t_cls.grad.cpu().numpy().reshape(-1)
    np.testing.assert_allclose(g[np.array(ref["grad_cls"]["pos"])], ref["grad_cls"]["val"], rtol=1e-5, atol=1e-9)
    gr = t_reg.grad.cpu().numpy().reshape(-1)
    np.testing.assert_allclose(gr[np.array(ref["grad_reg"]["pos"])], ref["grad_reg"]["val"], rtol=1e-5, atol=1e-9)


# --------------------------------------------------------------------------- the trainer's plumbing
def test_prefetcher_makes_the_labels_of_a_label_free_batch():
    """a ``_collate_centers`` batch through ``DevicePrefetcher``: the same entries come out as for a labelled batch, the labels being the
    host labels (reg_label bit for bit, cls_label within one fp32 unit), next to the sampling plan"""
    from ws3d_amd import train_rpn
    ds = [train_rpn.SyntheticCenters(4, npoints=4096, config_id=23, labels=flag) for flag in (True, False)]
    host = train_rpn._collate([ds[0][i] for i in range(4)])
    bare = train_rpn._collate_centers([ds[1][i] for i in range(4)])
    bare["gt_count"][1] = 0                                              # a scene whose annotations are all dropped
    want_cls, want_reg = host["rpn_cls_label"].copy(), host["rpn_reg_label"].copy()
    want_cls[1], want_reg[1] = 0, 0
    stream = train_rpn.DevicePrefetcher(iter([bare]), "cuda", (1024, 256, 64, 16))
    out = next(stream)
    torch.cuda.synchronize()
    assert set(out) == {"sample_id", "pts_input", "rpn_cls_label", "rpn_reg_label", "sampling_plan"} and out["sample_id"] == host["sample_id"]
    assert [tuple(p.shape) for p in out["sampling_plan"]] == [(4, m, 3) for m in (1024, 256, 64, 16)]
    assert np.array_equal(out["pts_input"].cpu().numpy(), host["pts_input"])
    cls, reg = out["rpn_cls_label"].cpu().numpy(), out["rpn_reg_label"].cpu().numpy()
    assert np.array_equal(reg, want_reg) and np.array_equal(cls > 0, want_cls > 0) and (want_cls[0] > 0).any()
    assert np.abs(cls.view(np.int32).astype(np.int64) - want_cls.view(np.int32).astype(np.int64)).max() <= 1
    with pytest.raises(StopIteration):
        next(stream)


# --------------------------------------------------------------------------- one step
def step_deviation(batch=2, npoints=4096, seed=3):
    """One ``train_step`` at (batch, npoints) on the torch loss and on the fused loss, from the same weights, batch and dropout seed, and
    the yardstick for their difference: how far the fp32 torch loss route is from its own float64 CPU run on that batch's head outputs.
    Only the loss has a float64 run (the network's kernels are fp32), so the gradient's yardstick is taken where both routes hand
    over, at d loss / d (rpn_cls, rpn_reg): the relative l2 distance of the fp32 route's gradient from the float64 one.  The backward
    pass is linear in that gradient, so it is the relative deviation the parameter gradient -- and with it ``grad_norm`` -- inherits.
    -> dict of figures (scripts/time_rpn_targets.py records them)"""
    from ws3d_amd import losses, stage1, train_rpn
    cfg = stage1.RPNConfig(num_points=npoints, npoints=(1024, 256, 64, 16)) if npoints == 4096 else stage1.DEFAULT_CFG
    tcfg = train_rpn.TrainConfig()
    ds = train_rpn.SyntheticCenters(batch, npoints=npoints, config_id=21)
    host = train_rpn._collate([ds[i] for i in range(batch)])
    torch.manual_seed(seed)
    model = stage1.Stage1Net(mode="TRAIN", cfg=cfg).cuda().train()
    start = copy.deepcopy(model.state_dict())

    # the yardstick: this batch's head outputs through the fp32 torch route on the device and through its float64 CPU run
    torch.manual_seed(seed + 1)
    out = model({"pts_input": torch.from_numpy(host["pts_input"]).cuda()})
    label, offsets = torch.from_numpy(host["rpn_cls_label"]).cuda(), torch.from_numpy(host["rpn_reg_label"]).cuda()
    heads = {}
    for tag, dev, dt in (("fp32", "cuda", torch.float32), ("fp64", "cpu", torch.float64)):
        c = out["rpn_cls"].detach().to(dev, dt).requires_grad_(True)
        r = out["rpn_reg"].detach().to(dev, dt).requires_grad_(True)
        loss, _ = losses.rpn_loss(c, r, label.to(dev, dt), offsets.to(dev, dt), cfg.loc_scope, cfg.loc_bin_size)
        loss.backward()
        heads[tag] = (float(loss.item()) if dt == torch.float64 else float(loss.detach().double().item()),
                      torch.cat([c.grad.reshape(-1), r.grad.reshape(-1)]).double().cpu())
    dev_loss = abs(heads["fp32"][0] - heads["fp64"][0])
    dev_grad = float((heads["fp32"][1] - heads["fp64"][1]).norm() / heads["fp64"][1].norm())

    steps = {}
    for fused in (None, False, True):       # (a step on the torch loss first, not recorded: the library picks its convolution algorithms there)
        model.load_state_dict(start)
        opt = train_rpn.AdamOneCycle(model.parameters(), 100, tcfg)
        torch.manual_seed(seed + 1)
        tb = train_rpn.train_step(model, opt, dict(host), 0, cfg, tcfg, torch.device("cuda"), fused_loss=bool(fused))
        steps[fused] = (float(tb["loss"]), float(tb["grad_norm"]), int(tb["rpn_fg_sum"]))
    return {"batch": batch, "npoints": npoints, "fp64_loss": heads["fp64"][0], "torch_route_loss_deviation": dev_loss,
            "torch_route_grad_deviation_rel": dev_grad, "loss_torch": steps[False][0], "loss_fused": steps[True][0],
            "grad_norm_torch": steps[False][1], "grad_norm_fused": steps[True][1], "fg_torch": steps[False][2], "fg_fused": steps[True][2]}


def test_train_step_on_the_fused_loss_stays_within_the_torch_routes_own_error():
    f = step_deviation()
    print(json.dumps(f, indent=1))
    assert f["fg_torch"] == f["fg_fused"] > 0
    assert abs(f["loss_fused"] - f["loss_torch"]) <= 4 * f["torch_route_loss_deviation"]
    assert abs(f["grad_norm_fused"] - f["grad_norm_torch"]) <= 4 * f["torch_route_grad_deviation_rel"] * f["grad_norm_torch"]
