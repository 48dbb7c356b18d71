"""Stage-2 training on the GPU: the paired 3-D IoU against the N x N route, the fused losses against the reference's float64 values
(tests/golden/stage2_losses.*), the network's training inputs on both routes."""
import math
import os

import numpy as np
import pytest
import torch

from tests import stage2_train_reference as tr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tr.load_cases(GOLDEN)
RCNN_IN = ("rcnn_cls", "rcnn_reg", "pred_boxes3d", "gt_boxes", "cls")
IOUN_IN = ("rcnn_iou", "rcnn_ref", "pred_boxes3d", "refined_box", "gt_boxes", "cls")
GRADS = {"rcnn": ("rcnn_cls", "rcnn_reg"), "ioun": ("rcnn_iou", "rcnn_ref")}


# --------------------------------------------------------------------------- paired IoU
def _pairs(n, seed):
    """n pairs: random boxes, then the special pairs written over the first rows that fit"""
    g = np.random.Generator(np.random.PCG64(seed))
    a = np.concatenate([g.uniform(-3, 3, (n, 1)), g.uniform(0.5, 2, (n, 1)), g.uniform(-3, 3, (n, 1)), g.uniform(1.0, 2.0, (n, 1)),
                        g.uniform(1.2, 2.0, (n, 1)), g.uniform(3.0, 4.5, (n, 1)), g.uniform(-math.pi, math.pi, (n, 1))], axis=1)
    b = a + g.normal(0, 0.5, (n, 7)) * np.array([1, 0.3, 1, 0.2, 0.2, 0.3, 0.6])
    special = []
    box = np.array([0.5, 1.0, -0.25, 1.5, 1.6, 3.9, 0.3])
    special.append((box, box))                                                          # identical
    special.append((box, box + np.array([30.0, 0, 30.0, 0, 0, 0, 1.0])))                # disjoint
    flat = np.array([0.0, 1.0, 0.0, 1.5, 2.0, 4.0, 0.0])
    special.append((flat, flat + np.array([4.0, 0, 0, 0, 0, 0, 0])))                    # sharing an edge (x extents [-2,2] and [2,6])
    special.append((flat, flat + np.array([0.0, 0, 2.0, 0, 0, 0, 0])))                  # sharing the other edge
    for k in range(4):                                                                  # ry at multiples of pi / 2
        special.append((np.array([0.2, 1.0, 0.1, 1.5, 1.6, 3.9, k * math.pi / 2]), np.array([0.0, 1.1, 0.0, 1.4, 1.7, 4.0, (k + 1) * math.pi / 2])))
    special.append((np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]), box))                # a degenerate zero-size box
    special.append((np.zeros(7), np.zeros(7)))
    for i, (x, y) in enumerate(special[:n] if n > 1 else special[:1]):
        a[n - 1 - i], b[n - 1 - i] = x, y
    return torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_paired_iou_is_the_diagonal_of_the_matrix_route_bit_for_bit(n):
    from ws3d_amd import compat as _C, iou3d_ops, kitti_utils
    a, b = _pairs(n, 100 + n)
    overlap, iou2d, iou3d = _C.boxes_iou3d_paired(a, b)
    pub2d, pub3d = iou3d_ops.boxes_iou3d_paired(a, b)
    want2d, want3d = iou3d_ops.boxes_iou3d_gpu(a, b)
    want_overlap = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    _C.boxes_overlap_bev_gpu(kitti_utils.boxes3d_to_bev_torch(a).contiguous(), kitti_utils.boxes3d_to_bev_torch(b).contiguous(), want_overlap)
    torch.cuda.synchronize()
    print("n", n, "iou3d > 0.5:", int((iou3d > 0.5).sum()), "zero overlap:", int((overlap == 0).sum()), "max iou3d", float(iou3d.max()))
    assert torch.equal(overlap, torch.diagonal(want_overlap))
    assert torch.equal(iou2d, torch.diagonal(want2d)) and torch.equal(iou3d, torch.diagonal(want3d))
    assert torch.equal(pub2d, iou2d) and torch.equal(pub3d, iou3d)
    assert iou3d.shape == (n,) and bool((overlap > 0).any())


def test_paired_iou_of_nothing_is_empty():
    from ws3d_amd import iou3d_ops
    e = torch.zeros((0, 7), dtype=torch.float32, device="cuda")
    iou2d, iou3d = iou3d_ops.boxes_iou3d_paired(e, e)
    assert iou2d.shape == (0,) and iou3d.shape == (0,) and iou3d.is_cuda


# --------------------------------------------------------------------------- fused losses
def _gpu_inputs(case, phase):
    names = RCNN_IN if phase == "rcnn" else IOUN_IN
    t = {k: torch.from_numpy(case[k]).cuda() for k in names}
    for k in GRADS[phase]:
        t[k].requires_grad_(True)
    return names, [t[k] for k in names]


def _run_fused(case, phase, upstream=None):
    from ws3d_amd import stage2_losses as sl
    names, args = _gpu_inputs(case, phase)
    loss, tb = (sl.rcnn_loss if phase == "rcnn" else sl.ioun_loss)(*args)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith(("_RcnnLossFn", "_IounLossFn")), type(loss.grad_fn).__name__
    loss.backward(None if upstream is None else torch.tensor(upstream, device="cuda"))
    grads = {k: a.grad.clone() for k, a in zip(names, args) if k in GRADS[phase]}
    return loss.detach().clone(), {k: v.clone() for k, v in tb.items()}, grads


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
def test_fused_loss_matches_the_reference_float64_run(name, phase):
    from ws3d_amd import losses
    case = CASES[name]
    m = case["meta"][phase]
    loss, tb, grads = _run_fused(case, phase)
    again = _run_fused(case, phase)
    half = _run_fused(case, phase, upstream=0.5)
    torch.cuda.synchronize()
    # bit-reproducible, and the backward only scales
    assert torch.equal(loss, again[0]) and all(torch.equal(v, again[1][k]) for k, v in tb.items())
    assert all(torch.equal(g, again[2][k]) for k, g in grads.items())
    assert all(torch.equal(half[2][k], g * 0.5) for k, g in grads.items())
    vals = losses.resolve_scalars(dict(tb))
    bad = []

    def check(label, got, want, yardstick):
        b = tr.bound(yardstick, want)
        err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
        print("%-5s %-8s %-18s err %.3g  bound %.3g  (yardstick %.3g, max|.| %.3g)" % (phase, name, label, err, b, yardstick, float(np.abs(want).max())))
        if not err <= b:
            bad.append((label, err, b))

    check("loss", float(loss), np.float64(m["loss"]), m["yardstick"]["loss"])
    for k, want in m["tb"].items():
        check(k, vals[k], np.float64(want), m["yardstick"]["tb"][k])
    for k, g in grads.items():
        check("grad_" + k, g.double().cpu().numpy(), case["grad_" + k], m["yardstick"]["grad"][k])
    assert not bad, bad
    assert float(loss) == vals["rcnn_loss" if phase == "rcnn" else "rcnn_loss_iou"]
    # the integer counts
    assert int(vals["fg_sum"]) == case["meta"]["fg_sum"]
    if phase == "rcnn":
        assert int(vals["iou_sum"]) == case["meta"]["iou_sum"]
        assert int(vals["rcnn_cls_fg"]) == int(m["tb"]["rcnn_cls_fg"]) and int(vals["rcnn_cls_bg"]) == int(m["tb"]["rcnn_cls_bg"])
    else:
        assert int(vals["valid_sum"]) == case["meta"]["valid_sum"]
    # exact zeros where the reference's host branches give zeros
    if case["meta"]["fg_sum"] == 0:
        zero = ("rcnn_loss_reg", "rcnn_loss_loc", "rcnn_loss_angle", "rcnn_loss_size", "rcnn_loss_corner") if phase == "rcnn" else \
            ("ioun_loss_loc", "ioun_loss_siz", "ioun_loss_ang", "loss_reg")
        assert all(vals[k] == 0.0 for k in zero)
        assert not grads["rcnn_reg" if phase == "rcnn" else "rcnn_ref"].any()
    if phase == "rcnn" and case["meta"]["iou_sum"] == 0:
        assert vals["rcnn_loss_corner"] == 0.0
    bg = torch.from_numpy(case["cls"]).cuda() <= 0
    assert not grads["rcnn_reg" if phase == "rcnn" else "rcnn_ref"][bg].any()


def test_fused_losses_agree_with_the_torch_route_on_the_gpu():
    """the module switch: FUSED_LOSSES = False takes the torch restatement (paired IoU kernel inside), same numbers within the bounds"""
    from ws3d_amd import stage2_losses as sl
    case = CASES["r65"]
    for phase in ("rcnn", "ioun"):
        fused = _run_fused(case, phase)
        names, args = _gpu_inputs(case, phase)
        old = sl.FUSED_LOSSES
        sl.FUSED_LOSSES = False
        try:
            loss, tb = (sl.rcnn_loss if phase == "rcnn" else sl.ioun_loss)(*args)
        finally:
            sl.FUSED_LOSSES = old
        assert not type(loss.grad_fn).__name__.startswith(("_RcnnLossFn", "_IounLossFn"))
        loss.backward()
        m = case["meta"][phase]
        # the torch route in fp32: a row's term is a chain of at most 16 fp32 operations, 2^-24 relative each
        assert abs(float(loss) - m["loss"]) <= 4 * m["yardstick"]["loss"] + 2.0 ** -20 * abs(m["loss"])
        for k, a in zip(names, args):
            if k in GRADS[phase]:
                want = case["grad_" + k]
                tol = 4 * m["yardstick"]["grad"][k] + 2.0 ** -20 * float(np.abs(want).max())
                assert float(np.abs(a.grad.double().cpu().numpy() - want).max()) <= tol, k
                assert float((a.grad - fused[2][k]).abs().max()) <= 2 * tol, k
        assert int(tb["fg_sum"]) == int(fused[1]["fg_sum"])


def test_fused_losses_write_only_their_rows():
    """R = 65 embedded at an offset inside larger buffers: the bytes on either side stay as they were"""
    from ws3d_amd import compat as _C
    case = CASES["r65"]
    R, pad, canary = 65, 37, -7.25
    cfg = (1.5, 0.5, 12, (1.5, 1.6, 3.9))

    def embed(arr, dtype=torch.float32):
        buf = torch.full((pad + arr.shape[0] + pad, *arr.shape[1:]), canary, dtype=dtype, device="cuda")
        buf[pad:pad + arr.shape[0]] = torch.from_numpy(arr).to(dtype)
        return buf, buf[pad:pad + arr.shape[0]]

    def outputs(shapes):
        bufs, views = [], []
        for sh, dt in [((8,), torch.float32), ((4,), torch.int32)] + [(sh, torch.float32) for sh in shapes]:
            buf = torch.full((pad + sh[0] + pad, *sh[1:]), canary if dt == torch.float32 else -7, dtype=dt, device="cuda")
            bufs.append(buf); views.append(buf[pad:pad + sh[0]])
        return bufs, views

    for phase, names, shapes in (("rcnn", RCNN_IN, [(R,), (R, 52)]), ("ioun", IOUN_IN, [(R,), (R, 7)])):
        ins = [embed(case[k]) for k in names]
        bufs, views = outputs(shapes)
        if phase == "rcnn":
            plain = _C.stage2_rcnn_loss(*[torch.from_numpy(case[k]).cuda() for k in names], *cfg)
            got = _C.stage2_rcnn_loss(*[v for _, v in ins], *cfg, out=views)
        else:
            plain = _C.stage2_ioun_loss(*[torch.from_numpy(case[k]).cuda() for k in names])
            got = _C.stage2_ioun_loss(*[v for _, v in ins], out=views)
        torch.cuda.synchronize()
        for p_, g_ in zip(plain, got):
            assert torch.equal(p_, g_)
        for buf in bufs + [b for b, _ in ins]:
            fill = canary if buf.dtype == torch.float32 else -7
            assert bool((buf[:pad] == fill).all()) and bool((buf[-pad:] == fill).all()), phase
        for (buf, view), k in zip(ins, names):
            assert torch.equal(view.cpu(), torch.from_numpy(case[k])), k


# --------------------------------------------------------------------------- the network's training inputs, one step per phase
@pytest.fixture(scope="module")
def step():
    return tr.load_step(GOLDEN)


def _step_model(meta, train, phase="ioun"):
    """Stage2Net with the step fixture's seeded weights (the generator filled the reference's PointRCNN the same way, key for key)"""
    from ws3d_amd import stage2
    from ws3d_amd.seeded import seeded_state_dict
    net = stage2.Stage2Net(mode="TRAIN" if train else "TEST")
    sd = seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, meta["seed"])
    for k in meta["scaled_keys"]:
        sd["rcnn_net." + k] = sd["rcnn_net." + k] * meta["last_layer_scale"]
    net.load_state_dict(sd)
    if train and phase == "ioun":
        net.rcnn_net.freeze_rcnn_tower()
    net = net.cuda()
    return net.train() if train else net.eval()


def _route(net, data, fast, **kw):
    from ws3d_amd import stage2
    old = stage2.CHANNELS_LAST_FASTPATH
    stage2.CHANNELS_LAST_FASTPATH = fast
    try:
        with torch.no_grad():
            return net.rcnn_net(data, **kw)
    finally:
        stage2.CHANNELS_LAST_FASTPATH = old


def _within(label, got, want, yardstick, bad):
    err = float(np.abs(got.double().cpu().numpy().reshape(want.shape) - want).max())
    print("%-28s err %.3g  bound %.3g  (yardstick %.3g, max|.| %.3g)" % (label, err, 4 * yardstick, yardstick, float(np.abs(want).max())))
    if not err <= 4 * yardstick:
        bad.append((label, err, 4 * yardstick))


@pytest.mark.parametrize("fast", [False, True])
def test_iou_noise_inputs_reproduce_the_reference_forward(step, fast):
    """eval mode, iou_trans / iou_scale / iou_ry present: pred_boxes3d, refined_box and the canonical cloud of the step fixture's ioun
    forward (the reference's RCNNNet under model_fn, float64) on both routes, every element, within 4 x the reference's fp32 error"""
    from ws3d_amd import train_rcnn as t2
    meta, arrays = step
    net = _step_model(meta, train=False)
    data = t2.prepare_batch(tr.step_batch(arrays, "ioun"), "cuda")
    inputs = {k: data[k] for k in ("cur_box_point", "cur_box_reflect", "train_mask") + t2.IOU_KEYS}
    out = _route(net, inputs, fast)
    plain = _route(net, {k: v for k, v in inputs.items() if k not in t2.IOU_KEYS}, fast)
    outs, bad = meta["phases"]["ioun"]["outputs"], []
    for k, name in (("pred_boxes3d", "pred_boxes3d"), ("refined_box", "refined_box"), ("canonical_xyz", "can_xyz"), ("rcnn_iou", "rcnn_iou"), ("rcnn_ref", "rcnn_ref")):
        _within("%s %s" % ("channels_last" if fast else "modules", k), out[k], arrays["ioun/" + name].astype(np.float64), outs[name]["yardstick"], bad)
    assert not bad, bad
    assert np.array_equal(out["canonical_xyz"].cpu().numpy() == 0, arrays["ioun/can_xyz"] == 0)
    assert torch.equal(out["rcnn_reg"], plain["rcnn_reg"]) and not torch.equal(out["box_ce"][:-1], plain["box_ce"][:-1])
    for k in ("box_ce", "pred_boxes3d", "refined_box", "rcnn_iou"):          # the padding cloud carries the identity noise
        assert torch.equal(out[k][-1], plain[k][-1]), k


@pytest.mark.parametrize("fast,training", [(False, False), (True, False), (False, True)])       # (training always takes the module route)
def test_towers_rcnn_returns_the_decoded_box(step, fast, training):
    from ws3d_amd import compat as _C, train_rcnn as t2
    meta, arrays = step
    net = _step_model(meta, train=training, phase="rcnn")
    data = t2.prepare_batch(tr.step_batch(arrays, "rcnn"), "cuda")
    inputs = {k: data[k] for k in ("cur_box_point", "cur_box_reflect", "train_mask")}
    both = _route(net, inputs, fast)
    one = _route(net, inputs, fast, towers='rcnn')
    assert "rcnn_iou" not in one and "refined_box" not in one and "box_ce" not in one
    assert torch.equal(one["rcnn_reg"], both["rcnn_reg"]) and torch.equal(one["rcnn_cls"], both["rcnn_cls"])
    c = net.cfg
    decoded, _ = _C.stage2_boxes(one["rcnn_reg"].contiguous(), c.loc_scope, c.loc_bin_size, c.num_head_bin, c.cls_mean_size)
    assert one["pred_boxes3d"].shape == (6, 1, 7) and torch.equal(one["pred_boxes3d"].view(6, 7), decoded)
    with pytest.raises(ValueError):
        _route(net, inputs, False, towers='iou')


@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
def test_one_training_step_matches_the_reference(step, phase):
    """forward, loss and backward of one step on the fixture's batch against the reference's model_fn in float64: the sampling of
    every level equal, head outputs / loss / tb within 4 x the reference's fp32 error, every parameter's sampled gradients and norm
    within 4 x the largest relative L2 error of the reference's fp32 gradients (as tests/test_train_step.py holds Stage 1's)"""
    from ws3d_amd import losses, stage2_losses as sl, train_rcnn as t2
    from tests import train_reference as t1
    meta, arrays = step
    m = meta["phases"][phase]
    net = _step_model(meta, train=True, phase=phase)
    data = t2.prepare_batch(tr.step_batch(arrays, phase), "cuda")
    inputs = {k: data[k] for k in ("cur_box_point", "cur_box_reflect", "train_mask") + t2.IOU_KEYS if k in data}
    trace = []
    out = net.rcnn_net(inputs, trace=trace, towers="rcnn" if phase == "rcnn" else "both")
    if phase == "rcnn":
        loss, tb = sl.rcnn_loss(out["rcnn_cls"], out["rcnn_reg"], out["pred_boxes3d"], data["gt_boxes"], data["cls"], net.cfg)
    else:
        loss, tb = sl.ioun_loss(out["rcnn_iou"], out["rcnn_ref"], out["pred_boxes3d"], out["refined_box"], data["gt_boxes"], data["cls"], net.cfg)
    assert type(loss.grad_fn).__name__.startswith(("_RcnnLossFn", "_IounLossFn"))
    loss.backward()
    # the sampling: three grouped levels per tower, in forward order (else every comparison below is void)
    assert len(trace) == len(m["index_tensors"]) // 2
    for i, lvl in enumerate(trace):
        assert np.array_equal(lvl["fps"].cpu().numpy(), arrays["%s/fps_%d" % (phase, i)].astype(np.int32)), ("fps", i)
        assert np.array_equal(lvl["bq"].cpu().numpy(), arrays["%s/bq_%d" % (phase, i)].astype(np.int32)), ("bq", i)
    bad = []
    names = {"canonical_xyz": "can_xyz"}
    for k in (("rcnn_cls", "rcnn_reg", "pred_boxes3d") if phase == "rcnn" else ("rcnn_iou", "rcnn_ref", "pred_boxes3d", "refined_box", "canonical_xyz")):
        name = names.get(k, k)
        _within("%s %s" % (phase, k), out[k].detach(), arrays["%s/%s" % (phase, name)].astype(np.float64), m["outputs"][name]["yardstick"], bad)
    vals = losses.resolve_scalars(dict(tb))
    for k, want in [("loss", m["loss"])] + list(m["tb"].items()):
        got = float(loss.detach()) if k == "loss" else vals[k]
        err, bound = abs(got - want), 4 * (m["yardstick"]["loss"] if k == "loss" else m["yardstick"]["tb"][k])
        print("%-28s err %.3g  bound %.3g  value %.6g" % (phase + " " + k, err, bound, want))
        if not err <= bound:
            bad.append((k, err, bound))
    assert int(vals["fg_sum"]) == m["fg_sum"]
    # gradients
    from ws3d_amd import stage2
    iou_tower = tuple("rcnn_net." + p for p in stage2.IOU_TOWER_PREFIXES)
    params = dict(net.named_parameters())
    if phase == "rcnn":     # the reference builds no IoU tower in phase 1; here it is there, idle
        idle = [k for k in params if k.startswith(iou_tower)]
        assert idle and all(params[k].grad is None for k in idle)
        params = {k: p for k, p in params.items() if k not in idle}
    assert list(params) == m["param_names"]
    absent = [k for k, p in params.items() if p.grad is None]
    assert absent == m["no_gradient"]
    if phase == "ioun":
        frozen = [k for k, p in params.items() if not p.requires_grad]
        assert frozen and all(params[k].grad is None for k in frozen) and sorted(set(params) - set(frozen)) == sorted(m["trainable"])
    bound = 4 * float(arrays[phase + "/grad_yardstick"].max())
    at, rows = 0, []
    for i, k in enumerate(k for k in m["param_names"] if k not in m["no_gradient"]):
        g = params[k].grad.double().cpu().numpy().reshape(-1)
        pos = t1.sample_positions(phase + ":" + k, g.size, meta["grad_samples"])
        want = arrays[phase + "/grad_values"][at:at + len(pos)].astype(np.float64)
        at += len(pos)
        l2 = float(arrays[phase + "/grad_l2"][i])
        rows.append((max(t1.rel_l2(g[pos], want), abs(float(np.linalg.norm(g)) - l2) / l2), k, float(arrays[phase + "/grad_yardstick"][i])))
    assert at == arrays[phase + "/grad_values"].size
    rows.sort(reverse=True)
    for w, k, yard in rows[:8]:
        print("%-60s worst of positions / norm %.3e  its fp32 yardstick %.3e  bound %.3e" % (k, w, yard, bound))
    bad += [(k, w, bound) for w, k, _ in rows if not w <= bound]
    assert not bad, bad


# --------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
def test_train_rcnn_runs_three_iterations_in_a_child_process(phase, tmp_path):
    import re
    import subprocess
    import sys
    from ws3d_amd import stage2, train_rcnn as t2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "ws3d_amd.train_rcnn", "--synthetic", "64", "--batch_size", "16", "--total_iters", "3", "--phase", phase,
           "--output_dir", str(tmp_path), "--seed", "1"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    found = [float(x) for x in re.findall(r"^it \d+/3  loss (\S+)", r.stdout, re.M)]
    assert len(found) == 3 and all(math.isfinite(x) for x in found)
    ck = torch.load(os.path.join(str(tmp_path), "ckpt", "checkpoint_%s_iter_00003.pth" % phase), map_location="cpu")
    assert ck["it"] == 3
    torch.manual_seed(1)
    start = stage2.Stage2Net(mode="TRAIN").state_dict()          # what train() built before its first step
    iou = tuple("rcnn_net." + p for p in stage2.IOU_TOWER_PREFIXES)
    used = lambda k: not k.startswith("rcnn_net.input_tansformer.")         # noqa: E731  (never called: no gradient in either phase)
    for k, v in ck["model_state"].items():
        trained = used(k) and (k.startswith(iou) == (phase == "ioun"))
        if not trained:
            assert torch.equal(v, start[k]), k
    moved = [k for k, v in ck["model_state"].items() if used(k) and k.startswith(iou) == (phase == "ioun") and not torch.equal(v, start[k])]
    assert len(moved) >= 20, moved
    net = stage2.Stage2Net()
    assert net.load_part_ckpt(ck) == len(start)
    net = net.cuda().eval()
    ds = t2.BoxDataset(t2.SyntheticBoxes(8, seed=2), "EVAL", seed=0)
    data = t2.prepare_batch(t2.collate([ds[i] for i in range(len(ds))]), "cuda")
    with torch.no_grad():
        out = net.rcnn_forward({k: data[k] for k in ("cur_box_point", "cur_box_reflect", "train_mask")})
    for k in ("rcnn_cls", "rcnn_reg", "rcnn_iou", "rcnn_ref", "refined_box"):
        assert bool(torch.isfinite(out[k]).all()), k
