"""One Stage-1 TRAINING step against the reference's own network in float64 (tests/golden/make_golden_train_step.py ->
train_step.npz / .json) and, kernel by kernel, against float64 re-evaluations of every hand-written training operator on the very
tensors the step feeds it (tests/train_reference.py).

The fixture holds the float64 result of the reference's PointRCNN(mode='TRAIN') step and, as the yardstick, the error of the
reference's OWN fp32 evaluation of the same step (one run, on one CPU thread).  Bounds here are 4 x that
yardstick (whole network) or 4 x the error of the library's fp32 evaluation of the same operator on the same inputs (per operator):
never a number taken from the kernels under test.

Not covered: losses.rpn_loss fed with the fixture's FULL logits on the CPU, because rpn_reg alone is
2 x 16384 x 40 values, 5 MiB, over the size limit of a committed file; tests/test_train.py pins losses.py against the reference on
seeded logits, and test_step_matches_float64_reference checks the loss of the real logits on the GPU.
"""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import train_reference as tr  # noqa: E402

G = os.path.join(HERE, "golden")
F64 = torch.float64
FACTOR = 4.0                    # bound = FACTOR x the yardstick: our summation orders are neither torch-CPU's nor the library's
BN_CAP, WGRAD_CAP = 2e-5, 3e-6  # the bounds of test_bn_relu_train_kernels_match_the_library_pair / test_conv1x1_wgrad_...: never looser
BAND_SHARE_CAP = 1e-4           # share of a tensor's elements that may sit too close to the ReLU's kink to be compared


@pytest.fixture(scope="module")
def fx():
    meta = json.load(open(os.path.join(G, "train_step.json")))
    return meta, np.load(os.path.join(G, "train_step.npz"))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import types
    from ws3d_amd import compat, nn_blocks, pn2_ops, stage1
    return types.SimpleNamespace(c=compat, pn=pn2_ops, nb=nn_blocks, s1=stage1)


def _keys():
    return json.load(open(os.path.join(G, "stage1_state_dict.json")))["keys"]


# ============================================================================= (a) the float64 references against torch's autograd
def _bn_case(shape, const_channel=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=F64) * 1.7 + 0.3
    if const_channel is not None:
        x[:, const_channel] = 0.5              # constant over the batch: variance exactly 0, invstd = eps^-1/2
    c = shape[1]
    return (x, torch.rand(c, generator=g, dtype=F64) + 0.5, torch.rand(c, generator=g, dtype=F64) - 0.4, torch.randn(c, generator=g, dtype=F64) * 0.1,
            torch.rand(c, generator=g, dtype=F64) + 0.5, torch.randn(shape, generator=g, dtype=F64))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape,const", [((2, 5, 7), None), ((3, 6, 4, 1), None), ((2, 7, 33, 16), 3), ((4, 3, 1), 1), ((1, 9, 50), None)])
def test_bn_reference_equals_double_autograd(shape, const, relu):
    """bn_train_ref / bn_train_bwd_ref against nn.BatchNorm{1,2}d(train) [+ ReLU] in double: outputs, saved statistics, the
    running-statistics update and all three gradients; C off a multiple of 4, row length 1, a constant channel, batch 1"""
    x, gamma, beta, rm, rv, dy = _bn_case(shape, const, seed=len(shape) + shape[1])
    cls = nn.BatchNorm2d if len(shape) == 4 else nn.BatchNorm1d
    m = cls(shape[1], momentum=0.3, eps=1e-5).double().train()
    with torch.no_grad():
        m.weight.copy_(gamma); m.bias.copy_(beta); m.running_mean.copy_(rm); m.running_var.copy_(rv)
    xa = x.clone().requires_grad_(True)
    pre = m(xa)
    y = torch.relu(pre) if relu else pre
    y.backward(dy)
    ref = tr.bn_train_ref(x, gamma, beta, rm, rv, 0.3, 1e-5, relu)
    _, save_mean, save_invstd = torch.native_batch_norm(x, gamma, beta, rm.clone(), rv.clone(), True, 0.3, 1e-5)
    dx, dgamma, dbeta, pre2 = tr.bn_train_bwd_ref(x, dy, gamma, beta, ref["mean"], ref["invstd"], relu)
    for got, want in ((ref["y"], y.detach()), (ref["pre"], pre.detach()), (pre2, pre.detach()), (ref["mean"], save_mean), (ref["invstd"], save_invstd),
                      (ref["running_mean"], m.running_mean), (ref["running_var"], m.running_var), (dx, xa.grad), (dgamma, m.weight.grad),
                      (dbeta, m.bias.grad)):
        assert tr.max_err(got.numpy(), want.numpy()) <= 1e-12
    if const is not None:
        assert float(ref["invstd"][const]) == pytest.approx(1e-5 ** -0.5, rel=1e-12)


def test_bn_reference_uses_the_unbiased_variance_and_every_backward_term():
    """the reference itself is sensitive to what it must catch: a biased running variance and a backward without its
    mean(dy * xh) term are far outside the 1e-12 the test above allows"""
    x, gamma, beta, rm, rv, dy = _bn_case((2, 5, 7), seed=1)
    ref = tr.bn_train_ref(x, gamma, beta, rm, rv, 0.3, 1e-5, True)
    n = 14
    biased = 0.7 * rv + 0.3 * x.transpose(0, 1).reshape(5, -1).var(dim=1, unbiased=False)
    assert tr.max_err(biased.numpy(), ref["running_var"].numpy()) > 1e-3 and n == x.numel() // 5
    dx, dgamma, dbeta, _ = tr.bn_train_bwd_ref(x, dy, gamma, beta, ref["mean"], ref["invstd"], True)
    xh = (x - ref["mean"][None, :, None]) * ref["invstd"][None, :, None]
    g = dy * (ref["pre"] > 0)
    dropped = (gamma * ref["invstd"])[None, :, None] * (g - dbeta[None, :, None] / n)
    assert tr.max_err(dropped.numpy(), dx.numpy()) > 1e-2 and torch.allclose((g * xh).sum(dim=(0, 2)), dgamma)


@pytest.mark.parametrize("B,C,O,shape", [(2, 5, 3, (7,)), (2, 6, 7, (4, 1)), (3, 7, 2, (5, 3)), (1, 1, 1, (9,))])
def test_wgrad_reference_equals_double_autograd(B, C, O, shape):
    g = torch.Generator().manual_seed(C * 10 + O)
    x = torch.randn((B, C) + shape, generator=g, dtype=F64)
    w = torch.randn((O, C) + (1,) * len(shape), generator=g, dtype=F64).requires_grad_(True)
    gy = torch.randn((B, O) + shape, generator=g, dtype=F64)
    (F.conv1d if len(shape) == 1 else F.conv2d)(x, w).backward(gy)
    assert tr.max_err(tr.conv1x1_wgrad_ref(gy, x).numpy(), w.grad.reshape(O, C).numpy()) <= 1e-12


@pytest.mark.parametrize("ns", [1, 3, 16])
def test_pool_reference_equals_double_autograd_modulo_ties(ns):
    """values equal F.max_pool2d's; the library's gradient is accepted by pool_grad_violations on rows WITH exact ties (duplicated
    columns, as ball-query padding produces them, and whole rows equal), and a gradient sent to the neighbour of the maximum is not"""
    g = torch.Generator().manual_seed(ns)
    x = torch.randn((2, 5, 9, ns), generator=g, dtype=F64)
    if ns > 1:
        x[:, :, 3:, ns // 2:] = x[:, :, 3:, :1]              # padding: the first hit repeated
        x[0, 1, 0, :] = 0.25                                 # a row of equal values
    xa = x.clone().requires_grad_(True)
    y = F.max_pool2d(xa, kernel_size=[1, ns]).squeeze(-1)
    go = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(go)
    out, ismax = tr.pool_nsample_ref(x)
    assert torch.equal(out, y.detach()) and bool((ismax.sum(-1) >= 1).all())
    assert tr.pool_grad_violations(x, go, xa.grad) == 0
    if ns > 1:
        assert int((ismax.sum(-1) > 1).sum()) > 10           # the ties are there
        last = torch.zeros_like(x).scatter_(-1, (ismax.long() * torch.arange(1, ns + 1)).argmax(-1, keepdim=True), go.unsqueeze(-1))
        assert tr.pool_grad_violations(x, go, last) == 0     # routed to the LAST of the equal maxima: the same function's gradient
        shifted = torch.roll(xa.grad, 1, dims=-1)            # routed to arg + 1
        assert tr.pool_grad_violations(x, go, shifted) > 0
        assert tr.pool_grad_violations(x, go, xa.grad * 2) > 0


@pytest.mark.parametrize("B,C,N,M,ns", [(2, 5, 11, 4, 3), (1, 3, 6, 7, 1), (2, 1, 5, 9, 4)])
def test_scatter_references_equal_double_autograd(B, C, N, M, ns):
    """grouping / gather (nsample = 1) and three-interpolate gradients against autograd through torch.gather and the weighted sum;
    neighbour lists with repeated entries (several slots of a row and several rows pointing at one source point)"""
    g = torch.Generator().manual_seed(N * M)
    idx = torch.randint(0, N, (B, M, ns), generator=g, dtype=torch.int32)
    idx[:, :, ns // 2:] = idx[:, :, :1]                      # duplicated slots
    f = torch.randn((B, C, N), generator=g, dtype=F64).requires_grad_(True)
    grouped = torch.gather(f, 2, idx.reshape(B, 1, -1).long().expand(B, C, -1)).view(B, C, M, ns)
    go = torch.randn(grouped.shape, generator=g, dtype=F64)
    grouped.backward(go)
    assert tr.max_err(tr.group_points_grad_ref(go, idx, N).numpy(), f.grad.numpy()) <= 1e-12
    if ns == 1:
        assert tr.max_err(tr.group_points_grad_ref(go.squeeze(-1), idx.squeeze(-1), N).numpy(), f.grad.numpy()) <= 1e-12
    i3 = torch.randint(0, N, (B, M, 3), generator=g, dtype=torch.int32)
    i3[:, 0, :] = 2                                          # one query whose three neighbours coincide
    w3 = torch.rand((B, M, 3), generator=g, dtype=F64)
    f2 = torch.randn((B, C, N), generator=g, dtype=F64).requires_grad_(True)
    out = sum(torch.gather(f2, 2, i3[:, :, k].long().unsqueeze(1).expand(B, C, M)) * w3[:, :, k].unsqueeze(1) for k in range(3))
    go = torch.randn(out.shape, generator=g, dtype=F64)
    out.backward(go)
    assert tr.max_err(tr.three_interpolate_grad_ref(go, i3, w3, N).numpy(), f2.grad.numpy()) <= 1e-12


# ============================================================================= (c) fixture hygiene
def _stat_slices(meta, case):
    """[(state_dict key, slice into '<case>/running_stats', flat positions or None)] in state_dict order"""
    keys, k = _keys(), meta["cases"][case]["case"]["stat_samples"]
    out, at = [], 0
    for key in meta["stat_keys"]:
        numel = int(np.prod(keys[key]))
        pos = None if k is None else tr.sample_positions(case + ":" + key, numel, k)
        n = numel if pos is None else len(pos)
        out.append((key, slice(at, at + n), pos))
        at += n
    return out, at


def _grad_slices(meta, case):
    keys, k = _keys(), meta["cases"][case]["case"]["grad_samples"]
    out, at = [], 0
    for key in meta["param_names"]:
        pos = tr.sample_positions(case + ":" + key, int(np.prod(keys[key])), k)
        out.append((key, slice(at, at + len(pos)), pos))
        at += len(pos)
    return out, at


def test_fixture_accounts_for_every_key_and_its_yardsticks_are_sane(fx):
    meta, arr = fx
    keys = _keys()
    assert len(keys) == 208
    assert sorted(meta["param_names"] + meta["stat_keys"] + meta["count_keys"]) == sorted(keys)
    assert len(set(meta["param_names"] + meta["stat_keys"] + meta["count_keys"])) == 208 and len(meta["param_names"]) == 106
    assert meta["config"]["RPN.DP_RATIO"] == 0.0
    assert set(meta["cases"]) == {"two_scenes", "no_centres"}
    for name, c in meta["cases"].items():
        y = c["yardstick"]
        flat = [y["loss"], y["rpn_cls"], y["rpn_reg"], y["running_mean"], y["running_var"]] + list(y["tb"].values())
        assert all(np.isfinite(v) and v >= 0 for v in flat)
        assert 0 < y["loss"] < 1e-5 and 0 < y["rpn_cls"] < 1e-4 and 0 < y["rpn_reg"] < 1e-4 and 0 < y["running_mean"] < 1e-5 and 0 < y["running_var"] < 1e-5
        assert set(y["tb"]) == set(c["tb"]) and y["tb"]["rpn_fg_sum"] == 0.0
        assert arr[name + "/running_stats"].size == _stat_slices(meta, name)[1] and arr[name + "/running_stats_max"].size == len(meta["stat_keys"])
        assert arr[name + "/grad_values"].size == _grad_slices(meta, name)[1]
        gy = arr[name + "/grad_yardstick"]
        assert gy.shape == (106,) and arr[name + "/grad_proj"].shape == (106, 4) and np.isfinite(gy).all() and np.isfinite(arr[name + "/grad_proj"]).all()
        # the recorded ceiling of the fp32-against-float64 spread of a parameter gradient: a regeneration that exceeds it has
        # broken something (a shim, the float64 switch), it has not found more round-off
        assert float(gy.max()) < 2e-2 and float(gy.max()) == pytest.approx(c["grad_yardstick_max"])
        absent = set(c["no_gradient"])
        assert all((arr[name + "/grad_l2"][i] == 0) == (k in absent) for i, k in enumerate(meta["param_names"]))
        # the float64 reference alone: per BatchNorm layer, the share of pre-activations within 4 x the library's fp32 forward error of 0
        assert c["relu_band_share"]["layers"] == 34 and c["relu_band_share"]["max"] <= BAND_SHARE_CAP
        assert len(c["fps_sha256"]) == 4 and len(c["ball_query_sha256"]) == 8
    assert meta["cases"]["two_scenes"]["no_gradient"] == [] and meta["cases"]["two_scenes"]["tb"]["rpn_fg_sum"] > 1000
    nc = meta["cases"]["no_centres"]
    assert nc["tb"]["rpn_fg_sum"] == 0 and nc["tb"]["rpn_loss_reg"] == 0 and all(k.startswith("rpn.rpn_reg_layer.") for k in nc["no_gradient"])
    assert len(nc["no_gradient"]) == 5
    total = sum(os.path.getsize(os.path.join(G, f)) for f in ("train_step.npz", "train_step.json"))
    assert total < 300 * 1024


# ============================================================================= the step on the GPU
_STEPS = {}


def _step(ops, meta, name, kernels=True, tap=False):
    """one forward + backward of the seeded Stage1Net on the fixture's inputs -> dict; cached per (case, path)"""
    key = (name, kernels)
    if key in _STEPS and (not tap or _STEPS[key]["log"] is not None):
        return _STEPS[key]
    from ws3d_amd import losses
    from ws3d_amd.seeded import seeded_state_dict
    case = meta["cases"][name]["case"]
    pc, centres = tr.case_inputs(case)
    labels = [losses.gaussian_center_labels(pc[b, :, :3], centres[b]) for b in range(pc.shape[0])]
    cls_label = torch.from_numpy(np.stack([np.asarray(l[0], dtype=np.float64) for l in labels])).float().cuda()
    reg_label = torch.from_numpy(np.stack([l[1] for l in labels])).float().cuda()
    cfg = ops.s1.RPNConfig(dp_ratio=0.0)
    model = ops.s1.Stage1Net(mode="TRAIN", cfg=cfg)
    model.load_state_dict(seeded_state_dict({k: tuple(v) for k, v in _keys().items()}, meta["seed"]))
    model = model.cuda().train()
    saved = (ops.nb.FUSED_BN_TRAIN, ops.nb.FUSED_CONV_WGRAD, ops.pn.DETERMINISTIC_BACKWARD)
    try:
        ops.nb.FUSED_BN_TRAIN = ops.nb.FUSED_CONV_WGRAD = ops.pn.DETERMINISTIC_BACKWARD = kernels
        with tr.train_taps() as log:
            out = model({"pts_input": torch.from_numpy(pc).cuda()})
            loss, tb = losses.rpn_loss(out["rpn_cls"], out["rpn_reg"], cls_label, reg_label, cfg.loc_scope, cfg.loc_bin_size)
            loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.nb.FUSED_BN_TRAIN, ops.nb.FUSED_CONV_WGRAD, ops.pn.DETERMINISTIC_BACKWARD = saved
    res = {"model": model, "loss": float(loss.item()), "tb": {k: float(v) for k, v in tb.items()},
           "rpn_cls": out["rpn_cls"].detach(), "rpn_reg": out["rpn_reg"].detach(), "log": log if tap else None, "labels": (cls_label, reg_label),
           "fps": [tr_sha(i) for i in log["fps"]], "bq": [[int(n), int(i.shape[-1]), tr_sha(i)] for n, i in zip(_bq_sizes(cfg), log["bq"])]}
    if not tap:
        log.clear()
    _STEPS[key] = res
    return res


def tr_sha(t):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy().astype(np.int32)).tobytes()).hexdigest()


def _bq_sizes(cfg):
    """the size of the cloud each ball query searches, in call order (two scales per level)"""
    sizes = [cfg.num_points] + list(cfg.npoints[:-1])
    return [s for s in sizes for _ in range(2)]


def _report(*cols):
    print("PARITY " + "  ".join(str(c) for c in cols))


TB_KEYS = ("rpn_loss_cls_pos", "rpn_loss_cls_neg", "rpn_loss_cls", "rpn_loss_reg", "rpn_loss", "rpn_fg_sum")
QUANTITIES = ("loss",) + tuple("tb." + k for k in TB_KEYS) + ("rpn_cls", "rpn_reg", "running_mean", "running_var")
_TIGHT = {}


def _tight_rows(meta, arr, name, got, label):
    """(d): {quantity: (error against the float64 fixture, 4 x the reference's fp32 error of that quantity)}; computed and printed once
    per (case, path)"""
    if (name, label) in _TIGHT:
        return _TIGHT[(name, label)]
    c = meta["cases"][name]
    y = c["yardstick"]
    rows = {"loss": (tr.rel_err(got["loss"], c["loss"]), FACTOR * y["loss"])}
    assert set(got["tb"]) == set(c["tb"]) == set(TB_KEYS)
    for k, v in c["tb"].items():
        rows["tb." + k] = (tr.rel_err(got["tb"][k], v), FACTOR * y["tb"][k])
    for q in ("rpn_cls", "rpn_reg"):
        ref = arr["%s/%s" % (name, q)]
        pos = tr.sample_positions(name + ":" + q, got[q].numel(), c["case"]["logit_samples"])
        val = got[q].reshape(-1)[torch.from_numpy(pos).cuda()].double().cpu().numpy()
        rows[q] = (float(np.abs(val - ref).max()) / c["logit_max"][q], FACTOR * y[q])
    state = got["model"].state_dict()
    stats, worst = arr[name + "/running_stats"], {"running_mean": 0.0, "running_var": 0.0}
    for i, (key, sl, pos) in enumerate(_stat_slices(meta, name)[0]):
        v = state[key].double().cpu().numpy().reshape(-1)
        v = v if pos is None else v[pos]
        kind = key.rsplit(".", 1)[1]
        worst[kind] = max(worst[kind], float(np.abs(v - stats[sl]).max()) / float(arr[name + "/running_stats_max"][i]))
    for kind, e in worst.items():
        rows[kind] = (e, FACTOR * y[kind])
    # where a loss scalar's error comes from: its fp32 evaluation on the device, or the logits it is evaluated on
    from ws3d_amd import losses
    _, tb64 = losses.rpn_loss(got["rpn_cls"].double(), got["rpn_reg"].double(), got["labels"][0], got["labels"][1], 4.0, 0.8)
    for k, v in c["tb"].items():
        _report("(d)", label, name, "tb." + k, "of which fp32 evaluation of the loss %.3e" % tr.rel_err(got["tb"][k], tb64[k]),
                "the logits' error %.3e" % tr.rel_err(tb64[k], v))
    for q, (e, bound) in rows.items():
        _report("(d)", label, name, q, "error %.3e" % e, "bound %.3e" % bound, "ok" if e <= bound else "EXCEEDED")
    assert set(rows) == set(QUANTITIES)
    _TIGHT[(name, label)] = rows
    return rows


def _check_indices_and_counters(meta, name, got):
    c = meta["cases"][name]
    state = got["model"].state_dict()
    assert all(int(state[k]) == 1 for k in meta["count_keys"])
    assert got["fps"] == c["fps_sha256"], "furthest point sampling indices differ from the oracle's"
    assert got["bq"] == c["ball_query_sha256"], "ball query neighbour lists differ from the oracle's"


def _check_gradients(meta, arr, name, got, label):
    """(f): every parameter gradient against float64 at the fixture's positions and through its 4 projections"""
    c = meta["cases"][name]
    bound = FACTOR * float(arr[name + "/grad_yardstick"].max())
    params = dict(got["model"].named_parameters())
    assert list(params) == meta["param_names"]
    absent = sorted(k for k, p in params.items() if p.grad is None or not bool(p.grad.any()))
    assert absent == sorted(c["no_gradient"])
    vals, rows = arr[name + "/grad_values"], []
    for i, (key, sl, pos) in enumerate(_grad_slices(meta, name)[0]):
        if key in c["no_gradient"]:
            continue
        g = params[key].grad.double().cpu().numpy().reshape(-1)
        l2 = float(arr[name + "/grad_l2"][i])
        e_pos = tr.rel_l2(g[pos], vals[sl])
        e_proj = float(np.abs(tr.projection_signs(key, g.size) @ g - arr[name + "/grad_proj"][i]).max()) / l2
        e_norm = abs(float(np.linalg.norm(g)) - l2) / l2
        rows.append((max(e_pos, e_proj, e_norm), e_pos, e_proj, e_norm, key, float(arr[name + "/grad_yardstick"][i])))
    rows.sort(reverse=True)
    for w, e_pos, e_proj, e_norm, key, yard in rows[:10]:
        _report("(f)", label, name, key, "positions %.3e" % e_pos, "projections %.3e" % e_proj, "norm %.3e" % e_norm, "fp32 yardstick %.3e" % yard,
                "bound %.3e" % bound, "ok" if w <= bound else "EXCEEDED")
    _report("(f)", label, name, "median over %d tensors" % len(rows), "%.3e" % float(np.median([r[0] for r in rows])))
    assert rows[0][0] <= bound, rows[0]


@pytest.mark.gpu
@pytest.mark.parametrize("quantity", QUANTITIES)
@pytest.mark.parametrize("name", ["two_scenes", "no_centres"])
def test_step_matches_float64_reference(ops, fx, name, quantity):
    """(d) TRAIN-mode forward, loss, every tb scalar and the BatchNorm running statistics of one step against the float64 fixture,
    each within 4 x the reference's own fp32 error of that quantity (one test per quantity; the step runs once per case).  A wrong
    momentum, a biased running variance or a mis-wired layer is off by >= 1e-3, orders of magnitude outside.

    KNOWN MISS: [two_scenes-tb.rpn_loss_cls_pos], bound 9.52e-7 (= 4 x 2.38e-7).  Measured on an MI355X: 1.16e-6 on the product
    path and 2.43e-6 on the library path of test_library_path_matches_float64_reference, bit-identical in fresh processes on one
    machine; other machines have given 2.0e-6 / 3.8e-6 and 3.2e-7 / 1.7e-7.  The forward's 1x1 convolutions are the library's, and
    which of its algorithms run decides the figure: on one machine, with nothing else changed, the library's default choice gives
    1.16e-6 / 2.43e-6, its deterministic-only choice 2.8e-8 / 1.02e-6 (31 of 34 convolution outputs differ in their last bits) and
    the framework's own GEMM convolution 1.16e-6 / 3.9e-7.  The test takes the error apart (printed with -s): the fp32 evaluation
    of the loss on the device contributes 1e-8 .. 6e-8, the rest is the error of the logits the loss is evaluated on, and those are
    inside their own bound on every path (rpn_cls 0.7e-5 .. 2.5e-5 of 3.5e-5).  rpn_loss_cls_pos is a sum over the few hundred
    points next to a centre, so a logit error that neighbouring points share does not average out: any fp32 forward lands between
    3e-8 and 4e-6, the reference's own fp32 run happened to land at 2.4e-7.  No kernel is at fault (each passes
    test_every_training_kernel_on_the_step_s_own_tensors with margin).  The bound stays as it is set and the convolution algorithm
    is not chosen to suit it, so this case and its library-path twin fail wherever the library's choice lands outside."""
    meta, arr = fx
    e, bound = _tight_rows(meta, arr, name, _step(ops, meta, name), "kernels")[quantity]
    assert e <= bound, (quantity, e, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two_scenes", "no_centres"])
def test_step_uses_the_oracle_s_samples_and_neighbours(ops, fx, name):
    """(d) everything else rests on this: the FPS and ball-query index tensors of the step are the oracle's (sha256 recorded by the
    fixture's generator from the oracle calls behind the reference's network); every num_batches_tracked is 1 after the step"""
    meta, arr = fx
    _check_indices_and_counters(meta, name, _step(ops, meta, name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two_scenes", "no_centres"])
def test_parameter_gradients_match_float64_reference(ops, fx, name):
    """(f) whole-network parameter gradients, loose by necessity: two correct fp32 evaluations of this step differ by 1e-3 .. 2e-2
    (relative L2 per tensor: ReLU masks and pooled argmaxes that flip on round-off, then sums over 1e5 .. 1e6 cancelling rows), so the
    bound is 4 x the LARGEST per-tensor fp32-against-float64 spread of the fixture.  What this sees: a missing BatchNorm term, a wrong
    scale, a gradient sent to the wrong point or parameter, a parameter without gradient (>= 1e-1).  What it cannot see: anything
    below ~1e-2 -- that is the job of test_every_training_kernel_on_the_step_s_own_tensors."""
    meta, arr = fx
    _check_gradients(meta, arr, name, _step(ops, meta, name), "kernels")


def _library_step(ops, meta, name):
    got = _step(ops, meta, name, kernels=False)
    assert (ops.nb.FUSED_BN_TRAIN, ops.nb.FUSED_CONV_WGRAD, ops.pn.DETERMINISTIC_BACKWARD) == (True, True, True)      # restored
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("quantity", QUANTITIES)
@pytest.mark.parametrize("name", ["two_scenes", "no_centres"])
def test_library_path_matches_float64_reference(ops, fx, name, quantity):
    """(g) the same step with FUSED_BN_TRAIN, FUSED_CONV_WGRAD and DETERMINISTIC_BACKWARD off -- the library's BatchNorm, weight
    gradient and atomic scatters in place of bn_relu.hip, conv_wgrad.hip and the two *_grad_det kernels -- against the same fixture
    and bounds: cross-checks the fixture from the other side.  pool_nsample and pool_nsample_grad have no switch and stay in this
    path too."""
    meta, arr = fx
    e, bound = _tight_rows(meta, arr, name, _library_step(ops, meta, name), "library")[quantity]
    assert e <= bound, (quantity, e, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two_scenes", "no_centres"])
def test_library_path_indices_and_parameter_gradients(ops, fx, name):
    """(g) ... and (f) on the library path, the case without centres included"""
    meta, arr = fx
    got = _library_step(ops, meta, name)
    _check_indices_and_counters(meta, name, got)
    _check_gradients(meta, arr, name, got, "library")


def test_default_dropout_keeps_keys_and_position():
    """(h) dp_ratio = 0.5 (the default) against the dp_ratio = 0.0 the fixture uses: same state_dict keys, Dropout at index 1"""
    from ws3d_amd import stage1
    small = dict(npoints=(64, 32, 16, 8), num_points=256)
    a, b = stage1.Stage1Net(mode="TRAIN", cfg=stage1.RPNConfig(**small)), stage1.Stage1Net(mode="TRAIN", cfg=stage1.RPNConfig(dp_ratio=0.0, **small))
    assert stage1.RPNConfig().dp_ratio == 0.5
    assert list(a.state_dict()) == list(b.state_dict()) == list(_keys())
    for net, p in ((a, 0.5), (b, 0.0)):
        for head in (net.rpn.rpn_cls_layer, net.rpn.rpn_reg_layer):
            assert isinstance(head[1], nn.Dropout) and head[1].p == p and len(head) == 3


# ============================================================================= (e) operator by operator
def _d(t):
    return t.detach().double()


def _ratio(err, scale, allow=None):
    """max over elements of (|err| - allow)+ / scale, where scale > 0; where the scale is 0 the value must be exact"""
    err = err.abs() if allow is None else (err.abs() - allow).clamp(min=0)
    pos = scale > 0
    assert not bool((err[~pos] != 0).any()), "non-zero where every term is zero"
    return float((err[pos] / scale[pos]).max()) if bool(pos.any()) else 0.0


def _bn_rows(log):
    """per BatchNorm call of the step: errors of ours and of the library's fp32 evaluation against float64, per output"""
    rows = []
    bwd = {c["x"].data_ptr(): c for c in log["bn_relu_train_bwd"]}
    assert len(bwd) == len(log["bn_relu_train_bwd"]) == len(log["bn_relu_train_fwd"])
    for f in log["bn_relu_train_fwd"]:
        x, gamma, beta = f["x"], f["gamma"], f["beta"]
        shape, C = tuple(x.shape), x.shape[1]
        rm0, rv0 = f["running_before"]
        ref = tr.bn_train_ref(_d(x), _d(gamma), _d(beta), _d(rm0), _d(rv0), f["momentum"], f["eps"], f["relu"])
        rm_l, rv_l = rm0.clone(), rv0.clone()
        out_l, mean_l, invstd_l = torch.native_batch_norm(x, gamma, beta, rm_l, rv_l, True, f["momentum"], f["eps"])
        y_l = torch.relu(out_l) if f["relu"] else out_l
        ymax = ref["y"].abs().max()
        e = {"y": (float((_d(f["y"]) - ref["y"]).abs().max() / ymax), float((_d(y_l) - ref["y"]).abs().max() / ymax))}
        stats_o = max(tr.max_err(a.double().cpu().numpy(), ref[k].cpu().numpy()) for a, k in
                      ((f["mean"], "mean"), (f["invstd"], "invstd"), (f["running_after"][0], "running_mean"), (f["running_after"][1], "running_var")))
        stats_l = max(tr.max_err(a.double().cpu().numpy(), ref[k].cpu().numpy()) for a, k in
                      ((mean_l, "mean"), (invstd_l, "invstd"), (rm_l, "running_mean"), (rv_l, "running_var")))
        e["stats"] = (stats_o, stats_l)
        del out_l, y_l
        # backward, from the kernel's own inputs (x, dy, the saved fp32 statistics)
        b = bwd[x.data_ptr()]
        assert b["relu"] == f["relu"] and torch.equal(b["mean"], f["mean"]) and torch.equal(b["invstd"], f["invstd"])
        mean, invstd = b["mean"], b["invstd"]
        dx_r, dg_r, db_r, pre_r = tr.bn_train_bwd_ref(_d(x), _d(b["dy"]), _d(gamma), _d(beta), _d(mean), _d(invstd), f["relu"])
        bc = (1, C) + (1,) * (x.dim() - 2)
        pre_l = ((x - mean.view(bc)) * invstd.view(bc)) * gamma.view(bc) + beta.view(bc)            # the library's fp32 forward from the same statistics
        g_l = b["dy"] * (pre_l > 0) if f["relu"] else b["dy"]
        dx_l, dg_l, db_l = torch.ops.aten.native_batch_norm_backward(g_l, x, gamma, None, None, mean, invstd, True, f["eps"], [True, True, True])
        # elements whose float64 pre-activation lies within the forward's round-off band of 0 may take either side of the ReLU
        band = FACTOR * float((_d(pre_l) - pre_r).abs().max()) if f["relu"] else 0.0
        amb = (pre_r.abs() < band) if f["relu"] else torch.zeros_like(pre_r, dtype=torch.bool)
        share = float(amb.double().mean())
        x3, n = tr._per_channel(_d(x))
        xh = (x3 - _d(mean)[None, :, None]) * _d(invstd)[None, :, None]
        dy3 = _d(b["dy"]).reshape(x3.shape)
        s_gamma, s_beta = (dy3.abs() * xh.abs()).sum(dim=(0, 2)), dy3.abs().sum(dim=(0, 2))
        amb3 = amb.reshape(x3.shape)
        a_gamma, a_beta = (dy3.abs() * xh.abs() * amb3).sum(dim=(0, 2)), (dy3.abs() * amb3).sum(dim=(0, 2))     # what the ambiguous elements can move
        a_dx = ((_d(gamma) * _d(invstd)).abs() * (a_beta + xh.abs().amax(dim=(0, 2)) * a_gamma) / n).view(bc)
        keep = ~amb
        dmax = dx_r.abs().max()
        e["dx"] = tuple(float((((_d(t) - dx_r).abs() - a_dx).clamp(min=0) * keep).max() / dmax) for t in (b["dx"], dx_l))
        e["dgamma"] = (_ratio(_d(b["dgamma"]) - dg_r, s_gamma, a_gamma), _ratio(_d(dg_l) - dg_r, s_gamma, a_gamma))
        e["dbeta"] = (_ratio(_d(b["dbeta"]) - db_r, s_beta, a_beta), _ratio(_d(db_l) - db_r, s_beta, a_beta))
        # the same two sums on the scale of the existing per-kernel test (max |reference|), for the record
        e["dgamma/max"] = tuple(float(((_d(t) - dg_r).abs() - a_gamma).clamp(min=0).max() / dg_r.abs().max()) for t in (b["dgamma"], dg_l))
        e["dbeta/max"] = tuple(float(((_d(t) - db_r).abs() - a_beta).clamp(min=0).max() / db_r.abs().max()) for t in (b["dbeta"], db_l))
        spread = (1.0 / ref["invstd"] ** 2 - f["eps"]).clamp(min=0).sqrt() / ref["mean"].abs().clamp(min=1e-30)
        rows.append((shape, f["relu"], e, share, int(amb.sum()), float(spread.min())))
        del ref, dx_r, pre_r, pre_l, g_l, dx_l, x3, xh, dy3, amb, amb3, keep
    return rows


def _module_counts(model):
    """how often one step must call each kernel, from the module tree"""
    from ws3d_amd import pn2_modules, pn2_ops
    bn = sum(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in model.modules())
    conv = sum(isinstance(m, (nn.Conv1d, nn.Conv2d)) for m in model.modules())
    sa = [m for m in model.modules() if isinstance(m, pn2_modules.PointnetSAModuleMSG)]
    pools = sum(len(m.groupers) for m in sa)
    # the first level groups the input intensities, which carry no gradient; every later grouper scatters one back
    group = sum(len(m.groupers) for m in sa[1:] if all(isinstance(g, pn2_ops.QueryAndGroup) for g in m.groupers))
    interp = sum(isinstance(m, pn2_modules.PointnetFPModule) for m in model.modules())
    return {"bn": bn, "wgrad": conv, "pool": pools, "group": group, "interp": interp}


@pytest.mark.gpu
def test_every_training_kernel_on_the_step_s_own_tensors(ops, fx):
    """(e) the sharp check: every call one real step makes to bn_relu.hip (forward, backward), conv_wgrad.hip, pool_nsample[_grad],
    group_points_grad_det and three_interpolate_grad_det -- all SA scales, all FP layers, both heads; (B,C,4096,16|32) down to
    (B,512,64,32), (B,C,16384,1), (B,128,16384); ball-query padding with its tied maxima -- is recomputed in float64 from the SAME
    fp32 inputs (a channel that is constant over the batch is the CPU tests' case: the smallest std / |mean| of a channel in this
    step is printed, not asserted).  Per operator class the bound is 4 x the worst error of the library's own fp32 evaluation of that operator on
    those inputs (native_batch_norm / its backward, bmm, scatter_add_), never looser than the existing per-kernel bound (for the weight
    gradient: wherever the library itself keeps that bound, see below).
      * elementwise outputs (y, dx, saved statistics) are normalised by max |reference| of the tensor;
      * sums (dgamma, dbeta, the weight gradient, the scatter gradients) by the sum of the absolute values of their terms, per
        output element: what their round-off is proportional to when the terms cancel;
      * BatchNorm+ReLU backward: an element whose float64 pre-activation is within 4 x the library's fp32 forward error of 0 may
        take either side of the ReLU.  Such elements are left out of the dx comparison (at most 1e-4 of a tensor), and what they
        could contribute to the channel's dgamma / dbeta -- and through those to dx -- is allowed on top of the bound;
      * max over nsample: values bit-equal; the recorded argmax holds the maximum; the gradient is compared modulo the routing
        among EQUAL values of a row (train_reference.pool_grad_violations).
    Measured figures: profiles/train_step_parity.txt."""
    meta, arr = fx
    got = _step(ops, meta, "two_scenes", tap=True)
    try:
        _check_every_kernel(got)
    finally:
        got["log"] = None                           # the recorded activations of a whole step: not kept for the rest of the session


def _check_every_kernel(got):
    log, counts = got["log"], _module_counts(got["model"])
    assert all(v > 0 for v in counts.values()) and counts["pool"] == 8 and counts["interp"] == 4, counts       # four levels, two scales each
    assert len(log["bn_relu_train_fwd"]) == len(log["bn_relu_train_bwd"]) == counts["bn"]
    assert len(log["conv1x1_wgrad"]) == counts["wgrad"]
    assert len(log["pool_nsample"]) == len(log["pool_nsample_grad"]) == counts["pool"]
    assert len(log["group_points_grad_det"]) == counts["group"] and len(log["three_interpolate_grad_det"]) == counts["interp"]
    failures = []

    def judge(cls, rows, cap=None):
        """rows: [(label, ours, library)] -> assert ours <= min(4 x worst library error of the class, cap)"""
        lib = max(r[2] for r in rows)
        bound = FACTOR * lib if cap is None else min(FACTOR * lib, cap)
        for label, ours, theirs in rows:
            _report("(e)", cls, label, "ours %.3e" % ours, "library %.3e" % theirs, "bound %.3e" % bound, "ok" if ours <= bound else "EXCEEDED")
            if not ours <= bound:
                failures.append((cls, label, ours, bound))

    # ---- BatchNorm + ReLU
    bn = _bn_rows(log)
    for shape, relu, e, share, n_amb, _ in bn:
        _report("(e)", "bn relu band", shape, "share %.2e" % share, "elements %d" % n_amb)
        assert share <= BAND_SHARE_CAP, (shape, share)
    judge("bn_fwd.y", [(s, *e["y"]) for s, _, e, _, _, _ in bn], BN_CAP)
    judge("bn_fwd.stats", [(s, *e["stats"]) for s, _, e, _, _, _ in bn], BN_CAP)
    judge("bn_bwd.dx", [(s, *e["dx"]) for s, _, e, _, _, _ in bn], BN_CAP)
    judge("bn_bwd.dgamma", [(s, *e["dgamma"]) for s, _, e, _, _, _ in bn], BN_CAP)
    judge("bn_bwd.dbeta", [(s, *e["dbeta"]) for s, _, e, _, _, _ in bn], BN_CAP)
    for s, _, e, _, _, _ in bn:
        _report("(e)", "bn_bwd sums on max|ref|", s, "dgamma ours %.3e library %.3e" % e["dgamma/max"], "dbeta ours %.3e library %.3e" % e["dbeta/max"],
                "existing bound %.0e" % BN_CAP)
        if max(e["dgamma/max"][0], e["dbeta/max"][0]) > BN_CAP:
            failures.append(("bn_bwd sums on max|ref|", s, e["dgamma/max"][0], e["dbeta/max"][0], BN_CAP))
    _report("(e)", "bn", "smallest std / |mean| of a channel in the step", "%.3e" % min(r[5] for r in bn))
    assert {len(s) for s, _, _, _, _, _ in bn} == {3, 4} and any(s[-1] == 1 and s[2] == 16384 for s, _, _, _, _, _ in bn)

    # ---- weight gradient of the 1x1 convolutions
    rows, rows_max = [], []
    for c in log["conv1x1_wgrad"]:
        gy, x = c["grad_out"], c["x"]
        B = x.shape[0]
        ref = tr.conv1x1_wgrad_ref(_d(gy), _d(x))
        scale = tr.conv1x1_wgrad_ref(_d(gy).abs(), _d(x).abs())
        lib = torch.bmm(gy.reshape(B, gy.shape[1], -1), x.reshape(B, x.shape[1], -1).transpose(1, 2)).sum(0)
        ours = c["gw"].reshape(ref.shape)
        label = (tuple(gy.shape), tuple(x.shape))
        rows.append((label, _ratio(_d(ours) - ref, scale), _ratio(_d(lib) - ref, scale)))
        rows_max.append((label, float((_d(ours) - ref).abs().max() / ref.abs().max()), float((_d(lib) - ref).abs().max() / ref.abs().max())))
    judge("wgrad", rows)
    # the existing per-kernel bound, 3e-6 x max |reference|, was set on random data, where products of both signs keep the partial
    # sums near sqrt(k) terms.  On the step's own tensors (inputs after a ReLU: one sign) the partial sums grow like k, and so does
    # the round-off of ANY fp32 accumulation: the library's own weight gradient misses that bound on several layers (measured: up to
    # 1.9e-5).  So the existing bound is required wherever the library keeps it; on the other layers the kernel must be no worse on
    # this scale than the library is on the same layer (no factor), on top of the sum-scaled class bound above.
    for label, o, l in rows_max:
        bound = max(WGRAD_CAP, l)
        _report("(e)", "wgrad on max|ref|", label, "ours %.3e" % o, "library %.3e" % l, "bound %.3e" % bound,
                "(the existing bound)" if l <= WGRAD_CAP else "(the library's error on this layer)", "ok" if o <= bound else "EXCEEDED")
        if not o <= bound:
            failures.append(("wgrad on max|ref|", label, o, bound))

    # ---- max over nsample and its gradient
    fwd = {c["arg"].data_ptr(): c for c in log["pool_nsample"]}
    tied = 0
    for c in log["pool_nsample_grad"]:
        f = fwd[c["arg"].data_ptr()]
        x, out, arg = f["x"], f["out"], f["arg"]
        ref, ismax = tr.pool_nsample_ref(x)
        assert torch.equal(out, ref) and torch.equal(out, F.max_pool2d(x, kernel_size=[1, x.shape[-1]]).squeeze(-1))
        assert torch.equal(x.gather(-1, arg.long().unsqueeze(-1)).squeeze(-1), ref), "the recorded argmax does not hold the maximum"
        assert c["nsample"] == x.shape[-1] and tuple(c["grad_x"].shape) == tuple(x.shape)
        bad = tr.pool_grad_violations(x, c["grad_out"], c["grad_x"])
        rows_tied = int((ismax.sum(-1) > 1).sum())
        tied += rows_tied
        _report("(e)", "pool", tuple(x.shape), "rows with tied maxima %d" % rows_tied, "violations %d" % bad)
        assert bad == 0, (tuple(x.shape), bad)
    assert tied > 0, "the step's data must exercise tied maxima (ball-query padding)"

    # ---- scatter gradients
    rows = []
    for c in log["group_points_grad_det"]:
        go, idx = c["grad_out"], c["idx"]
        B, C = go.shape[0], go.shape[1]
        go4 = go.reshape(B, C, c["npoints"], c["nsample"])
        ref, scale = tr.group_points_grad_ref(_d(go4), idx, c["n"]), tr.group_points_grad_ref(_d(go4).abs(), idx, c["n"])
        lib = tr.group_points_grad_ref(go4, idx, c["n"])                                    # fp32 scatter_add_ on the device
        rows.append(((tuple(go4.shape), c["n"]), _ratio(_d(c["grad_points"]) - ref, scale), _ratio(_d(lib) - ref, scale)))
    judge("group_points_grad", rows)
    rows = []
    for c in log["three_interpolate_grad_det"]:
        go, idx, w = c["grad_out"], c["idx"], c["weight"]
        ref = tr.three_interpolate_grad_ref(_d(go), idx, _d(w), c["m"])
        scale = tr.three_interpolate_grad_ref(_d(go).abs(), idx, _d(w).abs(), c["m"])
        lib = tr.three_interpolate_grad_ref(go, idx, w, c["m"])
        rows.append(((tuple(go.shape), c["m"]), _ratio(_d(c["grad_points"]) - ref, scale), _ratio(_d(lib) - ref, scale)))
    judge("three_interpolate_grad", rows)
    assert not failures, failures
