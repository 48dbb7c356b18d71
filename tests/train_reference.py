"""Plain-torch float64 references of the custom operators of the Stage-1 TRAINING step, written from the
math (nothing here shares code with csrc/ or with ws3d_amd's autograd functions), the error measures the
training-step fixture and its tests share, and a context manager that records every call of the step's
hand-written kernels.

  * bn_train_ref / bn_train_bwd_ref      BatchNorm(train) [+ ReLU]: outputs, saved statistics, running-statistics
                                         update (unbiased variance), dx / dgamma / dbeta
  * conv1x1_wgrad_ref                    weight gradient of a 1x1 convolution
  * pool_nsample_ref / pool_grad_violations   max over nsample; the gradient compared modulo the routing among EQUAL
                                         values of a row (ball-query padding repeats the first hit: such rows tie)
  * group_points_grad_ref / three_interpolate_grad_ref   scatter-add gradients of grouping / gather / 3-NN interpolation
  * train_taps()                         wraps the compat entry points of bn_relu.hip, conv_wgrad.hip, pool_nsample[_grad],
                                         group_points_grad_det, three_interpolate_grad_det for the duration of one step

Used by tests/test_train_step.py and by tests/golden/make_golden_train_step.py (which only needs the samplers and the
error measures, so that generator and test measure the same thing).
"""
from __future__ import annotations

import contextlib
import hashlib

import numpy as np
import torch


# ----------------------------------------------------------------------------- seeded samplers (fixture <-> test)
def _rng(*key) -> np.random.Generator:
    h = int.from_bytes(hashlib.sha256(":".join(str(k) for k in key).encode()).digest()[:8], "little")
    return np.random.Generator(np.random.PCG64(h))


def sample_positions(name: str, numel: int, k: int) -> np.ndarray:
    """flat positions at which the fixture keeps the values of tensor `name`: all of them when numel <= k,
    else k distinct seeded ones (ascending)"""
    if numel <= k:
        return np.arange(numel, dtype=np.int64)
    return np.sort(_rng("pos", name, numel, k).choice(numel, size=k, replace=False)).astype(np.int64)


def projection_signs(name: str, numel: int, count: int = 4) -> np.ndarray:
    """(count, numel) float64 of seeded +-1: `signs @ grad.ravel()` sees every element of a gradient tensor"""
    return _rng("sign", name, numel, count).integers(0, 2, size=(count, numel)).astype(np.float64) * 2.0 - 1.0


def case_inputs(case):
    """the scenes of a fixture case and their annotated centres (the first `cars` cars of each ray-cast scene): the one definition the
    fixture's generator and the tests both use"""
    from ws3d_amd import synth
    B = case["batch"]
    pc = synth.make_batch(case["kind"], B, case["n"], case["config_id"])
    centres = [synth.random_boxes3d(15, (1000 * case["config_id"] + b) * 7919 + 13)[:case["cars"], :3].astype(np.float32) for b in range(B)]
    return pc, centres


# ----------------------------------------------------------------------------- error measures
def rel_err(got: float, ref: float) -> float:
    """|got - ref| / |ref| (the plain difference where ref is 0)"""
    got, ref = float(got), float(ref)
    return abs(got - ref) / abs(ref) if ref != 0.0 else abs(got - ref)


def max_err(got, ref) -> float:
    """max |got - ref| / max |ref| over a tensor (the plain difference for an all-zero reference)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    d = float(np.abs(got - ref).max()) if ref.size else 0.0
    return d / scale if scale > 0 else d


def rel_l2(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    n = float(np.linalg.norm(ref))
    d = float(np.linalg.norm(got - ref))
    return d / n if n > 0 else d


# ----------------------------------------------------------------------------- BatchNorm(train) [+ ReLU]
def _per_channel(x):
    """x (B, C, ...) -> (x as (B, C, L), elements per channel)"""
    x3 = x.reshape(x.shape[0], x.shape[1], -1)
    return x3, x3.shape[0] * x3.shape[2]


def bn_train_ref(x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True):
    """training-mode batch normalisation over (batch, trailing axes) of a channels-first tensor, in the dtype of `x`:
    -> dict(y, pre (before the ReLU), mean, invstd, running_mean, running_var).  The normalisation uses the BIASED
    batch variance, the running variance is updated with the UNBIASED one (n / (n - 1)); running <- (1 - momentum) *
    running + momentum * batch."""
    x3, n = _per_channel(x)
    mean = x3.mean(dim=(0, 2))
    var = ((x3 - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    invstd = 1.0 / torch.sqrt(var + eps)
    pre = ((x3 - mean[None, :, None]) * invstd[None, :, None]) * gamma[None, :, None] + beta[None, :, None]
    out = {"pre": pre.reshape(x.shape), "y": (torch.clamp(pre, min=0) if relu else pre).reshape(x.shape), "mean": mean, "invstd": invstd}
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * running_mean + momentum * mean
        out["running_var"] = (1 - momentum) * running_var + momentum * (var * (n / (n - 1)) if n > 1 else var)
    return out


def bn_train_bwd_ref(x, dy, gamma, beta, mean, invstd, relu=True):
    """-> (dx, dgamma, dbeta, pre): with g = dy masked by the ReLU (pre > 0), xh the normalised input and n elements per channel,
    dbeta = sum g, dgamma = sum g * xh, dx = gamma * invstd * (g - dbeta / n - xh * dgamma / n)"""
    x3, n = _per_channel(x)
    g = dy.reshape(x3.shape)
    xh = (x3 - mean[None, :, None]) * invstd[None, :, None]
    pre = xh * gamma[None, :, None] + beta[None, :, None]
    if relu:
        g = g * (pre > 0)
    dbeta = g.sum(dim=(0, 2))
    dgamma = (g * xh).sum(dim=(0, 2))
    dx = (gamma * invstd)[None, :, None] * (g - dbeta[None, :, None] / n - xh * (dgamma[None, :, None] / n))
    return dx.reshape(x.shape), dgamma, dbeta, pre.reshape(x.shape)


# ----------------------------------------------------------------------------- 1x1 convolution: weight gradient
def conv1x1_wgrad_ref(grad_out, x):
    """grad_out (B, O, ...), x (B, C, ...) -> (O, C): sum over batch and positions of grad_out[o] * x[c]"""
    B = x.shape[0]
    return torch.einsum("bol,bcl->oc", grad_out.reshape(B, grad_out.shape[1], -1), x.reshape(B, x.shape[1], -1))


# ----------------------------------------------------------------------------- max over nsample
def pool_nsample_ref(x):
    """x (..., nsample) -> (max over the last axis, mask of the positions that hold it)"""
    out = x.amax(dim=-1)
    return out, x == out.unsqueeze(-1)


def pool_grad_violations(x, grad_out, grad_x) -> int:
    """how many rows of grad_x (..., nsample) are NOT a gradient of max over the last axis of x: the gradient may go to any
    position that holds the row's maximum (equal values are indistinguishable to the loss), so a row is right when it is zero
    off the maximal positions and its sum over them -- a single non-zero term, exact -- is grad_out"""
    _, ismax = pool_nsample_ref(x)
    off = ((grad_x != 0) & ~ismax).any(dim=-1)
    single = (grad_x != 0).sum(dim=-1) <= 1
    total = (grad_x * ismax).sum(dim=-1)
    return int((off | ~single | (total != grad_out)).sum())


# ----------------------------------------------------------------------------- scatter gradients
def group_points_grad_ref(grad_out, idx, n):
    """grad_out (B, C, M, ns), idx (B, M, ns) -> (B, C, n): every grouped copy sends its gradient back to its source point
    (nsample = 1 and grad_out (B, C, M): the gradient of gather_operation)"""
    B, C = grad_out.shape[0], grad_out.shape[1]
    flat = idx.reshape(B, 1, -1).long().expand(B, C, -1)
    return torch.zeros((B, C, n), dtype=grad_out.dtype, device=grad_out.device).scatter_add_(2, flat, grad_out.reshape(B, C, -1))


def three_interpolate_grad_ref(grad_out, idx, weight, m):
    """grad_out (B, C, n), idx / weight (B, n, 3) -> (B, C, m): out[:, :, j] = sum_k w[j, k] * f[:, :, idx[j, k]] transposed"""
    B, C, n = grad_out.shape
    terms = grad_out.unsqueeze(-1) * weight.unsqueeze(1).to(grad_out.dtype)            # (B, C, n, 3)
    return group_points_grad_ref(terms, idx, m)


# ----------------------------------------------------------------------------- taps of one training step
TAPPED = ("bn_relu_train_fwd", "bn_relu_train_bwd", "conv1x1_wgrad", "pool_nsample", "pool_nsample_grad",
          "group_points_grad_det", "three_interpolate_grad_det")


@contextlib.contextmanager
def train_taps():
    """record, for every call of the hand-written training kernels made inside the block, the call's inputs and outputs (device
    tensors, kept by reference; tensors a kernel updates in place are cloned before and after) -> dict: entry point -> list of
    calls.  Also the furthest-point-sampling and ball-query index tensors of the forward pass ('fps', 'bq')."""
    from ws3d_amd import compat, pn2_ops
    log = {k: [] for k in TAPPED + ("fps", "bq")}
    orig = {k: getattr(compat, k) for k in TAPPED}
    orig_fps, orig_qg = pn2_ops.furthest_point_sample_gather, pn2_ops.query_and_group

    def bn_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, relu=True, num_batches_tracked=None):
        before = None if running_mean is None else (running_mean.clone(), running_var.clone())
        y, mean, invstd = orig["bn_relu_train_fwd"](x, gamma, beta, running_mean, running_var, momentum, eps, relu, num_batches_tracked)
        log["bn_relu_train_fwd"].append(dict(x=x, gamma=gamma, beta=beta, momentum=momentum, eps=eps, relu=relu, running_before=before,
                                             running_after=None if before is None else (running_mean.clone(), running_var.clone()),
                                             y=y, mean=mean, invstd=invstd))
        return y, mean, invstd

    def bn_bwd(x, dy, gamma, beta, save_mean, save_invstd, relu=True):
        dx, dgamma, dbeta = orig["bn_relu_train_bwd"](x, dy, gamma, beta, save_mean, save_invstd, relu)
        log["bn_relu_train_bwd"].append(dict(x=x, dy=dy, gamma=gamma, beta=beta, mean=save_mean, invstd=save_invstd, relu=relu,
                                             dx=dx, dgamma=dgamma, dbeta=dbeta))
        return dx, dgamma, dbeta

    def wgrad(grad_out, x, shape=None):
        gw = orig["conv1x1_wgrad"](grad_out, x, shape)
        log["conv1x1_wgrad"].append(dict(grad_out=grad_out, x=x, gw=gw))
        return gw

    def pool(x):
        out, arg = orig["pool_nsample"](x)
        log["pool_nsample"].append(dict(x=x, out=out, arg=arg))
        return out, arg

    def pool_grad(grad_out, arg, nsample):
        grad_x = orig["pool_nsample_grad"](grad_out, arg, nsample)
        log["pool_nsample_grad"].append(dict(grad_out=grad_out, arg=arg, nsample=nsample, grad_x=grad_x))
        return grad_x

    def group_grad(b, c, n, npoints, nsample, grad_out, idx, grad_points):
        r = orig["group_points_grad_det"](b, c, n, npoints, nsample, grad_out, idx, grad_points)
        log["group_points_grad_det"].append(dict(n=n, npoints=npoints, nsample=nsample, grad_out=grad_out, idx=idx, grad_points=grad_points))
        return r

    def interp_grad(b, c, n, m, grad_out, idx, weight, grad_points):
        r = orig["three_interpolate_grad_det"](b, c, n, m, grad_out, idx, weight, grad_points)
        log["three_interpolate_grad_det"].append(dict(n=n, m=m, grad_out=grad_out, idx=idx, weight=weight, grad_points=grad_points))
        return r

    def fps_tap(xyz, npoint):
        r = orig_fps(xyz, npoint)
        log["fps"].append(r[0])
        return r

    def qg_tap(radius, nsample, xyz, new_xyz, features=None, use_xyz=True, return_idx=False, sorted_xyz=None):
        out, idx = orig_qg(radius, nsample, xyz, new_xyz, features, use_xyz, return_idx=True, sorted_xyz=sorted_xyz)
        log["bq"].append(idx)
        return (out, idx) if return_idx else out

    taps = dict(bn_relu_train_fwd=bn_fwd, bn_relu_train_bwd=bn_bwd, conv1x1_wgrad=wgrad, pool_nsample=pool, pool_nsample_grad=pool_grad,
                group_points_grad_det=group_grad, three_interpolate_grad_det=interp_grad)
    for k, f in taps.items():
        setattr(compat, k, f)
    pn2_ops.furthest_point_sample_gather, pn2_ops.query_and_group = fps_tap, qg_tap
    try:
        yield log
    finally:
        for k, f in orig.items():
            setattr(compat, k, f)
        pn2_ops.furthest_point_sample_gather, pn2_ops.query_and_group = orig_fps, orig_qg
