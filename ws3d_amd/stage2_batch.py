"""Stage-2 training batches from a device-resident box dataset: ``BoxDataset`` records -> the dict ``prepare_batch`` returns, by one
launch of csrc/stage2_batch.hip (``prepare_boxes``) or by the bit-exact host restatement below (``prepare_boxes_host``: the route of a
CPU device and the reference of every test).

The contract.  A prepared sample is ``train_rcnn.BoxDataset.sample`` -> ``collate`` ->
``prepare_batch`` as a function of (sample_seed, record, aug_flag, phase, mode) alone, with ONE departure: the per-point draws do
not come from the sample's ``RandomState``::

    h(e)    = splitmix64(splitmix64(sample_seed + 0x9E3779B97F4A7C15 * 1) + e)        for row e of the record
    flip(e) = (h(e) >> 32) < floor(0.05 * 2**32)                                      the 5 % mask flips, no float involved
    perm    = the rows ascending by ((h(e) & 0xffffffff) >> (32 - key_bits), e)       stands in for ``RandomState.shuffle``

Every floating-point draw is made on the host from ``RandomState(sample_seed)`` in the order ``sample`` consumes them
(``scalar_draws``), so no device ``log`` / ``cos`` has to match numpy's; the seven box numbers and the matrices ``revive_matrix``,
``Rot_y``, ``ext_noise`` and ``noise_scale`` are computed here on the host for both routes.  ``sample``'s float64 steps stay float64
(the 1.65 m ground shift, the comparisons against gt[0] / gt[2], the x flip, the ``aug_flag`` recentring), the result is rounded to
fp32 where ``collate`` does, then ``prepare_batch``'s fp32 expressions follow in its written order.  tests/test_stage2_batch.py pins
the twin to the existing chain bit for bit through a scripted random stream that replays these draws into ``BoxDataset.sample``.
"""
from __future__ import annotations

from typing import Iterator, Optional, Sequence

import numpy as np

from .scan_prepare import GOLDEN, splitmix64
from .train_rcnn import AUG_NUM, GROUND_Y, NPOINTS, BoxDataset, _rot_y4

_M64 = (1 << 64) - 1
FLIP_THRESHOLD = int(0.05 * 2 ** 32)        # 214748364
ROUTES = ("off", "device", "host")
F_TRAIN, F_DROP, F_X_GT, F_Z_GT, F_OR, F_NEG, F_XFLIP = 1, 2, 4, 8, 16, 32, 64
# S2bParams of csrc/stage2_batch.hip
PARAMS = np.dtype([("gt0", "<f8"), ("gt2", "<f8"), ("cx", "<f8"), ("cz", "<f8"), ("seed", "<u8"), ("record", "<i4"), ("flags", "<i4"),
                   ("cut", "<i4"), ("pad", "<i4"), ("revive0", "<f4", 16), ("revive1", "<f4", 16), ("rot", "<f4", 16), ("ext", "<f4", 3),
                   ("scale", "<f4")])
assert PARAMS.itemsize == 264


# ----------------------------------------------------------------------------- the draws
def point_draws(sample_seed: int, n: int, key_bits: int = 32):
    """the per-point draws of one sample -> (flip (n,) bool, perm (n,) int64)"""
    if not 1 <= key_bits <= 32:
        raise ValueError(f"key_bits={key_bits}")
    base = splitmix64((int(sample_seed) + GOLDEN * 1) & _M64)[0]
    e = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = splitmix64(base + e)
    flip = (h >> np.uint64(32)) < np.uint64(FLIP_THRESHOLD)
    key = (h & np.uint64(0xffffffff)) >> np.uint64(32 - key_bits)
    return flip, np.lexsort((e, key)).astype(np.int64)


def scalar_draws(sample_seed: int, phase: str, mode: str, cascade: int = 1, rng: Optional[np.random.RandomState] = None) -> dict:
    """the raw floating-point draws ``BoxDataset.sample`` consumes, in its order, from ``RandomState(sample_seed)``:
    drop (6,) (TRAIN only, else None), noise (6,), g_noise (3,), scale_noise (1,), ext (3,), iou (cascade, 6) (ioun and TRAIN, else None).
    rng: a ``RandomState`` to re-seed in place of building one (the same stream at a hundredth of the cost)"""
    assert mode in ("TRAIN", "EVAL") and phase in ("rcnn", "ioun")
    if rng is None:
        rng = np.random.RandomState(int(sample_seed))
    else:
        rng.seed(int(sample_seed))
    train = mode == "TRAIN"
    d = {"drop": rng.uniform(-1, 1, 6) if train else None, "noise": rng.uniform(-1, 1, 6), "g_noise": rng.normal(0, 0.1, 3),
         "scale_noise": rng.normal(0, 0.1, 1), "ext": rng.normal(0, 0.1, 3)}
    d["iou"] = np.stack([rng.normal(0, 0.1, 6) for _ in range(cascade)]) if phase == "ioun" and train else None
    return d


# ----------------------------------------------------------------------------- the host side of a sample: everything but its rows
def sample_plan(dataset: BoxDataset, index: int, sample_seed: int, draws: Optional[dict] = None, rng=None) -> dict:
    """the decisions and numbers of one sample that do not depend on its rows, as ``BoxDataset.sample`` takes them from the scalar
    draws (`draws`: a dict as ``scalar_draws`` returns, in its place): the drop-out decisions, the row cut, the x flip, the float64
    recentring offsets, the fp32 matrices and ``prepare_batch``'s box numbers.  Both routes are built on it."""
    if dataset.npoints != NPOINTS:
        raise ValueError(f"the prepared routes write {NPOINTS}-row clouds, the dataset asks for {dataset.npoints}")
    aug_flag, rec = dataset.records[index]
    train, fg = dataset.mode == "TRAIN", rec["foreground_flag"]
    dr = draws if draws is not None else scalar_draws(sample_seed, dataset.phase, dataset.mode, dataset.cascade, rng)
    gt = rec["gt_boxes"].copy()
    gt[1] -= GROUND_Y
    cls = np.ones(1) if fg else np.zeros(1)
    flags, cut = (F_TRAIN if train else 0), NPOINTS
    gt0, gt2 = float(gt[0]), float(gt[2])
    if train:
        drop = dr["drop"]
        if drop[0] > 0.5:
            flags |= F_DROP | (F_X_GT if drop[1] > 0.0 else 0) | (F_Z_GT if drop[2] > 0.5 else 0) | (F_OR if drop[5] > 0.0 else 0)
            flags |= F_NEG if drop[4] > 0.5 else 0
        if drop[3] > 0.5:
            cut = 32 if drop[3] > 0.7 else 128

    noise = np.array(dr["noise"], dtype=np.float64)
    if aug_flag == 0:
        noise = np.zeros(6)
    g_noise = dr["g_noise"]
    noise_x, noise_z, noise_y = g_noise[0], g_noise[1], noise[2]
    noise_flip, noise_ry = noise[5], noise[3] * np.pi / 2
    noise[4] = dr["scale_noise"][0] / 2
    noise_scale = 1. + noise[4] * 0.20
    ext_noise = 1. + np.asarray(dr["ext"], dtype=np.float64) * 0.20
    revive = np.stack((_rot_y4(-gt[6]), _rot_y4(gt[6])))
    if not train:
        noise_x = noise_y = noise_z = noise_ry = 0.0
        noise_scale, ext_noise = 1.0, np.ones(3)
    if fg:
        gt[6] = (gt[6] + noise_ry) % (2 * np.pi)
        if gt[6] > np.pi:
            gt[6] -= 2 * np.pi
    if noise_flip > 0:
        flags |= F_XFLIP
        gt[0] = -gt[0]
        gt[6] = (np.pi - gt[6]) % (2 * np.pi)
        if gt[6] >= np.pi:
            gt[6] -= 2 * np.pi
        noise_ry = -noise_ry
    rot = _rot_y4(noise_ry, noise_x, noise_y, noise_z)
    cx = cz = 0.0
    if aug_flag != 0 and train:
        cx, cz = float(gt[0]), float(gt[2])
        gt[0] = gt[2] = 0.0

    f32 = np.float32
    plan = {"flags": flags, "cut": cut, "gt0": gt0, "gt2": gt2, "cx": cx, "cz": cz, "revive": revive.astype(f32), "rot": rot.astype(f32),
            "ext": ext_noise.astype(f32).reshape(3), "scale": f32(noise_scale), "cls": f32(cls[0]),
            "sample_id": rec["sample_id"], "box_id": rec["box_id"]}
    # prepare_batch on the box: sizes through ext_noise and noise_scale, the centre through noise_scale and Rot_y
    g = (np.concatenate((gt, np.ones(1))).reshape(1, 8) * cls).astype(f32).reshape(8)
    g[3:6] = g[3:6] * plan["ext"]
    g[0:6] = g[0:6] * plan["scale"]
    m, (g0, g1, g2, g7) = plan["rot"], g[[0, 1, 2, 7]]         # _apply4 on the one row [x, y, z, cls], float32 scalars
    g[0:3] = [((g0 * m[l, 0] + g1 * m[l, 1]) + g2 * m[l, 2]) + g7 * m[l, 3] for l in range(3)]
    plan["gt_boxes"] = g[0:7].copy()
    if dataset.phase == "ioun":
        trans, scale, ry = [], [], []
        for c in range(dataset.cascade):
            iou_noise = dr["iou"][c] * np.power(0.5, dataset.cascade - 1) if train else np.zeros(6)
            trans.append(iou_noise[0:3].reshape(1, 3, 1))
            scale.append(np.reshape(1. + iou_noise[3] * 0.2, (1, 1, 1)))
            ry.append(np.reshape(iou_noise[4] * np.pi / 10 if train else iou_noise[4], (1, 1, 1)))
        plan.update({"iou_trans": np.concatenate(trans, axis=-1).astype(f32), "iou_scale": np.concatenate(scale, axis=-1).astype(f32),
                     "iou_ry": np.concatenate(ry, axis=-1).astype(f32)})
    return plan


def _apply4_rows(p: np.ndarray, m: np.ndarray) -> np.ndarray:
    """``train_rcnn._apply4`` for one sample in numpy fp32: p (P,4), m (4,4) -> (P,4)"""
    p0, p1, p2, p3 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    return np.stack([((p0 * m[l, 0] + p1 * m[l, 1]) + p2 * m[l, 2]) + p3 * m[l, 3] for l in range(4)], axis=-1)


def kept_rows(dataset: BoxDataset, index: int, sample_seed: int, plan: dict, key_bits: int = 32):
    """the rows of a sample -> (idx (512,) int64: the record's row behind every output row, prob (n,) float64 after the mask flips,
    info: kept count K, rows m before the wrap-around and whether the fall-back to all rows applied)"""
    _, rec = dataset.records[index]
    pts, prob, gtm = rec["cur_box_point"], rec["cur_prob_mask"][:, 0], rec["gt_mask"][:, 0]
    n = pts.shape[0]
    if n < 1:
        raise ValueError(f"record {index % max(len(dataset) // AUG_NUM, 1)} has no rows")
    flags = plan["flags"]
    fallback = False
    if flags & F_TRAIN:
        flip, perm = point_draws(sample_seed, n, key_bits)
        prob, gtm = np.where(flip, -prob, prob), np.where(flip, -gtm, gtm)
        if flags & F_DROP:
            side_x = pts[:, 0] > plan["gt0"] if flags & F_X_GT else pts[:, 0] < plan["gt0"]
            side_z = pts[:, 2] > plan["gt2"] if flags & F_Z_GT else pts[:, 2] < plan["gt2"]
            in_x, in_z = np.logical_and(prob > 0, side_x), np.logical_and(prob > 0, side_z)
            keep = np.logical_or(in_x, in_z) if flags & F_OR else np.logical_and(in_x, in_z)
            if flags & F_NEG:
                keep = np.logical_or(keep, prob < 0)
        else:
            keep = prob > -1
        if not np.logical_and(keep, gtm > 0).any():
            keep, fallback = prob > -1, True
        order = perm[keep[perm]]
    else:
        order = np.arange(n, dtype=np.int64)
    K = len(order)
    m = min(K, NPOINTS)
    if m == NPOINTS:
        m = plan["cut"]
    if m < 1:
        raise ValueError("no row of the record is kept (its prob column holds no number)")
    return order[np.arange(NPOINTS) % m], prob, {"kept": K, "m": m, "fallback": fallback}


def _cloud(dataset: BoxDataset, index: int, idx: np.ndarray, prob: np.ndarray, plan: dict):
    """the output rows: float64 shift / flip / recentring, fp32 where collate rounds, then prepare_batch's fp32 chain"""
    _, rec = dataset.records[index]
    f32 = np.float32
    src = rec["cur_box_point"][idx]
    x = -src[:, 0] if plan["flags"] & F_XFLIP else src[:, 0]
    p = np.stack((x - plan["cx"], src[:, 1] - GROUND_Y, src[:, 2] - plan["cz"], np.ones(len(idx))), axis=1).astype(f32)
    ext, scale = plan["ext"], plan["scale"]
    p = _apply4_rows(p, plan["revive"][0])
    p = np.concatenate((p[:, 0:3] * ext[[1, 0, 2]], p[:, 3:4]), axis=1)
    p = _apply4_rows(p, plan["revive"][1])
    p = np.concatenate((p[:, 0:3] * scale, p[:, 3:4]), axis=1)
    p = _apply4_rows(p, plan["rot"])[:, 0:3]
    return np.ascontiguousarray(p, dtype=f32), rec["cur_box_reflect"][idx].astype(f32), prob[idx].astype(f32).reshape(-1, 1)


def _collate_plans(plans) -> dict:
    out = {"gt_boxes": np.stack([p["gt_boxes"] for p in plans]).reshape(-1, 1, 7), "cls": np.array([p["cls"] for p in plans], dtype=np.float32)}
    if plans and "iou_trans" in plans[0]:
        out.update({k: np.stack([p[k] for p in plans]) for k in ("iou_trans", "iou_scale", "iou_ry")})
    out["sample_id"] = [p["sample_id"] for p in plans]
    out["box_id"] = [p["box_id"] for p in plans]
    return out


def prepare_boxes_host(dataset: BoxDataset, ids: Sequence[int], sample_seeds: Sequence[int], key_bits: int = 32, draws=None) -> dict:
    """the contract in numpy -> the dict ``prepare_batch`` returns as float32 arrays: cur_box_point (R,512,3), cur_box_reflect (R,512,1),
    train_mask (R,512,1), gt_boxes (R,1,7), cls (R,) [, iou_trans, iou_scale, iou_ry], plus the sample_id / box_id lists.
    draws: one ``scalar_draws`` dict per sample to use in place of the seeded ones (tests steer branches with it)."""
    if len(ids) != len(sample_seeds) or (draws is not None and len(draws) != len(ids)):
        raise ValueError("ids, sample_seeds and draws must have one entry per sample")
    R = len(ids)
    rng = np.random.RandomState(0)
    plans = [sample_plan(dataset, int(ids[r]), int(sample_seeds[r]), None if draws is None else draws[r], rng) for r in range(R)]
    out = {"cur_box_point": np.zeros((R, NPOINTS, 3), dtype=np.float32), "cur_box_reflect": np.zeros((R, NPOINTS, 1), dtype=np.float32),
           "train_mask": np.zeros((R, NPOINTS, 1), dtype=np.float32)}
    for r in range(R):
        idx, prob, _ = kept_rows(dataset, int(ids[r]), int(sample_seeds[r]), plans[r], key_bits)
        out["cur_box_point"][r], out["cur_box_reflect"][r], out["train_mask"][r] = _cloud(dataset, int(ids[r]), idx, prob, plans[r])
    out.update(_collate_plans(plans))
    return out


# ----------------------------------------------------------------------------- the device side
class DeviceBoxes:
    """the base records of a ``BoxDataset`` on `device`, uploaded once: ``rows`` (T,6) float32 [x, y, z, reflect, prob -+ 0.5,
    gt_mask - 0.5] and ``offsets`` (records + 1) int32.  Clouds are whole cylinders of any size (at least one row).  The boxes and
    foreground flags stay on the host, in `dataset`; nothing is kept per batch.  The kernel reads fp32 rows where ``BoxDataset``
    holds float64: a record whose numbers are not fp32 numbers would be prepared from other rows than on the host, and is refused."""

    def __init__(self, dataset: BoxDataset, device="cuda:0"):
        import torch
        self.dataset = dataset
        self.device = torch.device(device)
        self.base = len(dataset) // (AUG_NUM if dataset.mode == "TRAIN" else 1)
        recs = [rec for _, rec in dataset.records[:self.base]]
        sizes = np.array([rec["cur_box_point"].shape[0] for rec in recs], dtype=np.int64)
        if (sizes < 1).any():
            raise ValueError(f"record {int(np.flatnonzero(sizes < 1)[0])} has no rows")
        if int(sizes.sum()) > 0x7fffffff:
            raise ValueError("more than 2^31 - 1 rows")
        rows64 = np.concatenate([np.concatenate((rec["cur_box_point"], rec["cur_box_reflect"], rec["cur_prob_mask"], rec["gt_mask"]), axis=1)
                                 for rec in recs])
        rows = rows64.astype(np.float32)
        if not np.array_equal(rows.astype(np.float64), rows64, equal_nan=True):
            raise ValueError("the records hold numbers that are not float32 numbers: the device route would not see the host's rows")
        offsets = np.zeros(self.base + 1, dtype=np.int64)
        np.cumsum(sizes, out=offsets[1:])
        self.total = int(offsets[-1])
        self.rows = torch.from_numpy(rows).to(self.device)
        self.offsets = torch.from_numpy(offsets.astype(np.int32)).to(self.device)


def param_blocks(dataset: BoxDataset, ids: Sequence[int], sample_seeds: Sequence[int], draws=None):
    """-> (blocks (R,) of PARAMS, plans): the host work of the device route"""
    R = len(ids)
    base = len(dataset) // (AUG_NUM if dataset.mode == "TRAIN" else 1)
    rng = np.random.RandomState(0)
    plans = [sample_plan(dataset, int(ids[r]), int(sample_seeds[r]), None if draws is None else draws[r], rng) for r in range(R)]
    blocks = np.zeros(R, dtype=PARAMS)
    if R == 0:
        return blocks, plans
    for k in ("gt0", "gt2", "cx", "cz", "flags", "cut", "scale"):
        blocks[k] = [p[k] for p in plans]
    blocks["seed"] = np.array([int(s) & _M64 for s in sample_seeds], dtype=np.uint64)
    blocks["record"] = np.asarray(ids, dtype=np.int64) % base
    revive = np.stack([p["revive"] for p in plans])
    blocks["revive0"], blocks["revive1"] = revive[:, 0].reshape(R, 16), revive[:, 1].reshape(R, 16)
    blocks["rot"] = np.stack([p["rot"] for p in plans]).reshape(R, 16)
    blocks["ext"] = np.stack([p["ext"] for p in plans])
    return blocks, plans


def prepare_boxes(device_boxes: DeviceBoxes, ids: Sequence[int], sample_seeds: Sequence[int], key_bits: int = 32, draws=None) -> dict:
    """``prepare_boxes_host``'s dict as tensors on the records' device: the parameter blocks from the twin's own host code, ONE upload
    (blocks, box numbers and the iou_* draws in one buffer) and ONE ws3d_stage2_batch launch on the current stream; nothing is read
    back.  There is no fallback: a failing launch raises."""
    if len(ids) != len(sample_seeds) or (draws is not None and len(draws) != len(ids)):
        raise ValueError("ids, sample_seeds and draws must have one entry per sample")
    if not 1 <= key_bits <= 32:
        raise ValueError(f"key_bits={key_bits}")
    ds, R = device_boxes.dataset, len(ids)
    if R and not (0 <= min(int(i) for i in ids) and max(int(i) for i in ids) < len(ds)):
        raise IndexError("sample index out of range")
    blocks, plans = param_blocks(ds, ids, sample_seeds, draws)
    host = _collate_plans(plans) if R else {"gt_boxes": np.zeros((0, 1, 7), np.float32), "cls": np.zeros(0, np.float32), "sample_id": [], "box_id": []}
    return launch_blocks(device_boxes, blocks, host, key_bits)


def launch_blocks(device_boxes: DeviceBoxes, blocks: np.ndarray, host: dict, key_bits: int = 32) -> dict:
    """the device side of ``prepare_boxes``: `blocks` and the host-made arrays of `host` (``_collate_plans``) in one upload, one launch"""
    import torch
    from . import _lib
    lib = _lib.load()
    assert lib.ws3d_stage2_batch_param_bytes() == PARAMS.itemsize
    dev, R = device_boxes.device, len(blocks)
    small = [(k, host[k]) for k in ("gt_boxes", "cls", "iou_trans", "iou_scale", "iou_ry") if k in host]
    nbytes = blocks.nbytes + sum(v.nbytes for _, v in small)
    staging = torch.empty(max(nbytes, 8), dtype=torch.uint8, pin_memory=dev.type == "cuda")
    buf = staging.numpy()
    buf[:blocks.nbytes] = blocks.view(np.uint8)
    at = blocks.nbytes
    for _, v in small:
        buf[at:at + v.nbytes] = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
        at += v.nbytes
    with torch.cuda.device(dev):
        up = staging.to(dev, non_blocking=True)
        out = {"cur_box_point": torch.empty((R, NPOINTS, 3), dtype=torch.float32, device=dev),
               "cur_box_reflect": torch.empty((R, NPOINTS, 1), dtype=torch.float32, device=dev),
               "train_mask": torch.empty((R, NPOINTS, 1), dtype=torch.float32, device=dev)}
        rc = lib.ws3d_stage2_batch(R, up.data_ptr(), device_boxes.rows.data_ptr(), device_boxes.offsets.data_ptr(), device_boxes.base,
                                   device_boxes.total, key_bits, out["cur_box_point"].data_ptr(), out["cur_box_reflect"].data_ptr(),
                                   out["train_mask"].data_ptr(), None, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "stage2_batch")
    at = blocks.nbytes
    for k, v in small:
        out[k] = up[at:at + v.nbytes].view(torch.float32).reshape(v.shape)
        at += v.nbytes
    out["sample_id"], out["box_id"] = host["sample_id"], host["box_id"]
    return out


# ----------------------------------------------------------------------------- the driver's side
def batch_plan(dataset: BoxDataset, batch_size: int) -> Iterator[tuple]:
    """endless stream of (ids, sample_seeds): the batch composition ``train_rcnn.batches`` draws from the dataset's stream -- a fresh
    permutation per epoch and one ``randint`` seed per sample"""
    while True:
        order = dataset.rng.permutation(len(dataset))
        for i0 in range(0, len(order), batch_size):
            ids = order[i0:i0 + batch_size]
            yield ids, dataset.rng.randint(0, 2 ** 31 - 1, size=len(ids))


def prepared_batches(dataset: BoxDataset, batch_size: int, route: str, device, key_bits: int = 32) -> Iterator[dict]:
    """endless stream of prepared batches on `device`: route 'device' by the kernel from a ``DeviceBoxes`` made here, route 'host' by
    the twin (the same numbers), uploaded"""
    import torch
    if route not in ROUTES[1:]:
        raise ValueError(f"route must be one of {ROUTES[1:]}, got {route!r}")
    dev = torch.device(device)
    if route == "device":
        if dev.type != "cuda":
            raise ValueError("device_batches='device' needs a GPU device; 'host' is the route of a CPU device")
        boxes = DeviceBoxes(dataset, dev)
    for ids, seeds in batch_plan(dataset, batch_size):
        if route == "device":
            yield prepare_boxes(boxes, ids, seeds, key_bits)
        else:
            res = prepare_boxes_host(dataset, ids, seeds, key_bits)
            yield {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in res.items()}
