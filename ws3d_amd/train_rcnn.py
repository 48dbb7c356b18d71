"""Stage-2 training: the RCNN tower (phase ``rcnn``), then the IoU tower with the RCNN tower frozen (phase ``ioun``).

    python -m ws3d_amd.train_rcnn --data DIR/train_boxes.pkl | --synthetic N
                                  --phase rcnn|ioun [--batch_size 800] [--total_iters 40000]
                                  [--output_dir D] [--ckpt x.pth] [--pretrain_ckpt y.pth]
                                  [--ckpt_save_interval 20] [--seed S] [--workers W] [--device_batches off|device|host]

Counterpart of tools/train_cascade1.py (``get_rcnn_loss``) and tools/train_cascade_later.py (``get_ioun_loss``) on what
``gen_box_dataset`` writes:

  * ``BoxDataset`` prepares a sample as lib/datasets/kitti_boxplace_dataset.py:216-587 does: the 1.65 m ground shift, in TRAIN mode
    the 5 % mask flips, the shuffle, the region drop-out, the 512 / 128 / 32 truncation, then wrap-around padding to 512 points, the
    noise draws (translation, heading, flip, scale, the ``ext_noise`` stretch with its two ``revive_matrix`` turns), the ``aug_flag``
    recentring and, in phase ioun, the ``iou_*`` noise on the box the IoU tower is given.  Every record appears four times per
    epoch with aug_flag 0..3 (:132-175).  ``mode='EVAL'`` is the noise-free branch.  All draws come from ``RandomState``s the dataset
    seeds from its own stream, one per sample, so a batch does not depend on how many workers prepared it; reproducing the
    reference's global ``np.random`` stream draw for draw is not attempted, and its weak-label subset selection (:103-129) is left
    to whoever writes the pickle.
  * ``prepare_batch`` is the Stage-2 branch of ``model_fn`` (lib/net/train_functions.py:40-68): the 4 x 4 products are rotations about
    y plus a translation, written out element-wise in fp32 in a fixed order, not sent through a batched GEMM.
  * ``train_step``: forward by the module route (``towers`` by phase), the phase's loss (``stage2_losses``: one fused HIP launch),
    backward, ``clip_grad_norm_(1.0)``, Adam one-cycle with ``pct_start = 0.2`` (weaklyRCNN.yaml / weaklyIOUN.yaml; no BatchNorm, so
    no BN momentum schedule).  One host read per step, at its end.
  * ``SyntheticBoxes`` builds the same records from ``synth.roi_clouds`` with a known box per cloud, about half of them foreground.

  * ``--device_batches device`` (opt-in) takes the batches from ``stage2_batch``: the records uploaded once, one HIP launch per batch
    in place of ``BoxDataset.sample`` x batch, ``collate`` and ``prepare_batch``; ``host`` is its bit-exact numpy twin.  Same batch
    composition and sample seeds as ever, another random stream for the per-point flips and the shuffle.

Not here: the reference's per-20-iteration eval loop, TensorBoard, ``nn.DataParallel``, ``cur_pts_feature`` datasets.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import copy
import os
import pickle
import time
from typing import Iterator, Optional

import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_

from . import losses, stage2, stage2_losses, synth
from .train_rpn import AdamOneCycle, TrainConfig, checkpoint_state, load_checkpoint, save_checkpoint

STAGE2_TRAIN = TrainConfig(pct_start=0.2)       # the TRAIN block of weaklyRCNN.yaml / weaklyIOUN.yaml: Stage 1's but for PCT_START
GROUND_Y = 1.65
NPOINTS = 512
AUG_NUM = 4
SAMPLE_KEYS = ("Rot_y", "noise_scale", "gt_boxes", "ext_noise", "revive_matrix", "cls", "cur_box_point", "cur_box_reflect", "cur_prob_mask", "gt_mask")
IOU_KEYS = ("iou_trans", "iou_scale", "iou_ry")


# ----------------------------------------------------------------------------- data
def _rot_y4(angle, tx=0.0, ty=0.0, tz=0.0):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, tx], [0, 1, 0, ty], [-s, 0, c, tz], [0, 0, 0, 1]], dtype=np.float64)


class BoxDataset:
    """records of ``gen_box_dataset`` (a path to ``<split>_boxes.pkl`` or the list itself) -> training samples; see the module docstring.
    ``ds[i]`` draws the sample's seed from the dataset's stream; ``ds.sample(i, rng)`` prepares it from a given ``RandomState``."""

    def __init__(self, source, mode: str = "TRAIN", seed: int = 0, phase: str = "rcnn", npoints: int = NPOINTS, cascade: int = 1):
        assert mode in ("TRAIN", "EVAL") and phase in ("rcnn", "ioun")
        if isinstance(source, (str, os.PathLike)):
            with open(source, "rb") as f:
                source = pickle.load(f)
        self.mode, self.phase, self.npoints, self.cascade = mode, phase, npoints, cascade
        self.rng = np.random.RandomState(seed)
        base = []
        for d in source:        # kitti_boxplace_dataset.py:79-96: masks become +-0.5
            base.append({"sample_id": d["sample_id"], "box_id": d["box_id"], "center": np.asarray(d["center"], dtype=np.float64),
                         "gt_boxes": np.asarray(d["gt_boxes"], dtype=np.float64).reshape(7), "foreground_flag": bool(d["foreground_flag"]),
                         "cur_box_point": np.asarray(d["cur_box_point"], dtype=np.float64).reshape(-1, 3),
                         "cur_box_reflect": np.asarray(d["cur_box_reflect"], dtype=np.float64).reshape(-1, 1),
                         "cur_prob_mask": (np.asarray(d["cur_prob_mask"]) > 0.5).astype(np.float64).reshape(-1, 1) - 0.5,
                         "gt_mask": np.asarray(d["gt_mask"], dtype=np.float64).reshape(-1, 1) - 0.5})
        self.records = [(i, d) for i in range(AUG_NUM if mode == "TRAIN" else 1) for d in base]

    def __len__(self):
        return len(self.records)

    def __getitem__(self, index):
        return self.sample(index, np.random.RandomState(self.rng.randint(0, 2 ** 31 - 1)))

    def sample(self, index, rng) -> dict:
        aug_flag, rec = self.records[index]
        d = copy.deepcopy(rec)
        train = self.mode == "TRAIN"
        gt = d["gt_boxes"]
        cls = np.ones(1) if d["foreground_flag"] else np.zeros(1)
        pts, reflect, prob, gt_mask = d["cur_box_point"], d["cur_box_reflect"], d["cur_prob_mask"], d["gt_mask"]
        pts[:, 1] -= GROUND_Y
        gt[1] -= GROUND_Y
        if not train:
            gt_mask = prob.copy()
        rows = np.concatenate((pts, reflect, prob, gt_mask), axis=1)
        if train:
            flip = rng.uniform(0, 1, rows.shape[0]) > 0.95                   # :248-250
            rows[flip, 4] = -rows[flip, 4]
            rows[flip, 5] = -rows[flip, 5]
            rng.shuffle(rows)
            drop = rng.uniform(-1, 1, 6)
            if drop[0] > 0.5:                                                # :291-315
                side_x = rows[:, 0] > gt[0] if drop[1] > 0.0 else rows[:, 0] < gt[0]
                side_z = rows[:, 2] > gt[2] if drop[2] > 0.5 else rows[:, 2] < gt[2]
                in_x, in_z = np.logical_and(rows[:, 4] > 0, side_x), np.logical_and(rows[:, 4] > 0, side_z)
                keep = np.logical_or(in_x, in_z) if drop[5] > 0.0 else np.logical_and(in_x, in_z)
                if drop[4] > 0.5:
                    keep = np.logical_or(keep, rows[:, 4] < 0)
            else:
                keep = rows[:, 4] > -1
            if not np.logical_and(keep, rows[:, 5] > 0).any():
                keep = rows[:, 4] > -1
            rows = rows[keep]
            rows = rows[:min(rows.shape[0], self.npoints)]
            if rows.shape[0] == 512 and drop[3] > 0.5:                       # :328-331
                rows = rows[:32] if drop[3] > 0.7 else rows[:128]
        else:
            rows = rows[:min(rows.shape[0], self.npoints)]
        index_list = np.arange(rows.shape[0])                                # :333-337: wrap-around padding
        perm = index_list.copy()
        while index_list.shape[0] < self.npoints:
            index_list = np.concatenate((index_list, perm[:min(perm.shape[0], self.npoints - index_list.shape[0])]))
        rows = rows[index_list]
        pts = rows[:, 0:3].copy()

        noise = rng.uniform(-1, 1, 6)                                        # :351-378
        if aug_flag == 0:
            noise = np.zeros(6)
        g_noise = rng.normal(0, 0.1, 3)
        noise_x, noise_z, noise_y = g_noise[0], g_noise[1], noise[2]
        noise_flip, noise_ry = noise[5], noise[3] * np.pi / 2
        noise[4] = rng.normal(0, 0.1, 1)[0] / 2
        noise_scale = 1. + noise[4] * 0.20
        ext_noise = 1. + rng.normal(0, 0.1, 3) * 0.20
        revive = np.stack((_rot_y4(-gt[6]), _rot_y4(gt[6])))                  # from the heading BEFORE its noise
        if not train:
            noise_x = noise_y = noise_z = noise_ry = 0.0
            noise_scale, ext_noise = 1.0, np.ones(3)
        if d["foreground_flag"]:
            gt[6] = (gt[6] + noise_ry) % (2 * np.pi)
            if gt[6] > np.pi:
                gt[6] -= 2 * np.pi
        if noise_flip > 0:
            pts[:, 0] = -pts[:, 0]
            gt[0] = -gt[0]
            gt[6] = (np.pi - gt[6]) % (2 * np.pi)
            if gt[6] >= np.pi:
                gt[6] -= 2 * np.pi
            noise_ry = -noise_ry
        rot = _rot_y4(noise_ry, noise_x, noise_y, noise_z)
        if aug_flag != 0 and train:                                          # :431-435
            pts[:, 0] -= gt[0]
            pts[:, 2] -= gt[2]
            gt[0] = gt[2] = 0.0
        out = {"sample_id": d["sample_id"], "box_id": d["box_id"], "center": d["center"], "Rot_y": rot, "noise_scale": np.full((1, 1), noise_scale),
               "gt_boxes": np.concatenate((gt, np.ones(1))).reshape(1, 8) * cls, "ext_noise": ext_noise.reshape(1, 3), "revive_matrix": revive,
               "cls": cls, "cur_box_point": np.concatenate((pts, np.ones((pts.shape[0], 1))), axis=1), "cur_box_reflect": rows[:, 3:4].copy(),
               "cur_prob_mask": rows[:, 4:5].copy(), "gt_mask": rows[:, 5:6].copy()}
        if self.phase == "ioun":                                             # :504-534
            trans, scale, ry = [], [], []
            for _ in range(self.cascade):
                iou_noise = rng.normal(0, 0.1, 6) * np.power(0.5, self.cascade - 1) if train else np.zeros(6)
                trans.append(iou_noise[0:3].reshape(1, 3, 1))
                scale.append(np.reshape(1. + iou_noise[3] * 0.2, (1, 1, 1)))
                ry.append(np.reshape(iou_noise[4] * np.pi / 10 if train else iou_noise[4], (1, 1, 1)))
            out.update({"iou_trans": np.concatenate(trans, axis=-1), "iou_scale": np.concatenate(scale, axis=-1), "iou_ry": np.concatenate(ry, axis=-1)})
        return out


class SyntheticBoxes(list):
    """`count` records in ``gen_box_dataset``'s format from ``synth.roi_clouds``: a car-sized cloud turned by a seeded heading and
    shifted off the centre, with the box it was built from; about half of the records are foreground, the others carry no box"""

    def __init__(self, count: int, seed: int = 0, npoints: int = 640):
        super().__init__()
        g = np.random.Generator(np.random.PCG64(31000 + seed))
        clouds = synth.roi_clouds(count, npoints, 50 + seed).astype(np.float64)
        half = 0.66 * np.array([2.94, 1.5, 1.81])
        for i in range(count):
            fg = bool(g.uniform() < 0.5) if i > 1 else i == 0
            ry, dx, dz = g.uniform(-np.pi, np.pi), g.uniform(-0.4, 0.4), g.uniform(-0.4, 0.4)
            p = clouds[i] - np.array([0.0, -1.0, 0.0])
            inside = (np.abs(p) <= half * 1.2 + 1e-9).all(axis=1)
            c, s = np.cos(ry), np.sin(ry)
            pts = np.stack((c * p[:, 0] + s * p[:, 2] + dx, p[:, 1] - 1.0 + half[1] + GROUND_Y, -s * p[:, 0] + c * p[:, 2] + dz), axis=1)
            box = np.array([[dx, GROUND_Y, dz, 2 * half[1], 2 * half[2], 2 * half[0], ry]], dtype=np.float32)
            prob = np.clip(inside * 0.8 + g.uniform(0, 0.3, npoints), 0, 1)
            self.append({"instance_id": i, "sample_id": i // 4, "box_id": i % 4 if fg else -1, "center": np.zeros((1, 3), dtype=np.float32),
                         "foreground_flag": fg, "gt_boxes": box if fg else np.zeros((1, 7), dtype=np.float32),
                         "cur_box_point": pts.astype(np.float32), "cur_box_reflect": g.uniform(0, 1, (npoints, 1)).astype(np.float32),
                         "cur_prob_mask": prob.reshape(-1, 1).astype(np.float32),
                         "gt_mask": (inside if fg else np.zeros(npoints)).reshape(-1, 1).astype(np.float32)})


def collate(items) -> dict:
    keys = SAMPLE_KEYS + (IOU_KEYS if "iou_trans" in items[0] else ())
    out = {k: np.stack([np.asarray(it[k], dtype=np.float32) for it in items]) for k in keys}
    out["cls"] = out["cls"].reshape(-1)
    out["sample_id"] = [it["sample_id"] for it in items]
    out["box_id"] = [it["box_id"] for it in items]
    return out


def batches(dataset: BoxDataset, batch_size: int, workers: int = 0) -> Iterator[dict]:
    """endless stream of collated batches: a fresh permutation per epoch and one seed per sample, both from the dataset's stream"""
    pool = cf.ThreadPoolExecutor(max_workers=workers) if workers > 0 else None
    try:
        while True:
            order = dataset.rng.permutation(len(dataset))
            for i0 in range(0, len(order), batch_size):
                ids = order[i0:i0 + batch_size]
                seeds = dataset.rng.randint(0, 2 ** 31 - 1, size=len(ids))
                job = lambda a: dataset.sample(int(a[0]), np.random.RandomState(int(a[1])))      # noqa: E731
                yield collate(list(pool.map(job, zip(ids, seeds))) if pool else [job(a) for a in zip(ids, seeds)])
    finally:
        if pool:
            pool.shutdown()


# ----------------------------------------------------------------------------- model_fn's Stage-2 branch
def _apply4(p, m):
    """p (R,P,4) rows, m (R,4,4) -> rows . m^T, written out: column l = ((p0 m[l,0] + p1 m[l,1]) + p2 m[l,2]) + p3 m[l,3]"""
    p0, p1, p2, p3 = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    return torch.stack([((p0 * m[:, l, 0:1] + p1 * m[:, l, 1:2]) + p2 * m[:, l, 2:3]) + p3 * m[:, l, 3:4] for l in range(4)], dim=-1)


def prepare_batch(batch: dict, device=None, dtype=torch.float32) -> dict:
    """a collated batch (numpy or tensors) -> the network's and the loss's inputs in `dtype` (train_functions.py:40-68): the cloud goes
    through revive_matrix[0], the ``ext_noise`` stretch of (x, y, z) by (w, h, l), revive_matrix[1], ``noise_scale``, ``Rot_y``;
    the box's sizes through ``ext_noise`` and ``noise_scale``, its centre through ``noise_scale`` and ``Rot_y``.
    -> cur_box_point (R,P,3), cur_box_reflect, train_mask = cur_prob_mask (prob_mask_ratio = 1.0), gt_boxes (R,1,7), cls (R,) [, iou_*]"""
    def on(x):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
        return t.to(device=device, dtype=dtype)

    d = {k: on(batch[k]) for k in SAMPLE_KEYS + IOU_KEYS if k in batch}
    ext = d["ext_noise"].reshape(-1, 1, 3)
    scale = d["noise_scale"].reshape(-1, 1, 1)
    revive, rot = d["revive_matrix"], d["Rot_y"]
    pts, gt = d["cur_box_point"], d["gt_boxes"].clone()
    pts = _apply4(pts, revive[:, 0])
    pts = torch.cat((pts[..., 0:3] * ext[:, :, [1, 0, 2]], pts[..., 3:4]), dim=-1)
    gt[:, :, 3:6] = gt[:, :, 3:6] * ext
    pts = _apply4(pts, revive[:, 1])
    pts = torch.cat((pts[..., 0:3] * scale, pts[..., 3:4]), dim=-1)
    pts = _apply4(pts, rot)[..., 0:3]
    gt[:, :, 0:6] = gt[:, :, 0:6] * scale
    gt[:, :, 0:3] = _apply4(gt[:, :, [0, 1, 2, 7]], rot)[..., 0:3]
    out = {"cur_box_point": pts.contiguous(), "cur_box_reflect": d["cur_box_reflect"], "train_mask": d["cur_prob_mask"],
           "gt_boxes": gt[:, :, 0:7].contiguous(), "cls": d["cls"].reshape(-1)}
    out.update({k: d[k] for k in IOU_KEYS if k in d})
    return out


# ----------------------------------------------------------------------------- training
def train_step(model: stage2.Stage2Net, optimizer: AdamOneCycle, batch: dict, it: int, phase: str,
               train_cfg: TrainConfig = STAGE2_TRAIN, device=None, prepared: bool = False) -> dict:
    """one iteration: schedule, forward (``towers`` by phase), the phase's loss, backward, gradient clipping, optimizer step.
    prepared: `batch` is what ``prepare_batch`` returns already (``stage2_batch.prepared_batches``), on the model's device.
    -> the step's tb_dict as floats (+ loss, grad_norm, lr), read back in ONE host synchronisation at the end"""
    assert phase in ("rcnn", "ioun")
    optimizer.schedule(it)
    if not model.training:
        model.train()
    optimizer.zero_grad()
    data = batch if prepared else prepare_batch(batch, device if device is not None else next(model.parameters()).device)
    inputs = {k: data[k] for k in ("cur_box_point", "cur_box_reflect", "train_mask") + IOU_KEYS if k in data}
    if phase == "rcnn":
        out = model.rcnn_forward(inputs, towers="rcnn")
        loss, tb = stage2_losses.rcnn_loss(out["rcnn_cls"], out["rcnn_reg"], out["pred_boxes3d"], data["gt_boxes"], data["cls"], model.cfg)
    else:
        out = model.rcnn_forward(inputs)
        loss, tb = stage2_losses.ioun_loss(out["rcnn_iou"], out["rcnn_ref"], out["pred_boxes3d"], out["refined_box"], data["gt_boxes"], data["cls"],
                                           model.cfg)
    loss.backward()
    tb = dict(tb)
    tb["grad_norm"] = clip_grad_norm_([p for p in model.parameters() if p.requires_grad], train_cfg.grad_norm_clip)
    optimizer.step()
    tb["loss"] = loss.detach()
    losses.resolve_scalars(tb)
    tb["lr"] = optimizer.lr
    return tb


def build_model(phase: str, device, cfg: stage2.RCNNConfig = stage2.DEFAULT_CFG, pretrain_ckpt: Optional[str] = None) -> stage2.Stage2Net:
    """phase ioun starts from a phase-1 checkpoint (``pretrain_ckpt``; the IoU tower's keys may be absent) and freezes the RCNN tower"""
    model = stage2.Stage2Net(mode="TRAIN", cfg=cfg)
    if pretrain_ckpt:
        model.load_part_ckpt(torch.load(pretrain_ckpt, map_location="cpu"), allow_missing_iou=True)
    if phase == "ioun":
        model.rcnn_net.freeze_rcnn_tower()
    return model.to(device)


def trained_parameters(model: stage2.Stage2Net, phase: str):
    """what the phase's optimizer owns: phase rcnn the RCNN tower (the reference builds no IoU tower then: its weights must not even
    decay), phase ioun whatever ``freeze_rcnn_tower`` left trainable.  ``input_tansformer`` is never called and stays out: it would
    receive no gradient and only decay."""
    skip = ("rcnn_net.input_tansformer.",) + (() if phase == "ioun" else tuple("rcnn_net." + p for p in stage2.IOU_TOWER_PREFIXES))
    return [p for name, p in model.named_parameters() if p.requires_grad and not name.startswith(skip)]


def train(dataset: BoxDataset, phase: str, total_iters: int, batch_size: int = 800, output_dir: Optional[str] = None, ckpt: Optional[str] = None,
          pretrain_ckpt: Optional[str] = None, ckpt_save_interval: int = 20, seed: int = 0, workers: int = 0, device: str = "cuda:0",
          cfg: stage2.RCNNConfig = stage2.DEFAULT_CFG, train_cfg: TrainConfig = STAGE2_TRAIN, log=print, device_batches: str = "off"):
    """-> (model, history: the tb_dict of every step).  device_batches: 'off' -- ``batches`` + ``prepare_batch`` as ever; 'device' / 'host'
    -- prepared batches from ``stage2_batch`` (the kernel / its numpy twin; `workers` is not used)"""
    if device_batches not in ("off", "device", "host"):
        raise ValueError(f"device_batches must be one of off, device, host; got {device_batches!r}")
    torch.manual_seed(seed)
    dev = torch.device(device)
    model = build_model(phase, dev, cfg, pretrain_ckpt)
    optimizer = AdamOneCycle(trained_parameters(model, phase), total_iters, train_cfg)
    it = 0
    if ckpt:
        it, _ = load_checkpoint(model, optimizer, ckpt)
    ckpt_dir = os.path.join(output_dir, "ckpt") if output_dir else None
    if ckpt_dir:
        os.makedirs(ckpt_dir, exist_ok=True)
    history = []
    if device_batches == "off":
        stream = batches(dataset, batch_size, workers)
    else:
        from . import stage2_batch
        stream = stage2_batch.prepared_batches(dataset, batch_size, device_batches, dev)
    try:
        while it < total_iters:
            t0 = time.time()
            tb = train_step(model, optimizer, next(stream), it, phase, train_cfg, dev, prepared=device_batches != "off")
            it += 1
            history.append(tb)
            main_key = "rcnn_loss" if phase == "rcnn" else "rcnn_loss_iou"
            log("it %d/%d  loss %.5f  %s  grad_norm %.4f  lr %.6f  %.3f s" % (
                it, total_iters, tb["loss"], "  ".join("%s %.4f" % (k.replace("rcnn_loss_", "").replace("ioun_loss_", ""), tb[k])
                                                       for k in (stage2_losses.RCNN_KEYS if phase == "rcnn" else stage2_losses.IOUN_KEYS)
                                                       if k != main_key and "loss" in k), tb["grad_norm"], tb["lr"], time.time() - t0))
            if ckpt_dir and (it % ckpt_save_interval == 0 or it == total_iters):
                save_checkpoint(checkpoint_state(model, optimizer, it), os.path.join(ckpt_dir, "checkpoint_%s_iter_%05d" % (phase, it)))
    finally:
        stream.close()
    return model, history


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data", help="<split>_boxes.pkl written by ws3d_amd.gen_box_dataset")
    src.add_argument("--synthetic", type=int, metavar="N", help="N synthetic records instead of a pickle")
    ap.add_argument("--phase", choices=("rcnn", "ioun"), required=True)
    ap.add_argument("--batch_size", type=int, default=800)
    ap.add_argument("--total_iters", type=int, default=40000)
    ap.add_argument("--output_dir", default=None)
    ap.add_argument("--ckpt", default=None, help="resume: model, optimizer and iteration")
    ap.add_argument("--pretrain_ckpt", default=None, help="weights only (phase ioun: the phase-1 checkpoint)")
    ap.add_argument("--ckpt_save_interval", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workers", type=int, default=0, help="threads that prepare samples on the host; ignored with --device_batches device")
    ap.add_argument("--device_batches", choices=("off", "device", "host"), default="off",
                    help="device: the records live on the GPU and one HIP launch prepares a batch (stage2_batch); host: its bit-exact "
                         "numpy twin (the route of a CPU device); off: BoxDataset + prepare_batch as ever")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    source = SyntheticBoxes(a.synthetic, a.seed) if a.synthetic is not None else a.data
    dataset = BoxDataset(source, "TRAIN", a.seed, a.phase, cascade=stage2.DEFAULT_CFG.cascade)
    print("%d records -> %d samples per epoch, phase %s" % (len(dataset) // AUG_NUM, len(dataset), a.phase))
    train(dataset, a.phase, a.total_iters, a.batch_size, a.output_dir, a.ckpt, a.pretrain_ckpt, a.ckpt_save_interval, a.seed, a.workers, a.device,
          device_batches=a.device_batches)


if __name__ == "__main__":
    main()
