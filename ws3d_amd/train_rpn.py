"""Stage-1 (RPN) trainer: the counterpart of the reference's ``tools/train_rpn.py`` for this
repository's network and kernels.

    python -m ws3d_amd.train_rpn --synthetic 64 --batch_size 8 --total_iters 200 --output_dir out/
    python -m ws3d_amd.train_rpn --data_root /data/KITTI/object --batch_size 25 --total_iters 8000

Same flags as the reference (train_rpn.py:24-46): --batch_size, --total_iters, --ckpt_save_interval,
--workers, --output_dir, --mgpus, --ckpt, --pretrain_ckpt, --noise_kind, --weakly_num (+ --cfg_file,
accepted for command-line compatibility: the weaklyRPN.yaml values live in ``stage1.RPNConfig`` and
``TrainConfig``).  What it reproduces:
  * optimizer 'adam_onecycle' (train_rpn.py:84-101 + learning_schedules_fastai.py:54-77): Adam
    betas (mom, 0.99), decoupled weight decay p *= 1 - wd*lr on every parameter (fastai
    ``OptimWrapper(true_wd=True, bn_wd=True)``), one-cycle cosine lr / momentum schedule stepped
    every iteration; gradient-norm clipping at 1.0; BN-momentum step decay (train_rpn.py:113-118);
  * the loss (``ws3d_amd.losses.rpn_loss``) on Gaussian centre labels -- made per scene on the host like the
    reference's; ``--device_targets`` uploads scenes and centres instead, makes the labels on the device
    (``losses.center_labels_batch``) and takes loss and gradient from fused HIP (``losses.rpn_loss_fused``);
  * checkpoints ``ckpt/checkpoint_iter_%05d.pth`` = {'it', 'model_state', 'optimizer_state'}
    (train_utils.py:67-99) -- ``model_state`` interchanges with the reference (identical keys).
  * scene augmentation (rotation / scaling / flip, ``losses.scene_augmentation``) and the evaluation
    pass of ``Trainer.eval_epoch_rpn`` (``evaluate``: loss, point precision, centre recall);
  * the ground-truth paste augmentation (GT_AUG_ENABLED of weaklyRPN.yaml; kitti_rcnn_dataset.py:257-371, 404-414, 463-467) with
    ``--gt_aug PATH [--gt_aug_prob P]``: up to 15 objects of the database ``python -m ws3d_amd.gt_database`` writes are pasted into
    every training scene before it is filtered and sub-sampled, and their centres join the labels (``gt_paste``; host only, it runs
    in the loader processes).  What is drawn per scene is the reference's; what is STORED is the 100-point subset of the "mimic
    hard" objects, sampled once on the device when the database is built instead of once per draw -- the one place the scenes can
    differ from the reference's in bits (``gt_paste`` docstring).  ``--synthetic N --gt_aug synthetic`` builds a database in memory
    from ray-cast scenes, with easy_min_points lowered to 128 (about one ray-cast car in fifty exceeds the reference's 512 points).
    Off by default: no flag, no paste.  The paste, the re-sampling and the labels of the added centres are host work per scene:
    give --workers (measured at batch 8: 15 -> 51 ms/it without loader processes, 15 -> 17 ms/it with four; profiles/gt_paste.txt).
Not reproduced: tensorboard.  ``--mgpus`` maps to one process per GPU
(``torchrun``, DistributedDataParallel over RCCL) instead of ``nn.DataParallel``.
"""
from __future__ import annotations

import argparse
import logging
import math
import os
import random
import time
from dataclasses import dataclass
from typing import Iterator, Optional

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils import clip_grad_norm_

from . import gt_paste, kitti_io, loader, losses, pn2_ops, stage1


@dataclass(frozen=True)
class TrainConfig:
    """TRAIN block of tools/cfgs/weaklyRPN.yaml:69-96"""
    lr: float = 0.002
    weight_decay: float = 0.001
    moms: tuple = (0.95, 0.85)
    div_factor: float = 10.0
    pct_start: float = 0.4
    grad_norm_clip: float = 1.0
    bn_momentum: float = 0.1
    bn_decay: float = 0.5
    bnm_clip: float = 0.01
    bn_decay_step_list: tuple = (1000,)


# ----------------------------------------------------------------------------- schedules
def annealing_cos(start: float, end: float, pct: float) -> float:
    return end + (start - end) / 2 * (math.cos(math.pi * pct) + 1)


def one_cycle(step: int, total_step: int, lr_max: float, moms=(0.95, 0.85), div_factor: float = 10.0,
              pct_start: float = 0.4):
    """(lr, momentum) at iteration `step` (learning_schedules_fastai.py:40-77): cosine from
    lr_max/div_factor up to lr_max over the first pct_start of training, then down to 2e-6;
    momentum mirrors it between moms[0] and moms[1]"""
    a1 = int(pct_start * total_step)
    low = lr_max / div_factor
    if step >= a1:
        pct = (step - a1) / (total_step - a1)
        return annealing_cos(lr_max, 2e-6, pct), annealing_cos(moms[1], moms[0], pct)
    pct = step / a1
    return annealing_cos(low, lr_max, pct), annealing_cos(moms[0], moms[1], pct)


def bn_momentum_at(it: int, cfg: TrainConfig) -> float:
    decay = 1.0
    for s in cfg.bn_decay_step_list:
        if it >= s:
            decay *= cfg.bn_decay
    return max(cfg.bn_momentum * decay, cfg.bnm_clip)


def set_bn_momentum(model: nn.Module, momentum: float) -> None:
    """(the walk over ~400 modules is skipped while the value does not change: it changes at the
    few BN_DECAY steps only, and the step is launch-bound on the host)"""
    cache = model.__dict__.get("_ws3d_bn_momentum")
    if cache is not None and cache[0] == momentum and all(m.momentum == momentum for m in cache[1][:1]):
        return
    norms = [m for m in model.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d))]
    for m in norms:
        m.momentum = momentum
    model.__dict__["_ws3d_bn_momentum"] = (momentum, norms)


class AdamOneCycle:
    """Adam + decoupled weight decay + per-iteration one-cycle schedule (see module docstring)"""

    def __init__(self, params, total_step: int, cfg: TrainConfig = TrainConfig()):
        self.cfg, self.total_step = cfg, total_step
        self.opt = torch.optim.Adam([p for p in params if p.requires_grad], lr=cfg.lr / cfg.div_factor,
                                    betas=(cfg.moms[0], 0.99))
        self.lr, self.mom = cfg.lr / cfg.div_factor, cfg.moms[0]

    def schedule(self, it: int) -> None:
        self.lr, self.mom = one_cycle(it, self.total_step, self.cfg.lr, self.cfg.moms, self.cfg.div_factor, self.cfg.pct_start)
        for g in self.opt.param_groups:
            g["lr"] = self.lr
            g["betas"] = (self.mom, g["betas"][1])

    def zero_grad(self) -> None:
        self.opt.zero_grad(set_to_none=True)

    @torch.no_grad()
    def step(self) -> None:
        for g in self.opt.param_groups:     # decoupled weight decay, one multi-tensor launch per group
            torch._foreach_mul_([p for p in g["params"]], 1 - self.cfg.weight_decay * g["lr"])
        self.opt.step()

    def state_dict(self):
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd)


# ----------------------------------------------------------------------------- checkpoints
def checkpoint_state(model: Optional[nn.Module] = None, optimizer=None, it=None) -> dict:
    if isinstance(model, (nn.DataParallel, nn.parallel.DistributedDataParallel)):
        model = model.module
    return {"it": it, "model_state": None if model is None else model.state_dict(),
            "optimizer_state": None if optimizer is None else optimizer.state_dict()}


def save_checkpoint(state: dict, filename: str = "checkpoint") -> str:
    path = "{}.pth".format(filename)
    torch.save(state, path)
    return path


def load_checkpoint(model: Optional[nn.Module] = None, optimizer=None, filename: str = "checkpoint", logger=None):
    """-> (it, epoch).  ``model_state`` interchanges with the reference's train_utils.save_checkpoint (same keys).
    ``optimizer_state`` interchanges only between runs of THIS trainer: the reference's comes from fastai's OptimWrapper
    (two parameter groups from split_bn_bias), AdamOneCycle has one -- such a state is skipped with a warning and the
    optimizer starts fresh at iteration ``it`` of the one-cycle schedule."""
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    ck = torch.load(filename, map_location="cpu")
    if model is not None and ck.get("model_state") is not None:
        model.load_state_dict(ck["model_state"])
    if optimizer is not None and ck.get("optimizer_state") is not None:
        state = ck["optimizer_state"]
        ours = optimizer.state_dict()
        same = (isinstance(state, dict) and "param_groups" in state and len(state["param_groups"]) == len(ours["param_groups"])
                and [len(g["params"]) for g in state["param_groups"]] == [len(g["params"]) for g in ours["param_groups"]])
        if same:
            optimizer.load_state_dict(state)
        else:
            import warnings
            warnings.warn("load_checkpoint: optimizer_state of '%s' has another parameter-group layout (e.g. written by the "
                          "reference's OptimWrapper); it is skipped, only model_state and `it` are restored" % filename)
    if logger:
        logger.info("==> loaded checkpoint '%s' (it %s)", filename, ck.get("it"))
    return ck.get("it", 0), ck.get("epoch", -1)


# ----------------------------------------------------------------------------- data
class _PasteStreams:
    """the two random streams of the ground-truth paste: the dataset's numpy stream and a ``random.Random`` seeded from it on first
    use IN THIS PROCESS (a forked loader process re-seeds the numpy stream, ``loader._init``, and so gets its own)"""
    _pyrng = None

    def _paste_pyrng(self, rng):
        if self._pyrng is None or self._pyrng[0] != os.getpid():
            self._pyrng = (os.getpid(), random.Random(int(rng.randint(0, 2 ** 31 - 1))))
        return self._pyrng[1]


class SyntheticCenters(_PasteStreams):
    """`count` seeded KITTI-shaped scenes with car-centre annotations (the weak labels of WS3D are
    BEV centre clicks): {'pts_input' (N,4), 'gt_centers' (K,3), 'rpn_cls_label', 'rpn_reg_label'}.
    labels=False: the two label entries are left out and not computed (they are made on the device, ``train(device_targets=True)``);
    scenes, augmentation and the draws from `rng` are the same either way.
    gt_database (a ``gt_database.GtDatabase``): with probability gt_aug_prob the objects of one ``gt_paste`` draw are pasted into the
    scene cloud, which is then sub-sampled back to npoints like a scan (``kitti_io.sample_point_choice`` on z), and their centres join
    'gt_centers'.  None (the default): nothing is drawn, nothing changes."""

    def __init__(self, count: int, npoints: int = 16384, config_id: int = 8, augment: bool = False, rng=np.random, labels: bool = True,
                 gt_database=None, gt_aug_prob: float = 1.0):
        from . import synth
        self.synth, self.count, self.npoints, self.config_id = synth, count, npoints, config_id
        self.augment, self.rng, self.labels = augment, rng, labels
        self.gt_database, self.gt_aug_prob = gt_database, gt_aug_prob
        self._scenes, self._items = {}, {}   # generated scans (and, without augmentation, their labels) are kept

    def __len__(self):
        return self.count

    def __getitem__(self, i: int) -> dict:
        fixed = not self.augment and self.gt_database is None
        if fixed and i in self._items:
            return self._items[i]
        if i not in self._scenes:
            seed = 1000 * self.config_id + i
            self._scenes[i] = (self.synth.lidar_cloud(self.npoints, seed),
                               self.synth.random_boxes3d(15, seed * 7919 + 13)[:, :3].astype(np.float32))
        pc, centres = self._scenes[i]
        if self.gt_database is not None and self.rng.rand() < self.gt_aug_prob:
            keep, obj_pts, obj_int, extra = gt_paste.plan_paste(pc[:, :3], centres, self.gt_database, self.rng, self._paste_pyrng(self.rng))
            if keep is not None:        # the scene cloud carries intensity - 0.5, the database the raw value
                pasted = np.concatenate((np.concatenate(obj_pts), np.concatenate(obj_int).reshape(-1, 1) - 0.5), axis=1)
                pc = np.concatenate((pc[keep], pasted.astype(np.float32)), axis=0)
                pc = pc[kitti_io.sample_point_choice(pc[:, 2], self.npoints, self.rng)]
                centres = np.concatenate((centres, extra), axis=0)
        if self.augment:   # AUG_DATA (rotation / scaling / flip), like the reference's TRAIN loader
            xyz, centres, _ = losses.scene_augmentation(pc[:, :3], centres, self.rng)
            pc = np.concatenate((xyz.astype(np.float32), pc[:, 3:]), axis=1)
            centres = centres.astype(np.float32)
        item = {"sample_id": i, "pts_input": pc, "gt_centers": centres}
        if self.labels:
            cls, reg = losses.gaussian_center_labels(pc[:, :3], centres)
            item.update({"rpn_cls_label": cls.astype(np.float32), "rpn_reg_label": reg})
        if fixed:
            self._items[i] = item
        return item


class KittiCenters(_PasteStreams):
    """KITTI directory: scans through ``kitti_io`` (no augmentation), centre annotations from
    label_2 (``noise_kind`` selects another label directory like the reference's --noise_kind), the
    first ``weakly_num`` scenes that contain a Car/Van.  labels=False: items carry 'pts_input' and 'gt_centers' only (see
    SyntheticCenters).
    gt_database (a ``gt_database.GtDatabase``; GT_AUG_ENABLED): like the reference's get_rpn_sample, ``rng.rand() < gt_aug_prob``
    is drawn per scene and one ``gt_paste.paste_scene`` goes in between the projection to the camera frame and the validity filter;
    the pasted centres are appended to the scene's own before the scene augmentation and the labels.  None: untouched."""

    def __init__(self, root: str, split: str = "train", npoints: int = 16384, noise_kind: Optional[str] = None,
                 weakly_num: int = 500, rng=np.random, augment: bool = False, labels: bool = True, gt_database=None,
                 gt_aug_prob: float = 1.0):
        self.augment, self.labels = augment, labels
        self.gt_database, self.gt_aug_prob = gt_database, gt_aug_prob
        self.scenes = kitti_io.KittiScenes(root, split, npoints=npoints, rng=rng)
        self.label_sub = noise_kind or "label_2"
        keep = []
        for sid in self.scenes.sample_id_list:
            if self._objects(sid):
                keep.append(sid)
            if len(keep) >= weakly_num:
                break
        self.ids = keep

    def _objects(self, sid):
        """Car / Van objects inside PC_AREA_SCOPE: the reference's TRAIN-mode filtrate_objects (kitti_rcnn_dataset.py:
        115-135: class whitelist incl. Van, then check_pc_range on obj.pos) -- applied BEFORE the 'scene has an object'
        test and before the centres become labels, so the weakly_num subset and the labels match the reference's"""
        path = os.path.join(self.scenes.imageset_dir, self.label_sub, "%06d.txt" % sid)
        objs = kitti_io.read_label_file(path) if os.path.isfile(path) else []
        (x0, x1), (y0, y1), (z0, z1) = kitti_io.PC_AREA_SCOPE
        return [o for o in objs if o.cls_type in ("Car", "Van")
                and x0 <= o.pos[0] <= x1 and y0 <= o.pos[1] <= y1 and z0 <= o.pos[2] <= z1]

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i: int) -> dict:
        sid = self.ids[i]
        centres = np.array([o.pos for o in self._objects(sid)], dtype=np.float32).reshape(-1, 3)
        paste, extra = None, []
        if self.gt_database is not None:
            rng = self.scenes.rng

            def paste(pts_rect, intensity):
                if rng.rand() < self.gt_aug_prob:
                    pts_rect, intensity, added = gt_paste.paste_scene(pts_rect, intensity, centres, self.gt_database, rng,
                                                                      self._paste_pyrng(rng))
                    extra.append(added)
                return pts_rect, intensity
        pts = kitti_io.rpn_input_from_scan(self.scenes.get_lidar(sid), self.scenes.get_calib(sid),
                                           self.scenes.get_image_shape(sid), self.scenes.npoints, True, self.scenes.rng, paste=paste)
        if extra:
            centres = np.concatenate((centres, extra[0]), axis=0)
        if self.augment:
            xyz, centres, _ = losses.scene_augmentation(pts[:, :3], centres, self.scenes.rng)
            pts = np.concatenate((xyz, pts[:, 3:]), axis=1)
            centres = centres.astype(np.float32)
        item = {"sample_id": sid, "pts_input": pts.astype(np.float32), "gt_centers": centres}
        if self.labels:
            cls, reg = losses.gaussian_center_labels(pts[:, :3], centres)
            item.update({"rpn_cls_label": cls.astype(np.float32), "rpn_reg_label": reg})
        return item


def _collate(items) -> dict:
    return {"pts_input": np.stack([s["pts_input"] for s in items]).astype(np.float32),
            "rpn_cls_label": np.stack([s["rpn_cls_label"] for s in items]),
            "rpn_reg_label": np.stack([s["rpn_reg_label"] for s in items]),
            "sample_id": [s["sample_id"] for s in items]}


def _collate_centers(items) -> dict:
    """the batch of the device-target route: scenes and their annotated centres, no labels.  'gt_centers' (B,Kmax,3) is padded with
    zeros behind each scene's 'gt_count' (B,) int32 centres (Kmax = the batch's largest count, 0 when no scene has one); label entries
    an item may carry are dropped"""
    count = np.array([np.asarray(s["gt_centers"]).reshape(-1, 3).shape[0] for s in items], dtype=np.int32)
    centres = np.zeros((len(items), int(count.max()) if len(items) else 0, 3), dtype=np.float32)
    for b, s in enumerate(items):
        centres[b, :count[b]] = np.asarray(s["gt_centers"], dtype=np.float32).reshape(-1, 3)
    return {"pts_input": np.stack([s["pts_input"] for s in items]).astype(np.float32), "gt_centers": centres, "gt_count": count,
            "sample_id": [s["sample_id"] for s in items]}


def device_labels(batch: dict, device) -> dict:
    """a ``_collate_centers`` batch -> {'pts_input', 'rpn_cls_label', 'rpn_reg_label'} tensors on `device`: scenes, centres and counts go
    up, the labels are made there (``losses.center_labels_batch``: one HIP launch on the current stream; numpy on a CPU device)"""
    pts = torch.from_numpy(np.ascontiguousarray(batch["pts_input"], dtype=np.float32)).to(device)
    centres = torch.from_numpy(np.ascontiguousarray(batch["gt_centers"], dtype=np.float32)).to(device)
    count = torch.from_numpy(np.ascontiguousarray(batch["gt_count"], dtype=np.int32)).to(device)
    cls, reg = losses.center_labels_batch(pts, centres, count)
    return {"pts_input": pts, "rpn_cls_label": cls, "rpn_reg_label": reg}


def batches(dataset, batch_size: int, rng: np.random.RandomState, rank: int = 0, world: int = 1, workers: int = 0,
            ahead: int = 3, collate=_collate) -> Iterator[dict]:
    """endless shuffled mini-batches (drop_last, like the reference's DataLoader); with world > 1
    every rank takes its own slice of each global batch.  workers > 0 (the reference's --workers):
    the scenes of the next `ahead` batches are read / sampled / labelled by that many forked
    processes -- same batch composition and order as workers = 0; scenes whose preparation draws
    random numbers (the 16384-point sampler, augmentation) then use per-process streams."""
    n = len(dataset)
    if n < batch_size * world:
        raise ValueError(f"{n} scenes < global batch {batch_size * world}")

    def id_batches():
        while True:
            order = rng.permutation(n)
            for i0 in range(0, n - batch_size * world + 1, batch_size * world):
                yield [int(i) for i in order[i0 + rank * batch_size:i0 + (rank + 1) * batch_size]]

    worker_seed = int(rng.get_state()[1][0]) % (2 ** 31)      # derived without drawing: the batch order must not depend on `workers`
    for items in loader.item_batches(dataset, id_batches(), workers, ahead, seed=worker_seed):
        yield collate(items)


class DevicePrefetcher:
    """Keeps one mini-batch ahead of the training step, on a side HIP stream.

    ``advance()`` takes the next host batch from `source`, uploads it on the side stream and runs the
    backbone's furthest-point-sampling chain there (``pointnet2_utils.sampling_plan``).  FPS is the one long serial kernel of the step -- 4095
    dependent rounds, one workgroup per scene, 5.5 ms at batch 8 with 8 of 256 CUs busy -- and it
    needs nothing but the input coordinates, so it runs beside the previous step's backward GEMM /
    BN kernels instead of heading the critical path.  ``train_step`` calls ``advance`` right after
    it has enqueued the backward pass (the host is otherwise idle until the gradient norm is read
    back), so building the next batch on the host overlaps device work too.  Everything happens on
    the calling thread: a worker thread was measured 30 % SLOWER than no prefetching at all (it
    competes with the kernel-launching thread for the interpreter lock).
    ``next()`` yields dicts of DEVICE tensors: ``pts_input``, ``rpn_cls_label`` / ``rpn_reg_label``
    (float32), ``sampling_plan``, plus ``sample_id``; the current stream is made to wait for the
    upload + sampling first.  A source batch without labels (``_collate_centers``: 'gt_centers' +
    'gt_count') gets them here: centres and counts are uploaded and ``device_labels`` makes the labels on
    the side stream, next to the sampling plan -- the same two entries come out."""

    KEYS = ("pts_input", "rpn_cls_label", "rpn_reg_label")

    def __init__(self, source: Iterator[dict], device, npoints):
        self.source, self.device, self.npoints = iter(source), torch.device(device), tuple(npoints)
        self.side = torch.cuda.Stream(device=self.device)
        self.pending = None                # (batch, ready event) | exception raised by the source
        self.timing = None                 # set to a list to collect (start, end) HIP events of the sampling chain

    def advance(self) -> None:
        """start the next batch (no-op if one is already pending)"""
        if self.pending is not None:
            return
        try:
            batch = next(self.source)
        except BaseException as exc:       # StopIteration included: re-raised by __next__
            self.pending = exc
            return
        with torch.no_grad(), torch.cuda.stream(self.side):
            out = {"sample_id": batch.get("sample_id")}
            if "rpn_cls_label" not in batch:
                out.update(device_labels(batch, self.device))
            else:
                for key in self.KEYS:
                    # plain pageable upload: staging through pinned buffers + non_blocking copies was measured
                    # slower here (36 vs 23 ms per iteration at batch 8)
                    out[key] = torch.from_numpy(np.ascontiguousarray(batch[key], dtype=np.float32)).to(self.device)
            xyz = out["pts_input"][..., 0:3].contiguous()
            if self.timing is not None:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(self.side)
            out["sampling_plan"] = pn2_ops.sampling_plan(xyz, self.npoints)
            if self.timing is not None:
                t1.record(self.side)
                self.timing.append((t0, t1))
            ready = torch.cuda.Event()
            ready.record(self.side)
        self.pending = (out, ready)

    def __iter__(self):
        return self

    def __next__(self) -> dict:
        self.advance()
        pending, self.pending = self.pending, None
        if isinstance(pending, BaseException):
            raise pending
        out, ready = pending
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ready)
        for v in list(out.values()) + list(out["sampling_plan"]):
            if torch.is_tensor(v):
                v.record_stream(cur)          # allocated on the side stream, consumed on this one
        return out

    def close(self):
        self.pending = None


def _on_device(x, device) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.from_numpy(x)
    return t.to(device).float()


# ----------------------------------------------------------------------------- training
def train_step(model: nn.Module, optimizer: AdamOneCycle, batch: dict, it: int, net_cfg: stage1.RPNConfig,
               train_cfg: TrainConfig, device, overlap=None, fused_loss: bool = False) -> dict:
    """one iteration of Trainer._train_it (train_utils.py:137-147) with the per-iteration schedules.
    overlap: host work to do once the backward pass is enqueued (DevicePrefetcher.advance)
    fused_loss: ``losses.rpn_loss_fused`` (value and gradient from fused HIP, no read-back in the middle of the step) instead of
    ``losses.rpn_loss``; a batch that carries centres instead of labels gets its labels on the device first"""
    set_bn_momentum(model, bn_momentum_at(it, train_cfg))
    optimizer.schedule(it)
    if not model.training:
        model.train()
    optimizer.zero_grad()
    if "rpn_cls_label" not in batch:
        batch = {**batch, **device_labels(batch, device)}
    inputs = {"pts_input": _on_device(batch["pts_input"], device)}
    if batch.get("sampling_plan") is not None:
        inputs["sampling_plan"] = batch["sampling_plan"]
    out = model(inputs)
    if fused_loss:
        loss, tb = losses.rpn_loss_fused(out["rpn_cls"], out["rpn_reg"], _on_device(batch["rpn_cls_label"], device),
                                         _on_device(batch["rpn_reg_label"], device), net_cfg.loc_scope, net_cfg.loc_bin_size)
    else:
        loss, tb = losses.rpn_loss(out["rpn_cls"], out["rpn_reg"], _on_device(batch["rpn_cls_label"], device),
                                   _on_device(batch["rpn_reg_label"], device), net_cfg.loc_scope, net_cfg.loc_bin_size, lazy=True)
    loss.backward()
    if overlap is not None:
        overlap()
    tb["grad_norm"] = clip_grad_norm_(model.parameters(), train_cfg.grad_norm_clip)    # stays on the device ...
    optimizer.step()
    tb["loss"] = loss
    losses.resolve_scalars(tb)                       # ... the step's scalars are read back once, at its end
    tb["lr"] = optimizer.lr
    return tb


@torch.no_grad()
def evaluate(model: nn.Module, dataset, net_cfg: stage1.RPNConfig = stage1.DEFAULT_CFG, device="cuda:0",
             max_scenes: Optional[int] = None) -> dict:
    """Trainer.eval_epoch_rpn (train_utils.py:149-249), batch size 1 like the reference: mean loss,
    point precision = P(label > 0.3 | sigmoid(cls) > 0.3), centre recall = annotated centres with a
    decoded foreground centre within 1.4 m (BEV), and the mean BEV offset of matched predictions."""
    dev = torch.device(device)
    was_training = model.training
    model.eval()
    tot_loss, n, pt_hit, pt_fg, gt_hit, gt_cnt, offs = 0.0, 0, 0.0, 0.0, 0, 0, []
    for i in range(len(dataset) if max_scenes is None else min(max_scenes, len(dataset))):
        s = dataset[i]
        if "rpn_cls_label" not in s:          # a labels=False dataset
            cls, reg = losses.gaussian_center_labels(s["pts_input"][:, :3], np.asarray(s["gt_centers"], dtype=np.float32).reshape(-1, 3))
            s = {**s, "rpn_cls_label": cls.astype(np.float32), "rpn_reg_label": reg}
        pts = torch.from_numpy(s["pts_input"][None].astype(np.float32)).to(dev)
        out = model({"pts_input": pts})
        label = torch.from_numpy(s["rpn_cls_label"][None]).to(dev).float()
        loss, _ = losses.rpn_loss(out["rpn_cls"], out["rpn_reg"], label, torch.from_numpy(s["rpn_reg_label"][None]).to(dev).float(),
                                  net_cfg.loc_scope, net_cfg.loc_bin_size)
        tot_loss += float(loss.item()); n += 1
        score = torch.sigmoid(out["rpn_cls"]).view(-1)
        fg = score > 0.3
        pt_hit += float((fg & (label.view(-1) > 0.3)).sum()); pt_fg += float(fg.sum())
        gt = torch.from_numpy(np.asarray(s["gt_centers"], dtype=np.float32).reshape(-1, 3)).to(dev)
        if int(fg.sum()) and gt.shape[0]:
            xyz = pts[0, :, :3][fg]
            pred = stage1.decode_center_target(torch.zeros_like(xyz), out["rpn_reg"][0][fg], net_cfg.loc_scope,
                                               net_cfg.loc_bin_size) + xyz
            d = torch.cdist(pred[:, [0, 2]], gt[:, [0, 2]])                  # (P, K)
            dmin, arg = d.min(dim=1)
            gt_hit += len(set(arg[dmin < 1.4].tolist())); gt_cnt += gt.shape[0]
            if bool((dmin < 2.0).any()):
                offs.append(dmin[dmin < 2.0])
    if was_training:
        model.train()
    return {"val_loss": tot_loss / max(n, 1), "point_precision": pt_hit / max(pt_fg, 1.0),
            "gt_recall": gt_hit / max(gt_cnt, 1), "mean_offset": float(torch.cat(offs).mean()) if offs else float("nan")}


def train(dataset, total_iters: int, batch_size: int, output_dir: Optional[str] = None, ckpt: Optional[str] = None,
          pretrain_ckpt: Optional[str] = None, ckpt_save_interval: int = 20, seed: int = 0, device: str = "cuda:0",
          net_cfg: stage1.RPNConfig = stage1.DEFAULT_CFG, train_cfg: TrainConfig = TrainConfig(), logger=None,
          distributed: bool = False, prefetch: bool = True, workers: int = 0, device_targets: bool = False) -> dict:
    """-> {'model', 'optimizer', 'it', 'history' (loss per iteration), 'checkpoints'}
    prefetch: build / upload the next batch and run its furthest point sampling on a side stream
    while the current step computes (DevicePrefetcher); same losses either way.
    device_targets: scenes and centres go up instead of labels (``_collate_centers``; give a ``labels=False`` dataset to skip the host
    label computation), the labels are made on the device -- by the prefetcher on its side stream, inside the step without one -- and
    the loss is ``losses.rpn_loss_fused``.  Off by default: the host route of the reference."""
    log = logger or logging.getLogger("ws3d_amd.train_rpn")
    rank, world = 0, 1
    if distributed:
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
    torch.manual_seed(seed)
    dev = torch.device(device)
    model = stage1.Stage1Net(mode="TRAIN", cfg=net_cfg).to(dev)
    optimizer = AdamOneCycle(model.parameters(), total_iters, train_cfg)
    it = 0
    if pretrain_ckpt:
        load_checkpoint(model, None, pretrain_ckpt, log)
        it = int(total_iters * 9 / 30)                   # train_rpn.py:186
    if ckpt:
        it, _ = load_checkpoint(model, optimizer, ckpt, log)
        it = int(it)
    net = nn.parallel.DistributedDataParallel(model, device_ids=[dev.index]) if distributed else model
    ckpt_dir = os.path.join(output_dir, "ckpt") if output_dir else None
    if ckpt_dir and rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    per_epoch = max(len(dataset) // (batch_size * world), 1)
    n_epochs = max(int(total_iters / per_epoch), 1)
    save_every = max(int(n_epochs / min(n_epochs, ckpt_save_interval)), 1) * per_epoch
    source = batches(dataset, batch_size, np.random.RandomState(seed), rank, world, workers=workers,
                     collate=_collate_centers if device_targets else _collate)
    stream = DevicePrefetcher(source, dev, net_cfg.npoints) if prefetch and dev.type == "cuda" else source
    history, saved = [], []
    try:
        return _train_loop(net, model, optimizer, stream, it, total_iters, net_cfg, train_cfg, dev, rank, log, ckpt_dir,
                           save_every, history, saved, fused_loss=device_targets)
    finally:
        if isinstance(stream, DevicePrefetcher):
            stream.close()
        source.close()                      # stops the loader processes


def _train_loop(net, model, optimizer, stream, it, total_iters, net_cfg, train_cfg, dev, rank, log, ckpt_dir, save_every,
                history, saved, fused_loss: bool = False) -> dict:
    t_mark, it_mark, step_ms = time.perf_counter(), it, []
    while it < total_iters:
        ahead = stream.advance if isinstance(stream, DevicePrefetcher) and it + 1 < total_iters else None
        tb = train_step(net, optimizer, next(stream), it, net_cfg, train_cfg, dev, overlap=ahead, fused_loss=fused_loss)
        it += 1
        history.append(tb["loss"])
        if rank == 0 and (it % 10 == 0 or it == total_iters):
            now = time.perf_counter()            # train_step ends on loss.item(): the device is idle here
            step_ms.append((now - t_mark) * 1e3 / max(it - it_mark, 1))
            t_mark, it_mark = now, it
            log.info("it %5d  loss %.4f  cls %.4f  reg %.4f  fg %d  lr %.2e  %.1f ms/it", it, tb["loss"], tb["rpn_loss_cls"],
                     tb["rpn_loss_reg"], tb["rpn_fg_sum"], tb["lr"], step_ms[-1])
        if ckpt_dir and rank == 0 and (it % save_every == 0 or it == total_iters):
            saved.append(save_checkpoint(checkpoint_state(model, optimizer, it),
                                         os.path.join(ckpt_dir, "checkpoint_iter_%05d" % it)))
    return {"model": model, "optimizer": optimizer, "it": it, "history": history, "checkpoints": saved,
            "step_ms": step_ms}


def synthetic_gt_database(log=None, scenes: int = 8):
    """a paste database built in memory from `scenes` ray-cast scenes.  Only about one ray-cast car in fifty exceeds the reference's
    512 points, too few to draw 10 easy objects from, so this route lowers easy_min_points to 128 (and says so)"""
    from . import gt_database as gdb
    records = gdb.build_gt_database(gdb.synthetic_scenes(scenes), easy_min_points=gdb.SYNTHETIC_EASY_MIN_POINTS)
    db = gdb.GtDatabase(records)
    if log:
        log.info("synthetic gt database from %d ray-cast scenes: %d easy (more than %d points, NOT the reference's 512), %d hard",
                 scenes, len(db.easy), gdb.SYNTHETIC_EASY_MIN_POINTS, len(db.hard))
    return db


def _load_gt_aug(path, last_sample_id):
    if not path:
        return None
    from . import gt_database as gdb
    return gdb.load_gt_database(path, last_sample_id)


def main():
    ap = argparse.ArgumentParser(description="Stage-1 RPN trainer (flags of the reference's tools/train_rpn.py)")
    ap.add_argument("--cfg_file", type=str, default="cfgs/", help="accepted for compatibility; weaklyRPN values are built in")
    ap.add_argument("--batch_size", type=int, default=25)
    ap.add_argument("--total_iters", type=int, default=8000)
    ap.add_argument("--ckpt_save_interval", type=int, default=20)
    ap.add_argument("--workers", type=int, default=0, help="loader processes preparing the next batches (0: in the training process)")
    ap.add_argument("--output_dir", type=str, default=None)
    ap.add_argument("--mgpus", action="store_true", default=False, help="one process per GPU under torchrun (DDP over RCCL)")
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--pretrain_ckpt", type=str, default=None)
    ap.add_argument("--noise_kind", type=str, default="label_noise")
    ap.add_argument("--weakly_num", type=int, default=500)
    ap.add_argument("--data_root", type=str, default=None, help="KITTI object directory (ImageSets/, training/)")
    ap.add_argument("--no_prefetch", action="store_true", default=False,
                    help="build / upload / sample the next batch inside the step instead of one step ahead")
    ap.add_argument("--synthetic", type=int, default=0, help="train on this many seeded synthetic scenes instead")
    ap.add_argument("--device_targets", action="store_true", default=False,
                    help="upload scenes and centres, make the labels on the device and take the loss from fused HIP (off: labels on the host)")
    ap.add_argument("--gt_aug", type=str, default=None,
                    help="ground-truth paste augmentation: the database written by `python -m ws3d_amd.gt_database`, or 'synthetic' "
                         "(with --synthetic: built in memory from ray-cast scenes).  Off without the flag")
    ap.add_argument("--gt_aug_prob", type=float, default=1.0, help="GT_AUG_APPLY_PROB: share of the scenes that get a paste")
    a = ap.parse_args()
    logging.basicConfig(level=logging.INFO, format="%(asctime)s  %(levelname)5s  %(message)s")
    out_dir = a.output_dir or os.path.join("output", "rpn", "weaklyRPN")
    distributed = a.mgpus and int(os.environ.get("WORLD_SIZE", "1")) > 1
    local = 0
    if distributed:
        from . import dist as wdist
        _, _, local = wdist.init()
    if a.synthetic:
        db = synthetic_gt_database(logging.getLogger("ws3d_amd.train_rpn")) if a.gt_aug == "synthetic" else _load_gt_aug(a.gt_aug, None)
        ds = SyntheticCenters(a.synthetic, labels=not a.device_targets, gt_database=db, gt_aug_prob=a.gt_aug_prob)
    elif a.data_root:
        label_dir = a.noise_kind if os.path.isdir(os.path.join(a.data_root, "training", a.noise_kind)) else None
        ds = KittiCenters(a.data_root, "train", noise_kind=label_dir, weakly_num=a.weakly_num, labels=not a.device_targets,
                          gt_aug_prob=a.gt_aug_prob)
        if a.gt_aug:                        # the reader's filter: objects of the scans up to the last training scene (:78)
            ds.gt_database = _load_gt_aug(a.gt_aug, ds.ids[-1] if ds.ids else None)
    else:
        ap.error("give --data_root or --synthetic N")
    res = train(ds, a.total_iters, a.batch_size, out_dir, a.ckpt, a.pretrain_ckpt, a.ckpt_save_interval,
                device=f"cuda:{local}", distributed=distributed, prefetch=not a.no_prefetch, workers=a.workers,
                device_targets=a.device_targets)
    if int(os.environ.get("RANK", "0")) == 0:
        logging.getLogger("ws3d_amd.train_rpn").info("done: it %d, last checkpoint %s, median %.1f ms/it", res["it"],
                                                     res["checkpoints"][-1] if res["checkpoints"] else None,
                                                     float(np.median(res["step_ms"])) if res["step_ms"] else float("nan"))


if __name__ == "__main__":
    main()
