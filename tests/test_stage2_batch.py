"""CPU tests of ws3d_amd/stage2_batch.py: the numpy twin of csrc/stage2_batch.hip IS the existing chain ``BoxDataset.sample`` ->
``collate`` -> ``prepare_batch``, bit for bit, once the twin's draws are replayed into ``sample`` through a scripted random stream.

The cases (CASES below; every one runs in phase rcnn and in phase ioun with two cascade stages, and the records again in EVAL mode):

    record (rows, kind)       aug_flag  steering of the scalar draws                          branch
    R1    (1, foreground)       0..3    -                                                      kept count 1; a 1-row record
    R2    (2, background)       0..3    -                                                      kept count 2; fall-back (no gt_mask > 0 at all)
    R511  (511, foreground)     1       drop[3] = 0.8                                          kept 511: no cut although drop[3] asks
    R512  (512, foreground)     0       drop off, drop[3] = 0                                  kept 512, no cut; aug_flag 0
    R512                        1       drop[3] = 0.6, x flip on                               the 128 cut
    R512                        2       drop[3] = 0.8, x flip off                              the 32 cut
    R513  (513, background)     3       drop[3] = 0.6                                          kept 513 -> 512 -> the 128 cut
    R600  (600, foreground)     0       drop on: x >, z <, OR, with the drop[4] clause         drop-out
    R600                        3       drop on: x <, z >, AND, without it                     drop-out
    R4200 (4200, foreground)    1       drop on: x >, z >, OR, without it; x flip on           drop-out on a record of >= 4096 rows
    R4200                       2       drop on: x <, z <, AND, with it, drop[3] = 0.6         drop-out, then the 128 cut
    RFB   (40, foreground,      1       drop on, AND, without the drop[4] clause               the rule keeps flipped rows only, none with
           prob <= 0.5, all in the box)                                                        gt_mask > 0: fall-back to all rows
    every record                0..3    none (seeded draws)                                    whatever the seeds give
"""
import os

import numpy as np
import pytest
import torch

from ws3d_amd import stage2_batch as sb
from ws3d_amd import train_rcnn as t2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"R1": 1, "R2": 2, "R511": 511, "R512": 512, "R513": 513, "R600": 600, "R4200": 4200, "RFB": 40}
NAMES = list(SIZES)
FOREGROUND = {"R1": True, "R2": False, "R511": True, "R512": True, "R513": False, "R600": True, "R4200": True, "RFB": True}


def make_records():
    """small hand-made records in gen_box_dataset's format, every number a float32 number"""
    g = np.random.Generator(np.random.PCG64(2024))
    recs = []
    for i, name in enumerate(NAMES):
        n, fg = SIZES[name], FOREGROUND[name]
        box = np.array([[g.uniform(-0.5, 0.5), 1.65 + g.uniform(-0.2, 0.2), g.uniform(-0.5, 0.5), 1.5, 1.6, 3.9, g.uniform(-3, 3)]], dtype=np.float32)
        pts = (g.uniform(-2.5, 2.5, (n, 3)) + box[0, 0:3]).astype(np.float32)
        prob = g.uniform(0, 1, (n, 1)).astype(np.float32)
        inside = (g.uniform(0, 1, (n, 1)) < 0.6).astype(np.float32)
        if name == "RFB":
            prob, inside = np.full((n, 1), 0.25, dtype=np.float32), np.ones((n, 1), dtype=np.float32)
        recs.append({"sample_id": 100 + i, "box_id": i % 3 if fg else -1, "center": np.zeros((1, 3), dtype=np.float32), "foreground_flag": fg,
                     "gt_boxes": box if fg else np.zeros((1, 7), dtype=np.float32), "cur_box_point": pts,
                     "cur_box_reflect": g.uniform(0, 1, (n, 1)).astype(np.float32), "cur_prob_mask": prob,
                     "gt_mask": inside if fg else np.zeros((n, 1), dtype=np.float32)})
    return recs


def drop6(on, x_gt=True, z_gt=True, use_or=True, neg=False, cut=0.0):
    return np.array([0.9 if on else 0.0, 0.5 if x_gt else -0.5, 0.9 if z_gt else 0.0, cut, 0.9 if neg else 0.0, 0.5 if use_or else -0.5])


NOISE_FLIP = np.array([0.3, -0.2, 0.5, 0.4, 0.0, 0.7])
NOISE_NOFLIP = np.array([-0.6, 0.1, -0.3, -0.8, 0.0, -0.7])
# (record, aug_flag, overrides of the scalar draws, what kept_rows must report: kept count or None, rows before the wrap-around or None, fall-back or None)
CASES = [(r, a, {}, (SIZES[r], SIZES[r], None)) for r in ("R1", "R2") for a in range(4)] + [
    ("R511", 1, {"drop": drop6(False, cut=0.8)}, (511, 511, False)),
    ("R512", 0, {"drop": drop6(False, cut=0.0)}, (512, 512, False)),
    ("R512", 1, {"drop": drop6(False, cut=0.6), "noise": NOISE_FLIP}, (512, 128, False)),
    ("R512", 2, {"drop": drop6(False, cut=0.8), "noise": NOISE_NOFLIP}, (512, 32, False)),
    ("R513", 3, {"drop": drop6(False, cut=0.6)}, (513, 128, None)),
    ("R600", 0, {"drop": drop6(True, True, False, True, True)}, (None, None, False)),
    ("R600", 3, {"drop": drop6(True, False, True, False, False)}, (None, None, False)),
    ("R4200", 1, {"drop": drop6(True, True, True, True, False), "noise": NOISE_FLIP}, (None, 512, False)),
    ("R4200", 2, {"drop": drop6(True, False, False, False, True, cut=0.6)}, (None, 128, False)),
    ("RFB", 1, {"drop": drop6(True, True, True, False, False)}, (40, 40, True)),
] + [(r, a, {}, (None, None, None)) for r in NAMES for a in range(4)]
EVAL_CASES = [(r, 0, {}, (SIZES[r], min(SIZES[r], 512), False)) for r in NAMES]


class Scripted:
    """stands in for the sample's ``RandomState``: replays the twin's draws and asserts what ``sample`` asks for"""

    def __init__(self, n, flip, perm, draws, train):
        self.n, self.flip, self.perm, self.train = n, flip, perm, train
        self.uniforms = ([draws["drop"]] if train else []) + [draws["noise"]]
        self.normals = [draws["g_noise"], draws["scale_noise"], draws["ext"]] + ([] if draws["iou"] is None else list(draws["iou"]))

    def uniform(self, lo, hi, size):
        if (lo, hi) == (0, 1):
            assert self.train and size == self.n
            return np.where(self.flip, 0.975, 0.5)
        assert (lo, hi) == (-1, 1) and size == 6
        return np.array(self.uniforms.pop(0), dtype=np.float64)

    def shuffle(self, rows):
        assert self.train and rows.shape == (self.n, 6)
        rows[:] = rows[self.perm]

    def normal(self, mu, sd, size):
        assert (mu, sd) == (0, 0.1)
        out = np.array(self.normals.pop(0), dtype=np.float64)
        assert out.shape == (size,)
        return out


def dataset(mode, phase):
    return t2.BoxDataset(make_records(), mode, 0, phase, cascade=2 if phase == "ioun" else 1)


def batch_of(ds, cases, seed0, key_bits=32):
    """-> (ids, seeds, draws of every sample with the case's overrides applied)"""
    base = len(NAMES)
    ids = [a * base + NAMES.index(r) for r, a, _, _ in cases]
    seeds = [seed0 + 7919 * i for i in range(len(cases))]
    draws = []
    for (_, _, over, _), s in zip(cases, seeds):
        d = sb.scalar_draws(s, ds.phase, ds.mode, ds.cascade)
        d.update({k: v for k, v in over.items() if d[k] is not None})
        draws.append(d)
    return ids, seeds, draws


def chain(ds, ids, seeds, draws, key_bits=32):
    """the existing chain on the scripted stream"""
    items = []
    for i, s, d in zip(ids, seeds, draws):
        n = ds.records[i][1]["cur_box_point"].shape[0]
        flip, perm = sb.point_draws(s, n, key_bits)
        rng = Scripted(n, flip, perm, d, ds.mode == "TRAIN")
        items.append(ds.sample(i, rng))
        assert not rng.uniforms and not rng.normals
    coll = t2.collate(items)
    out = t2.prepare_batch(coll, device="cpu")
    out["sample_id"], out["box_id"] = coll["sample_id"], coll["box_id"]
    return out


def assert_same(want, got):
    assert set(want) == set(got), (sorted(want), sorted(got))
    for k, v in want.items():
        if k in ("sample_id", "box_id"):
            assert list(got[k]) == list(v), k
            continue
        w, g = (x.cpu().numpy() if torch.is_tensor(x) else x for x in (v, got[k]))
        assert g.dtype == np.float32 and g.shape == w.shape, (k, g.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=k)


@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
@pytest.mark.parametrize("mode", ["TRAIN", "EVAL"])
@pytest.mark.parametrize("key_bits", [32, 4])
def test_the_twin_is_the_existing_chain(mode, phase, key_bits):
    ds = dataset(mode, phase)
    cases = CASES if mode == "TRAIN" else EVAL_CASES
    ids, seeds, draws = batch_of(ds, cases, 1000 + key_bits)
    got = sb.prepare_boxes_host(ds, ids, seeds, key_bits, draws=draws)
    assert_same(chain(ds, ids, seeds, draws, key_bits), got)
    assert got["cur_box_point"].shape == (len(ids), 512, 3) and got["gt_boxes"].shape == (len(ids), 1, 7)
    assert ("iou_trans" in got) == (phase == "ioun")
    # the cases reach the branches they are listed for
    seen = set()
    for (r, a, over, (kept, m, fallback)), i, s, d in zip(cases, ids, seeds, draws):
        plan = sb.sample_plan(ds, i, s, d)
        _, _, info = sb.kept_rows(ds, i, s, plan, key_bits)
        assert kept is None or info["kept"] == kept, (r, a, info)
        assert m is None or info["m"] == m, (r, a, info)
        assert fallback is None or info["fallback"] == fallback, (r, a, info)
        assert 1 <= info["m"] <= min(info["kept"], 512)
        seen.add((plan["flags"] & ~sb.F_TRAIN, info["m"] if info["kept"] >= 512 else 0, info["fallback"]))
    if mode == "TRAIN":
        flags = {f for f, _, _ in seen}
        D = sb.F_DROP
        rules = {f & ~sb.F_XFLIP for f in flags}
        for want in (D | sb.F_X_GT | sb.F_OR | sb.F_NEG, D | sb.F_Z_GT, D | sb.F_X_GT | sb.F_Z_GT | sb.F_OR, D | sb.F_NEG, D | sb.F_X_GT | sb.F_Z_GT, 0):
            assert want in rules, (want, sorted(rules))
        assert any(f & sb.F_XFLIP for f in flags) and any(not f & sb.F_XFLIP for f in flags)
        assert {c for _, c, _ in seen} >= {0, 32, 128, 512} and {fb for _, _, fb in seen} == {False, True}
        # drop[1] / drop[2] / drop[5] / drop[4] each seen on both sides among the drop-out cases
        on = [f for f in flags if f & D]
        for bit in (sb.F_X_GT, sb.F_Z_GT, sb.F_OR, sb.F_NEG):
            assert any(f & bit for f in on) and any(not f & bit for f in on)


def test_seeded_draws_need_no_override():
    """without `draws` the twin takes ``scalar_draws`` of the seeds: the same batch as with them passed in"""
    ds = dataset("TRAIN", "ioun")
    ids, seeds = list(range(len(ds))), [31 * i + 2 for i in range(len(ds))]
    draws = [sb.scalar_draws(s, "ioun", "TRAIN", 2) for s in seeds]
    got = sb.prepare_boxes_host(ds, ids, seeds)
    assert_same(sb.prepare_boxes_host(ds, ids, seeds, draws=draws), got)
    assert_same(chain(ds, ids, seeds, draws), got)


def test_ties_fall_back_to_the_row_number():
    flip, perm = sb.point_draws(77, 600, key_bits=4)
    assert sorted(perm.tolist()) == list(range(600))
    base = sb.splitmix64((77 + sb.GOLDEN) & ((1 << 64) - 1))[0]
    with np.errstate(over="ignore"):
        h = sb.splitmix64(base + np.arange(600, dtype=np.uint64))
    key = ((h & np.uint64(0xffffffff)) >> np.uint64(28)).astype(np.int64)
    assert len(set(key.tolist())) <= 16
    pairs = list(zip(key[perm].tolist(), perm.tolist()))
    assert pairs == sorted(pairs)
    np.testing.assert_array_equal(flip, (h >> np.uint64(32)).astype(np.int64) < int(0.05 * 2 ** 32))
    # 32 bits: the same rule with (practically) unique keys
    _, perm32 = sb.point_draws(77, 600)
    key32 = (h & np.uint64(0xffffffff)).astype(np.int64)
    pairs = list(zip(key32[perm32].tolist(), perm32.tolist()))
    assert pairs == sorted(pairs)


def test_a_sample_does_not_depend_on_its_batch():
    ds = dataset("TRAIN", "ioun")
    g = np.random.RandomState(5)
    ids, seeds = g.permutation(len(ds))[:16].tolist(), g.randint(0, 2 ** 31 - 1, size=16).tolist()
    whole = sb.prepare_boxes_host(ds, ids, seeds)
    back = sb.prepare_boxes_host(ds, ids[::-1], seeds[::-1])
    for r in range(16):
        alone = sb.prepare_boxes_host(ds, ids[r:r + 1], seeds[r:r + 1])
        for k, v in alone.items():
            if k in ("sample_id", "box_id"):
                assert v[0] == whole[k][r] == back[k][15 - r]
            else:
                np.testing.assert_array_equal(v[0], whole[k][r], err_msg=k)
                np.testing.assert_array_equal(v[0], back[k][15 - r], err_msg=k)


def test_flip_share_is_five_percent():
    """65536 draws, expectation 0.05, bound +- 0.005: about six standard deviations (sqrt(0.05 * 0.95 / 65536) = 0.00085)"""
    flips = np.concatenate([sb.point_draws(seed, 16384)[0] for seed in (0, 1, 2, 3)])
    assert flips.size == 65536
    share = flips.mean()
    print("flip share", share)
    assert abs(share - 0.05) <= 0.005


def test_reseeding_one_stream_gives_the_draws_of_a_fresh_one():
    rng = np.random.RandomState(0)
    for seed in (0, 1, 2, 12345, 2 ** 31 - 2):
        a, b = sb.scalar_draws(seed, "ioun", "TRAIN", 2), sb.scalar_draws(seed, "ioun", "TRAIN", 2, rng)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_param_blocks_carry_the_plan():
    ds = dataset("TRAIN", "rcnn")
    ids, seeds, draws = batch_of(ds, CASES, 50)
    blocks, plans = sb.param_blocks(ds, ids, seeds, draws)
    assert blocks.dtype == sb.PARAMS and blocks.dtype.itemsize == 264 and blocks.shape == (len(ids),)
    for b, p, i, s in zip(blocks, plans, ids, seeds):
        assert (b["record"], b["flags"], b["cut"], int(b["seed"])) == (i % len(NAMES), p["flags"], p["cut"], s)
        assert (b["gt0"], b["gt2"], b["cx"], b["cz"]) == (p["gt0"], p["gt2"], p["cx"], p["cz"])
        np.testing.assert_array_equal(b["revive0"], p["revive"][0].reshape(16))
        np.testing.assert_array_equal(b["revive1"], p["revive"][1].reshape(16))
        np.testing.assert_array_equal(b["rot"], p["rot"].reshape(16))
        np.testing.assert_array_equal(b["ext"], p["ext"])
        assert b["scale"] == p["scale"]


def test_records_that_are_not_fp32_numbers_are_refused():
    recs = make_records()[:2]
    sb.DeviceBoxes(t2.BoxDataset(recs, "TRAIN"), "cpu")
    recs[1]["cur_box_point"] = recs[1]["cur_box_point"].astype(np.float64) + 1e-12
    with pytest.raises(ValueError, match="float32"):
        sb.DeviceBoxes(t2.BoxDataset(recs, "TRAIN"), "cpu")


def test_device_boxes_pack_the_records():
    ds = dataset("TRAIN", "rcnn")
    boxes = sb.DeviceBoxes(ds, "cpu")
    sizes = [SIZES[r] for r in NAMES]
    assert boxes.base == len(NAMES) and boxes.total == sum(sizes)
    assert boxes.offsets.dtype == torch.int32 and boxes.offsets.tolist() == [0] + np.cumsum(sizes).tolist()
    assert boxes.rows.dtype == torch.float32 and tuple(boxes.rows.shape) == (sum(sizes), 6)
    rec = ds.records[2][1]
    want = np.concatenate((rec["cur_box_point"], rec["cur_box_reflect"], rec["cur_prob_mask"], rec["gt_mask"]), axis=1).astype(np.float32)
    np.testing.assert_array_equal(boxes.rows[boxes.offsets[2]:boxes.offsets[3]].numpy(), want)
    assert set(np.unique(want[:, 4:6])) <= {-0.5, 0.5}


# ----------------------------------------------------------------------------- plumbing
def test_the_entry_is_declared_bound_and_built():
    from ws3d_amd import _lib, build
    with open(os.path.join(ROOT, "include", "ws3d_ops.h")) as f:
        header = f.read()
    assert "WS3D_API int ws3d_stage2_batch(int samples," in header and "Additive to ABI 6" in header
    assert "ws3d_stage2_batch" in _lib.SIGNATURES and "ws3d_stage2_batch_param_bytes" in _lib.SIGNATURES
    assert "stage2_batch.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "ws3d_amd", "csrc", "stage2_batch.hip"))


class _TinyNet(torch.nn.Module):
    """stands in for Stage2Net on a CPU (the box network's ops run on the GPU alone): enough of its interface for ``train`` to drive"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Linear(3, 1)
        self.cfg = None

    def rcnn_forward(self, inputs, towers=None):
        x = inputs["cur_box_point"] * inputs["train_mask"] + inputs["cur_box_reflect"]
        return {"score": self.w(x).mean(dim=(1, 2))}


def test_prepared_batches_follow_the_dataset_stream():
    """'host' takes the batch composition of ``batches``: the epoch permutation and one randint seed per sample from the dataset's
    stream, then the twin -- on a CPU device, as float32 tensors"""
    ds_a = t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", 3, "rcnn")
    ds_b = t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", 3, "rcnn")
    stream = sb.prepared_batches(ds_a, 48, "host", "cpu")
    order = ds_b.rng.permutation(len(ds_b))
    for i0 in (0, 48, 96):
        ids = order[i0:i0 + 48]
        seeds = ds_b.rng.randint(0, 2 ** 31 - 1, size=len(ids))
        got = next(stream)
        assert all(torch.is_tensor(got[k]) and got[k].dtype == torch.float32 and got[k].device.type == "cpu"
                   for k in ("cur_box_point", "cur_box_reflect", "train_mask", "gt_boxes", "cls"))
        assert_same(sb.prepare_boxes_host(ds_b, ids, seeds), got)
    stream.close()
    with pytest.raises(ValueError):
        next(sb.prepared_batches(ds_a, 8, "device", "cpu"))
    with pytest.raises(ValueError):
        next(sb.prepared_batches(ds_a, 8, "off", "cpu"))


def test_train_step_takes_a_prepared_batch_as_it_is(monkeypatch):
    """prepared=True: ``prepare_batch`` is not called and the dict reaches the forward and the loss unchanged"""
    from ws3d_amd import stage2_losses
    ds = t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", 0, "rcnn")
    batch = next(sb.prepared_batches(ds, 16, "host", "cpu"))
    seen = {}

    def rcnn_loss(cls_, reg, boxes, gt, c, cfg):
        seen["gt"], seen["cls"] = gt, c
        v = ((cls_ - c) ** 2).mean()
        return v, {"rcnn_loss": v.detach()}

    class Net(_TinyNet):
        def rcnn_forward(self, inputs, towers=None):
            seen["inputs"] = inputs
            s = super().rcnn_forward(inputs)["score"]
            return {"rcnn_cls": s, "rcnn_reg": s, "pred_boxes3d": s}
    monkeypatch.setattr(stage2_losses, "rcnn_loss", rcnn_loss)
    monkeypatch.setattr(t2, "prepare_batch", lambda *a, **k: pytest.fail("prepare_batch called for a prepared batch"))
    model = Net()
    opt = t2.AdamOneCycle(list(model.parameters()), 4, t2.STAGE2_TRAIN)
    tb = t2.train_step(model, opt, batch, 0, "rcnn", device="cpu", prepared=True)
    assert np.isfinite(tb["loss"])
    assert seen["gt"] is batch["gt_boxes"] and seen["cls"] is batch["cls"]
    assert all(seen["inputs"][k] is batch[k] for k in ("cur_box_point", "cur_box_reflect", "train_mask"))


def _train_tiny(monkeypatch, route, seed=4):
    """``train`` on a CPU with the box network and its loss replaced by a tiny torch module (the network has no CPU route)"""
    from ws3d_amd import stage2_losses

    def rcnn_loss(cls_, reg, boxes, gt, c, cfg):
        v = ((cls_ - c) ** 2).mean() + 0.01 * gt.abs().mean()
        return v, {k: v.detach() for k in stage2_losses.RCNN_KEYS}

    class Net(_TinyNet):
        def rcnn_forward(self, inputs, towers=None):
            s = super().rcnn_forward(inputs)["score"]
            return {"rcnn_cls": s, "rcnn_reg": s, "pred_boxes3d": s}
    monkeypatch.setattr(stage2_losses, "rcnn_loss", rcnn_loss)
    monkeypatch.setattr(t2, "build_model", lambda phase, device, cfg=None, pretrain_ckpt=None: Net().to(device))
    monkeypatch.setattr(t2, "trained_parameters", lambda model, phase: list(model.parameters()))
    ds = t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", seed, "rcnn")
    return ds, Net, rcnn_loss


def test_train_runs_on_the_host_route_on_a_cpu(monkeypatch):
    ds, _, _ = _train_tiny(monkeypatch, "host")
    _, hist = t2.train(ds, "rcnn", 2, batch_size=16, seed=4, device="cpu", device_batches="host", log=lambda s: None)
    assert len(hist) == 2 and all(np.isfinite(h["loss"]) for h in hist)
    with pytest.raises(ValueError):
        t2.train(ds, "rcnn", 1, batch_size=16, device="cpu", device_batches="gpu", log=lambda s: None)


def test_off_is_the_untouched_route(monkeypatch):
    """device_batches='off' (the default) gives the history of ``batches`` + ``train_step`` called directly, for the same seed"""
    ds, Net, _ = _train_tiny(monkeypatch, "off")
    _, hist = t2.train(ds, "rcnn", 3, batch_size=16, seed=4, device="cpu", log=lambda s: None)
    _, hist_off = t2.train(t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", 4, "rcnn"), "rcnn", 3, batch_size=16, seed=4, device="cpu",
                           device_batches="off", log=lambda s: None)
    torch.manual_seed(4)
    model = Net()
    opt = t2.AdamOneCycle(list(model.parameters()), 3, t2.STAGE2_TRAIN)
    stream = t2.batches(t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", 4, "rcnn"), 16, 0)
    direct = [t2.train_step(model, opt, next(stream), it, "rcnn", t2.STAGE2_TRAIN, torch.device("cpu")) for it in range(3)]
    stream.close()
    assert hist == direct and hist_off == direct
