"""GPU tests of csrc/stage2_batch.hip: the kernel writes what its numpy twin (ws3d_amd/stage2_batch.py, pinned to the existing
BoxDataset -> collate -> prepare_batch chain by tests/test_stage2_batch.py) writes, bit for bit; bad arguments touch nothing; the
driver's 'device' and 'host' routes train on the same batches."""
import numpy as np
import pytest
import torch

from tests import test_stage2_batch as cpu

pytestmark = pytest.mark.gpu

RAGGED = (1, 2, 31, 33, 127, 129, 511, 512, 513, 640, 1500, 4099)
# the drop-out draws the 24 samples of the ragged batch cycle through: off; every side choice with AND / OR and with / without the
# drop[4] clause; the 128 and the 32 cut
DROPS = [cpu.drop6(False), cpu.drop6(True, True, True, True, False), cpu.drop6(True, False, False, False, True), cpu.drop6(False, cut=0.6),
         cpu.drop6(True, True, False, True, True, cut=0.8), cpu.drop6(True, False, True, False, False, cut=0.6), cpu.drop6(False, cut=0.8)]


def ragged_records():
    g = np.random.Generator(np.random.PCG64(77))
    recs = []
    for i, n in enumerate(RAGGED):
        fg = i % 3 != 1
        box = np.array([[g.uniform(-0.5, 0.5), 1.65 + g.uniform(-0.2, 0.2), g.uniform(-0.5, 0.5), 1.5, 1.6, 3.9, g.uniform(-3, 3)]], dtype=np.float32)
        recs.append({"sample_id": 500 + i, "box_id": i % 4 if fg else -1, "center": np.zeros((1, 3), dtype=np.float32), "foreground_flag": fg,
                     "gt_boxes": box if fg else np.zeros((1, 7), dtype=np.float32),
                     "cur_box_point": (g.uniform(-2.5, 2.5, (n, 3)) + box[0, 0:3]).astype(np.float32),
                     "cur_box_reflect": g.uniform(0, 1, (n, 1)).astype(np.float32), "cur_prob_mask": g.uniform(0, 1, (n, 1)).astype(np.float32),
                     "gt_mask": (g.uniform(0, 1, (n, 1)) < 0.6).astype(np.float32) if fg else np.zeros((n, 1), dtype=np.float32)})
    return recs


def ragged_batch(ds, seed0, reverse):
    """24 samples: every record twice, the aug_flags 0..3 in turn (aug_flag 0 alone in EVAL mode), the drop-out draws of DROPS in turn"""
    from ws3d_amd import stage2_batch as sb
    train = ds.mode == "TRAIN"
    base = len(RAGGED)
    ids = [((j + j // base) % 4 if train else 0) * base + j % base for j in range(24)]
    seeds = [seed0 + 104729 * j for j in range(24)]
    draws = []
    for j, s in enumerate(seeds):
        d = sb.scalar_draws(s, ds.phase, ds.mode, ds.cascade)
        if train:
            d["drop"] = DROPS[j % len(DROPS)]
        draws.append(d)
    if reverse:
        ids, seeds, draws = ids[::-1], seeds[::-1], draws[::-1]
    return ids, seeds, draws


def assert_device_equals_twin(ds, boxes, ids, seeds, draws, key_bits):
    from ws3d_amd import stage2_batch as sb
    want = sb.prepare_boxes_host(ds, ids, seeds, key_bits, draws=draws)
    got = sb.prepare_boxes(boxes, ids, seeds, key_bits, draws=draws)
    assert all(torch.is_tensor(v) and v.device.type == "cuda" and v.is_contiguous() for k, v in got.items() if k not in ("sample_id", "box_id"))
    cpu.assert_same(want, got)


@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
@pytest.mark.parametrize("mode", ["TRAIN", "EVAL"])
@pytest.mark.parametrize("key_bits", [32, 4])
def test_kernel_equals_twin(mode, phase, key_bits):
    from ws3d_amd import stage2_batch as sb, train_rcnn as t2
    ds = t2.BoxDataset(ragged_records(), mode, 0, phase, cascade=2 if phase == "ioun" else 1)
    boxes = sb.DeviceBoxes(ds, "cuda:0")
    assert_device_equals_twin(ds, boxes, *ragged_batch(ds, 4242, False), key_bits)
    assert_device_equals_twin(ds, boxes, *ragged_batch(ds, 977, True), key_bits)          # reversed, another seed
    ids, seeds, _ = ragged_batch(ds, 31337, False)
    assert_device_equals_twin(ds, boxes, ids, seeds, None, key_bits)                      # the seeded draws, no steering
    # the branch cases of the CPU test as inputs
    ds = cpu.dataset(mode, phase)
    boxes = sb.DeviceBoxes(ds, "cuda:0")
    cases = cpu.CASES if mode == "TRAIN" else cpu.EVAL_CASES
    assert_device_equals_twin(ds, boxes, *cpu.batch_of(ds, cases, 1000 + key_bits), key_bits)


def test_a_sample_does_not_depend_on_its_batch_on_the_device():
    from ws3d_amd import stage2_batch as sb, train_rcnn as t2
    ds = t2.BoxDataset(ragged_records(), "TRAIN", 0, "rcnn")
    boxes = sb.DeviceBoxes(ds, "cuda:0")
    ids, seeds, draws = ragged_batch(ds, 5, False)
    whole = sb.prepare_boxes(boxes, ids, seeds, draws=draws)
    for r in (0, 9, 23):
        alone = sb.prepare_boxes(boxes, ids[r:r + 1], seeds[r:r + 1], draws=draws[r:r + 1])
        for k in ("cur_box_point", "cur_box_reflect", "train_mask", "gt_boxes", "cls"):
            assert torch.equal(alone[k][0], whole[k][r]), k


def test_bad_arguments_touch_nothing():
    from ws3d_amd import _lib, stage2_batch as sb, train_rcnn as t2
    lib = _lib.load()
    ds = t2.BoxDataset(ragged_records(), "TRAIN", 0, "rcnn")
    boxes = sb.DeviceBoxes(ds, "cuda:0")
    ids, seeds = [3, 11, 5], [1, 2, 3]           # records 3, 11 (the last one: its rows end at T) and 5
    blocks, _ = sb.param_blocks(ds, ids, seeds)
    blocks_bad = blocks.copy()
    blocks_bad["record"][2] = len(RAGGED)        # a record index past the last record
    up = torch.from_numpy(blocks.view(np.uint8).copy()).cuda()
    up_bad = torch.from_numpy(blocks_bad.view(np.uint8).copy()).cuda()
    outs = [torch.full((3, 512, 3), 7.0, device="cuda"), torch.full((3, 512, 1), 7.0, device="cuda"), torch.full((3, 512, 1), 7.0, device="cuda")]
    status = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(samples=3, params=up, rows=boxes.rows.data_ptr(), offsets=boxes.offsets.data_ptr(), records=boxes.base, total=boxes.total,
             key_bits=32, pts="out"):
        return lib.ws3d_stage2_batch(samples, None if params is None else params.data_ptr(), rows, offsets, records, total, key_bits,
                                     None if pts is None else outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), status.data_ptr(), stream)

    for kw in ({"params": None}, {"rows": None}, {"offsets": None}, {"pts": None}, {"samples": -1}, {"records": -1}, {"total": -1},
               {"key_bits": 0}, {"key_bits": 33}, {"rows": boxes.rows.data_ptr() + 4}):
        assert call(**kw) == _lib.E_INVALID, kw
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs) and bool((status == -9).all()), kw
    assert call(samples=0) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((status == -9).all())
    # offsets that run past the row count the call states: the sample they belong to is refused on the device and left alone, and so is
    # the one with a record index past the last record; the others are written
    assert call(params=up_bad, total=boxes.total - 1) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 3, 3]
    want = sb.prepare_boxes_host(ds, ids[:1], seeds[:1])
    np.testing.assert_array_equal(outs[0][0].cpu().numpy(), want["cur_box_point"][0])
    np.testing.assert_array_equal(outs[2][0].cpu().numpy(), want["train_mask"][0])
    assert all(bool((o[1:] == 7.0).all()) for o in outs)


def _histories_agree(a, b, spread_runs):
    """per-iteration losses of two routes against the spread of one route run twice: bit-equal when that is zero, else within twice it"""
    s0, s1 = spread_runs
    for it in range(len(a)):
        spread = abs(s0[it]["loss"] - s1[it]["loss"])
        diff = abs(a[it]["loss"] - b[it]["loss"])
        print("it %d  loss %.9g / %.9g  diff %.3g  spread of the reference route %.3g" % (it, a[it]["loss"], b[it]["loss"], diff, spread))
        assert np.isfinite(a[it]["loss"]) and np.isfinite(b[it]["loss"])
        assert diff == 0.0 if spread == 0.0 else diff <= 2 * spread, (it, diff, spread)


@pytest.fixture
def deterministic_torch():
    """the library's own run-to-run noise (atomics in its GEMMs and index kernels: the third ioun loss of two seeded runs differs in
    the 7th digit without this) taken out, so that a difference between two runs is a difference between their batches"""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


@pytest.mark.parametrize("phase", ["rcnn", "ioun"])
def test_driver_trains_on_the_same_batches_by_both_routes(phase, deterministic_torch):
    from ws3d_amd import stage2, stage2_batch as sb, train_rcnn as t2

    def run(route):
        ds = t2.BoxDataset(t2.SyntheticBoxes(64), "TRAIN", 0, phase, cascade=stage2.DEFAULT_CFG.cascade)
        return t2.train(ds, phase, 3, batch_size=32, seed=0, device="cuda:0", device_batches=route, log=lambda s: None)[1]
    host0, host1, dev = run("host"), run("host"), run("device")
    assert len(dev) == len(host0) == 3
    _histories_agree(dev, host0, (host0, host1))
    # their batches: the two preparers on the stream's ids and seeds
    ds = t2.BoxDataset(t2.SyntheticBoxes(64), "TRAIN", 0, phase, cascade=stage2.DEFAULT_CFG.cascade)
    boxes = sb.DeviceBoxes(ds, "cuda:0")
    plan = sb.batch_plan(ds, 32)
    for _ in range(3):
        ids, seeds = next(plan)
        cpu.assert_same(sb.prepare_boxes_host(ds, ids, seeds), sb.prepare_boxes(boxes, ids, seeds))


def test_off_is_the_untouched_route_with_the_box_network(deterministic_torch):
    """device_batches='off' against ``batches`` + ``train_step`` called directly, same seed (the network runs on the GPU alone, so
    this check lives here; tests/test_stage2_batch.py makes it on a CPU with a stand-in network)"""
    from ws3d_amd import train_rcnn as t2

    def direct():
        torch.manual_seed(0)
        dev = torch.device("cuda:0")
        model = t2.build_model("rcnn", dev)
        opt = t2.AdamOneCycle(t2.trained_parameters(model, "rcnn"), 2, t2.STAGE2_TRAIN)
        stream = t2.batches(t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", 0, "rcnn"), 16, 0)
        try:
            return [t2.train_step(model, opt, next(stream), it, "rcnn", t2.STAGE2_TRAIN, dev) for it in range(2)]
        finally:
            stream.close()
    off = t2.train(t2.BoxDataset(t2.SyntheticBoxes(32), "TRAIN", 0, "rcnn"), "rcnn", 2, batch_size=16, seed=0, device="cuda:0", log=lambda s: None)[1]
    d0, d1 = direct(), direct()
    _histories_agree(off, d0, (d0, d1))
