"""CPU checks of the Stage-2 box network (ws3d_amd/stage2.py): the state_dict layout against the reference's (fixture), checkpoint
loading, the torch restatements of the reference's box helpers against the fixture's float64 run, the detection tail against a
literal restatement of the reference's loop, and the resources of csrc/stage2.hip from the compile remarks."""
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import stage2_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return ref.fixture()


def test_state_dict_keys_and_shapes_equal_the_reference(fx):
    from ws3d_amd import stage2
    _, meta, keys = fx
    model = stage2.RCNNNet()
    sd = model.state_dict()
    assert list(sd.keys()) == list(keys)
    assert {k: list(v.shape) for k, v in sd.items()} == keys
    assert not any(k.endswith("identity") for k in sd) and model.input_tansformer.identity.shape == (9,)
    assert [k for k in keys if k.startswith("cls_layer.")] == ["cls_layer.%d.conv.%s" % (i, p) for i in (0, 2, 3) for p in ("weight", "bias")]
    model.load_state_dict(ref.fixture_state_dict(meta, keys), strict=True)
    cfg = stage2.DEFAULT_CFG
    assert cfg.reg_channel == 52 and keys["reg_layer.3.conv.weight"] == [52, 256, 1] and keys["ref_layer.0.3.conv.weight"] == [7, 256, 1]


def test_config_defaults_are_the_fixtures_effective_config():
    import json
    from ws3d_amd import stage2
    conf = json.load(open(os.path.join(ref.GOLDEN, "stage2_state_dict.json")))["config"]
    c = stage2.DEFAULT_CFG
    for name in ("RCNN.SA_CONFIG", "IOUN.SA_CONFIG"):
        sa = conf[name]
        assert [None if n == -1 else n for n in sa["NPOINTS"]] == list(c.npoints) and sa["RADIUS"] == list(c.radius)
        assert sa["NSAMPLE"] == list(c.nsample) and sa["MLPS"] == [list(m) for m in c.mlps]
    assert conf["RCNN.XYZ_UP_LAYER"] == list(c.xyz_up_layer) and conf["RCNN.CLS_FC"] == conf["IOUN.CLS_FC"] == list(c.cls_fc)
    assert conf["RCNN.REG_FC"] == conf["IOUN.REG_FC"] == list(c.reg_fc)
    assert conf["RCNN.USE_BN"] is conf["IOUN.USE_BN"] is c.use_bn is False and conf["RCNN.DP_RATIO"] == conf["IOUN.DP_RATIO"] == c.dp_ratio == 0.0
    assert (conf["RCNN.LOC_SCOPE"], conf["RCNN.LOC_BIN_SIZE"], conf["RCNN.NUM_HEAD_BIN"], conf["RCNN.LOC_Y_BY_BIN"]) == (c.loc_scope, c.loc_bin_size, c.num_head_bin, c.loc_y_by_bin)
    assert np.array_equal(np.asarray(conf["CLS_MEAN_SIZE"], dtype=np.float32), np.asarray(c.cls_mean_size, dtype=np.float32))
    assert (conf["CASCADE"], conf["ATTENTION"], conf["RCNN.SCORE_THRESH"], conf["IOUN.SCORE_THRESH"]) == (c.cascade, c.attention, c.rcnn_score_thresh, c.ioun_score_thresh)


def test_reference_checkpoint_loads_into_stage2net(fx):
    from ws3d_amd import stage2
    _, meta, keys = fx
    sd = ref.fixture_state_dict(meta, keys)
    ckpt = {"epoch": 3, "it": 7, "model_state": {**{"rcnn_net." + k: v for k, v in sd.items()}, "rpn.backbone_net.SA_modules.0.mlps.0.layer0.conv.weight": torch.zeros(16, 4, 1, 1),
                                                 "rpn.rpn_cls_layer.0.conv.weight": torch.zeros(128, 128, 1)}}
    net = stage2.Stage2Net()
    assert net.load_part_ckpt(ckpt) == len(keys)
    for k, v in net.rcnn_net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    broken = dict(ckpt["model_state"])
    del broken["rcnn_net.reg_layer.3.conv.bias"]
    with pytest.raises(RuntimeError, match="reg_layer.3.conv.bias"):
        stage2.Stage2Net().load_part_ckpt(broken)


def test_box_helpers_reproduce_the_fixture(fx):
    """decode / box2center_box / canonical_points / center_box2box / refine_box from the fixture's recorded rcnn_reg / rcnn_ref, in float64:
    mask flags exact, values within 4 x the reference's own fp32 error"""
    from ws3d_amd import stage2
    a, meta, _ = fx
    e = meta["e_ref"]
    c = stage2.DEFAULT_CFG
    reg, rcnn_ref = torch.from_numpy(a["rcnn_reg"]), torch.from_numpy(a["rcnn_ref"])
    R = reg.shape[0]
    mean = torch.from_numpy(np.asarray(c.cls_mean_size, dtype=np.float32)).double()
    dec = stage2.decode_bbox_target_stage_2(torch.zeros((R, 3), dtype=torch.float64), reg, anchor_size=mean, loc_scope=c.loc_scope,
                                            loc_bin_size=c.loc_bin_size, num_head_bin=c.num_head_bin, get_xz_fine=False,
                                            loc_y_scope=c.loc_y_scope, loc_y_bin_size=c.loc_y_bin_size, get_ry_fine=False)
    ce = stage2.box2center_box(dec)
    err = {"box_ce": float((ce - torch.from_numpy(a["box_ce"])).abs().max())}
    can = stage2.canonical_points(torch.from_numpy(a["pts"][..., :3]).double(), torch.from_numpy(a["box_ce"]), c.extend_factor)
    want = torch.from_numpy(a["can_xyz"]).double()
    assert torch.equal(can == 0, want == 0)
    inside = [int(v) for v in (want.abs().amax(-1) > 0).sum(1)]
    assert inside == meta["points_inside_box"] and min(inside[:-1]) < 256 < max(inside[:-1])
    err["can_xyz"] = float((can - want).abs().max())
    pred = stage2.center_box2box(torch.from_numpy(a["box_ce"]))
    err["pred_boxes3d"] = float((pred - torch.from_numpy(a["pred_boxes3d"]).view(R, 7)).abs().max())
    refined = stage2.refine_box(pred, rcnn_ref)
    err["refined_box"] = float((refined - torch.from_numpy(a["refined_box"]).view(R, 7)).abs().max())
    print("errors", err, "bounds", {k: 4 * e[k] for k in err})
    for k, v in err.items():
        assert v <= 4 * e[k], (k, v, 4 * e[k])
    # the independent restatements agree with the package's functions
    dec2, _ = ref.decode_ref(reg)
    assert torch.allclose(dec, dec2, rtol=0, atol=1e-12)
    assert torch.allclose(ref.canonical_ref(torch.from_numpy(a["pts"][..., :3]).double(), torch.from_numpy(a["box_ce"])), can, rtol=0, atol=1e-12)


def test_decode_takes_the_first_maximum_and_wraps_ry():
    from ws3d_amd import stage2
    reg = torch.zeros((3, 52), dtype=torch.float64)
    reg[0, 25 + 3] = reg[0, 25 + 7] = 1.0          # a tie between bins 3 and 7 -> bin 3
    reg[0, 37 + 3], reg[0, 37 + 7] = 0.5, -0.5
    reg[1, 25 + 11] = 2.0                          # bin 11 + a positive residual: beyond 2 pi - ... wraps to a small negative angle
    reg[1, 37 + 11] = 0.5
    reg[2, 25 + 6] = 1.0                           # bin 6 = pi: only ry > pi is shifted
    dec = stage2.decode_bbox_target_stage_2(torch.zeros((3, 3), dtype=torch.float64), reg, 1.5, 0.5, 12, (1.5, 1.6, 3.9), get_xz_fine=False)
    apc = 2 * np.pi / 12
    tol = 1e-6          # bin * angle_per_class is an fp32 product (``.float()``): half an ulp of 6 is 2.4e-7; neighbouring bins are 0.52 apart
    assert abs(float(dec[0, 6]) - (3 * apc + 0.5 * apc / 2)) < tol
    assert abs(float(dec[1, 6]) - (11 * apc + 0.5 * apc / 2 - 2 * np.pi)) < tol
    assert abs(abs(float(dec[2, 6])) - np.pi) < tol         # bin 6 is pi up to that rounding: pi or, wrapped, -pi
    assert torch.allclose(dec[:, 3:6], torch.tensor([[1.5, 1.6, 3.9]], dtype=torch.float64).expand(3, 3))


def test_detections_on_a_hand_built_set():
    """select_boxes + the host sweep against the literal restatement of the reference's loop: a score on each threshold, a size on the
    window's edge, a padding slot, overlapping pairs, a wrapped heading"""
    from ws3d_amd import stage2
    hb = ref.hand_built_set()
    t = {k: torch.from_numpy(v) for k, v in hb.items()}
    out = {"box_ce": t["box_ce"].view(-1, 7), "rcnn_ref": t["rcnn_ref"].view(-1, 7), "rcnn_cls": t["rcnn_cls"].view(-1, 1), "rcnn_iou": t["rcnn_iou"].view(-1, 1)}

    def iou_fn(b):
        n = b.shape[0]
        return torch.tensor([[ref.bev_iou(b[i].numpy(), b[j].numpy()) for j in range(n)] for i in range(n)], dtype=torch.float32)

    boxes, scores, count = stage2.detections(out, t["center"], t["num"], iou_fn=iou_fn)
    want_boxes, want_keep = ref.select_ref(hb["box_ce"], hb["rcnn_ref"], hb["rcnn_cls"], hb["rcnn_iou"], hb["center"], hb["num"])
    want = ref.detections_ref(want_boxes.astype(np.float64), want_keep, hb["rcnn_iou"])
    print("keep", want_keep.tolist(), "h of slot 5", want_boxes[0, 5, 3], "kept slots", want)
    on_edge = bool(want_keep[0, 5])         # h = fp32(1.5 * (1 + fp32(2.3 / 1.5 - 1))) against fp32(2.3): whichever side fp32 puts it
    assert want_keep.tolist() == [[True, False, True, True, True, on_edge, False, False], [True, True, False] + [False] * 5]
    assert want == [([5] if on_edge else []) + [0, 3, 2], [1]]
    assert count.tolist() == [len(w) for w in want]
    for b, slots in enumerate(want):
        assert np.array_equal(boxes[b, :len(slots)].numpy(), want_boxes[b, slots]), b
        assert np.array_equal(scores[b, :len(slots)].numpy(), hb["rcnn_iou"][b, slots])
        assert not boxes[b, len(slots):].any() and not scores[b, len(slots):].any()
    assert abs(float(want_boxes[0, 2, 6]) - (3.5 - 2 * np.pi)) < 1e-6           # the wrapped heading


def test_stage2_kernels_have_no_spills_no_scratch_and_the_claimed_occupancy(tmp_path):
    """compile remarks only: csrc/stage2.hip with the library's flags.  The embed kernel's comment claims registers for >= 2 waves
    per SIMD (its 117,504 bytes of LDS, dynamic and invisible to the remark, are what limits it to one workgroup per CU)"""
    from ws3d_amd import build
    src = os.path.join(ROOT, "ws3d_amd", "csrc", "stage2.hip")
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "stage2.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    report, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([\w \[\]/]+?): (\S+) \[-Rpass", line)
        if m and name:
            report[name][m.group(1).strip()] = m.group(2)
    assert sorted(k.split("stage2_")[1].split("_kernel")[0] for k in report) == ["boxes", "embed", "select"], sorted(report)
    for k, v in report.items():
        assert v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0", (k, v)
        assert v["ScratchSize [bytes/lane]"] == "0", (k, v)
        assert int(v["Occupancy [waves/SIMD]"]) >= (2 if "embed" in k else 8), (k, v)
    text = open(src).read()
    lds = (128 * 65 + 256 * 65 + 2 * 16 * 128) * 4 + 5 * 64 * 4
    assert lds == 117504 and "117,504 bytes" in text and lds <= 160 * 1024
    embed = next(v for k, v in report.items() if "embed" in k)
    assert int(embed["LDS Size [bytes/block]"]) == 5 * 64 * 4        # the static part; the rest is the launch's dynamic LDS
