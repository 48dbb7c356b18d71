"""ws3d_rpn_heads: the RPN's two heads in one launch on the bf16 matrix cores at fp32 accuracy (split product),
against float64, against the fp32 ws3d_mlp2_rows on the same data, on exact small-integer data, on edge values, for determinism
(two launches, workgroup counts, graph replay) and on the headline network with the switch on and off."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ws3d_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _weights(g, o2, bias, wscale=11.0):
    w1t = (torch.randn(128, 128, generator=g) / wscale).cuda()
    w2t = (torch.randn(128, o2, generator=g) / wscale).cuda()
    b1 = torch.randn(128, generator=g).cuda() if bias else None
    b2 = torch.randn(o2, generator=g).cuda() if bias else None
    return w1t, b1, w2t, b2


def _ref(x, w1t, b1, w2t, b2, relu2):
    h = x.double() @ w1t.double()
    if b1 is not None:
        h = h + b1.double()
    h = h.clamp_min(0)
    y = h @ w2t.double()
    if b2 is not None:
        y = y + b2.double()
    return y.clamp_min(0) if relu2 else y


def _heads(x, w1t, b1, w2t, b2, relu2, workgroups=0):
    """one head through ws3d_rpn_heads: o2 = 1 as the classification head, else as the regression head"""
    from ws3d_amd import compat as C
    o2 = w2t.size(1)
    blob = C.rpn_heads_pack(w1t, b1, True, w2t, b2, relu2)
    assert blob is not None
    tickets = torch.zeros(2, dtype=torch.int32, device="cuda")
    if o2 == 1:
        r = C.rpn_heads(x, 1, blob, None, 0, tickets, workgroups)
        assert r is not None and r[1] is None
        return r[0]
    r = C.rpn_heads(x, 2, None, blob, o2, tickets, workgroups)
    assert r is not None and r[0] is None
    return r[1]


@pytest.mark.parametrize("rows,o2,relu2,bias", [(32, 1, False, True), (4096, 40, False, True), (16384 + 32, 1, False, True),
                                                 (2048, 64, True, True), (1024, 33, True, False), (131072, 40, False, True),
                                                 (131072, 1, False, True)])
def test_rpn_heads_matches_float64_and_fp32_kernel(rows, o2, relu2, bias):
    """error <= 2e-5 of max|ref| against float64, and rms / max error within 1.25 x those of the fp32 ws3d_mlp2_rows on the same data"""
    from ws3d_amd import compat as C
    g = torch.Generator().manual_seed(rows + o2)
    x = torch.randn(rows, 128, generator=g).cuda()
    w1t, b1, w2t, b2 = _weights(g, o2, bias)
    y = _heads(x, w1t, b1, w2t, b2, relu2)
    assert y.shape == (rows, o2)
    y32 = C.mlp2_rows(x, w1t, b1, True, w2t, b2, relu2)
    ref = _ref(x, w1t, b1, w2t, b2, relu2)
    scale = max(1.0, ref.abs().max().item())
    e, e32 = (y.double() - ref).abs(), (y32.double() - ref).abs()
    assert e.max().item() <= 2e-5 * scale, e.max().item()
    rms, rms32 = e.pow(2).mean().sqrt().item(), e32.pow(2).mean().sqrt().item()
    print("rpn_heads rows=%d o2=%d: max err %.3e (fp32 kernel %.3e), rms %.3e (%.3e), of max|ref| %.3e"
          % (rows, o2, e.max().item(), e32.max().item(), rms, rms32, scale))
    assert rms <= 1.25 * rms32, (rms, rms32)
    assert e.max().item() <= 1.25 * e32.max().item(), (e.max().item(), e32.max().item())


def test_rpn_heads_both_in_one_launch_equal_one_at_a_time():
    from ws3d_amd import compat as C
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8192, 128, generator=g).cuda()
    wc, wr = _weights(g, 1, True), _weights(g, 40, True)
    bc, br = C.rpn_heads_pack(wc[0], wc[1], True, wc[2], wc[3], False), C.rpn_heads_pack(wr[0], wr[1], True, wr[2], wr[3], False)
    both = C.rpn_heads(x, 3, bc, br, 40, torch.zeros(2, dtype=torch.int32, device="cuda"))
    cls = C.rpn_heads(x, 1, bc, None, 0, torch.zeros(2, dtype=torch.int32, device="cuda"))[0]
    reg = C.rpn_heads(x, 2, None, br, 40, torch.zeros(2, dtype=torch.int32, device="cuda"))[1]
    assert torch.equal(both[0], cls) and torch.equal(both[1], reg)
    # shapes outside the cover: None, nothing launched
    t = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert C.rpn_heads(x[:31], 3, bc, br, 40, t) is None
    assert C.rpn_heads(x[:, :64].contiguous(), 3, bc, br, 40, t) is None
    assert C.rpn_heads_pack(wr[0], wr[1], True, torch.zeros(128, 65, device="cuda"), None, False) is None
    assert int(t.sum()) == 0


@pytest.mark.parametrize("o2", [1, 40, 64, 33])
def test_rpn_heads_exact_on_small_integers(o2):
    """small-integer data: every product, piece and partial sum is exact, so the outputs equal float64 bit for bit -- a wrong lane
    map or k permutation of either layer shows here"""
    g = torch.Generator().manual_seed(100 + o2)
    ri = lambda *s: torch.randint(-3, 4, s, generator=g).float().cuda()
    x, w1t, w2t, b1, b2 = ri(4096, 128), ri(128, 128), ri(128, o2), ri(128), ri(o2)
    y = _heads(x, w1t, b1, w2t, b2, False)
    ref = _ref(x, w1t, b1, w2t, b2, False)
    assert torch.equal(y.double(), ref), (y.double() - ref).abs().max().item()


def test_rpn_heads_edge_values():
    """zeros, |x| near 1e30 and 1e-30, subnormal inputs: accurate; a row holding Inf or NaN: non-finite outputs in that row only"""
    g = torch.Generator().manual_seed(9)
    for o2 in (1, 40):
        w1t, b1, w2t, b2 = _weights(g, o2, True)
        for name, x in (("zeros", torch.zeros(256, 128)), ("1e30", torch.randn(256, 128, generator=g) * 1e30),
                        ("1e-30", torch.randn(256, 128, generator=g) * 1e-30), ("subnormal", torch.randn(256, 128, generator=g) * 1e-39),
                        ("mixed", torch.randn(256, 128, generator=g) * torch.tensor([1e-39, 1e-30, 1.0, 1e30]).repeat(32))):
            x = x.float().cuda()
            y = _heads(x, w1t, b1, w2t, b2, False)
            ref = _ref(x, w1t, b1, w2t, b2, False)
            assert torch.isfinite(y).all(), name
            err = (y.double() - ref).abs().max().item()
            assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (name, o2, err)
        x = torch.randn(256, 128, generator=g).cuda()
        x[3, 5] = float("inf")
        x[70, 0] = float("-inf")
        x[200, 127] = float("nan")
        y = _heads(x, w1t, b1, w2t, b2, False)
        bad = torch.zeros(256, dtype=torch.bool, device="cuda")
        bad[[3, 70, 200]] = True
        assert not torch.isfinite(y[bad]).any(dim=1).any(), o2
        assert torch.isfinite(y[~bad]).all(), o2
        ref = _ref(x[~bad], w1t, b1, w2t, b2, False)
        assert (y[~bad].double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


def test_rpn_heads_deterministic_across_launches_workgroups_and_graph_replay():
    """the ticket order changes no bit: two launches, other workgroup counts (the capture-time cap among them) and a graph replay
    are bit-equal"""
    from ws3d_amd import compat as C, pipeline
    g = torch.Generator().manual_seed(11)
    x = torch.randn(131072, 128, generator=g).cuda()
    wc, wr = _weights(g, 1, True), _weights(g, 40, True)
    bc, br = C.rpn_heads_pack(wc[0], wc[1], True, wc[2], wc[3], False), C.rpn_heads_pack(wr[0], wr[1], True, wr[2], wr[3], False)

    def run(wgs):
        return C.rpn_heads(x, 3, bc, br, 40, torch.zeros(2, dtype=torch.int32, device="cuda"), wgs)
    base = run(0)
    cap = 2 * pipeline.THROUGHPUT_GEOMETRY["mlp2_wgs"]
    for wgs in (0, cap, 7, 2, 1000):
        got = run(wgs)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), wgs
    tickets = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tickets.zero_()
        C.rpn_heads(x, 3, bc, br, 40, tickets, cap)            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tickets.zero_()
        out = C.rpn_heads(x, 3, bc, br, 40, tickets, cap)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1])


def test_fused_heads_on_the_headline_network():
    """FUSED_HEADS on against off on the headline network (seeded weights, 8 hdl64 scenes): the heads agree to 2e-5 of their scale;
    the differences of the reg-bin argmax, the top-9000 order and the NMS keep lists are counted and each must be a near-tie.
    With the switch off the heads are bit-equal to the two ws3d_mlp2_rows launches."""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.DEFAULT_CFG
    model = stage1.Stage1Net(mode="TEST", cfg=cfg)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 6))
    model = model.cuda().eval()
    pts = torch.from_numpy(np.stack([synth.cloud("hdl64", 16384, 4000 + s) for s in range(8)])).cuda()
    saved = fastpath.FUSED_HEADS

    def run(on):
        fastpath.FUSED_HEADS = on
        with torch.no_grad():
            out = model.rpn_forward({"pts_input": pts})
            props = stage1.proposals_from_rpn(out, cfg)
        torch.cuda.synchronize()
        return out, props
    try:
        off, p_off = run(False)
        on, p_on = run(True)
    finally:
        fastpath.FUSED_HEADS = saved
    # switch off: the two mlp2_rows launches, bit for bit
    rows = off["backbone_features_nlc"].reshape(-1, 128)
    assert torch.equal(off["rpn_cls"].reshape(-1, 1), fastpath.mlp_rows(rows, model.rpn.rpn_cls_layer))
    assert torch.equal(off["rpn_reg"].reshape(rows.size(0), -1), fastpath.mlp_rows(rows, model.rpn.rpn_reg_layer))
    assert torch.equal(off["backbone_features_nlc"], on["backbone_features_nlc"])
    report = {}
    for k in ("rpn_cls", "rpn_reg"):
        scale = max(1.0, float(off[k].abs().max()))
        d = float((on[k] - off[k]).abs().max())
        report[k + "_max_diff_of_scale"] = d / scale
        assert d <= 2e-5 * scale, (k, d, scale)
    tol = 4e-5 * max(1.0, float(off["rpn_reg"].abs().max()))
    nb = int(cfg.loc_scope / cfg.loc_bin_size) * 2
    report["reg_bin_argmax_diffs"] = 0
    for sl in (slice(0, nb), slice(nb, 2 * nb)):
        a, b = off["rpn_reg"][..., sl], on["rpn_reg"][..., sl]
        ia, ib = a.argmax(-1), b.argmax(-1)
        diff = ia != ib
        report["reg_bin_argmax_diffs"] += int(diff.sum())
        # a differing argmax: the two bins' logits tie within the heads' tolerance
        va, vb = a.gather(-1, ia[..., None])[..., 0], a.gather(-1, ib[..., None])[..., 0]
        assert bool(((va - vb).abs()[diff] <= tol).all())
    top = min(cfg.rpn_pre_nms_top_n, pts.size(1))
    sa, ia = off["rpn_cls"][..., 0].topk(top, dim=1)
    sb, ib = on["rpn_cls"][..., 0].topk(top, dim=1)
    diff = ia != ib
    report["top9000_order_diffs"] = int(diff.sum())
    # where the order differs, the scores at that rank tie within the heads' tolerance
    tol_c = 4e-5 * max(1.0, float(off["rpn_cls"].abs().max()))
    assert bool(((sa - sb).abs() <= tol_c).all())
    cnt_a, cnt_b = p_off[2], p_on[2]
    report["nms_count_diffs"] = int((cnt_a != cnt_b).sum())
    same_count = cnt_a == cnt_b
    box_diff = ((p_off[0] - p_on[0]).abs().amax(-1) > 1e-3)
    report["nms_kept_box_diffs"] = int(box_diff.sum())
    print("FUSED_HEADS on vs off, headline network:", report)
    # the keep lists may differ only through near-ties: at most a handful of boxes per scene
    assert report["nms_count_diffs"] <= 8 and report["nms_kept_box_diffs"] <= 0.02 * box_diff.numel(), report
    assert bool(same_count.any())
