"""ws3d_gemm_rows_split: a row GEMM on the bf16 matrix cores at fp32 accuracy (split product) -- against
float64 with an analytic bound and against a k-ordered float32 chain computed here on the CPU, on exact small-integer data, on edge
values, for determinism (two launches, graph replay, packing twice), outside its cover, and on the Stage-1 network with
fastpath.SPLIT_GEMMS on and off."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ws3d_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

EPILOGUES = ("none", "bias", "bias_relu", "relu")
SAMPLE_ROWS = 256


def _run(a, wt, bias, relu, out=None):
    from ws3d_amd import compat as C
    pack = C.gemm_rows_pack(wt)
    assert pack is not None
    y = C.gemm_rows_split(a, pack, wt.size(1), bias, relu, out)
    assert y is not None and tuple(y.shape) == (a.size(0), wt.size(1))
    return y


def _epilogue(y, bias, relu):
    if bias is not None:
        y = y + bias
    return y.clamp_min(0) if relu else y


@functools.lru_cache(maxsize=None)
def _case(rows, K, N):
    """inputs and references of one shape, computed once and shared by the four epilogues: A = ReLU of normals, W ~ N(0, 1/K), a
    bias ~ N(0, 1); float64 product and sum of |a w| over all rows; a k-ordered float32 fma chain over a fixed sample of rows"""
    g = torch.Generator().manual_seed(1000 * K + N + rows)
    a = torch.randn(rows, K, generator=g).clamp_min(0)
    wt = torch.randn(K, N, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    ref = a.double() @ wt.double()
    mag = a.double().abs() @ wt.double().abs()
    sample = torch.randperm(rows, generator=g)[:SAMPLE_ROWS].sort().values
    a64, w64 = a[sample].double().numpy(), wt.double().numpy()
    chain = np.zeros((len(sample), N), dtype=np.float32)
    for k in range(K):        # fl32(acc + a w): the product of two float32 is exact in float64
        chain = (chain.astype(np.float64) + a64[:, k:k + 1] * w64[k:k + 1, :]).astype(np.float32)
    return a, wt, bias, ref, mag, sample, torch.from_numpy(chain)


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("rows,K,N", [(64, 32, 64), (128, 96, 128), (4096, 256, 256), (2048, 512, 512), (512, 1024, 512)])
def test_gemm_rows_split_matches_float64_and_the_fp32_chain(rows, K, N, epilogue):
    """every element within (2^-23 + R 2^-24) sum_k |a w| of float64, R = 6 K / 16 accumulator roundings (six MFMAs per k-step of
    16); on a fixed sample of 256 rows rms error <= 1.25 x and max error <= 1.5 x those of a k-ordered float32 fma chain"""
    a, wt, bias, ref, mag, sample, chain = _case(rows, K, N)
    b = bias if epilogue.startswith("bias") else None
    relu = epilogue.endswith("relu")
    y = _run(a.cuda(), wt.cuda(), None if b is None else b.cuda(), relu).cpu()
    want = _epilogue(ref, None if b is None else b.double(), relu)
    err = (y.double() - want).abs()
    bound = (2.0 ** -23 + (6 * K // 16) * 2.0 ** -24) * mag
    worst = float((err / bound).max())
    e_s = err[sample]
    e_c = (_epilogue(chain, b, relu).double() - want[sample]).abs()
    rms, rms_c = float(e_s.pow(2).mean().sqrt()), float(e_c.pow(2).mean().sqrt())
    mx, mx_c = float(e_s.max()), float(e_c.max())
    print("gemm_rows_split %dx%d->%d %s: max err / bound %.3f; sample rms %.3e (chain %.3e, x%.2f), max %.3e (chain %.3e, x%.2f)"
          % (rows, K, N, epilogue, worst, rms, rms_c, rms / rms_c, mx, mx_c, mx / mx_c))
    assert bool((err <= bound).all()), worst
    assert rms <= 1.25 * rms_c, (rms, rms_c)
    assert mx <= 1.5 * mx_c, (mx, mx_c)


@pytest.mark.parametrize("rows,N,epilogue", [(128, 64, "bias"), (192, 192, "bias_relu"), (64, 512, "none"), (256, 128, "relu")])
def test_gemm_rows_split_exact_on_small_integers(rows, N, epilogue):
    """integers in [-3, 3] at K = 1024: every piece, product and partial sum is exact, so the outputs equal float64 bit for bit -- a
    wrong lane map, piece order or k permutation shows here (both tile shapes: N % 128 == 0 and not)"""
    g = torch.Generator().manual_seed(7 + N)
    ri = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    a, wt, bias = ri(rows, 1024), ri(1024, N), ri(N)
    b = bias if epilogue.startswith("bias") else None
    relu = epilogue.endswith("relu")
    y = _run(a.cuda(), wt.cuda(), None if b is None else b.cuda(), relu).cpu()
    want = _epilogue(a.double() @ wt.double(), None if b is None else b.double(), relu)
    assert torch.equal(y.double(), want), float((y.double() - want).abs().max())


def test_gemm_rows_split_edge_values():
    """zeros, |a| near 1e30 and 1e-30, subnormal inputs: finite and within the analytic bound (plus the flush of products below the
    smallest normal: the matrix cores do not keep subnormals); a row holding Inf or NaN: non-finite outputs in that row only"""
    K, N, rows = 256, 128, 256
    g = torch.Generator().manual_seed(9)
    wt = torch.randn(K, N, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    tiny = K * 2.0 ** -126          # every product or piece that is flushed loses less than the smallest normal
    for name, a in (("zeros", torch.zeros(rows, K)), ("1e30", torch.randn(rows, K, generator=g) * 1e30),
                    ("1e-30", torch.randn(rows, K, generator=g) * 1e-30), ("subnormal", torch.randn(rows, K, generator=g) * 1e-39),
                    ("mixed", torch.randn(rows, K, generator=g) * torch.tensor([1e-39, 1e-30, 1.0, 1e30]).repeat(K // 4))):
        a = a.float()
        for b in (None, bias):
            if b is not None and name == "1e30":
                continue            # (a bias of order 1 is below the rounding of 1e30: nothing to see)
            y = _run(a.cuda(), wt.cuda(), None if b is None else b.cuda(), False).cpu()
            want = _epilogue(a.double() @ wt.double(), None if b is None else b.double(), False)
            assert bool(torch.isfinite(y).all()), name
            bound = (2.0 ** -23 + (6 * K // 16) * 2.0 ** -24) * (a.double().abs() @ wt.double().abs()) + tiny
            if b is not None:
                bound = bound + 2.0 ** -24 * want.abs()          # the rounding of the bias add
            err = (y.double() - want).abs()
            assert bool((err <= bound).all()), (name, float((err / bound).max()))
    a = torch.randn(rows, K, generator=g)
    a[3, 5] = float("inf")
    a[70, 0] = float("-inf")
    a[200, K - 1] = float("nan")
    bad = torch.zeros(rows, dtype=torch.bool)
    bad[[3, 70, 200]] = True
    for relu in (False, True):
        y = _run(a.cuda(), wt.cuda(), bias.cuda(), relu).cpu()
        assert not bool(torch.isfinite(y[bad]).any()), relu
        assert bool(torch.isfinite(y[~bad]).all()), relu
        want = _epilogue(a[~bad].double() @ wt.double(), bias.double(), relu)
        bound = (2.0 ** -23 + (6 * K // 16) * 2.0 ** -24) * (a[~bad].double().abs() @ wt.double().abs()) + 2.0 ** -24 * want.abs()
        assert bool(((y[~bad].double() - want).abs() <= bound).all())


def test_gemm_rows_split_is_deterministic():
    """two launches and a graph replay are bit-equal (no split-K, no atomics: one wave sums an element in ascending k); packing
    twice gives identical bytes"""
    from ws3d_amd import compat as C
    g = torch.Generator().manual_seed(11)
    a = torch.randn(8192, 512, generator=g).clamp_min(0).cuda()
    wt = (torch.randn(512, 256, generator=g) / 512 ** 0.5).cuda()
    bias = torch.randn(256, generator=g).cuda()
    p1, p2 = C.gemm_rows_pack(wt), C.gemm_rows_pack(wt)
    assert p1.data_ptr() != p2.data_ptr() and torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert p1.numel() * 4 == 512 * 256 * 6
    base = C.gemm_rows_split(a, p1, 256, bias, True)
    assert torch.equal(C.gemm_rows_split(a, p2, 256, bias, True), base)
    out = torch.empty_like(base)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        C.gemm_rows_split(a, p1, 256, bias, True, out)        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        C.gemm_rows_split(a, p1, 256, bias, True, out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, base)


def test_gemm_rows_split_tile_shape_changes_no_bit():
    """32768 rows x 256 columns run on 128-row tiles (512 of them: the threshold), the same rows in two halves on 64-row tiles: the
    same bits, and both within the analytic bound of float64"""
    from ws3d_amd import compat as C
    g = torch.Generator().manual_seed(17)
    K, N = 96, 256
    a = torch.randn(32768, K, generator=g).clamp_min(0).cuda()
    wt = (torch.randn(K, N, generator=g) / K ** 0.5).cuda()
    bias = torch.randn(N, generator=g).cuda()
    pack = C.gemm_rows_pack(wt)
    whole = C.gemm_rows_split(a, pack, N, bias, True)
    halves = torch.cat([C.gemm_rows_split(a[:16384], pack, N, bias, True), C.gemm_rows_split(a[16384:], pack, N, bias, True)])
    assert torch.equal(whole, halves)
    want = (a.double() @ wt.double() + bias.double()).clamp_min(0)
    bound = (2.0 ** -23 + (6 * K // 16) * 2.0 ** -24) * (a.double().abs() @ wt.double().abs()) + 2.0 ** -24 * want.abs()
    assert bool(((whole.double() - want).abs() <= bound).all())


def test_gemm_rows_split_declines_outside_its_cover():
    """rows = 63, K = 100, N = 48, misaligned pointers: None, nothing launched, nothing written"""
    from ws3d_amd import compat as C, _lib
    g = torch.Generator().manual_seed(13)
    wt = (torch.randn(128, 128, generator=g) / 11).cuda()
    pack = C.gemm_rows_pack(wt)
    a = torch.randn(128, 128, generator=g).cuda()
    assert C.gemm_rows_pack(torch.zeros(100, 128, device="cuda")) is None
    assert C.gemm_rows_pack(torch.zeros(128, 48, device="cuda")) is None
    lib = _lib.load()
    assert lib.ws3d_gemm_rows_pack_bytes(100, 128) == 0 and lib.ws3d_gemm_rows_pack_bytes(128, 48) == 0 and lib.ws3d_gemm_rows_pack_bytes(0, 64) == 0
    assert lib.ws3d_gemm_rows_pack_bytes(1024, 512) == 1024 * 512 * 6
    sentinel = torch.full((128, 128), 7.0, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((sentinel == 7.0).all())
    assert C.gemm_rows_split(a[:63], pack, 128, None, False, sentinel[:63]) is None and untouched()
    flat = torch.randn(128 * 128 + 4, generator=g).cuda()
    off_a = flat[1:1 + 128 * 128].view(128, 128)                  # contiguous, 4 bytes past a 16-byte boundary
    assert C.gemm_rows_split(off_a, pack, 128, None, False, sentinel) is None and untouched()
    off_out = torch.full((128 * 128 + 4,), 7.0, device="cuda")
    assert C.gemm_rows_split(a, pack, 128, None, False, off_out[1:1 + 128 * 128].view(128, 128)) is None
    torch.cuda.synchronize()
    assert bool((off_out == 7.0).all())
    off_b = torch.zeros(132, device="cuda")[1:129]
    assert C.gemm_rows_split(a, pack, 128, off_b, False, sentinel) is None and untouched()
    # the C entry point itself: unsupported shapes return WS3D_E_UNSUPPORTED before any launch
    for rows, K, N in ((63, 128, 128), (128, 100, 128), (128, 128, 48)):
        rc = lib.ws3d_gemm_rows_split(rows, K, N, a.data_ptr(), pack.data_ptr(), None, 0, sentinel.data_ptr(), None)
        assert rc == _lib.E_UNSUPPORTED, (rows, K, N, rc)
    assert untouched()
    assert C.gemm_rows_split(a[:, :100].contiguous(), pack, 128) is None
    assert C.gemm_rows_split(a, pack, 128, None, False, sentinel) is sentinel and not untouched()


def test_replacing_a_blocks_weights_rebuilds_its_pack():
    from ws3d_amd import fastpath, nn_blocks
    torch.manual_seed(3)
    block = nn_blocks.Conv1d(256, 128, bn=True).cuda().eval()
    x = torch.randn(512, 256, device="cuda").clamp_min(0)
    saved = fastpath.SPLIT_GEMMS
    try:
        fastpath.SPLIT_GEMMS = True
        with torch.no_grad():
            y1 = fastpath._layer(x, block)
            ent1 = block.__dict__["_gemm_rows_packs"]["row"]
            assert fastpath._layer(x, block) is not None and block.__dict__["_gemm_rows_packs"]["row"] is ent1       # cached
            block.conv.weight.mul_(2.0)                                # in place: the fold cache sees the version change
            y2 = fastpath._layer(x, block)
            ent2 = block.__dict__["_gemm_rows_packs"]["row"]
            fastpath.SPLIT_GEMMS = False
            lib = fastpath._layer(x, block)
    finally:
        fastpath.SPLIT_GEMMS = saved
    assert ent2 is not ent1 and ent2[0] is not ent1[0] and not torch.equal(ent1[1], ent2[1])
    assert [p_.data_ptr() for p_ in fastpath.gemm_rows_packs(block)] == [ent2[1].data_ptr()]
    assert float((y2 - lib).abs().max()) <= 2e-5 * float(lib.abs().max())
    assert float((y2 - y1).abs().max()) > 1e-2 * float(y1.abs().max())


def test_split_gemms_on_the_stage1_network_and_in_the_pipeline():
    """SPLIT_GEMMS on against off on the seeded Stage-1 net, 2 hdl64 scenes: rpn_cls, rpn_reg and backbone_features agree within
    2e-4 of their scale (the bound of test_fast_path_switches_agree); the kernel really ran (packs on the modules); a depth-4
    Stage1Pipeline replays the bits of its own eager priming order with the switch on"""
    from ws3d_amd import fastpath, stage1
    from ws3d_amd.pipeline import Stage1Pipeline
    from ws3d_amd.seeded import seeded_state_dict
    cfg = stage1.RPNConfig(rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=50)
    model = stage1.Stage1Net(mode="TEST", cfg=cfg)
    model.load_state_dict(seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 6))
    model = model.cuda().eval()
    pts_np = np.stack([synth.cloud("hdl64", 16384, 4000 + s) for s in range(2)])
    pts = torch.from_numpy(pts_np).cuda()
    keys = ("rpn_cls", "rpn_reg", "backbone_features")
    saved = fastpath.SPLIT_GEMMS

    def run(on):
        fastpath.SPLIT_GEMMS = on
        with torch.no_grad():
            out = model.rpn_forward({"pts_input": pts})
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in keys}
    try:
        off = run(False)
        assert not fastpath.gemm_rows_packs(model)
        on = run(True)
        assert len(fastpath.gemm_rows_packs(model)) >= 8
        for k in keys:
            scale = max(1.0, float(off[k].abs().max()))
            d = float((on[k] - off[k]).abs().max())
            print("SPLIT_GEMMS on vs off %s: max diff %.3e of scale %.3e" % (k, d, scale))
            assert d <= 2e-4 * scale, (k, d, scale)
        fastpath.SPLIT_GEMMS = True
        pipe = Stage1Pipeline(model, cfg, batch=2, n_points=16384, depth=4, tune_gemms=False)
        got = []
        for _ in range(5):                                                         # the fifth replays slot 0 a second time
            rpn = pipe.result(pipe.submit(pts_np))["rpn"]
            got.append({k: rpn[k].clone() for k in keys})
        assert pipe.graph_error is None and all(len(s["gemm_rows_packs"]) >= 8 for s in pipe.slots)
        with fastpath.geometry_ahead(False), fastpath.compact_only_scales(pipe.compact_only), torch.no_grad():
            eager = model.rpn_forward({"pts_input": pts})
        torch.cuda.synchronize()
        for o in got:
            for k in keys:
                assert torch.equal(o[k], eager[k]), k
    finally:
        fastpath.SPLIT_GEMMS = saved
