"""CPU check of which search kernel every ball-query call of tests/test_gpu_parity.py launches: ws3d_ball_query_plan is the launchers'
own decision (csrc/ballquery_group.hip bq_plan) without the launch.  The calls listed by tests/helpers.py bq_plan_calls() must reach
all 13 search instantiations of the file between them -- a kernel that no GPU test runs fails here, without a GPU -- and the plan
refuses what the launchers refused before the plan was split from the launch."""
import ctypes as C

from tests import helpers as H

BRUTE, SLAB, LANE, COOP = 0, 1, 2, 3
# (family, bits of a list index, FUSED, waves per workgroup): ball_query_kernel<uint16_t | int32_t, FUSED>, ball_query_sorted_kernel<FUSED>,
# ball_query_grid_kernel<FUSED>, ball_query_grid_coop_kernel<FUSED, 4 | 16>, ball_query_grid_coop_kernel<false, 8>
INSTANTIATIONS = ({(BRUTE, bits, f, 4) for bits in (16, 32) for f in (0, 1)} | {(fam, 16, f, 4) for fam in (SLAB, LANE) for f in (0, 1)} |
                  {(COOP, 16, f, nw) for f in (0, 1) for nw in (4, 16)} | {(COOP, 16, 0, 8)})
E_INVALID, E_UNSUPPORTED = -1, -4


def _plan(call):
    from ws3d_amd import _lib
    out = (C.c_int32 * 8)()
    rc = _lib.load().ws3d_ball_query_plan(*call, C.cast(out, C.c_void_p))
    return rc, list(out)


def test_the_tested_shapes_reach_every_search_kernel():
    assert len(INSTANTIATIONS) == 13
    reached = {}
    for call in H.bq_plan_calls():
        rc, (family, bits, fused, nw, gz, lds, gx, gy) = _plan(call)
        assert rc == 0 and gx > 0 and gz >= 1 and gy >= 1 and 0 < lds <= 160 * 1024, (call, rc)
        assert fused == call[5] and gy == {COOP: call[9], LANE: 1}.get(family, call[0]), call       # grid y: scales | 1 | scenes
        reached.setdefault((family, bits, fused, nw), []).append(call)
    assert set(reached) == INSTANTIATIONS, sorted(set(reached) ^ INSTANTIATIONS)
    # both tile decodes (scenes a multiple of eight: XCD-aware; else plain) of every kernel that has them
    for key in [k for k in INSTANTIATIONS if k[0] in (LANE, COOP)]:
        assert {c[0] % 8 == 0 for c in reached[key]} == {True, False}, key
    # the cases meant for a kernel reach it
    for B, N, M, r, ns in H.BQ_LANE_CASES:
        assert _plan((B, N, M, 0, ns, 0, 0, 1, 0, 1, 0))[1][:4] == [LANE, 16, 0, 4]
    B, N, M, r, ns, c = H.BQ_WIDE_INDEX_CASE
    assert _plan((B, N, M, 0, ns, 0, 0, -1, 0, 1, 0))[1][:4] == [BRUTE, 32, 0, 4]
    for B, N, M, r, ns in H.BQ_MANY_SCENES_CASES:
        assert _plan((B, N, M, 0, ns, 0, 0, 1, 0, 1, 0))[1][:4] == [COOP, 16, 0, 4]


def test_the_plan_sizes_the_cooperative_launch_once():
    """the LDS bytes and the 4 / 16 / 8 waves of the one-wave-per-centre kernel, single scale and two scales, from one formula"""
    def lds(ns, nw):
        return 16 * 64 + 4 * 64 + 2 * (((64 * (ns + 1) + 7) & ~7) + nw * 1024 + 64 * 64)
    assert _plan((8, 16384, 4096, 0, 32, 0, 0, 1, 0, 1, 0)) == (0, [COOP, 16, 0, 16, 1, lds(32, 16), 512, 1])
    assert _plan((8, 16384, 4096, 0, 32, 0, 0, 1, 0, 1, 8)) == (0, [COOP, 16, 0, 16, 1, lds(32, 16), 512, 1])      # key 5: two scales only
    assert _plan((8, 16384, 4096, 0, 32, 0, 0, 1, 1, 2, 0)) == (0, [COOP, 16, 0, 16, 1, lds(32, 16), 512, 2])
    assert _plan((8, 16384, 4096, 0, 32, 0, 0, 1, 1, 2, 8)) == (0, [COOP, 16, 0, 8, 1, lds(32, 8), 512, 2])
    assert _plan((16, 16384, 4096, 0, 32, 0, 0, 1, 1, 2, 8)) == (0, [COOP, 16, 0, 4, 1, lds(32, 4), 1024, 2])      # 2 x 1024 tiles fill the chip
    assert _plan((512, 16384, 4096, 1, 64, 1, 0, 1, 0, 1, 0)) == (0, [COOP, 16, 1, 4, 1, lds(64, 4), 32768, 1])    # the c2 block
    # the fused emit's split: channels-first by channels, channels-last by rows, until 1024 workgroups
    assert _plan((2, 4096, 1024, 128, 32, 1, 0, 1, 0, 1, 0))[1][3:5] == [16, 16]     # 128 / 16 = 8 channels per workgroup
    assert _plan((2, 4096, 1024, 128, 32, 1, 1, 1, 0, 1, 0))[1][3:5] == [16, 32]     # 64 * 32 / 32 = 64 rows per workgroup
    assert _plan((2, 4096, 1024, 8, 32, 1, 0, 1, 0, 1, 0))[1][3:5] == [16, 1]


def test_the_plan_refuses_what_the_launchers_refuse():
    zero = [0] * 8
    assert _plan((2, 4096, 256, 0, 16, 0, 0, -1, 1, 1, 0)) == (E_UNSUPPORTED, zero)       # pairs without a binned copy
    assert _plan((2, 4096, 256, 0, 16, 0, 0, 0, 1, 1, 0)) == (E_UNSUPPORTED, zero)        # ... with x slabs
    assert _plan((2, 16400, 256, 0, 16, 0, 0, 1, 1, 1, 0)) == (E_UNSUPPORTED, zero)       # ... with more points than a binned copy takes
    assert _plan((2, 4096, 256, 0, 72, 0, 0, 1, 1, 1, 0)) == (E_UNSUPPORTED, zero)        # pairs with nsample > 64
    assert _plan((2, 4096, 256, 0, 72, 0, 0, 1, 1, 2, 0)) == (E_UNSUPPORTED, zero)
    assert _plan((2, 4096, 256, 0, 32, 0, 0, 0, 1, 2, 0)) == (E_UNSUPPORTED, zero)        # two scales on a buffer that is not fine-grid
    assert _plan((1, 4096, 256, 0, 70000, 0, 0, -1, 0, 1, 0)) == (E_UNSUPPORTED, zero)    # nsample too long for LDS
    assert _plan((1, 4096, 256, 0, 70000, 0, 0, 1, 0, 1, 0)) == (E_UNSUPPORTED, zero)
    assert _plan((65536, 64, 1, 0, 8, 0, 0, -1, 0, 1, 0)) == (E_UNSUPPORTED, zero)        # b > 65535
    assert _plan((65536, 64, 1, 0, 8, 0, 0, 1, 0, 1, 0)) == (E_UNSUPPORTED, zero)
    for bad in ((-1, 64, 1, 0, 8), (1, 0, 1, 0, 8), (1, 64, -1, 0, 8), (1, 64, 1, -1, 8), (1, 64, 1, 0, 0)):
        assert _plan(bad + (0, 0, -1, 0, 1, 0)) == (E_INVALID, zero)
    assert _plan((1, 64, 1, 0, 8, 0, 0, -1, 0, 3, 0))[0] == E_INVALID
    assert _plan((0, 64, 1, 0, 8, 0, 0, -1, 0, 1, 0)) == (0, zero) and _plan((1, 64, 0, 0, 8, 0, 0, -1, 0, 1, 0)) == (0, zero)     # nothing to launch
    # what is not refused: longer lists on a fine-grid buffer step down to one lane per centre
    assert _plan((2, 4096, 256, 0, 72, 0, 0, 1, 0, 1, 0))[1][0] == LANE
