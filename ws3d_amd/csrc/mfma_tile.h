// mfma_tile.h -- the building blocks of the fp32 matrix-core kernels of gemm_pool.hip (v_mfma_f32_32x32x2_f32: fp32 in, fp32
// accumulate).  A workgroup of 256 threads = 4 waves as 2 (rows) x 2 (cols) computes a (64 MB) x (64 NB) output tile, each wave
// MB x NB accumulators of 32 x 32.  Every piece exists once: the wave geometry and the accumulator's row layout, the
// double-buffered K loop "global -> registers -> LDS -> MFMA", the layer multiplied out of an activation tile in LDS, the
// per-point first layer, the epilogues and the XCD-aware tile order.  A kernel is then a choice of A-operand loader and epilogue.
// (The compact atomic epilogue is compact_pool.h.)
//
// Arithmetic contract of every block: accumulators start where the caller says (zero, or the gathered row of P), k ascends, two
// k per matrix instruction, zero padding behind the k extent, then bias -> ReLU -> max / store.
#pragma once
#include "common.h"

namespace ws3d {

constexpr int GP_KT = 16;          // K step per LDS tile
constexpr int GP_XS = 65;          // padded row length of a k-major 64-row tile

__device__ __forceinline__ float gp_nanmax(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void acc_zero(floatx16 &acc) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
}

// ---- geometry.  Wave w of the workgroup owns the sub-tiles of row block wm = w % 2 and column block wn = w / 2; a lane feeds
// row / column l32 = lane % 32 of a sub-tile and the k of parity kh = lane / 32 of each matrix instruction.
struct Wave {
    int tid, lane, wm, wn, l32, kh;
    int ar, bc;                    // this lane's row / column of a 64 x 64 tile (MB = NB = 1)
    __device__ __forceinline__ Wave() {
        tid = threadIdx.x; lane = tid & 63; wm = (tid >> 6) & 1; wn = tid >> 7; l32 = lane & 31; kh = lane >> 5;
        ar = wm * 32 + l32; bc = wn * 32 + l32;
    }
};
// first tile row of the wave's accumulator i of MB, first tile column of its accumulator j of NB.  SPLIT: the wave's columns are
// 64 apart (j * 64 + wn * 32: the layout of the activation tiles, where every 64-column block is shared by all four waves)
template <int MB> __device__ __forceinline__ int sub_row(const Wave &w, int i) { return 32 * (MB * w.wm + i); }
template <int NB, bool SPLIT> __device__ __forceinline__ int sub_col(const Wave &w, int j) { return SPLIT ? 64 * j + 32 * w.wn : 32 * (NB * w.wn + j); }
// THE accumulator layout of a 32 x 32 sub-tile: register v of a lane holds row acc_row(v, lane / 32) of column lane % 32
__device__ __forceinline__ int acc_row(int v, int kh) { return 8 * (v / 4) + 4 * kh + v % 4; }

// ---- XCD-aware tile order of a 1-D grid of col_tiles * row_tiles workgroups: workgroup g runs on XCD g % 8 (observed dispatch
// order).  The col tiles of a row tile read the SAME rows: next to each other on ONE XCD the second .. last read hits that L2
// (with col tiles on blockIdx.x they ran on different XCDs and the activation -- 100 MB at SA2 -- came out of HBM once per col
// tile).  PER_SCENE (the gather-GEMMs): with tps row tiles per scene and a batch that is a multiple of 8,
//   scene = (g / 8 / (col_tiles * tps)) * 8 + g % 8,   row tile = (g / 8 / col_tiles) % tps,   col tile = (g / 8) % col_tiles
// also keeps all tiles of a scene on ONE XCD -- the rows they gather (4 MB of features per scene at FP1) stay in that L2 instead
// of being pulled through all eight.  Without PER_SCENE tps is a flag (row tiles % 8 == 0).  tps = 0: plain order.
template <bool PER_SCENE>
__device__ __forceinline__ void gg_tile(int col_tiles, int tps, long g, long &row_tile, int &col_tile) {
    if (tps > 0) {
        const long j = g >> 3;
        col_tile = (int)(j % col_tiles);
        const long jj = j / col_tiles;
        row_tile = PER_SCENE ? ((jj / tps) * 8 + (g & 7)) * tps + jj % tps : jj * 8 + (g & 7);
    } else {
        col_tile = (int)(g % col_tiles);
        row_tile = g / col_tiles;
    }
}

// ---- A-operand loader "contiguous rows": p[i] = the row of x this thread stages for accumulator row block i (the caller clamps
// it where rows end early); k_dim % 4 == 0
template <int MB>
struct RowsA {
    const float *p[MB];
    int k_dim;
    __device__ __forceinline__ float4 operator()(int i, int k) const { return k < k_dim ? *reinterpret_cast<const float4 *>(p[i] + k) : f4_zero(); }
};

// ---- K loop: acc = A (64 MB x k_dim) . Wt[0:k_dim, col0 : col0 + 64 NB] over the LDS buffers xs ([k][row], rows padded by one) and
// ws ([k][col], 16-byte aligned), double-buffered through registers.  load_a(i, k) returns A[row, k .. k + 3] of the
// thread's row (tid / 4 + 64 i) of the tile, zero behind the k extent; Wt rows are o_dim long and zero behind k_dim.
template <int MB, int NB, bool SPLIT, class LoadA>
__device__ __forceinline__ void mfma_k_loop(const Wave &w, floatx16 (&acc)[MB][NB], float (&xs)[2][GP_KT][64 * MB + 1], float (&ws)[2][GP_KT][64 * NB], int k_dim, const LoadA &load_a,
                                            const float *__restrict__ wt, int o_dim, int col0) {
    const int xr = w.tid >> 2, xk = (w.tid & 3) * 4;
    float4 xv[MB], wv[NB];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < MB; ++i) xv[i] = load_a(i, k0 + xk);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int idx = w.tid + 256 * j, k = k0 + idx / (16 * NB), c = (idx % (16 * NB)) * 4;
            wv[j] = k < k_dim ? *reinterpret_cast<const float4 *>(wt + (long)k * o_dim + col0 + c) : f4_zero();
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const int r = xr + 64 * i;
            xs[buf][xk + 0][r] = xv[i].x; xs[buf][xk + 1][r] = xv[i].y; xs[buf][xk + 2][r] = xv[i].z; xs[buf][xk + 3][r] = xv[i].w;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int idx = w.tid + 256 * j;
            *reinterpret_cast<float4 *>(&ws[buf][idx / (16 * NB)][(idx % (16 * NB)) * 4]) = wv[j];
        }
    };
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc_zero(acc[i][j]);
    load(0);
    stage(0);
    __syncthreads();
    const int ntiles = (k_dim + GP_KT - 1) / GP_KT;
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) load((t + 1) * GP_KT);
#pragma unroll
        for (int k = 0; k < GP_KT; k += 2) {
            float a[MB], bq[NB];
#pragma unroll
            for (int i = 0; i < MB; ++i) a[i] = xs[cur][k + w.kh][sub_row<MB>(w, i) + w.l32];
#pragma unroll
            for (int j = 0; j < NB; ++j) bq[j] = ws[cur][k + w.kh][sub_col<NB, SPLIT>(w, j) + w.l32];
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bq[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < ntiles) stage(cur ^ 1);
        __syncthreads();
    }
}

// ---- the next layer out of a 64-row activation tile in LDS (act[k][GP_XS], nt k-tiles of GP_KT, zero-padded by its writer):
// 64 NQ output columns per pass, passes c_first, c_first + c_step, .. ; the W tiles (GP_KT x 64 NQ, rows behind k_dim and columns
// behind o_dim zero; o_dim % 4 == 0: a float4 is inside or outside as a whole) are double-buffered in wbuf[2][GP_KT][64 NQ].
// epi(acc, col) receives each accumulator with this lane's output column (which may lie behind o_dim).
// NQ = 2 (two accumulators per wave): half the barriers and half the reads of the activation of a 64-column pass.
template <int NQ, class Epi>
__device__ __forceinline__ void lds_layer(const Wave &w, const float *act, int nt, const float *__restrict__ wt, int k_dim, int o_dim,
                                          float *wbuf, int c_first, int c_step, Epi epi) {
    constexpr int TN = 64 * NQ;
    const int wk = w.tid / (16 * NQ), wc = (w.tid % (16 * NQ)) * 4;      // NQ float4 per thread: rows wk + (GP_KT / NQ) q
    const int npass = (o_dim + TN - 1) / TN;
    for (int c = c_first; c < npass; c += c_step) {
        const int col0 = c * TN;
        float4 wv[NQ];
        auto load = [&](int t) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int k = t * GP_KT + wk + (GP_KT / NQ) * q;
                wv[q] = (k < k_dim && col0 + wc < o_dim) ? *reinterpret_cast<const float4 *>(wt + (long)k * o_dim + col0 + wc) : f4_zero();
            }
        };
        auto stage = [&](int buf) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) *reinterpret_cast<float4 *>(wbuf + buf * GP_KT * TN + (wk + (GP_KT / NQ) * q) * TN + wc) = wv[q];
        };
        floatx16 acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc_zero(acc[q]);
        load(0);
        __syncthreads();                    // the activation tile is complete / the previous pass has left wbuf
        stage(0);
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const int cur = t & 1;
            if (t + 1 < nt) load(t + 1);
            const float *wl = wbuf + cur * GP_KT * TN;
#pragma unroll
            for (int k = 0; k < GP_KT; k += 2) {
                const float a = act[(t * GP_KT + k + w.kh) * GP_XS + w.ar];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wl[(k + w.kh) * TN + q * 64 + w.bc], acc[q], 0, 0, 0);
            }
            if (t + 1 < nt) stage(cur ^ 1);
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) epi(acc[q], col0 + q * 64 + w.bc);
    }
}

// ---- epilogues.  bias may be NULL; relu keeps a NaN (y < 0 ? 0 : y), like relu_
__device__ __forceinline__ float bias_relu(float y, float bv, int relu) {
    y += bv;
    if (relu) y = y < 0.f ? 0.f : y;
    return y;
}

// rows rbase .. rbase + 31 of the sub-tile -> out[row, col], rows < t_end only (t_end < 0: all).  acc_row is additive in its two
// arguments: the lane's part goes into the base pointer, the register's part is a constant multiple of ld per store
__device__ __forceinline__ void store_rows(const Wave &w, const floatx16 &acc, const float *__restrict__ bias, int relu, float *__restrict__ out,
                                           int ld, long rbase, int col, long t_end = -1) {
    const float bv = bias ? bias[col] : 0.f;
    const long r0 = rbase + acc_row(0, w.kh);
    float *o = out + r0 * (long)ld + col;
#pragma unroll
    for (int v = 0; v < 16; ++v)
        if (t_end < 0 || r0 + acc_row(v, 0) < t_end) o[(long)acc_row(v, 0) * ld] = bias_relu(acc[v], bv, relu);
}

// the wave's rows of channel col of an activation tile act[channel][GP_XS].  Columns o_valid .. (the zero padding of the next
// layer's k dimension) are written as zeros; o_valid < 0: none
__device__ __forceinline__ void store_act(const Wave &w, const floatx16 &acc, const float *__restrict__ bias, int relu, float *act, int col,
                                          int o_valid = -1) {
    const bool in = o_valid < 0 || col < o_valid;
    const float bv = (in && bias) ? bias[col] : 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const float y = bias_relu(acc[v], bv, relu);
        act[col * GP_XS + w.wm * 32 + acc_row(v, w.kh)] = in ? y : 0.f;
    }
}

// max over the groups of NS = 16 | 32 rows of the sub-tile that starts at row rbase (bias add and ReLU are monotone: they follow
// the max); a NaN propagates (gp_nanmax), like torch's relu + max_pool2d -- the compact pools differ on purpose (compact_pool.h)
template <int NS>
__device__ __forceinline__ void pool_rows(const Wave &w, const floatx16 &acc, const float *__restrict__ bias, int relu, float *__restrict__ out,
                                          long out_stride, long rbase, int col) {
    // G groups per sub-tile, R registers per group: rows 16 g .. 16 g + 15 are registers 8 g .. 8 g + 7 of the two halves of the wave
    constexpr int G = 32 / NS, R = 16 / G;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        float m = acc[R * gi];
#pragma unroll
        for (int v = 1; v < R; ++v) m = gp_nanmax(m, acc[R * gi + v]);
        m = gp_nanmax(m, __shfl_xor(m, 32));
        if (w.lane < 32) out[(rbase / NS + gi) * out_stride + col] = bias_relu(m, bv, relu);
    }
}

// ---- layer 1 of a set-abstraction SharedMLP per point (gemm_pool.hip, pgather_gemm2_kernel): the accumulators START at the
// gathered row of P = feats @ W_f and take two matrix steps for the centred coordinates [dx dy | dz 0] against W_x (3 x 64 NB1),
// then bias + ReLU into act[64 NB1][GP_XS].  src_of(tile row) -> {scene, scene * m + centre, source point}
struct PairRow { long scene, cm; int src; };
template <int NB1, class SrcOf>
__device__ __forceinline__ void ppoint_layer1(const Wave &w, SrcOf src_of, int n, const float *__restrict__ pmat, int p_stride,
                                              const float *__restrict__ xyz, const float *__restrict__ new_xyz, const float *__restrict__ w1x,
                                              const float *__restrict__ b1, int relu1, float *act) {
    constexpr int O1 = NB1 * 64;
    // this lane's row of the A operand: the centred coordinates, k = 0..3 -> (dx, dy | dz, 0) over the two halves of the wave
    float a0, a1;
    {
        const PairRow r = src_of(w.ar);
        const float *pr = xyz + ((size_t)r.scene * n + (size_t)r.src) * 3, *cr = new_xyz + (size_t)r.cm * 3;
        const float dx = pr[0] - cr[0], dy = pr[1] - cr[1], dz = pr[2] - cr[2];     // grouped_xyz -= new_xyz
        a0 = w.kh ? dy : dx;
        a1 = w.kh ? 0.f : dz;
    }
    floatx16 acc[NB1];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const PairRow r = src_of(w.wm * 32 + acc_row(v, w.kh));
        const float *prow = pmat + ((size_t)r.scene * n + (size_t)r.src) * p_stride + w.bc;
#pragma unroll
        for (int j = 0; j < NB1; ++j) acc[j][v] = prow[j * 64];
    }
#pragma unroll
    for (int j = 0; j < NB1; ++j) {
        const int col = j * 64 + w.bc;
        const float wb0 = w1x[w.kh * O1 + col];                         // k = 0 | 1: the x | y row of W_x
        const float wb1 = w.kh ? 0.f : w1x[2 * O1 + col];               // k = 2 | 3: the z row | the zero pad
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, wb0, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, wb1, acc[j], 0, 0, 0);
        store_act(w, acc[j], b1, relu1, act, col);
    }
}

}  // namespace ws3d
