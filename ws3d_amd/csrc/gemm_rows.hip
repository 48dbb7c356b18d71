// gemm_rows.hip -- a plain row GEMM on the bf16 matrix cores at fp32 accuracy: out (rows, N) = act(A (rows, K) @ Wt (K, N) + bias).
// Takes over, shape by shape, the products the channels-last Stage-1 path otherwise hands to the BLAS library (fastpath._split_gemm):
// those run at the fp32 MFMA roof (v_mfma_f32_32x32x2_f32) once 20 graphs are in flight, and only a cheaper product moves that roof
// (DESIGN.md section 10.3).
//
// The product is the split-bf16 one of split_bf16.h (as csrc/rpn_heads.hip): three bf16 pieces per fp32
// operand, six products per k-step on v_mfma_f32_32x32x16_bf16 into one fp32 accumulator.
//
// Geometry.  A workgroup of four waves computes one tile of 64 rows x 128 columns (128 x 128 from 512 such tiles on; N % 128 != 0:
// 64 x 64), TRANSPOSED like the heads: the MFMA's A operand is the weights (row = output column), its B operand the rows of A (col =
// row of the tile), so a lane ends up with four consecutive output columns of one row per register quad -- 16-byte stores.  Wave w
// owns the 32-column block w of the tile and all its 32-row blocks (64 x 64 tile: one block per wave).  K is walked in blocks of 32:
//   * Wt is split ONCE (ws3d_gemm_rows_pack: the folded inference weights are constant from call to call) into the exact image the
//     kernel reads: per k-block, per 32-column block, per k-step of 16, per piece one 1 KiB FRAGMENT = lane l's eight bf16 at byte
//     16 l (lane (r, h): column 32 nb + r, k = 32 kb + 16 s + 8 h .. + 7).  A wave fetches the six fragments of its column block and
//     k-block with six coalesced 16-byte loads STRAIGHT INTO REGISTERS, one k-block ahead of their use: no other wave of the
//     workgroup reads them, so they never pass through LDS (the first version staged them there: profiles/gemm_rows_vs_library.txt).
//   * A is read as fp32 (global -> registers while the current block's MFMAs run), split in registers, and its pieces are written to
//     LDS in the same fragment order (lane (r, h): row 32 mb + r), double-buffered, ONE barrier per k-block; every wave reads all of
//     them.  A ds_read_b128 of a fragment touches every bank once.  No pre-split copy of A exists in HBM.  The staging lanes take
//     eight consecutive rows per eight lanes: their 16-byte LDS writes fill one 128-byte bank row, their loads cover whole lines.
// Per wave and k-step: 6 ds_read_b128 for 12 MFMAs (128-row tile: 12 for 24).  24 KiB of LDS and <= 128 VGPRs (128-row tile: 48 KiB,
// 192 VGPRs): at least two workgroups per CU, two waves per SIMD.
//
// No split-K, no atomics: every output element is summed by one wave in ascending k, so the grid and the tile order change no bit.
// Bias is added in fp32 after the accumulation; the ReLU keeps a NaN (a row that holds Inf / NaN gives non-finite outputs in that row
// only: its pieces meet the other rows' columns of the MFMA's B operand nowhere).
#include "common.h"
#include "split_bf16.h"

namespace ws3d {

typedef unsigned rows_u4 __attribute__((ext_vector_type(4)));      // 16 bytes of the packed image
typedef float rows_f4 __attribute__((ext_vector_type(4)));

constexpr int GR_THREADS = 256;
constexpr int GR_TM = 64;                    // rows % GR_TM == 0 is the cover; a tile is 64 or 128 rows
constexpr int GR_KB = 32;                    // k per LDS stage: two k-steps of 16
constexpr int GR_FRAG = 1024;                // bytes of one fragment (64 lanes x 8 bf16)
#ifndef WS3D_GR_TALL_MIN_TILES
#define WS3D_GR_TALL_MIN_TILES 512
#endif
constexpr int GR_TALL_MIN_TILES = WS3D_GR_TALL_MIN_TILES;       // 128-row tiles from this many on (a tuning macro for A/B builds)
constexpr int GR_MAX_DIM = 4096;             // K, N (the grid and every index stay far inside 32 / 64 bits)
__host__ __device__ constexpr int gr_tile_rows(int nbt, int mbw) { return nbt == 4 ? 32 * mbw : 64 * mbw; }
__host__ __device__ constexpr int gr_a_stage(int tm) { return tm / 32 * 2 * 3 * GR_FRAG; }       // [row block][k-step 2][piece 3]
__host__ __device__ constexpr int gr_lds_bytes(int tm) { return 2 * gr_a_stage(tm); }              // double-buffered
static_assert(gr_lds_bytes(128) <= 64 * 1024 && gr_lds_bytes(128) * 2 <= 160 * 1024, "inside the default per-workgroup cap, two workgroups per CU");

// one thread per (k-block, column block, k-step, lane): eight weights of one column -> the lane's 16 bytes of three fragments
__global__ __launch_bounds__(256) void gemm_rows_pack_kernel(int K, int N, const float *__restrict__ wt, rows_u4 *__restrict__ pack) {
    const int nb_all = N / 32;
    const long total = (long)(K / GR_KB) * nb_all * 2 * 64;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63), s = (int)((i >> 6) & 1);
        const long f = i >> 7;                         // kb * nb_all + nb
        const int nb = (int)(f % nb_all), kb = (int)(f / nb_all);
        const int col = nb * 32 + (lane & 31), k0 = kb * GR_KB + 16 * s + 8 * (lane >> 5);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = wt[(long)(k0 + j) * N + col];
        bf16x8 q1, q2, q3;
        split8(v, q1, q2, q3);
        rows_u4 *dst = pack + ((f * 2 + s) * 3) * 64 + lane;
        dst[0] = __builtin_bit_cast(rows_u4, q1);
        dst[64] = __builtin_bit_cast(rows_u4, q2);
        dst[128] = __builtin_bit_cast(rows_u4, q3);
    }
}

// NBT: 32-column blocks of a tile, 4 (N % 128 == 0: wave w owns column block w and all MBW row blocks) or 2 (wave w owns column block
// w & 1 and the MBW row blocks of row half w >> 1).  MBW: 32-row blocks per wave.  Rows of a tile: 32 MBW (NBT 4), 64 MBW (NBT 2).
template <int NBT, int MBW>
__global__ __launch_bounds__(GR_THREADS, 2) void gemm_rows_kernel(int K, int N, int ntn, const float *__restrict__ a, const rows_u4 *__restrict__ pack,
                                                                  const float *__restrict__ bias, int relu, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_rows[];
    constexpr int TM = gr_tile_rows(NBT, MBW);
    constexpr int UNITS = TM / 64;                                // (row, 8 k) units a thread stages per k-block
    constexpr int STAGE = gr_a_stage(TM);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int tn = (int)(blockIdx.x % (unsigned)ntn);             // the column tiles of one row tile are neighbours in the grid: A is read from HBM once
    const long tm = blockIdx.x / (unsigned)ntn;
    const int nb_all = N / 32, nkb = K / GR_KB;
    const int nbl = NBT == 4 ? w : (w & 1), mb0 = NBT == 4 ? 0 : (w >> 1) * MBW;

    // staging role: unit u = row srow + 64 u of the tile, k = 8 skq .. + 7 of the block (eight lanes = eight consecutive rows)
    const int srow = (lane & 7) + 8 * (lane >> 5) + 16 * w, skq = (lane >> 3) & 3;
    const rows_f4 *ap = reinterpret_cast<const rows_f4 *>(a + (tm * TM + srow) * (long)K + 8 * skq);
    const size_t a_unit = (size_t)16 * K;                         // 64 rows further, in 16-byte steps
    const int a_wr = ((srow >> 5) * 2 + (skq >> 1)) * 3 * GR_FRAG + ((skq & 1) * 32 + (srow & 31)) * 16;
    // the wave's own six weight fragments of a k-block ([k-step 2][piece 3]) straight from the packed image: no other wave of the
    // workgroup reads them, so they do not pass through LDS
    const rows_u4 *wp = pack + (size_t)(tn * NBT + nbl) * 6 * 64 + lane;
    const size_t w_kb = (size_t)nb_all * 6 * 64;

    floatx16 acc[MBW];
#pragma unroll
    for (int m = 0; m < MBW; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    rows_u4 wc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) wc[i] = rows_u4{0u, 0u, 0u, 0u};

    // pass kb = -1 only fetches block 0; pass kb computes block kb while block kb + 1 travels global -> registers, then splits its rows
    // into the LDS buffer every wave left before the last barrier
    for (int kb = -1; kb < nkb; ++kb) {
        const bool more = kb + 1 < nkb;
        rows_f4 ra[UNITS][2];
        rows_u4 wn[6];
        if (more) {
#pragma unroll
            for (int u = 0; u < UNITS; ++u) {
                ra[u][0] = ap[u * a_unit + (kb + 1) * (GR_KB / 4)];
                ra[u][1] = ap[u * a_unit + (kb + 1) * (GR_KB / 4) + 1];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) wn[i] = wp[(kb + 1) * w_kb + i * 64];
        }
        if (kb >= 0) {
            const unsigned char *buf = smem_rows + (kb & 1) * STAGE + lane * 16;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 w1 = __builtin_bit_cast(bf16x8, wc[3 * s]), w2 = __builtin_bit_cast(bf16x8, wc[3 * s + 1]),
                               w3 = __builtin_bit_cast(bf16x8, wc[3 * s + 2]);
                bf16x8 a1[MBW], a2[MBW], a3[MBW];
#pragma unroll
                for (int m = 0; m < MBW; ++m) {
                    const unsigned char *af = buf + ((mb0 + m) * 2 + s) * 3 * GR_FRAG;
                    a1[m] = *reinterpret_cast<const bf16x8 *>(af);
                    a2[m] = *reinterpret_cast<const bf16x8 *>(af + GR_FRAG);
                    a3[m] = *reinterpret_cast<const bf16x8 *>(af + 2 * GR_FRAG);
                }
                // the row blocks' chains interleaved (each accumulator is summed in the same order)
                split_mfma6<MBW>(w1, w2, w3, a1, a2, a3, acc);
            }
        }
        if (more) {
            unsigned char *nxt = smem_rows + ((kb + 1) & 1) * STAGE + a_wr;
#pragma unroll
            for (int u = 0; u < UNITS; ++u) {
                const float v[8] = {ra[u][0][0], ra[u][0][1], ra[u][0][2], ra[u][0][3], ra[u][1][0], ra[u][1][1], ra[u][1][2], ra[u][1][3]};
                bf16x8 q1, q2, q3;
                split8(v, q1, q2, q3);
                *reinterpret_cast<bf16x8 *>(nxt + u * 12 * GR_FRAG) = q1;                 // 64 rows = two row blocks of [k-step 2][piece 3] further
                *reinterpret_cast<bf16x8 *>(nxt + u * 12 * GR_FRAG + GR_FRAG) = q2;
                *reinterpret_cast<bf16x8 *>(nxt + u * 12 * GR_FRAG + 2 * GR_FRAG) = q3;
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) wc[i] = wn[i];
        }
        __syncthreads();
    }

    // register v of a block = output column 32 nb + (v & 3) + 8 (v >> 2) + 4 h of row 32 mb + r
    const int n0 = (tn * NBT + nbl) * 32 + 4 * h;
    rows_f4 b4[4];
    if (bias) {
#pragma unroll
        for (int g = 0; g < 4; ++g) b4[g] = *reinterpret_cast<const rows_f4 *>(bias + n0 + 8 * g);
    }
#pragma unroll
    for (int m = 0; m < MBW; ++m) {
        float *orow = out + (tm * TM + (mb0 + m) * 32 + r) * (long)N + n0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            rows_f4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = acc[m][4 * g + e];
            if (bias) y = y + b4[g];                              // fp32, after the accumulation (no bias: -0 stays -0)
            if (relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = relu_keep_nan(y[e]);
            }
            *reinterpret_cast<rows_f4 *>(orow + 8 * g) = y;
        }
    }
}

static bool gr_dims_ok(int K, int N) { return K >= GR_KB && K <= GR_MAX_DIM && K % GR_KB == 0 && N >= 64 && N <= GR_MAX_DIM && N % 64 == 0; }

}  // namespace ws3d

extern "C" size_t ws3d_gemm_rows_pack_bytes(int k_dim, int n_dim) {
    return ws3d::gr_dims_ok(k_dim, n_dim) ? (size_t)k_dim * n_dim * 6 : 0;
}

extern "C" int ws3d_gemm_rows_pack(int k_dim, int n_dim, const float *wt, void *pack, ws3d_stream_t stream) {
    using namespace ws3d;
    if (!wt || !pack || (reinterpret_cast<uintptr_t>(pack) & 15) || (reinterpret_cast<uintptr_t>(wt) & 3)) {
        set_error("ws3d_gemm_rows_pack: invalid argument");
        return WS3D_E_INVALID;
    }
    if (!gr_dims_ok(k_dim, n_dim)) {
        set_error("ws3d_gemm_rows_pack: unsupported shape K=%d N=%d (K %% 32, N %% 64, both <= %d)", k_dim, n_dim, GR_MAX_DIM);
        return WS3D_E_UNSUPPORTED;
    }
    const long threads = (long)(k_dim / GR_KB) * (n_dim / 32) * 128;
    hipLaunchKernelGGL(gemm_rows_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream), k_dim, n_dim, wt,
                       static_cast<rows_u4 *>(pack));
    return check_launch("ws3d_gemm_rows_pack");
}

extern "C" int ws3d_gemm_rows_split(long rows, int k_dim, int n_dim, const float *a, const void *pack, const float *bias, int relu, float *out,
                                    ws3d_stream_t stream) {
    using namespace ws3d;
    if (rows < 0 || k_dim <= 0 || n_dim <= 0 || !a || !pack || !out) {
        set_error("ws3d_gemm_rows_split: invalid argument (rows=%ld K=%d N=%d)", rows, k_dim, n_dim);
        return WS3D_E_INVALID;
    }
    const uintptr_t al = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(pack) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(bias);
    const int nbt = n_dim % 128 == 0 ? 4 : 2;
    if (!gr_dims_ok(k_dim, n_dim) || rows % GR_TM || (al & 15) || (rows / GR_TM) * (n_dim / (32 * nbt)) > 0x7fffffffL) {
        set_error("ws3d_gemm_rows_split: unsupported shape or alignment (rows=%ld K=%d N=%d; rows %% 64, K %% 32, N %% 64, 16-byte pointers)", rows,
                  k_dim, n_dim);
        return WS3D_E_UNSUPPORTED;
    }
    if (rows == 0) return WS3D_OK;
    const int ntn = n_dim / (32 * nbt);
    // 128-row tiles (each weight fragment fetched once per 128 rows, four MFMA chains per wave) where they still give every CU two
    // workgroups; the tile shape changes no bit
    const bool tall = nbt == 4 && rows % 128 == 0 && (rows / 128) * ntn >= GR_TALL_MIN_TILES;
    const int tm = tall ? 128 : 64;
    const unsigned grid = (unsigned)((rows / tm) * ntn);
    auto go = [&](auto kern) -> int {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(GR_THREADS), (size_t)gr_lds_bytes(tm), as_stream(stream), k_dim, n_dim, ntn, a,
                           static_cast<const rows_u4 *>(pack), bias, relu ? 1 : 0, out);
        return WS3D_OK;
    };
    if (int rc = nbt == 2 ? go(gemm_rows_kernel<2, 1>) : tall ? go(gemm_rows_kernel<4, 4>) : go(gemm_rows_kernel<4, 2>)) return rc;
    return check_launch("ws3d_gemm_rows_split");
}
