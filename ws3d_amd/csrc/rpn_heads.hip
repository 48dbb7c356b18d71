// rpn_heads.hip -- the RPN's two heads (classification 128 -> 128 -> 1, regression 128 -> 128 -> o2) in ONE launch on the bf16
// matrix cores at fp32 accuracy.  Replaces, where the shapes fit, the two ws3d_mlp2_rows launches (sa_mlp.hip), which run the same
// two layers on v_mfma_f32_32x32x2_f32 at 64 cycles per k = 2 and are bound by it.
//
// The product is the split-bf16 one of split_bf16.h (three bf16 pieces per fp32 operand, six products per k-step on
// v_mfma_f32_32x32x16_bf16).
//
// A workgroup serves ONE head (one head's split first layer takes 104 KB of LDS; both do not fit): the first wg_cls workgroups of
// the grid the classification head, the others the regression head, each walking its head's 32-row tiles in chunks of 8 (one per
// wave) handed out by that head's ticket counter.  Both tickets hand out the tiles in ascending order at about the same pace, so the
// second head's read of a row tile finds it in the caches.  Per wave and tile:
//   * layer 1 TRANSPOSED, H^T = W1 X^T: A = W1's pieces (row = output channel, from LDS), B = the tile's rows split in registers
//     (col = row of the tile).  The four accumulators hold channel blk * 32 + (v & 3) + 8 (v >> 2) + 4 h of row (lane & 31) in
//     register v -- the layout in which the next product sums over the accumulator's ROW index with no lane movement.
//   * bias + ReLU in fp32 (a NaN stays NaN: a row that holds Inf / NaN gives non-finite outputs, as the fp32 kernels do).
//   * regression: Y^T = W2 H^T with B = the activations split in registers: registers 8 s .. 8 s + 7 of block blk are the
//     fragment of k-step (blk, s), element j of lane half h = channel blk * 32 + 16 s + 8 (j >> 2) + 4 h + (j & 3); W2 is packed
//     in that k order (ws3d_rpn_heads_pack).  The result has the output channel in the registers: four float4 stores per block.
//   * classification (o2 = 1): an fp32 dot product over the lane's 64 channels plus one add across the half-waves (an MFMA would
//     compute 31 padding columns).
// Every output element is computed by one wave in a fixed order: the ticket order changes no bit.
#include <algorithm>

#include "common.h"
#include "split_bf16.h"

namespace ws3d {

constexpr int HEADS_K = 128;                 // input channels = first-layer width
constexpr int HEADS_KS = HEADS_K + 8;        // bf16 row stride of a packed matrix: 272 B, ds_read_b128 conflict-free over 32 rows
constexpr int HEADS_THREADS = 512;           // 8 waves: two per SIMD, one workgroup per CU
constexpr int HEADS_MAX_O2 = 64;

// blob (= the LDS image) of one head, byte offsets; every piece 16-byte aligned
//   header   int {o2, relu1, relu2, 0}
//   W1P      [3][128][HEADS_KS] bf16: piece p of W1[o][k] (k contiguous, zero for k >= 128)
//   B1       [128] f32, B2 [64] f32 (zero behind o2; NULL biases pack as zero)
//   W2       o2 == 1: [128] f32, W2[0][k] in natural order;  o2 > 1: [3][o2][HEADS_KS] bf16, piece p of W2[o][ch(kk)] (k order above)
constexpr int HB_W1P = 16;
constexpr int HB_B1 = HB_W1P + 3 * HEADS_K * HEADS_KS * 2;
constexpr int HB_B2 = HB_B1 + 4 * HEADS_K;
constexpr int HB_W2 = HB_B2 + 4 * HEADS_MAX_O2;
__host__ __device__ constexpr int heads_blob_bytes(int o2) { return HB_W2 + (o2 == 1 ? 4 * HEADS_K : 3 * o2 * HEADS_KS * 2); }
static_assert(HB_W2 % 16 == 0 && heads_blob_bytes(HEADS_MAX_O2) <= 160 * 1024, "rpn_heads blob layout");

// packed k position kk (0 .. 127) of the regression head's second layer -> its input channel
__host__ __device__ constexpr int heads_w2_channel(int kk) {
    return (kk & ~31) + 16 * ((kk >> 4) & 1) + 8 * ((kk & 7) >> 2) + 4 * ((kk >> 3) & 1) + (kk & 3);
}

__global__ __launch_bounds__(256) void rpn_heads_pack_kernel(int o2, const float *__restrict__ w1t, const float *__restrict__ b1, int relu1,
                                                             const float *__restrict__ w2t, const float *__restrict__ b2, int relu2,
                                                             unsigned char *__restrict__ blob) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    if (t == 0) {
        int *hdr = reinterpret_cast<int *>(blob);
        hdr[0] = o2; hdr[1] = relu1; hdr[2] = relu2; hdr[3] = 0;
    }
    __bf16 *w1p = reinterpret_cast<__bf16 *>(blob + HB_W1P);
    for (int i = t; i < HEADS_K * HEADS_KS; i += nt) {
        const int o = i / HEADS_KS, k = i - o * HEADS_KS;
        __bf16 p1, p2, p3;
        split3(k < HEADS_K ? w1t[k * HEADS_K + o] : 0.f, p1, p2, p3);
        w1p[i] = p1; w1p[HEADS_K * HEADS_KS + i] = p2; w1p[2 * HEADS_K * HEADS_KS + i] = p3;
    }
    float *bb1 = reinterpret_cast<float *>(blob + HB_B1), *bb2 = reinterpret_cast<float *>(blob + HB_B2);
    for (int i = t; i < HEADS_K; i += nt) bb1[i] = b1 ? b1[i] : 0.f;
    for (int i = t; i < HEADS_MAX_O2; i += nt) bb2[i] = (b2 && i < o2) ? b2[i] : 0.f;
    if (o2 == 1) {
        float *w2 = reinterpret_cast<float *>(blob + HB_W2);
        for (int i = t; i < HEADS_K; i += nt) w2[i] = w2t[i];
    } else {
        __bf16 *w2p = reinterpret_cast<__bf16 *>(blob + HB_W2);
        for (int i = t; i < o2 * HEADS_KS; i += nt) {
            const int o = i / HEADS_KS, kk = i - o * HEADS_KS;
            __bf16 p1, p2, p3;
            split3(kk < HEADS_K ? w2t[heads_w2_channel(kk) * o2 + o] : 0.f, p1, p2, p3);
            w2p[i] = p1; w2p[o2 * HEADS_KS + i] = p2; w2p[2 * o2 * HEADS_KS + i] = p3;
        }
    }
}

// one head's share of the tiles; `lds` = the head's blob
template <int NB2>      // 0: the classification head (o2 = 1, VALU); 1 / 2: 32-column blocks of the regression head's second layer
__device__ __forceinline__ void rpn_head_walk(long tiles, const float *__restrict__ x, const unsigned char *lds, float *__restrict__ out,
                                              int *__restrict__ ticket, int *next_chunk, long chunk) {
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int *hdr = reinterpret_cast<const int *>(lds);
    const int o2 = hdr[0], relu1 = hdr[1], relu2 = hdr[2];
    const __bf16 *w1p = reinterpret_cast<const __bf16 *>(lds + HB_W1P) + r * HEADS_KS + 8 * h;
    const float *b1s = reinterpret_cast<const float *>(lds + HB_B1), *b2s = reinterpret_cast<const float *>(lds + HB_B2);
    constexpr int PIECE1 = HEADS_K * HEADS_KS;
    for (int par = 0; chunk * 8 < tiles; par ^= 1) {
        int ahead = 0;
        if (tid == 0) ahead = atomicAdd(ticket, 1);        // the next chunk, consumed after this chunk's work
        const long tile = chunk * 8 + (tid >> 6);
        if (tile < tiles) {
            // lane (r, h) feeds x[row r][16 s + 8 h + j] to k-step s (the B operand's map)
            float xv[64];
            const float4 *xp = reinterpret_cast<const float4 *>(x + (tile * 32 + r) * HEADS_K + 8 * h);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const float4 t0 = xp[4 * s], t1 = xp[4 * s + 1];
                xv[8 * s] = t0.x; xv[8 * s + 1] = t0.y; xv[8 * s + 2] = t0.z; xv[8 * s + 3] = t0.w;
                xv[8 * s + 4] = t1.x; xv[8 * s + 5] = t1.y; xv[8 * s + 6] = t1.z; xv[8 * s + 7] = t1.w;
            }
            floatx16 acc[4];
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[blk][i] = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                bf16x8 q1, q2, q3;
                split8(xv + 8 * s, q1, q2, q3);
#pragma unroll
                for (int blk = 0; blk < 4; ++blk) {
                    const __bf16 *wr = w1p + blk * 32 * HEADS_KS + 16 * s;
                    const bf16x8 a1 = *reinterpret_cast<const bf16x8 *>(wr);
                    const bf16x8 a2 = *reinterpret_cast<const bf16x8 *>(wr + PIECE1);
                    const bf16x8 a3 = *reinterpret_cast<const bf16x8 *>(wr + 2 * PIECE1);
                    split_mfma6<1>(a1, a2, a3, &q1, &q2, &q3, &acc[blk]);
                }
            }
            // bias + ReLU: register v of block blk = channel blk * 32 + (v & 3) + 8 (v >> 2) + 4 h of row r
#pragma unroll
            for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float y = acc[blk][v] + b1s[blk * 32 + (v & 3) + 8 * (v >> 2) + 4 * h];
                    acc[blk][v] = relu1 ? relu_keep_nan(y) : y;
                }
            if constexpr (NB2 == 0) {
                const float *w2s = reinterpret_cast<const float *>(lds + HB_W2);
                float p = 0.f;
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int v = 0; v < 16; ++v) p = __builtin_fmaf(acc[blk][v], w2s[blk * 32 + (v & 3) + 8 * (v >> 2) + 4 * h], p);
                const float q = __shfl_xor(p, 32);
                float y = (h ? q + p : p + q) + b2s[0];          // half 0's sum + half 1's in both halves
                if (relu2) y = relu_keep_nan(y);
                if (h == 0) out[tile * 32 + r] = y;
            } else {
                const __bf16 *w2p = reinterpret_cast<const __bf16 *>(lds + HB_W2);
                const int piece2 = o2 * HEADS_KS;
                floatx16 y[NB2];
#pragma unroll
                for (int ob = 0; ob < NB2; ++ob)
#pragma unroll
                    for (int i = 0; i < 16; ++i) y[ob][i] = 0.f;
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        bf16x8 q1, q2, q3;
                        float av[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[j] = acc[blk][8 * s + j];
                        split8(av, q1, q2, q3);
#pragma unroll
                        for (int ob = 0; ob < NB2; ++ob) {
                            // rows o >= o2 compute outputs nobody stores: they read the last row (no padding in the blob)
                            const int o = min(ob * 32 + r, o2 - 1);
                            const __bf16 *wr = w2p + o * HEADS_KS + blk * 32 + 16 * s + 8 * h;
                            const bf16x8 a1 = *reinterpret_cast<const bf16x8 *>(wr);
                            const bf16x8 a2 = *reinterpret_cast<const bf16x8 *>(wr + piece2);
                            const bf16x8 a3 = *reinterpret_cast<const bf16x8 *>(wr + 2 * piece2);
                            split_mfma6<1>(a1, a2, a3, &q1, &q2, &q3, &y[ob]);
                        }
                    }
                // register v of block ob = output channel ob * 32 + (v & 3) + 8 (v >> 2) + 4 h of row r
                float *orow = out + (tile * 32 + r) * (long)o2;
#pragma unroll
                for (int ob = 0; ob < NB2; ++ob)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int o0 = ob * 32 + 8 * g + 4 * h;
                        if (o0 < o2) {
                            float v4[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v4[e] = y[ob][4 * g + e] + b2s[o0 + e];
                                if (relu2) v4[e] = relu_keep_nan(v4[e]);
                            }
                            if (o2 % 4 == 0) {
                                *reinterpret_cast<float4 *>(orow + o0) = make_float4(v4[0], v4[1], v4[2], v4[3]);
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (o0 + e < o2) orow[o0 + e] = v4[e];
                            }
                        }
                    }
            }
        }
        if (tid == 0) next_chunk[par ^ 1] = ahead;
        __syncthreads();
        chunk = next_chunk[par ^ 1];
    }
}

template <int NB2>
__global__ __launch_bounds__(HEADS_THREADS) void rpn_heads_kernel(long tiles, const float *__restrict__ x, int wg_cls,
                                                                  const unsigned char *__restrict__ blob_cls, float *__restrict__ out_cls,
                                                                  int *__restrict__ ticket_cls, const unsigned char *__restrict__ blob_reg,
                                                                  float *__restrict__ out_reg, int *__restrict__ ticket_reg, int o2_reg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_heads[];
    __shared__ int next_chunk[2];
    const bool cls = (int)blockIdx.x < wg_cls;
    const unsigned char *blob = cls ? blob_cls : blob_reg;
    int *ticket = cls ? ticket_cls : ticket_reg;
    const int tid = threadIdx.x;
    if (tid == 0) next_chunk[0] = atomicAdd(ticket, 1);
    const int n16 = heads_blob_bytes(cls ? 1 : o2_reg) / 16;
    for (int i = tid; i < n16; i += HEADS_THREADS) reinterpret_cast<uint4 *>(smem_heads)[i] = reinterpret_cast<const uint4 *>(blob)[i];
    __syncthreads();
    const long chunk = next_chunk[0];
    if (cls)
        rpn_head_walk<0>(tiles, x, smem_heads, out_cls, ticket, next_chunk, chunk);
    else
        rpn_head_walk<NB2>(tiles, x, smem_heads, out_reg, ticket, next_chunk, chunk);
}

}  // namespace ws3d

extern "C" size_t ws3d_rpn_heads_blob_bytes(int o2) {
    return (o2 >= 1 && o2 <= ws3d::HEADS_MAX_O2) ? (size_t)ws3d::heads_blob_bytes(o2) : 0;
}

extern "C" int ws3d_rpn_heads_pack(int o2, const float *w1t, const float *b1, int relu1, const float *w2t, const float *b2, int relu2, void *blob,
                                   ws3d_stream_t stream) {
    using namespace ws3d;
    if (!w1t || !w2t || !blob || (reinterpret_cast<uintptr_t>(blob) & 15)) { set_error("ws3d_rpn_heads_pack: invalid argument"); return WS3D_E_INVALID; }
    if (ws3d_rpn_heads_blob_bytes(o2) == 0) {
        set_error("ws3d_rpn_heads_pack: unsupported o2 = %d (1 .. %d)", o2, HEADS_MAX_O2);
        return WS3D_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(rpn_heads_pack_kernel, dim3(64), dim3(256), 0, as_stream(stream), o2, w1t, b1, relu1 ? 1 : 0, w2t, b2, relu2 ? 1 : 0,
                       static_cast<unsigned char *>(blob));
    return check_launch("ws3d_rpn_heads_pack");
}

extern "C" int ws3d_rpn_heads(long rows, const float *x_rows, int heads, const void *blob_cls, float *out_cls, int *ticket_cls, int o2_reg,
                              const void *blob_reg, float *out_reg, int *ticket_reg, int workgroups, ws3d_stream_t stream) {
    using namespace ws3d;
    const bool do_cls = heads & 1, do_reg = heads & 2;
    const uintptr_t al = reinterpret_cast<uintptr_t>(x_rows) | reinterpret_cast<uintptr_t>(do_cls ? blob_cls : nullptr) |
                         reinterpret_cast<uintptr_t>(do_reg ? blob_reg : nullptr) | reinterpret_cast<uintptr_t>(do_reg && o2_reg % 4 == 0 ? out_reg : nullptr);
    if (rows < 0 || (heads & ~3) || !heads || !x_rows || (al & 15) || (do_cls && (!blob_cls || !out_cls || !ticket_cls)) ||
        (do_reg && (!blob_reg || !out_reg || !ticket_reg))) {
        set_error("ws3d_rpn_heads: invalid argument (rows=%ld heads=%d)", rows, heads);
        return WS3D_E_INVALID;
    }
    if ((rows & 31) || (do_reg && ws3d_rpn_heads_blob_bytes(o2_reg) == 0) || (do_reg && o2_reg == 1)) {
        set_error("ws3d_rpn_heads: unsupported shape (rows=%ld o2=%d; rows %% 32, 2 <= o2 <= %d)", rows, o2_reg, HEADS_MAX_O2);
        return WS3D_E_UNSUPPORTED;
    }
    if (rows == 0) return WS3D_OK;
    const long tiles = rows / 32, chunks = (tiles + 7) / 8;
    // the regression head's tile costs 288 bf16 MFMAs, the classification head's 192 + a dot product: 2 : 3 of the workgroups
    const long wgs_all = workgroups > 0 ? workgroups : cu_count();
    long wg_cls = 0, wg_reg = 0;
    if (do_cls && do_reg) {
        wg_cls = std::max(1L, std::min(chunks, (wgs_all * 2 + 2) / 5));
        wg_reg = std::max(1L, std::min(chunks, wgs_all - wg_cls));
    } else {
        (do_cls ? wg_cls : wg_reg) = std::max(1L, std::min(chunks, wgs_all));
    }
    const size_t lds = (size_t)std::max(heads_blob_bytes(1), do_reg ? heads_blob_bytes(o2_reg) : 0);
    auto go = [&](auto kern) -> int {
        if (int rc = raise_lds_cap((const void *)kern, lds, "ws3d_rpn_heads")) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)(wg_cls + wg_reg)), dim3(HEADS_THREADS), lds, as_stream(stream), tiles, x_rows, (int)wg_cls,
                           static_cast<const unsigned char *>(blob_cls), out_cls, ticket_cls, static_cast<const unsigned char *>(blob_reg), out_reg,
                           ticket_reg, o2_reg);
        return WS3D_OK;
    };
    if (int rc = (do_reg && o2_reg > 32) ? go(rpn_heads_kernel<2>) : go(rpn_heads_kernel<1>)) return rc;
    return check_launch("ws3d_rpn_heads");
}
