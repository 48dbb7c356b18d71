// stage2_ragged.hip -- the geometry of Stage 2 on WHOLE instance clouds of different sizes (include/ws3d_ops.h): what the first
// set-abstraction level and the IoU tower's canonical transform need so that a packed batch of ragged clouds runs as one call instead
// of one rcnn_forward per cloud (tools/eval_auto.py:286-403 feeds every cylinder as it is, 1 to several thousand points).
// Cloud i owns the packed rows offsets[i] .. offsets[i+1] throughout.
//   ws3d_stage2_canonical_ragged                 the canonical transform of ws3d_stage2_embed, the box keyed by the row's cloud
//   ws3d_furthest_point_sampling_ragged_gather   fps_ragged.hip's sampler + the sampled coordinates, m may exceed n_i
//   ws3d_ball_query_ragged                       ball_query_kernel_fast per cloud, lists local or as rows of the packed array
#include <math.h>

#include "fps_ragged.h"
#include "mfma_tile.h"

namespace ws3d {

// the cloud of packed row r: the last i with offsets[i] <= r (offsets ascending, offsets[0] = 0, r < offsets[clouds])
__device__ __forceinline__ int ragged_cloud_of(const int32_t *__restrict__ offsets, int clouds, int r) {
    int lo = 0, hi = clouds;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ canonical transform
// One thread per row; the row finds its cloud by a binary search over offsets (9 cached loads for 511 clouds), so nothing depends on
// clouds being aligned to anything.  The arithmetic is stage2_embed_kernel's, statement for statement (rcnn_net.py:338-351).
__global__ __launch_bounds__(256) void stage2_canonical_ragged_kernel(int rows, int clouds, const int32_t *__restrict__ offsets,
                                                                      const float *__restrict__ pts, const float *__restrict__ box_ce,
                                                                      float extend, float *__restrict__ pts_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float *p = pts + (size_t)r * 5;
    float x = p[0], y = p[1], z = p[2];
    const float f0 = p[3], f1 = p[4];
    const float *b = box_ce + (size_t)ragged_cloud_of(offsets, clouds, r) * 7;
    x = x - b[0]; y = y - b[1]; z = z - b[2];
    const float a = -b[6], c = cosf_cr(a), s = sinf_cr(a);
    float cx = x * c + z * s;
    float cz = x * (-s) + z * c;
    cx = cx / (b[5] / 2.f);
    float cy = y / (b[3] / 2.f);
    cz = cz / (b[4] / 2.f);
    const float m = gp_nanmax(gp_nanmax(fabsf(cx), fabsf(cy)), fabsf(cz));
    const bool outside = m > extend;
    float *o = pts_out + (size_t)r * 5;
    o[0] = outside ? 0.f : cx; o[1] = outside ? 0.f : cy; o[2] = outside ? 0.f : cz; o[3] = f0; o[4] = f1;
}

// ------------------------------------------------------------------------------------------------ sampling + gather
// fps_ragged_kernel with the n < m gate lifted and the coordinates written.  Nothing in ragged_cloud needs m <= n: once the
// distinct points are used up every running minimum is 0, every valid slot ties, and "lowest slot, lowest lane, lowest wave" returns
// tie-order position 0 = point 0 -- what sampling_gpu.cu:93-209 returns (every thread keeps its first k, the tree keeps thread 0).
__global__ __launch_bounds__(RAGGED_NT) void fps_ragged_gather_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ offsets,
                                                                      int32_t *__restrict__ idx, float *__restrict__ new_xyz, int total, int m,
                                                                      int limit) {
    __shared__ float4 s_cand[2][16];
    __shared__ int s_k[2][16];
    const int c = blockIdx.x;
    const int off = offsets[c];
    const int n = offsets[c + 1] - off;
    // larger clouds belong to the per-cloud kernel (the C entry launches it); a device array that disagrees with the validated host
    // sizes touches nothing
    if (n < 1 || n > limit || off < 0 || n > total - off) return;
    xyz += (size_t)off * 3;
    idx += (size_t)c * m;
    new_xyz += (size_t)c * m * 3;
    int log2bs = 31 - __builtin_clz((unsigned)n);
    if (log2bs > 10) log2bs = 10;
    const int bs = 1 << log2bs;
    const int S = (n + bs - 1) / bs;
    const int R = bs * S;
    const int ppt = (R + RAGGED_NT - 1) / RAGGED_NT;
    if (threadIdx.x == 0) {
        idx[0] = 0;
        new_xyz[0] = xyz[0]; new_xyz[1] = xyz[1]; new_xyz[2] = xyz[2];
    }
    if (ppt <= 1) ragged_cloud<1>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 2) ragged_cloud<2>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 4) ragged_cloud<4>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 8) ragged_cloud<8>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else ragged_cloud<16>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    // positions -> point indices and the coordinates, off the critical path (thread 0 wrote idx[])
    __syncthreads();
    for (int j = 1 + threadIdx.x; j < m; j += RAGGED_NT) {
        const int p = idx[j];
        const int rb = p / S, sl = p - rb * S;
        int k = ragged_bitrev(rb, log2bs) + sl * bs;
        k = k < n ? k : 0;                                // (never taken: a chosen position is a valid one)
        idx[j] = k;
        new_xyz[j * 3 + 0] = xyz[k * 3 + 0]; new_xyz[j * 3 + 1] = xyz[k * 3 + 1]; new_xyz[j * 3 + 2] = xyz[k * 3 + 2];
    }
}

// ------------------------------------------------------------------------------------------------ ball query
// Grid = (cloud, tile of BQR_CT centres): a 4500-point cloud with 128 centres spreads over 8 workgroups, a 67-point cloud costs 8
// short ones.  256 threads = 4 waves; wave w owns BQR_CW = 4 centres of the tile.  The cloud streams through LDS in chunks of BQR_CH
// points (xyz interleaved as in memory: a lane's three reads have stride 3 words, conflict free); per step of 64 points a lane reads
// ITS point once and tests it against the wave's four centres.  The reference's ascending order (ball_query_gpu.cu:29-44) comes from
// ballot + prefix popcount: hit number cnt + mbcnt(mask) goes to slot of that number, slots >= nsample are dropped.  The lists live
// in an LDS row per centre until the end, when lane l writes slot l: hits first, then the first hit repeated (the reference fills all
// slots at its first hit), 0 for a centre without a hit; global_rows adds the cloud's first row to every entry.
// A centre leaves the scan when it is full (wave-uniform test) and the workgroup leaves the chunk loop when all 16 are: in the IoU
// tower most of a cylinder is zeroed to the origin, a centre there fills from its first 64-point step, and a tile of such centres
// reads one chunk however long the cloud is.
// LDS: 3 * 1024 floats + 16 rows of 64 ints + 4 flags = 16,400 bytes; no atomics, no scratch, every element of idx written.
// Compile remarks (tests/test_stage2_ragged.py): no spills, no scratch; registers for 8 waves per SIMD in the canonical and the
// ball-query kernel (whose 16,400 bytes of LDS allow 9 workgroups = 9 waves per SIMD on a CU: no tighter), 6 in the sampler, which
// holds up to 16 points per lane in registers like fps_ragged_kernel and 640 bytes of LDS.
constexpr int BQR_NT = 256, BQR_NW = BQR_NT / WS3D_WAVE, BQR_CW = 4, BQR_CT = BQR_NW * BQR_CW, BQR_CH = 1024, BQR_MAX_NS = 64;

__global__ __launch_bounds__(BQR_NT) void ball_query_ragged_kernel(int tiles, int m, float radius, int nsample, const int32_t *__restrict__ offsets,
                                                                   const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                                   int global_rows, int32_t *__restrict__ idx) {
    __shared__ float s_pts[BQR_CH * 3];
    __shared__ int s_row[BQR_CT][BQR_MAX_NS];
    __shared__ int s_full[BQR_NW];
    const int cloud = blockIdx.x / tiles, tile = blockIdx.x - cloud * tiles;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int off = offsets[cloud];
    int n = offsets[cloud + 1] - off;
    if (off < 0 || n < 0) n = 0;                          // offsets that describe nothing: no point is read, the rows get zeros
    const float radius2 = radius * radius;
    const int c0 = tile * BQR_CT + w * BQR_CW;            // this wave's first centre
    float cx[BQR_CW], cy[BQR_CW], cz[BQR_CW];
    int cnt[BQR_CW];
#pragma unroll
    for (int c = 0; c < BQR_CW; ++c) {
        const bool real = c0 + c < m;
        const float *q = new_xyz + ((size_t)cloud * m + (real ? c0 + c : 0)) * 3;
        cx[c] = q[0]; cy[c] = q[1]; cz[c] = q[2];
        cnt[c] = real ? 0 : nsample;                      // a centre past the tile's tail is full from the start
    }
    const float *src = xyz + (size_t)off * 3;
    for (int base = 0; base < n; base += BQR_CH) {
        const int cn = min(BQR_CH, n - base);
        for (int i = tid; i < cn * 3; i += BQR_NT) s_pts[i] = src[(size_t)base * 3 + i];
        __syncthreads();
        for (int q0 = 0; q0 < cn; q0 += 64) {
            bool open = false;
#pragma unroll
            for (int c = 0; c < BQR_CW; ++c) open = open || cnt[c] < nsample;
            if (!open) break;
            const int q = q0 + lane;
            const bool in = q < cn;
            const int qc = in ? q : 0;
            const float px = s_pts[qc * 3 + 0], py = s_pts[qc * 3 + 1], pz = s_pts[qc * 3 + 2];
#pragma unroll
            for (int c = 0; c < BQR_CW; ++c) {
                if (cnt[c] < nsample) {                   // wave-uniform
                    const bool hit = in && sqdist3(cx[c] - px, cy[c] - py, cz[c] - pz) < radius2;
                    const uint64_t mask = __ballot(hit);
                    const int pos = cnt[c] + mbcnt(mask);
                    if (hit && pos < nsample) s_row[w * BQR_CW + c][pos] = base + q;
                    cnt[c] = min(cnt[c] + (int)__popcll(mask), nsample);
                }
            }
        }
        bool full = true;
#pragma unroll
        for (int c = 0; c < BQR_CW; ++c) full = full && cnt[c] >= nsample;
        if (lane == 0) s_full[w] = full ? 1 : 0;
        __syncthreads();                                  // the chunk is consumed, the flags and the rows are visible
        int all = 1;
#pragma unroll
        for (int v = 0; v < BQR_NW; ++v) all &= s_full[v];
        if (all) break;                                   // block-uniform
    }
    // (an empty cloud never entered the loop and wrote nothing to s_row: cnt == 0 reads none of it)
    const int add = global_rows ? off : 0;
    if (lane < nsample) {
#pragma unroll
        for (int c = 0; c < BQR_CW; ++c) {
            if (c0 + c < m) {
                const int *row = s_row[w * BQR_CW + c];
                const int v = cnt[c] == 0 ? 0 : row[lane < cnt[c] ? lane : 0];
                idx[((size_t)cloud * m + c0 + c) * nsample + lane] = v + add;
            }
        }
    }
}

// the host copy of the sizes: every cloud non-empty, the total within the 32-bit offsets; -> total, or -1 after set_error
static long ragged_total(const char *what, int clouds, const int32_t *sizes_host) {
    long total = 0;
    for (int i = 0; i < clouds; ++i) {
        if (sizes_host[i] < 1) {
            set_error("%s: invalid argument (cloud %d holds %d points)", what, i, sizes_host[i]);
            return -1;
        }
        total += sizes_host[i];
    }
    if (total > 0x7fffffffL / 5) {
        set_error("%s: invalid argument (%ld points exceed the 32-bit offsets)", what, total);
        return -1;
    }
    return total;
}

}  // namespace ws3d

using namespace ws3d;

extern "C" int ws3d_stage2_canonical_ragged(int rows, int clouds, const int32_t *offsets, const float *pts, const float *box_ce, float extend,
                                            float *pts_out, ws3d_stream_t stream) {
    if (rows < 0 || clouds < 0 || (rows > 0 && (clouds < 1 || !offsets || !pts || !box_ce || !pts_out)) || rows > 0x7fffffff / 5) {
        set_error("ws3d_stage2_canonical_ragged: invalid argument (rows=%d clouds=%d)", rows, clouds);
        return WS3D_E_INVALID;
    }
    if (rows == 0) return WS3D_OK;
    hipLaunchKernelGGL(stage2_canonical_ragged_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, as_stream(stream), rows, clouds, offsets,
                       pts, box_ce, extend, pts_out);
    return check_launch("ws3d_stage2_canonical_ragged");
}

extern "C" int ws3d_furthest_point_sampling_ragged_gather(int clouds, const int32_t *offsets, const int32_t *sizes_host, int m, const float *xyz,
                                                          int32_t *idx, float *new_xyz, ws3d_stream_t stream) {
    const char *what = "ws3d_furthest_point_sampling_ragged_gather";
    if (clouds < 0 || m < 0 || (clouds > 0 && (!offsets || !sizes_host || !xyz || ((!idx || !new_xyz) && m > 0)))) {
        set_error("%s: invalid argument (clouds=%d m=%d)", what, clouds, m);
        return WS3D_E_INVALID;
    }
    if (clouds == 0) return WS3D_OK;
    const long total = ragged_total(what, clouds, sizes_host);
    if (total < 0) return WS3D_E_INVALID;
    if (m == 0) return WS3D_OK;
    const int limit = ragged_limit();
    hipLaunchKernelGGL(fps_ragged_gather_kernel, dim3(clouds), dim3(RAGGED_NT), 0, as_stream(stream), xyz, offsets, idx, new_xyz, (int)total, m, limit);
    if (int rc = check_launch(what)) return rc;
    long off = 0;
    for (int i = 0; i < clouds; ++i) {
        if (sizes_host[i] > limit)
            if (int rc = ws3d_furthest_point_sampling_gather(1, sizes_host[i], m, xyz + off * 3, nullptr, idx + (size_t)i * m,
                                                             new_xyz + (size_t)i * m * 3, stream))
                return rc;
        off += sizes_host[i];
    }
    return WS3D_OK;
}

extern "C" int ws3d_ball_query_ragged(int clouds, const int32_t *offsets, int m, float radius, int nsample, const float *xyz, const float *new_xyz,
                                      int global_rows, int32_t *idx, ws3d_stream_t stream) {
    if (clouds < 0 || m < 0 || nsample < 1 || ((long)clouds * m > 0 && (!offsets || !xyz || !new_xyz || !idx))) {
        set_error("ws3d_ball_query_ragged: invalid argument (clouds=%d m=%d nsample=%d)", clouds, m, nsample);
        return WS3D_E_INVALID;
    }
    if (nsample > BQR_MAX_NS) {
        set_error("ws3d_ball_query_ragged: nsample=%d, at most %d are supported", nsample, BQR_MAX_NS);
        return WS3D_E_UNSUPPORTED;
    }
    if (clouds == 0 || m == 0) return WS3D_OK;
    const int tiles = (m + BQR_CT - 1) / BQR_CT;
    if ((long)clouds * tiles > 0x7fffffffL) {
        set_error("ws3d_ball_query_ragged: %d clouds x %d centres are too many for one launch", clouds, m);
        return WS3D_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(ball_query_ragged_kernel, dim3((unsigned)((long)clouds * tiles)), dim3(BQR_NT), 0, as_stream(stream), tiles, m, radius, nsample,
                       offsets, xyz, new_xyz, global_rows, idx);
    return check_launch("ws3d_ball_query_ragged");
}
