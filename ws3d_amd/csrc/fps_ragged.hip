// fps_ragged.hip -- furthest point sampling of MANY clouds of different sizes in one launch (ws3d extension; the
// ground-truth database builder samples every object of a chunk of scans at once, ws3d_amd/gt_database.py).
//
// One 256-thread workgroup per cloud.  Cloud i holds the points offsets[i] .. offsets[i+1] of a packed (total,3) array.  As in
// fps.hip the whole cloud and its running minimum distance live in VGPRs for the entire kernel: thread u keeps PPT points, PPT
// chosen PER WORKGROUP from {1,2,4,8,16} by the cloud's own size (a block-uniform switch over instantiations of one device
// function, so a 600-point cloud sweeps 4 slots per lane, not 16).  256 x 16 = 4096 points is what the kernel holds; larger
// clouds are forwarded by the C entry to ws3d_furthest_point_sampling, one launch each on the same stream.  No global scratch.
//
// Bit-equal to ws3d_furthest_point_sampling(1, n_i, m, ...) on each cloud alone: the tie rule depends on the cloud's size through
// bs = opt_n_threads(n_i) and is carried by fps.hip's tie-order POSITION p = bitrev(k mod bs) * S + k / bs (S = ceil(n/bs)):
// thread u owns the contiguous positions [u*PPT, (u+1)*PPT), and "lowest slot, lowest lane, lowest wave wins" is the reference's
// order for any workgroup size.  Distances through sqdist3 (common.h), so every WS3D_DIST_MODE build follows its oracle.
#include <cmath>
#include <vector>

#include "common.h"

namespace ws3d {

constexpr int RAGGED_NT = 256;
constexpr int RAGGED_MAX_PPT = 16;
constexpr int RAGGED_CAP = RAGGED_NT * RAGGED_MAX_PPT;   // 4096 tie-order positions = 4096 points (R <= 4096 <=> n <= 4096)

__device__ __forceinline__ int ragged_bitrev(int v, int bits) {
    return bits == 0 ? 0 : (int)(__builtin_bitreverse32((uint32_t)v) >> (32 - bits));
}

template <int N> struct RVecF { typedef float type __attribute__((ext_vector_type(N))); };
template <> struct RVecF<1> { typedef float type; };
template <int N> __device__ __forceinline__ float rvec_get(const typename RVecF<N>::type &v, int i) { return v[i]; }
template <> __device__ __forceinline__ float rvec_get<1>(const RVecF<1>::type &v, int) { return v; }
template <int N> __device__ __forceinline__ void rvec_set(typename RVecF<N>::type &v, int i, float x) { v[i] = x; }
template <> __device__ __forceinline__ void rvec_set<1>(RVecF<1>::type &v, int, float x) { v = x; }

// the m - 1 dependent steps of one cloud; idx[1..m-1] receives tie-order POSITIONS (the caller maps them to point indices)
template <int PPT>
__device__ __forceinline__ void ragged_cloud(const float *__restrict__ xyz, int32_t *__restrict__ idx, int n, int m, int bs, int log2bs,
                                             int S, float4 (*s_cand)[16], int (*s_k)[16]) {
    constexpr int NW = RAGGED_NT / WS3D_WAVE;
    const int u = threadIdx.x, lane = u & 63, w = u >> 6;
    typename RVecF<PPT>::type px, py, pz;
    float t[PPT];
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
        const int p = u * PPT + s;
        const int rb = p / S, sl = p - rb * S;
        const int k = ragged_bitrev(rb, log2bs) + sl * bs;
        const bool valid = (rb < bs) && (k < n);
        const int kc = valid ? k : 0;                   // clamped, never out of the cloud
        const float x = xyz[kc * 3 + 0], y = xyz[kc * 3 + 1], z = xyz[kc * 3 + 2];
        rvec_set<PPT>(px, s, valid ? x : 0.f);
        rvec_set<PPT>(py, s, valid ? y : 0.f);
        rvec_set<PPT>(pz, s, valid ? z : 0.f);
        t[s] = valid ? 1e10f : -1.0f;                   // -1 never beats a real candidate (>= 0)
    }
    float ox = xyz[0], oy = xyz[1], oz = xyz[2];
    for (int j = 1; j < m; ++j) {
        float best = -1.0f;
        int bslot = 0;
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const float d = sqdist3(rvec_get<PPT>(px, s) - ox, rvec_get<PPT>(py, s) - oy, rvec_get<PPT>(pz, s) - oz);
            const float d2 = min_f32(d, t[s]);          // == fminf: t[s] is never NaN
            t[s] = d2;
            const bool gt = d2 > best;                  // strict: the lowest slot keeps exact ties
            bslot = gt ? s : bslot;
            best = gt ? d2 : best;
        }
        // wave argmax: lowest lane among the lanes holding the wave maximum
        const float wmax = wave_max(best);
        const uint64_t eq = __ballot(best == wmax);
        const int wl = (int)__builtin_ctzll(eq);
        const int wslot = __builtin_amdgcn_readlane(bslot, wl);
        const float cx = readlane_f(rvec_get<PPT>(px, wslot), wl);
        const float cy = readlane_f(rvec_get<PPT>(py, wslot), wl);
        const float cz = readlane_f(rvec_get<PPT>(pz, wslot), wl);
        const int kw = (w * 64 + wl) * PPT + wslot;
        // one record per wave, double buffered by step parity: ONE barrier per step
        const int buf = j & 1;
        if (lane == 0) {
            s_cand[buf][w] = make_float4(wmax, cx, cy, cz);
            s_k[buf][w] = kw;
        }
        lds_barrier();
        const int e = lane & 15;
        const float4 c = s_cand[buf][e];
        const int kc = s_k[buf][e];
        const float v = e < NW ? c.x : -2.0f;
        const float vm = row16_max(v);
        const uint64_t eq2 = __ballot(v == vm);
        const int sel = (int)__builtin_ctzll(eq2);     // lowest wave among ties
        ox = readlane_f(c.y, sel);
        oy = readlane_f(c.z, sel);
        oz = readlane_f(c.w, sel);
        const int old = __builtin_amdgcn_readlane(kc, sel);
        if (u == 0) idx[j] = old;
    }
}

__global__ __launch_bounds__(RAGGED_NT) void fps_ragged_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ offsets,
                                                               int32_t *__restrict__ idx, int total, int m, int limit) {
    __shared__ float4 s_cand[2][16];
    __shared__ int s_k[2][16];
    const int c = blockIdx.x;
    const int off = offsets[c];
    const int n = offsets[c + 1] - off;
    // larger clouds belong to the per-cloud kernel (the C entry launches it); anything that does not lie inside the packed array is
    // not touched (the entry validated the host copy of the sizes -- this guards a device array that disagrees with it)
    if (n < 1 || n > limit || n < m || off < 0 || n > total - off) return;
    xyz += (size_t)off * 3;
    idx += (size_t)c * m;
    // bs = opt_n_threads(n) = the largest power of two <= n, capped at 1024 (the entry checked that the launcher's libm expression
    // agrees with this for every n <= limit)
    int log2bs = 31 - __builtin_clz((unsigned)n);
    if (log2bs > 10) log2bs = 10;
    const int bs = 1 << log2bs;
    const int S = (n + bs - 1) / bs;
    const int R = bs * S;                                // tie-order positions, <= 4096 for n <= 4096
    const int ppt = (R + RAGGED_NT - 1) / RAGGED_NT;
    if (threadIdx.x == 0) idx[0] = 0;
    if (ppt <= 1) ragged_cloud<1>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 2) ragged_cloud<2>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 4) ragged_cloud<4>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 8) ragged_cloud<8>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else ragged_cloud<16>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    // positions -> point indices, off the critical path (thread 0 wrote idx[])
    __syncthreads();
    for (int j = 1 + threadIdx.x; j < m; j += RAGGED_NT) {
        const int p = idx[j];
        const int rb = p / S, sl = p - rb * S;
        idx[j] = ragged_bitrev(rb, log2bs) + sl * bs;
    }
}

// cuda_utils.h:10-14, the launcher's own libm expression (as in fps.hip)
static int ragged_opt_n_threads(int work_size) {
    const int pow_2 = (int)(std::log(static_cast<double>(work_size)) / std::log(2.0));
    int v = 1 << pow_2;
    if (v > 1024) v = 1024;
    if (v < 1) v = 1;
    return v;
}

// the largest L <= 4096 such that the kernel's integer block size equals the launcher's for every n <= L
static int ragged_limit() {
    static const int limit = [] {
        int n = 1;
        for (; n <= RAGGED_CAP; ++n) {
            int p = 1;
            while (p * 2 <= n && p < 1024) p *= 2;
            if (ragged_opt_n_threads(n) != p) break;
        }
        return n - 1;
    }();
    return limit;
}

}  // namespace ws3d

extern "C" int ws3d_fps_ragged_limit(void) { return ws3d::ragged_limit(); }

extern "C" int ws3d_furthest_point_sampling_ragged(int clouds, const int32_t *offsets, const int32_t *sizes_host, int m, const float *xyz,
                                                   int32_t *idx, ws3d_stream_t stream) {
    using namespace ws3d;
    if (clouds < 0 || m < 0 || (clouds > 0 && (!offsets || !sizes_host || !xyz || (!idx && m > 0)))) {
        set_error("ws3d_furthest_point_sampling_ragged: invalid argument (clouds=%d m=%d)", clouds, m);
        return WS3D_E_INVALID;
    }
    if (clouds == 0) return WS3D_OK;
    long total = 0;
    for (int i = 0; i < clouds; ++i) {
        if (sizes_host[i] < 1 || sizes_host[i] < m) {
            set_error("ws3d_furthest_point_sampling_ragged: invalid argument (cloud %d holds %d points, m=%d)", i, sizes_host[i], m);
            return WS3D_E_INVALID;
        }
        total += sizes_host[i];
    }
    if (total > 0x7fffffffL / 3) {
        set_error("ws3d_furthest_point_sampling_ragged: invalid argument (%ld points exceed the 32-bit offsets)", total);
        return WS3D_E_INVALID;
    }
    if (m == 0) return WS3D_OK;
    const int limit = ragged_limit();
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(fps_ragged_kernel, dim3(clouds), dim3(RAGGED_NT), 0, st, xyz, offsets, idx, (int)total, m, limit);
    if (int rc = check_launch("furthest_point_sampling_ragged")) return rc;
    long off = 0;
    for (int i = 0; i < clouds; ++i) {
        if (sizes_host[i] > limit)
            if (int rc = ws3d_furthest_point_sampling(1, sizes_host[i], m, xyz + off * 3, nullptr, idx + (size_t)i * m, stream)) return rc;
        off += sizes_host[i];
    }
    return WS3D_OK;
}
