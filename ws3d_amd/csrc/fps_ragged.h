// fps_ragged.h -- the device and host pieces shared by the ragged furthest-point-sampling kernels: fps_ragged.hip (indices only,
// n_i >= m) and stage2_ragged.hip (indices + sampled coordinates, any n_i >= 1).  See fps_ragged.hip for the scheme.
#pragma once
#include <cmath>

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
