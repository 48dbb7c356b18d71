// fps_pruned.hip -- pruned furthest point sampling for 16384 < n <= 65536 points (gfx950), out of a caller-provided workspace:
// ws3d_furthest_point_sampling_ws / ws3d_fps_workspace_bytes (include/ws3d_ops.h).  DESIGN.md section 5.1c.
//
// Same contract as fps.hip: indices, the min-distance buffer and the gathered centres are bit-equal to the reference's, ties
// included; what changes is the work per step.  fps_big_kernel (fps.hip), the plain entry's kernel for these sizes, evaluates the
// distance of EVERY point to every new sample.  After j samples the running distance of every point is <= the maximum that
// selected sample j, so a new sample q only changes points near q.  Two kernels, one workgroup of 1024 threads per scene each:
//
//   fps_pruned_setup_kernel   counting-sorts the scene into 128 x 128 Z-order cells of its (x, z) bounding box (histogram in LDS)
//       and writes, in sorted order, one float4 {x, y, z, point index k as bits} and one running distance (the caller's temp[k],
//       or 1e10) per point into the workspace.  The sorted sequence is cut into NB = ceil(n / 64) <= 1024 buckets of 64
//       consecutive points; the last one is padded with {k = -1, distance -1}: such a lane never wins and min(d, -1) stays -1.
//
//   fps_pruned_kernel   bucket B = 16 l + w belongs to lane l of wave w for the whole kernel, which keeps its bounding box, its
//       largest running distance `bmax`, and the rank, coordinates and index of the point that holds it IN REGISTERS.  A step:
//       (a) every lane evaluates sqdist3 on the per-axis gaps between q and its bucket's box: by monotonicity of the fp32
//           sub / mul / fma roundings this is a lower bound L of the distance the update would compute for any point of the
//           bucket (for all three WS3D_DIST_MODE expressions), so L >= bmax proves min(d, t) == t for the whole bucket: the skip
//           is exact (the argument of fps_bucket.hip, under test there).  One ballot gives the wave its surviving buckets;
//       (b) the wave walks them, one point per lane: float4 and running distance from the workspace, d = sqdist3(p - q),
//           t = min(d, t) stored back, wave argmax -> the bucket's new record in lane l's registers;
//       (c) a wave whose buckets changed re-picks its best record; the 16 wave records meet in LDS (double-buffered by step
//           parity, ONE LDS-only barrier per step) and every wave reduces them to the next sample, whose coordinates travel in
//           the record: no dependent global load between steps.
//       A bucket's running distances are only ever read and written by the wave that owns it, in program order, so no step waits
//       for a global store; neighbouring buckets of the Z-order (which a sample reaches together) belong to different waves.
//
// Ties.  Above 1023 points the reference's block has 1024 threads and picks, among the points that hold the maximum, the smallest
// (bitrev10(k & 1023), k) (fps.hip header).  For n <= 65536, rank(k) = bitrev10(k & 1023) * 64 + (k >> 10) is that order as one
// unique 16-bit number: every reduction here compares (value descending, rank ascending), and slot, lane or wave order never
// decides anything.
//
// No workgroup waits for another; every loop is bounded by the number of buckets, cells, points or samples.
#include <cstdlib>

#include "common.h"

namespace ws3d {

constexpr int FPP_NT = 1024, FPP_NW = 16;
constexpr int FPP_MIN_N = 16384, FPP_MAX_N = 65536;      // serves FPP_MIN_N < n <= FPP_MAX_N
constexpr int FPP_GRID_BITS = 7, FPP_GRID = 1 << FPP_GRID_BITS, FPP_CELLS = FPP_GRID * FPP_GRID;
constexpr size_t FPP_SETUP_LDS = sizeof(int) * FPP_CELLS + sizeof(float) * 4 * FPP_NW + sizeof(int) * FPP_NW;

__device__ __forceinline__ int fpp_zcell(float x, float z, float xmin, float zmin, float ix, float iz) {
    const float fx = (x - xmin) * ix, fz = (z - zmin) * iz;
    constexpr float top = (float)(FPP_GRID - 1);
    const unsigned cx = fx > 0.f ? (fx < top ? (unsigned)fx : (unsigned)(FPP_GRID - 1)) : 0u;  // NaN -> 0
    const unsigned cz = fz > 0.f ? (fz < top ? (unsigned)fz : (unsigned)(FPP_GRID - 1)) : 0u;
    unsigned code = 0;
#pragma unroll
    for (int i = 0; i < FPP_GRID_BITS; ++i) code |= ((cx >> i) & 1u) << (2 * i) | ((cz >> i) & 1u) << (2 * i + 1);
    return (int)code;
}

__device__ __forceinline__ unsigned fpp_row16_min_u32(unsigned v) {
    unsigned r;
    asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v));
    asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=v"(v) : "v"(r));
    asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v));
    asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xf" : "=v"(v) : "v"(r));
    return v;
}
__device__ __forceinline__ unsigned fpp_wave_min_u32(unsigned v) {
    v = fpp_row16_min_u32(v);
    const unsigned a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const unsigned c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ float fpp_wave_min(float v) { return -wave_max(-v); }
__device__ __forceinline__ float fpp_max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// the reference's tie order among points that hold the maximum, as one number (unique for k < 65536; the padding's k = -1 never gets here)
__device__ __forceinline__ unsigned fpp_rank(int k) {
    return ((__builtin_bitreverse32((uint32_t)k & 1023u) >> 22) << 6) + ((uint32_t)k >> 10);
}
// (value descending, rank ascending) over the 64 points of a bucket: the maximum, the winner's rank and its lane
__device__ __forceinline__ void fpp_argmax(float t, int k, float &bm, unsigned &km, int &wl) {
    bm = wave_max(t);
    const unsigned key = (t == bm) ? fpp_rank(k) : 0xFFFFFFFFu;
    km = fpp_wave_min_u32(key);
    wl = (int)__builtin_ctzll(__ballot(key == km));      // some lane always matches, also when no lane equals bm (NaN distances)
}

// workspace of one scene: P float4 {x, y, z, k}, then P running distances; P = 64 * ceil(n / 64)
static inline int fpp_padded(int n) { return ((n + 63) / 64) * 64; }
static inline size_t fpp_scene_bytes(int n) { return (size_t)fpp_padded(n) * (sizeof(float4) + sizeof(float)); }

__global__ __launch_bounds__(FPP_NT) void fps_pruned_setup_kernel(const float *__restrict__ xyz, const float *__restrict__ temp,
                                                                  char *__restrict__ ws, int n, int P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *hist = reinterpret_cast<int *>(smem);                      // FPP_CELLS
    float *red = reinterpret_cast<float *>(hist + FPP_CELLS);       // 4 * FPP_NW
    int *wsum = reinterpret_cast<int *>(red + 4 * FPP_NW);          // FPP_NW

    const int b = blockIdx.x;
    xyz += (size_t)b * n * 3;
    if (temp) temp += (size_t)b * n;
    float4 *pts = reinterpret_cast<float4 *>(ws + (size_t)b * P * (sizeof(float4) + sizeof(float)));
    float *tt = reinterpret_cast<float *>(pts + P);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    // the scene's (x, z) bounding box over its finite coordinates
    float xmn = INFINITY, xmx = -INFINITY, zmn = INFINITY, zmx = -INFINITY;
    for (int k = tid; k < n; k += FPP_NT) {
        const float x = xyz[(size_t)k * 3], z = xyz[(size_t)k * 3 + 2];
        if (fabsf(x) < INFINITY) { xmn = fminf(xmn, x); xmx = fmaxf(xmx, x); }
        if (fabsf(z) < INFINITY) { zmn = fminf(zmn, z); zmx = fmaxf(zmx, z); }
    }
    xmn = fpp_wave_min(xmn); xmx = wave_max(xmx); zmn = fpp_wave_min(zmn); zmx = wave_max(zmx);
    if (lane == 0) { red[w * 4 + 0] = xmn; red[w * 4 + 1] = xmx; red[w * 4 + 2] = zmn; red[w * 4 + 3] = zmx; }
    for (int i = tid; i < FPP_CELLS; i += FPP_NT) hist[i] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FPP_NW; ++i) {
        xmn = fminf(xmn, red[i * 4 + 0]); xmx = fmaxf(xmx, red[i * 4 + 1]);
        zmn = fminf(zmn, red[i * 4 + 2]); zmx = fmaxf(zmx, red[i * 4 + 3]);
    }
    const float x0 = xmn <= xmx ? xmn : 0.f, z0 = zmn <= zmx ? zmn : 0.f;
    const float ix = (xmn < xmx) ? (float)FPP_GRID / (xmx - xmn) : 0.f, iz = (zmn < zmx) ? (float)FPP_GRID / (zmx - zmn) : 0.f;
    // counting sort by Z-order cell (the order inside a cell is the order of the atomics: it changes no result, see the header)
    for (int k = tid; k < n; k += FPP_NT)
        atomicAdd(&hist[fpp_zcell(xyz[(size_t)k * 3], xyz[(size_t)k * 3 + 2], x0, z0, ix, iz)], 1);
    __syncthreads();
    {   // exclusive scan of the counters: FPP_CELLS / FPP_NT per thread
        constexpr int CPT = FPP_CELLS / FPP_NT;
        int a[CPT], v = 0;
#pragma unroll
        for (int i = 0; i < CPT; ++i) { a[i] = hist[CPT * tid + i]; v += a[i]; }
        const int mine = v;
        for (int o = 1; o < 64; o <<= 1) { const int t2 = __shfl_up(v, o); if (lane >= o) v += t2; }
        if (lane == 63) wsum[w] = v;
        __syncthreads();
        int off = 0;
        for (int i = 0; i < w; ++i) off += wsum[i];
        int excl = off + v - mine;
#pragma unroll
        for (int i = 0; i < CPT; ++i) { hist[CPT * tid + i] = excl; excl += a[i]; }
    }
    __syncthreads();
    for (int k = tid; k < n; k += FPP_NT) {
        const float x = xyz[(size_t)k * 3], y = xyz[(size_t)k * 3 + 1], z = xyz[(size_t)k * 3 + 2];
        const int pos = atomicAdd(&hist[fpp_zcell(x, z, x0, z0, ix, iz)], 1);
        if ((unsigned)pos < (unsigned)n) {       // always: the two passes compute the same cell
            pts[pos] = make_float4(x, y, z, __int_as_float(k));
            tt[pos] = temp ? temp[k] : 1e10f;
        }
    }
    for (int pos = n + tid; pos < P; pos += FPP_NT) {
        pts[pos] = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        tt[pos] = -1.0f;
    }
}

__global__ __launch_bounds__(FPP_NT) void fps_pruned_kernel(const float *__restrict__ xyz, float *__restrict__ temp, int32_t *__restrict__ idx,
                                                            float *__restrict__ new_xyz, char *__restrict__ ws, int n, int m, int P) {
    __shared__ float4 s_cand[2][FPP_NW];     // {value, x, y, z} of every wave's best point
    __shared__ int2 s_kk[2][FPP_NW];         // {k, rank}

    const int b = blockIdx.x;
    xyz += (size_t)b * n * 3;
    idx += (size_t)b * m;
    if (temp) temp += (size_t)b * n;
    if (new_xyz) new_xyz += (size_t)b * m * 3;
    const float4 *pts = reinterpret_cast<const float4 *>(ws + (size_t)b * P * (sizeof(float4) + sizeof(float)));
    float *tt = reinterpret_cast<float *>(ws + (size_t)b * P * (sizeof(float4) + sizeof(float)) + (size_t)P * sizeof(float4));
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NB = P >> 6;

    // ---- lane l: the record of bucket 16 l + w (bmax = -2: no such bucket)
    float blx = INFINITY, bhx = -INFINITY, bly = INFINITY, bhy = -INFINITY, blz = INFINITY, bhz = -INFINITY;
    float bmax = -2.0f, cx = 0.f, cy = 0.f, cz = 0.f;
    unsigned rk = 0xFFFFFFFFu;
    int ck = 0;
    for (int s = 0; s < 64; ++s) {
        const int B = s * FPP_NW + w;
        if (B >= NB) break;
        const int pos = (B << 6) + lane;
        const float4 p = pts[pos];
        const float t = tt[pos];
        const int k = __float_as_int(p.w);
        const bool valid = k >= 0;
        // (NaN coordinates are ignored by v_min / v_max: the running distance of such a point never changes, it needs no coverage)
        const float lx = fpp_wave_min(valid ? p.x : INFINITY), hx = wave_max(valid ? p.x : -INFINITY);
        const float ly = fpp_wave_min(valid ? p.y : INFINITY), hy = wave_max(valid ? p.y : -INFINITY);
        const float lz = fpp_wave_min(valid ? p.z : INFINITY), hz = wave_max(valid ? p.z : -INFINITY);
        float bm; unsigned km; int wl;
        fpp_argmax(t, k, bm, km, wl);
        const float X = readlane_f(p.x, wl), Y = readlane_f(p.y, wl), Z = readlane_f(p.z, wl);
        const int K = __builtin_amdgcn_readlane(k, wl);
        if (lane == s) { blx = lx; bhx = hx; bly = ly; bhy = hy; blz = lz; bhz = hz; bmax = bm; rk = km; cx = X; cy = Y; cz = Z; ck = K; }
    }

    float qx = xyz[0], qy = xyz[1], qz = xyz[2];
    if (tid == 0) {
        idx[0] = 0;
        if (new_xyz) { new_xyz[0] = qx; new_xyz[1] = qy; new_xyz[2] = qz; }
    }
    // the wave's best record
    float wv = -2.0f, wx = 0.f, wy = 0.f, wz = 0.f;
    int wk = 0, wrank = 0;
    bool have = false;
#ifdef WS3D_FPP_PROF
    unsigned long long prof_upd = 0;      // bucket updates of this wave
#endif
    for (int j = 1; j < m; ++j) {
        // ---- (a) which of my buckets can change?  L: the kernel's own distance expression on the gaps between q and the box (0 inside)
        const float L = sqdist3(fpp_max3(blx - qx, qx - bhx, 0.f), fpp_max3(bly - qy, qy - bhy, 0.f), fpp_max3(blz - qz, qz - bhz, 0.f));
        uint64_t need = __ballot(L < bmax);
        // ---- (b) update them; the next bucket's loads are in flight while this one is reduced
        if (need) {
#ifdef WS3D_FPP_PROF
            prof_upd += (unsigned long long)__builtin_popcountll(need);
#endif
            int s = (int)__builtin_ctzll(need);
            need &= need - 1;
            int pos = ((s * FPP_NW + w) << 6) + lane;
            float4 p = pts[pos];
            float t = tt[pos];
            for (;;) {
                const bool more = need != 0;
                int s2 = 0, pos2 = 0;
                float4 p2 = p;
                float t2 = 0.f;
                if (more) {
                    s2 = (int)__builtin_ctzll(need);
                    need &= need - 1;
                    pos2 = ((s2 * FPP_NW + w) << 6) + lane;
                    p2 = pts[pos2];
                    t2 = tt[pos2];
                }
                const float d = sqdist3(p.x - qx, p.y - qy, p.z - qz);
                const float tn = min_f32(d, t);  // == fminf: t is never NaN
                if (tn != t) tt[pos] = tn;
                const int k = __float_as_int(p.w);
                float bm; unsigned km; int wl;
                fpp_argmax(tn, k, bm, km, wl);
                const float X = readlane_f(p.x, wl), Y = readlane_f(p.y, wl), Z = readlane_f(p.z, wl);
                const int K = __builtin_amdgcn_readlane(k, wl);
                if (lane == s) { bmax = bm; rk = km; cx = X; cy = Y; cz = Z; ck = K; }
                if (!more) break;
                s = s2; pos = pos2; p = p2; t = t2;
            }
            have = false;
        }
        // ---- (c) the wave's best record (unchanged while none of its buckets changed), then the best of the 16 waves
        if (!have) {
            wv = wave_max(bmax);
            const unsigned key = (bmax == wv) ? rk : 0xFFFFFFFFu;
            const unsigned km = fpp_wave_min_u32(key);
            const int sl = (int)__builtin_ctzll(__ballot(key == km));
            wx = readlane_f(cx, sl); wy = readlane_f(cy, sl); wz = readlane_f(cz, sl);
            wk = __builtin_amdgcn_readlane(ck, sl);
            wrank = (int)km;
            have = true;
        }
        const int buf = j & 1;
        if (lane == 0) {
            s_cand[buf][w] = make_float4(wv, wx, wy, wz);
            s_kk[buf][w] = make_int2(wk, wrank);
        }
        lds_barrier();
        const int e = lane & (FPP_NW - 1);
        const float4 c = s_cand[buf][e];
        const int2 kk = s_kk[buf][e];
        const float vm = row16_max(c.x);
        const unsigned k2 = (c.x == vm) ? (unsigned)kk.y : 0xFFFFFFFFu;
        const unsigned kmin = fpp_row16_min_u32(k2);
        const int sel = (int)__builtin_ctzll(__ballot(k2 == kmin));
        qx = readlane_f(c.y, sel); qy = readlane_f(c.z, sel); qz = readlane_f(c.w, sel);
        const int qk = __builtin_amdgcn_readlane(kk.x, sel);      // (outside the branch: inside it only lane 0 would hold its record)
        if (tid == 0) {
            idx[j] = qk;
            if (new_xyz) { new_xyz[j * 3 + 0] = qx; new_xyz[j * 3 + 1] = qy; new_xyz[j * 3 + 2] = qz; }
        }
    }

    // ---- the min-distance buffer as the reference leaves it (a skipped bucket kept its values: they ARE the reference's)
    if (temp) {
        for (int s = 0; s < 64; ++s) {
            const int B = s * FPP_NW + w;
            if (B >= NB) break;
            const int pos = (B << 6) + lane;
            const int k = __float_as_int(pts[pos].w);
            if ((unsigned)k < (unsigned)n) temp[k] = tt[pos];     // (the padding holds k = -1)
        }
    }
#ifdef WS3D_FPP_PROF
    // profiling build only: the scene's bucket updates, summed over its waves, into the first 8 bytes of its workspace (dead by now)
    __syncthreads();
    if (tid == 0) *reinterpret_cast<unsigned long long *>(ws + (size_t)b * P * (sizeof(float4) + sizeof(float))) = 0ull;
    __syncthreads();
    if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(ws + (size_t)b * P * (sizeof(float4) + sizeof(float))), prof_upd);
#endif
}

}  // namespace ws3d

extern "C" size_t ws3d_fps_workspace_bytes(int b, int n) {
    if (b <= 0 || n <= ws3d::FPP_MIN_N || n > ws3d::FPP_MAX_N) return 0;
    return (size_t)b * ws3d::fpp_scene_bytes(n);
}

extern "C" int ws3d_furthest_point_sampling_ws(int b, int n, int m, const float *xyz, float *temp, int32_t *idx, float *new_xyz,
                                               void *workspace, size_t workspace_bytes, ws3d_stream_t stream) {
    using namespace ws3d;
    // WS3D_FPS_PRUNED=0: always the plain entry (A/B runs, tests)
    static const int pruned = getenv("WS3D_FPS_PRUNED") ? atoi(getenv("WS3D_FPS_PRUNED")) : 1;
    const size_t need = ws3d_fps_workspace_bytes(b, n);
    if (!pruned || need == 0 || !workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || m <= 0 ||
        !xyz || !idx)
        return ws3d_furthest_point_sampling_gather(b, n, m, xyz, temp, idx, new_xyz, stream);
    hipStream_t st = as_stream(stream);
    const int P = fpp_padded(n);
    if (int rc = raise_lds_cap((const void *)fps_pruned_setup_kernel, FPP_SETUP_LDS, "furthest_point_sampling_ws")) return rc;
    hipLaunchKernelGGL(fps_pruned_setup_kernel, dim3(b), dim3(FPP_NT), FPP_SETUP_LDS, st, xyz, (const float *)temp, (char *)workspace, n, P);
    hipLaunchKernelGGL(fps_pruned_kernel, dim3(b), dim3(FPP_NT), 0, st, xyz, temp, idx, new_xyz, (char *)workspace, n, m, P);
    return check_launch("furthest_point_sampling_ws");
}
