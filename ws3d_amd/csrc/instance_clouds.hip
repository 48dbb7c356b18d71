// instance_clouds.hip -- the Stage-2 instance clouds of WS3D for gfx950: every kept centre's cylinder of scene points
// (sqrt(dx^2 + dz^2) < radius, y free), in scene order, shifted to the centre, with reflectance and a score channel.
// Replaces the (N x K) distance matrix + Python loop over the centres with boolean-mask indexing of
// generate_box_dataset.py:197-229 / tools/eval_auto.py:286-292, 323-372 (one device synchronisation and a handful of tiny
// launches per centre) and the pad-to-512 rule of lib/datasets/kitti_boxplace_dataset.py:327-337.
//
// Design, after roipool3d.hip's scanning kernel.  One 256-lane workgroup owns one (scene, centre):
//   1. each of the 4 waves scans a contiguous quarter of the scene, 4 x 64 points a trip: membership -> __ballot -> mbcnt
//      prefix -> ordered append (ascending point index; no atomics, no barrier inside the scan).  The scan runs to the end of
//      the scene -- count is the TRUE number of members -- only the append stops at S;
//   2. fixed form: the 4 lists are concatenated (their ranges are ordered), cut to S and wrapped (row j >= t repeats row
//      j mod t) in LDS; the S x 5 block is built in LDS one row per lane (one 16-byte load per point) and streamed out with
//      aligned 16-byte stores, then the S x C feature block is gathered row by row (32 lanes per 512-byte row, aligned 16-byte
//      loads and streaming stores);
//   3. ragged form: a counting kernel (scan only), then an emitting kernel that counts its quarters again to place each wave
//      inside the centre's range and writes the members of every 64-point step straight to their rows.
// No B*N*K matrix, no allocation, no host synchronisation, no atomics; every output element of the fixed form is written.
#include <cmath>

#include "common.h"

namespace ws3d {

typedef float ic_f4 __attribute__((ext_vector_type(4)));
typedef ic_f4 ic_f4u __attribute__((aligned(4)));  // 16-byte access, 4-byte aligned

// lib/utils/distance.py:3 distance_2 on (x, z): the two squares rounded separately and added x first (the library is built
// with -ffp-contract=off), correctly rounded sqrtf; a NaN distance compares false = outside.
__device__ __forceinline__ bool ic_member(float cx, float cz, float radius, float px, float pz) {
    const float dx = cx - px, dz = cz - pz;
    return sqrtf(dx * dx + dz * dz) < radius;
}

// generate_box_dataset.py:222 (mode 0: the score itself) / tools/eval_auto.py:345, 367 (mode 1: (score > thresh) - 0.5)
__device__ __forceinline__ float ic_mask_value(float s, int mask_mode, float thresh) {
    return mask_mode ? ((s > thresh ? 1.0f : 0.0f) - 0.5f) : s;
}

// One wave's scan of the points [start, end) of a scene (pts: the scene's (n, 4) rows), 4 x 64 points a trip: the four loads
// of a trip are independent and issued together.  on_step(first point of the step, ballot, members found before it) is called
// for every 64-point step that has a member; returns the number of members in the range.  Everything but the lane's own
// coordinates is wave-uniform.
template <class F>
__device__ __forceinline__ int ic_scan(const float *__restrict__ pts, int start, int end, int n, float cx, float cz, float radius,
                                       int lane, F &&on_step) {
    int cnt = 0;
    for (int k0 = start; k0 < end; k0 += 256) {
        float x[4], z[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * 64 + lane;  // clamped, never branched; a lane past the range gets x = NaN = outside
            const ic_f4 p = *reinterpret_cast<const ic_f4u *>(pts + (size_t)min(k, n - 1) * 4);
            x[u] = k < end ? p.x : __builtin_nanf("");
            z[u] = p.z;
        }
        uint64_t mask[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) mask[u] = __builtin_amdgcn_ballot_w64(ic_member(cx, cz, radius, x[u], z[u]));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (mask[u]) {  // wave-uniform
                on_step(k0 + u * 64, mask[u], cnt);
                cnt += (int)__builtin_popcountll(mask[u]);
            }
        }
    }
    return cnt;
}

struct IcScene {
    int b, k, lane, w, start, end;
    bool valid;
    float cx, cy, cz;
};

// (scene, centre) of this workgroup and the wave's quarter of the scene; valid: the slot is below num[b] and the scene has points
__device__ __forceinline__ IcScene ic_scene(int pts_num, int centres_num, const float *__restrict__ centres, const int32_t *__restrict__ num) {
    IcScene s;
    const int bk = blockIdx.x;
    s.b = bk / centres_num;
    s.k = bk - s.b * centres_num;
    s.lane = threadIdx.x & 63;
    s.w = threadIdx.x >> 6;
    const int Q = (((pts_num + 3) / 4 + 63) / 64) * 64;
    s.start = (int)min((long)s.w * Q, (long)pts_num);
    s.end = (int)min((long)s.start + Q, (long)pts_num);
    s.valid = pts_num > 0 && (!num || s.k < num[s.b]);
    const float *c = centres + (size_t)bk * 3;
    s.cx = c[0]; s.cy = c[1]; s.cz = c[2];
    return s;
}

// ---- fixed form ---------------------------------------------------------------------------------------------------------------
// dynamic LDS: 5 * S floats (the 4 per-wave lists of S point indices while scanning, then the S x 5 block) + S ints (selection)
__global__ __launch_bounds__(256) void instance_clouds_kernel(int pts_num, int centres_num, int feat_len, int S, float radius, int mask_mode,
                                                              float mask_thresh, const float *__restrict__ pts, const float *__restrict__ score,
                                                              const float *__restrict__ feats, const float *__restrict__ centres,
                                                              const int32_t *__restrict__ num, float *__restrict__ cloud,
                                                              float *__restrict__ cloud_feats, int32_t *__restrict__ count,
                                                              int32_t *__restrict__ pts_idx) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *lists = reinterpret_cast<int *>(smem);          // 4 * S, dead once sel is built
    float *stage = reinterpret_cast<float *>(smem);      // 5 * S
    int *sel = reinterpret_cast<int *>(smem) + 5 * S;    // S
    __shared__ int wcnt_s[4];

    const IcScene s = ic_scene(pts_num, centres_num, centres, num);
    const int tid = threadIdx.x;
    const size_t bk = blockIdx.x;
    pts += (size_t)s.b * pts_num * 4;
    score += (size_t)s.b * pts_num;
    feats += (size_t)s.b * pts_num * feat_len;

    int wc = 0;
    if (s.valid) {
        int *mine = lists + s.w * S;
        wc = ic_scan(pts, s.start, s.end, pts_num, s.cx, s.cz, radius, s.lane, [&](int k0, uint64_t mk, int before) {
            const int pos = before + mbcnt(mk);  // a full list takes no more appends, the count goes on
            if (((mk >> s.lane) & 1ull) && pos < S) mine[pos] = k0 + s.lane;
        });
    }
    if (s.lane == 0) wcnt_s[s.w] = wc;
    __syncthreads();
    const int n0 = wcnt_s[0], n1 = wcnt_s[1], n2 = wcnt_s[2], n3 = wcnt_s[3];
    const int total = n0 + n1 + n2 + n3;
    const int t = min(total, S);
    if (tid == 0) count[bk] = total;

    float *out = cloud + bk * (size_t)S * 5;
    float *fout = cloud_feats + bk * (size_t)S * feat_len;
    const bool out_vec = ((S * 5) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    if (t == 0) {  // workgroup-uniform: an empty cylinder or a slot past num[b] -- all-zero rows, written here
        const ic_f4 zero = {0.f, 0.f, 0.f, 0.f};
        if (out_vec) for (int q = tid; q < (S * 5) >> 2; q += 256) reinterpret_cast<ic_f4 *>(out)[q] = zero;
        else for (int q = tid; q < S * 5; q += 256) out[q] = 0.f;
        if (feat_len > 0) for (size_t q = tid; q < (size_t)S * (feat_len >> 2); q += 256) __builtin_nontemporal_store(zero, reinterpret_cast<ic_f4 *>(fout) + q);
        if (pts_idx) for (int q = tid; q < S; q += 256) pts_idx[bk * S + q] = 0;
        return;
    }
    const int c0 = min(n0, S), c1 = min(n1, S), c2 = min(n2, S);
    for (int q = tid; q < S; q += 256) {
        int j = q < t ? q : q % t;  // kitti_boxplace_dataset.py:333-337: the first t rows repeated cyclically
        int v;
        if (j < c0) v = lists[j];
        else if ((j -= c0) < c1) v = lists[S + j];
        else if ((j -= c1) < c2) v = lists[2 * S + j];
        else v = lists[3 * S + (j - c2)];
        sel[q] = v;
        if (pts_idx) pts_idx[bk * S + q] = v;
    }
    __syncthreads();  // lists are dead from here: their space becomes the S x 5 block
    for (int q = tid; q < S; q += 256) {
        const int src = sel[q];
        const ic_f4 p = *reinterpret_cast<const ic_f4u *>(pts + (size_t)src * 4);
        const float m = ic_mask_value(score[src], mask_mode, mask_thresh);
        float *r = stage + q * 5;  // stride 5: conflict-free
        r[0] = p.x - s.cx; r[1] = p.y - s.cy; r[2] = p.z - s.cz; r[3] = p.w; r[4] = m;
    }
    __syncthreads();
    if (out_vec) for (int q = tid; q < (S * 5) >> 2; q += 256) reinterpret_cast<ic_f4 *>(out)[q] = reinterpret_cast<const ic_f4 *>(stage)[q];
    else for (int q = tid; q < S * 5; q += 256) out[q] = stage[q];

    if (feat_len > 0) {
        // 32 lanes move one feature row with aligned 16-byte loads and stores (host: C % 4 == 0, 16-byte aligned pointers), 4 rows
        // per half-wave and trip keep the loads in flight; streaming stores: the output is never re-read here, the gathered rows
        // are (overlapping cylinders share points)
        const int half = tid >> 5, l32 = tid & 31, f4 = feat_len >> 2;
        for (int r0 = half * 4; r0 < S; r0 += 32) {
            int src[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) src[u] = sel[min(r0 + u, S - 1)];
            for (int c = l32; c < f4; c += 32) {
                ic_f4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const ic_f4 *>(feats + (size_t)src[u] * feat_len)[c];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (r0 + u < S) __builtin_nontemporal_store(v[u], reinterpret_cast<ic_f4 *>(fout + (size_t)(r0 + u) * feat_len) + c);
            }
        }
    }
}

// ---- ragged form ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void instance_clouds_count_kernel(int pts_num, int centres_num, float radius, const float *__restrict__ pts,
                                                                    const float *__restrict__ centres, const int32_t *__restrict__ num,
                                                                    int32_t *__restrict__ count) {
    __shared__ int wcnt_s[4];
    const IcScene s = ic_scene(pts_num, centres_num, centres, num);
    pts += (size_t)s.b * pts_num * 4;
    int wc = 0;
    if (s.valid) wc = ic_scan(pts, s.start, s.end, pts_num, s.cx, s.cz, radius, s.lane, [](int, uint64_t, int) {});
    if (s.lane == 0) wcnt_s[s.w] = wc;
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = wcnt_s[0] + wcnt_s[1] + wcnt_s[2] + wcnt_s[3];
}

// Centre (b, k)'s members go to rows offsets[b * K + k] ... in ascending point index.  A wave's first row is the centre's offset plus
// the members of the quarters before its own, so every wave counts its quarter first (a second scan of a scene that sits in L2)
// and then emits step by step: the step's member indices are appended in order to a 64-entry list of the wave in LDS, from
// which the step's 5-float rows (contiguous in the output) and feature rows are written.  Rows past offsets[b * K + k + 1] are
// dropped: a count that no longer matches the inputs cannot make the kernel write outside the centre's range.
__global__ __launch_bounds__(256) void instance_clouds_emit_kernel(int pts_num, int centres_num, int feat_len, float radius, int mask_mode,
                                                                   float mask_thresh, const float *__restrict__ pts, const float *__restrict__ score,
                                                                   const float *__restrict__ feats, const float *__restrict__ centres,
                                                                   const int32_t *__restrict__ num, const int64_t *__restrict__ offsets,
                                                                   float *__restrict__ rows, float *__restrict__ row_feats, int32_t *__restrict__ row_idx) {
    __shared__ int wcnt_s[4];
    __shared__ int step_s[4][64];
    const IcScene s = ic_scene(pts_num, centres_num, centres, num);
    if (!s.valid) return;  // workgroup-uniform
    pts += (size_t)s.b * pts_num * 4;
    score += (size_t)s.b * pts_num;
    feats += (size_t)s.b * pts_num * feat_len;
    const int wc = ic_scan(pts, s.start, s.end, pts_num, s.cx, s.cz, radius, s.lane, [](int, uint64_t, int) {});
    if (s.lane == 0) wcnt_s[s.w] = wc;
    __syncthreads();
    long before_w = 0;
    for (int i = 0; i < s.w; ++i) before_w += wcnt_s[i];
    const long first = offsets[blockIdx.x] + before_w, limit = offsets[blockIdx.x + 1];
    if (wc == 0 || first < 0) return;  // wave-uniform; no barrier below
    int *mine = step_s[s.w];
    const int l32 = s.lane & 31, hi = s.lane >> 5, f4 = feat_len >> 2;
    ic_scan(pts, s.start, s.end, pts_num, s.cx, s.cz, radius, s.lane, [&](int k0, uint64_t mk, int before) {
        const int pc = (int)__builtin_popcountll(mk);
        if ((mk >> s.lane) & 1ull) mine[mbcnt(mk)] = k0 + s.lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // one wave, in-order LDS: only the compiler must not reorder
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const long row0 = first + before;
        const int room = (int)max(0L, min((long)pc, limit - row0));  // rows of this step inside the centre's range
        for (int e = s.lane; e < room * 5; e += 64) {
            const int r = e / 5, j = e - r * 5;
            const int src = mine[r];
            float v;
            if (j < 3) v = pts[(size_t)src * 4 + j] - (j == 0 ? s.cx : j == 1 ? s.cy : s.cz);
            else if (j == 3) v = pts[(size_t)src * 4 + 3];
            else v = ic_mask_value(score[src], mask_mode, mask_thresh);
            rows[row0 * 5 + e] = v;
        }
        if (row_idx && s.lane < room) row_idx[row0 + s.lane] = mine[s.lane];
        if (feat_len > 0) {
            for (int r0 = 0; r0 < room; r0 += 8) {  // 32 lanes per row, 4 rows per half-wave in flight
                int src[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) src[u] = mine[min(r0 + hi * 4 + u, pc - 1)];
                for (int c = l32; c < f4; c += 32) {
                    ic_f4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const ic_f4 *>(feats + (size_t)src[u] * feat_len)[c];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (r0 + hi * 4 + u < room)
                            __builtin_nontemporal_store(v[u], reinterpret_cast<ic_f4 *>(row_feats + (size_t)(row0 + r0 + hi * 4 + u) * feat_len) + c);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the list is overwritten by the next step
        __builtin_amdgcn_wave_barrier();
    });
}

static int ic_check(const char *what, int batch, int pts_num, int centres_num, int feat_len, float radius, int mask_mode) {
    if (batch < 0 || pts_num < 0 || centres_num < 0 || feat_len < 0 || (feat_len & 3) != 0 || !std::isfinite(radius) || !(radius > 0.f) ||
        (mask_mode != 0 && mask_mode != 1)) {
        set_error("%s: invalid argument (B=%d N=%d K=%d C=%d radius=%g mask_mode=%d; C must be a multiple of 4, radius finite and > 0)", what,
                  batch, pts_num, centres_num, feat_len, (double)radius, mask_mode);
        return WS3D_E_INVALID;
    }
    if ((long)batch * centres_num >= (1L << 24)) {  // a 1-D grid of 256-lane workgroups
        set_error("%s: B * K = %ld centres in one call are not supported (limit 2^24)", what, (long)batch * centres_num);
        return WS3D_E_UNSUPPORTED;
    }
    return WS3D_OK;
}

static bool ic_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace ws3d

extern "C" int ws3d_instance_clouds(int batch, int pts_num, int centres_num, int feat_len, int sampled_pts_num, float radius, int mask_mode,
                                    float mask_thresh, const float *pts, const float *score, const float *feats, const float *centres,
                                    const int32_t *num, float *cloud, float *cloud_feats, int32_t *count, int32_t *pts_idx,
                                    ws3d_stream_t stream) {
    using namespace ws3d;
    if (int rc = ic_check("ws3d_instance_clouds", batch, pts_num, centres_num, feat_len, radius, mask_mode)) return rc;
    if (sampled_pts_num <= 0) {
        set_error("ws3d_instance_clouds: invalid argument (S=%d)", sampled_pts_num);
        return WS3D_E_INVALID;
    }
    if (batch == 0 || centres_num == 0) return WS3D_OK;
    if ((pts_num > 0 && (!pts || !score || (feat_len > 0 && !feats))) || !centres || !cloud || !count || (feat_len > 0 && !cloud_feats)) {
        set_error("ws3d_instance_clouds: invalid argument (a required pointer is NULL)");
        return WS3D_E_INVALID;
    }
    if (feat_len > 0 && (ic_misaligned(feats) || ic_misaligned(cloud_feats))) {
        set_error("ws3d_instance_clouds: invalid argument (feats / cloud_feats must be 16-byte aligned)");
        return WS3D_E_INVALID;
    }
    const size_t smem = sizeof(int) * 6 * (size_t)sampled_pts_num;
    if (smem > 150 * 1024) {
        set_error("ws3d_instance_clouds: sampled_pts_num=%d unsupported (limit %d)", sampled_pts_num, 150 * 1024 / 24);
        return WS3D_E_UNSUPPORTED;
    }
    if (int rc = raise_lds_cap((const void *)instance_clouds_kernel, smem, "ws3d_instance_clouds")) return rc;
    hipLaunchKernelGGL(instance_clouds_kernel, dim3((unsigned)(batch * centres_num)), dim3(256), smem, as_stream(stream), pts_num, centres_num,
                       feat_len, sampled_pts_num, radius, mask_mode, mask_thresh, pts, score, feats, centres, num, cloud, cloud_feats, count, pts_idx);
    return check_launch("ws3d_instance_clouds");
}

extern "C" int ws3d_instance_clouds_count(int batch, int pts_num, int centres_num, float radius, const float *pts, const float *centres,
                                          const int32_t *num, int32_t *count, ws3d_stream_t stream) {
    using namespace ws3d;
    if (int rc = ic_check("ws3d_instance_clouds_count", batch, pts_num, centres_num, 0, radius, 0)) return rc;
    if (batch == 0 || centres_num == 0) return WS3D_OK;
    if (pts_num == 0 && !count) return WS3D_OK;
    if ((pts_num > 0 && !pts) || !centres || !count) {
        set_error("ws3d_instance_clouds_count: invalid argument (a required pointer is NULL)");
        return WS3D_E_INVALID;
    }
    hipLaunchKernelGGL(instance_clouds_count_kernel, dim3((unsigned)(batch * centres_num)), dim3(256), 0, as_stream(stream), pts_num, centres_num,
                       radius, pts, centres, num, count);
    return check_launch("ws3d_instance_clouds_count");
}

extern "C" int ws3d_instance_clouds_emit(int batch, int pts_num, int centres_num, int feat_len, float radius, int mask_mode, float mask_thresh,
                                         const float *pts, const float *score, const float *feats, const float *centres, const int32_t *num,
                                         const int64_t *offsets, float *rows, float *row_feats, int32_t *row_idx, ws3d_stream_t stream) {
    using namespace ws3d;
    if (int rc = ic_check("ws3d_instance_clouds_emit", batch, pts_num, centres_num, feat_len, radius, mask_mode)) return rc;
    if (batch == 0 || centres_num == 0 || pts_num == 0) return WS3D_OK;
    if (!pts || !score || (feat_len > 0 && (!feats || !row_feats)) || !centres || !offsets || !rows) {
        set_error("ws3d_instance_clouds_emit: invalid argument (a required pointer is NULL)");
        return WS3D_E_INVALID;
    }
    if (feat_len > 0 && (ic_misaligned(feats) || ic_misaligned(row_feats))) {
        set_error("ws3d_instance_clouds_emit: invalid argument (feats / row_feats must be 16-byte aligned)");
        return WS3D_E_INVALID;
    }
    hipLaunchKernelGGL(instance_clouds_emit_kernel, dim3((unsigned)(batch * centres_num)), dim3(256), 0, as_stream(stream), pts_num, centres_num,
                       feat_len, radius, mask_mode, mask_thresh, pts, score, feats, centres, num, offsets, rows, row_feats, row_idx);
    return check_launch("ws3d_instance_clouds_emit");
}
