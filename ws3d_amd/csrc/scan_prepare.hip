// scan_prepare.hip -- raw KITTI scans to pts_input on the device (ws3d extension; the host counterpart is
// kitti_io.rpn_input_from_scan, the bit-exact host restatement of THIS contract is ws3d_amd/scan_prepare.py).
//
// Per scene: project every raw point to the rectified camera frame and the image, classify it (invalid | near | far), draw the
// npoints-row sample with a counter-based generator and write the rows in a keyed order.  The result is a function of the inputs and
// (seed, scene_key) alone: keys are recomputed from the entry number, every reduction is an integer count, and the final order comes
// from a sort over unique 64-bit keys, so neither launch geometry nor the arrival order of waves can show in an output.
//
//   scan_classify_kernel   grid (ceil(max_scan_points / 256), scenes): one thread per raw point -> one class byte of workspace
//   scan_sample_kernel     one 1024-thread workgroup per scene:
//     1. V and F from the class bytes (ballots + LDS integer atomics)
//     2. the cut: an 8 x 8-bit radix select of the k-th smallest composite (sel << 32 | e) -- unique because e is -- with the
//        histogram in LDS and the keys recomputed from e in every pass, never stored.  V <= npoints enumerates the tiled entries
//        e = r n + i through a list of the valid indices in workspace (reps V < 2 npoints entries, not reps n)
//     3. the kept entries compacted as (ord << 32 | e) into dynamic LDS (P = npoints rounded up to a power of two, 8 P bytes:
//        128 KiB at 16384, above the default cap, hence raise_lds_cap), padded with ~0 and sorted by a bitonic network
//     4. rows gathered: the projection of point e mod n recomputed with the classify pass's own expression, refl - 0.5f appended
//
// Arithmetic: fp32, the source order below, no contraction (-ffp-contract=off), correctly rounded division (hipcc's default), a NaN
// compares false and makes the point invalid.
#include "common.h"

namespace ws3d {

constexpr int SCAN_NT = 1024;            // threads of scan_sample_kernel
constexpr int SCAN_CLS_NT = 256;         // threads of scan_classify_kernel
constexpr int SCAN_LIMIT = 16384;        // 8 B x 16384 keys = 128 KiB of the CU's 160 KiB
enum : int { SCAN_INVALID = 0, SCAN_NEAR = 1, SCAN_FAR = 2 };
enum : int { SCAN_OK = 0, SCAN_EMPTY = 1, SCAN_TOO_FAR = 2, SCAN_BAD_OFFSETS = 3 };

struct ScanScope {
    int on;
    float v[6];      // x0 x1 y0 y1 z0 z1
};

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// (sel << 32 | e) and (ord << 32 | e) of entry e; base = splitmix64(seed + golden * scene_key)
__device__ __forceinline__ uint64_t scan_sel_key(uint64_t base, uint32_t e, int shift) {
    const uint64_t h = splitmix64(base + e);
    return ((uint64_t)((uint32_t)(h >> 32) >> shift) << 32) | e;
}
__device__ __forceinline__ uint64_t scan_ord_key(uint64_t base, uint32_t e, int shift) {
    const uint64_t h = splitmix64(base + e);
    return ((uint64_t)((uint32_t)h >> shift) << 32) | e;
}

// r_j = ((x T[0][j] + y T[1][j]) + z T[2][j]) + T[3][j]
__device__ __forceinline__ void scan_rect(const float *__restrict__ c, float x, float y, float z, float &r0, float &r1, float &r2) {
    r0 = ((x * c[0] + y * c[3]) + z * c[6]) + c[9];
    r1 = ((x * c[1] + y * c[4]) + z * c[7]) + c[10];
    r2 = ((x * c[2] + y * c[5]) + z * c[8]) + c[11];
}

// the scene's slice of the packed arrays, or false when the device offsets do not describe one (nothing of it is then touched)
__device__ __forceinline__ bool scan_slice(const int32_t *__restrict__ offsets, int b, long total, int max_n, int &off, int &n) {
    off = offsets[b];
    const int end = offsets[b + 1];
    n = end - off;
    return off >= 0 && end >= off && (long)end <= total && n <= max_n;
}

__global__ __launch_bounds__(SCAN_CLS_NT) void scan_classify_kernel(const int32_t *__restrict__ offsets, long total, int max_n,
                                                                    const float *__restrict__ raw, const float *__restrict__ calib,
                                                                    const int32_t *__restrict__ img_hw, ScanScope scope,
                                                                    uint8_t *__restrict__ cls) {
    const int b = blockIdx.y;
    int off, n;
    if (!scan_slice(offsets, b, total, max_n, off, n)) return;
    const int i = blockIdx.x * SCAN_CLS_NT + threadIdx.x;
    if (i >= n) return;
    const float *c = calib + (size_t)b * 24, *P = c + 12;
    const float H = (float)img_hw[b * 2], W = (float)img_hw[b * 2 + 1];
    const float4 p = reinterpret_cast<const float4 *>(raw)[(size_t)off + i];
    float r0, r1, r2;
    scan_rect(c, p.x, p.y, p.z, r0, r1, r2);
    const float h0 = ((r0 * P[0] + r1 * P[1]) + r2 * P[2]) + P[3];
    const float h1 = ((r0 * P[4] + r1 * P[5]) + r2 * P[6]) + P[7];
    const float h2 = ((r0 * P[8] + r1 * P[9]) + r2 * P[10]) + P[11];
    const float u = h0 / r2, v = h1 / r2, depth = h2 - P[11];
    bool valid = u >= 0.0f && u < W && v >= 0.0f && v < H && depth >= 0.0f;
    if (scope.on)
        valid = valid && r0 >= scope.v[0] && r0 <= scope.v[1] && r1 >= scope.v[2] && r1 <= scope.v[3] && r2 >= scope.v[4] && r2 <= scope.v[5];
    cls[(size_t)off + i] = (uint8_t)(!valid ? SCAN_INVALID : (depth < 40.0f ? SCAN_NEAR : SCAN_FAR));
}

struct ScanShared {
    int hist[256];
    int wsum[4];
    int bin, below;
    int count[2];
    int fill;
};

// The k-th smallest (1-based) composite among the candidates; `cand(t, e)` says whether enumeration slot t < slots holds a
// candidate and gives its entry.  Every thread returns the same value.
template <class Cand>
__device__ __forceinline__ uint64_t scan_select(ScanShared &s, uint64_t base, int shift, uint32_t slots, int k, Cand cand) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint64_t prefix = 0;
    for (int pass = 7; pass >= 0; --pass) {
        if (tid < 256) s.hist[tid] = 0;
        __syncthreads();
        for (uint32_t t = tid; t < slots; t += SCAN_NT) {
            uint32_t e;
            if (!cand(t, e)) continue;
            const uint64_t key = scan_sel_key(base, e, shift);
            const bool in = pass == 7 || (key >> (8 * pass + 8)) == (prefix >> (8 * pass + 8));
            if (in) atomicAdd(&s.hist[(int)((key >> (8 * pass)) & 255)], 1);
        }
        __syncthreads();
        int v = 0, incl = 0;
        if (tid < 256) {
            v = s.hist[tid];
            incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            if (lane == 63) s.wsum[w] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            for (int q = 0; q < w; ++q) incl += s.wsum[q];
            const int excl = incl - v;
            if (excl < k && k <= incl) {
                s.bin = tid;
                s.below = excl;
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s.bin << (8 * pass);
        k -= s.below;
    }
    return prefix;
}

// keep(t, e): slot t holds a kept entry; its order key goes to the next free place of keys[] (any place: the sort follows)
template <class Keep>
__device__ __forceinline__ void scan_compact(ScanShared &s, uint64_t *keys, int cap, uint64_t base, int shift, uint32_t slots, Keep keep) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t0 = threadIdx.x - lane; t0 < slots; t0 += SCAN_NT) {     // wave-uniform trip count: the ballot sees whole waves
        const uint32_t t = t0 + lane;
        uint32_t e = 0;
        const bool k = t < slots && keep(t, e);
        const uint64_t m = __ballot(k);
        if (m == 0) continue;
        int at = 0;
        if (lane == (int)__builtin_ctzll(m)) at = atomicAdd(&s.fill, (int)__builtin_popcountll(m));
        at = __builtin_amdgcn_readlane(at, (int)__builtin_ctzll(m)) + (int)__builtin_popcountll(m & ((1ull << lane) - 1));
        if (k && at < cap) keys[at] = scan_ord_key(base, e, shift);
    }
}

__global__ __launch_bounds__(SCAN_NT) void scan_sample_kernel(const int32_t *__restrict__ offsets, long total, int max_n,
                                                              const float *__restrict__ raw, const float *__restrict__ calib, int npoints,
                                                              int P2, uint64_t seed, const int64_t *__restrict__ scene_key, int key_bits,
                                                              const uint8_t *__restrict__ cls_all, int32_t *__restrict__ list_all,
                                                              float *__restrict__ pts_input, int32_t *__restrict__ src_index,
                                                              int32_t *__restrict__ valid_count, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];
    __shared__ ScanShared s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    float4 *rows = reinterpret_cast<float4 *>(pts_input) + (size_t)b * npoints;
    int32_t *src = src_index + (size_t)b * npoints;
    int off, n;
    const bool slice_ok = scan_slice(offsets, b, total, max_n, off, n);
    if (!slice_ok) n = 0;
    const uint8_t *cls = cls_all + (slice_ok ? off : 0);
    int32_t *list = list_all + (size_t)b * npoints;

    // 1. V and F
    if (tid < 2) s.count[tid] = 0;
    if (tid == 0) s.fill = 0;
    __syncthreads();
    for (int i0 = tid - lane; i0 < n; i0 += SCAN_NT) {
        const int i = i0 + lane;
        const int c = i < n ? cls[i] : SCAN_INVALID;
        const uint64_t mv = __ballot(c != SCAN_INVALID), mf = __ballot(c == SCAN_FAR);
        if (lane == 0 && mv) {
            atomicAdd(&s.count[0], (int)__builtin_popcountll(mv));
            if (mf) atomicAdd(&s.count[1], (int)__builtin_popcountll(mf));
        }
    }
    __syncthreads();
    const int V = s.count[0], F = s.count[1];
    const int st = !slice_ok ? SCAN_BAD_OFFSETS : V == 0 ? SCAN_EMPTY : (V > npoints && F > npoints) ? SCAN_TOO_FAR : SCAN_OK;
    if (tid == 0) {
        valid_count[b] = V;
        status[b] = st;
    }
    if (st != SCAN_OK) {
        for (int j = tid; j < npoints; j += SCAN_NT) {
            rows[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            src[j] = -1;
        }
        return;
    }
    const uint64_t base = splitmix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)scene_key[b]);
    const int shift = 32 - key_bits;

    // 2. + 3. the cut, then the kept entries' order keys into LDS
    if (V > npoints) {
        const int k = npoints - F;       // near points to keep, 0 .. npoints
        uint64_t cut = 0;
        if (k > 0)
            cut = scan_select(s, base, shift, (uint32_t)n, k, [&](uint32_t t, uint32_t &e) { e = t; return cls[t] == SCAN_NEAR; });
        scan_compact(s, s_keys, npoints, base, shift, (uint32_t)n, [&](uint32_t t, uint32_t &e) {
            e = t;
            const int c = cls[t];
            return c == SCAN_FAR || (k > 0 && c == SCAN_NEAR && scan_sel_key(base, t, shift) <= cut);
        });
    } else {
        // the valid indices, in any order (the entries they stand for are keyed by e, not by their place in the list)
        for (int i0 = tid - lane; i0 < n; i0 += SCAN_NT) {
            const int i = i0 + lane;
            const bool ok = i < n && cls[i] != SCAN_INVALID;
            const uint64_t m = __ballot(ok);
            if (m == 0) continue;
            int at = 0;
            if (lane == (int)__builtin_ctzll(m)) at = atomicAdd(&s.fill, (int)__builtin_popcountll(m));
            at = __builtin_amdgcn_readlane(at, (int)__builtin_ctzll(m)) + (int)__builtin_popcountll(m & ((1ull << lane) - 1));
            if (ok && at < npoints) list[at] = i;
        }
        __syncthreads();                 // (workgroup scope: the list is read back by this workgroup alone)
        if (tid == 0) s.fill = 0;
        const int reps = (npoints + V - 1) / V;
        const uint32_t slots = (uint32_t)reps * (uint32_t)V;         // < 2 npoints
        auto entry = [&](uint32_t t, uint32_t &e) {
            const uint32_t r = t / (uint32_t)V;
            e = r * (uint32_t)n + (uint32_t)list[t - r * (uint32_t)V];      // < npoints * max_scan_points < 2^32 (checked by the entry)
            return true;
        };
        const uint64_t cut = scan_select(s, base, shift, slots, npoints, entry);
        scan_compact(s, s_keys, npoints, base, shift, slots,
                     [&](uint32_t t, uint32_t &e) { entry(t, e); return scan_sel_key(base, e, shift) <= cut; });
    }
    for (int j = npoints + tid; j < P2; j += SCAN_NT) s_keys[j] = ~0ull;
    __syncthreads();

    // bitonic network over P2 keys, ascending
    for (int kk = 2; kk <= P2; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P2 >> 1); t += SCAN_NT) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t a = s_keys[lo], c = s_keys[hi];
                if ((a > c) == ((lo & kk) == 0)) {
                    s_keys[lo] = c;
                    s_keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }

    // 4. the rows
    const float *cal = calib + (size_t)b * 24;
    const float4 *pts = reinterpret_cast<const float4 *>(raw) + off;
    for (int j = tid; j < npoints; j += SCAN_NT) {
        const uint32_t e = (uint32_t)s_keys[j];
        const int i = (int)(e % (uint32_t)n);
        const float4 p = pts[i];
        float r0, r1, r2;
        scan_rect(cal, p.x, p.y, p.z, r0, r1, r2);
        rows[j] = make_float4(r0, r1, r2, p.w - 0.5f);
        src[j] = i;
    }
}

static size_t scan_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace ws3d

extern "C" int ws3d_scan_prepare_limit(void) { return ws3d::SCAN_LIMIT; }

// class bytes of every raw point, then one npoints-slot index list per scene (sized for the limit: the query does not know npoints)
extern "C" size_t ws3d_scan_prepare_workspace_bytes(int scenes, long total_points) {
    if (scenes <= 0 || total_points < 0) return 0;
    return ws3d::scan_align((size_t)total_points) + (size_t)scenes * ws3d::SCAN_LIMIT * sizeof(int32_t);
}

extern "C" int ws3d_scan_prepare(int scenes, const int32_t *offsets, long total_points, int max_scan_points, const float *raw, const float *calib,
                                 const int32_t *img_hw, const float *scope, int npoints, uint64_t seed, const int64_t *scene_key, int key_bits,
                                 float *pts_input, int32_t *src_index, int32_t *valid_count, int32_t *status, void *workspace,
                                 size_t workspace_bytes, ws3d_stream_t stream) {
    using namespace ws3d;
    if (scenes < 0 || total_points < 0 || max_scan_points < 0 || npoints <= 0 || key_bits < 1 || key_bits > 32 || total_points > 0x7fffffffL) {
        set_error("ws3d_scan_prepare: invalid argument (scenes=%d total_points=%ld max_scan_points=%d npoints=%d key_bits=%d)", scenes, total_points,
                  max_scan_points, npoints, key_bits);
        return WS3D_E_INVALID;
    }
    if (scenes == 0) return WS3D_OK;
    if (!offsets || (!raw && total_points > 0) || !calib || !img_hw || !scene_key || !pts_input || !src_index || !valid_count || !status ||
        !workspace) {
        set_error("ws3d_scan_prepare: invalid argument (null pointer)");
        return WS3D_E_INVALID;
    }
    if ((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(pts_input)) & 15) {
        set_error("ws3d_scan_prepare: invalid argument (raw and pts_input must be 16-byte aligned)");
        return WS3D_E_INVALID;
    }
    if (workspace_bytes < ws3d_scan_prepare_workspace_bytes(scenes, total_points) || (reinterpret_cast<uintptr_t>(workspace) & 3)) {
        set_error("ws3d_scan_prepare: invalid argument (workspace of %zu bytes, %zu needed, 4-byte aligned)", workspace_bytes,
                  ws3d_scan_prepare_workspace_bytes(scenes, total_points));
        return WS3D_E_INVALID;
    }
    // a tiled entry number r n + i stays below npoints * max_scan_points: it must fit the 32 bits the composite keys give it
    if (npoints > SCAN_LIMIT || (uint64_t)npoints * (uint64_t)max_scan_points > 0xffffffffull || scenes > 65535) {
        set_error("ws3d_scan_prepare: unsupported (npoints=%d above %d, npoints * max_scan_points above 2^32, or more than 65535 scenes)", npoints,
                  SCAN_LIMIT);
        return WS3D_E_UNSUPPORTED;
    }
    ScanScope sc;
    sc.on = scope != nullptr;
    for (int q = 0; q < 6; ++q) sc.v[q] = scope ? scope[q] : 0.f;
    uint8_t *cls = static_cast<uint8_t *>(workspace);
    int32_t *list = reinterpret_cast<int32_t *>(cls + scan_align((size_t)total_points));
    hipStream_t st = as_stream(stream);
    if (max_scan_points > 0 && total_points > 0) {
        hipLaunchKernelGGL(scan_classify_kernel, dim3((max_scan_points + SCAN_CLS_NT - 1) / SCAN_CLS_NT, scenes), dim3(SCAN_CLS_NT), 0, st, offsets,
                           total_points, max_scan_points, raw, calib, img_hw, sc, cls);
        if (int rc = check_launch("ws3d_scan_prepare (classify)")) return rc;
    }
    int P2 = 2;
    while (P2 < npoints) P2 <<= 1;
    const size_t lds = (size_t)P2 * sizeof(uint64_t);
    if (int rc = raise_lds_cap((const void *)scan_sample_kernel, lds, "ws3d_scan_prepare")) return rc;
    hipLaunchKernelGGL(scan_sample_kernel, dim3(scenes), dim3(SCAN_NT), lds, st, offsets, total_points, max_scan_points, raw, calib, npoints, P2, seed,
                       scene_key, key_bits, cls, list, pts_input, src_index, valid_count, status);
    return check_launch("ws3d_scan_prepare (sample)");
}
