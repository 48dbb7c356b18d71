// stage2_batch.hip -- Stage-2 training batches from a device-resident box dataset (ws3d extension; the host counterpart is
// train_rcnn.BoxDataset.sample -> collate -> prepare_batch, the bit-exact host restatement of THIS contract is
// ws3d_amd/stage2_batch.py).
//
// One launch per batch, one 256-thread workgroup per sample.  The records lie on the device as packed rows
// [x, y, z, reflect, prob -+ 0.5, gt_mask - 0.5]; every floating-point draw of a sample was made on the host and arrives in the
// sample's parameter block, the per-row draws (5 % mask flips, the shuffle) come from a counter-based hash of the row number:
//
//   h(e) = splitmix64(splitmix64(sample_seed + golden) + e);  flip(e) = hi32(h) < floor(0.05 * 2^32);  ord(e) = lo32(h) >> (32 - key_bits)
//
//   stage2_batch_kernel
//     1. per row: the hash, the flip, the keep rule of the region drop-out in double; the counts of the rows the rule keeps and of the
//        rows `prob > -1` keeps, and whether the rule keeps a row with gt_mask > 0 (ballots + LDS integer atomics)
//     2. the fall-back to `prob > -1` when it keeps none; K kept rows; m = min(K, 512), cut to 128 / 32 by the block when that is 512
//     3. K > m: an 8 x 8-bit radix select of the m-th smallest composite (ord << 32 | e) among the kept rows -- unique because e
//        is -- with the histogram in LDS and the keys recomputed from e in every pass, never stored: a record of any size streams
//     4. the m kept keys compacted into LDS, padded with ~0 to a power of two and sorted by a bitonic network
//     5. output row j = row e of sorted[j mod m]: the double-precision ground shift / x flip / recentring, rounded to fp32, then
//        prepare_batch's chain revive_matrix[0], ext_noise, revive_matrix[1], noise_scale, Rot_y; reflect and prob pass through
//
// Every reduction is an integer count and the order comes from unique keys: launch geometry cannot show in an output.
// Arithmetic: the source order below, no contraction (-ffp-contract=off); a NaN compares false.
// Static LDS: 5160 bytes (512 keys of 8 bytes, a 256-bin histogram, 10 ints).  No scratch, no atomics on floats.
#include "common.h"

namespace ws3d {

constexpr int S2B_NT = 256;                     // threads of stage2_batch_kernel
constexpr int S2B_NP = 512;                     // rows of an output cloud
constexpr uint32_t S2B_FLIP = 214748364u;       // floor(0.05 * 2^32)
constexpr double S2B_GROUND_Y = 1.65;
enum : int { S2B_TRAIN = 1, S2B_DROP = 2, S2B_X_GT = 4, S2B_Z_GT = 8, S2B_OR = 16, S2B_NEG = 32, S2B_XFLIP = 64 };
enum : int { S2B_OK = 0, S2B_BAD_OFFSETS = 3 };

// ws3d_amd/stage2_batch.py PARAMS is this struct as a numpy dtype
struct S2bParams {
    double gt0, gt2;        // the box centre the drop-out compares x and z against
    double cx, cz;          // the recentring offsets (0 when aug_flag is 0 or in EVAL mode)
    uint64_t seed;
    int32_t record, flags, cut, pad;
    float revive0[16], revive1[16], rot[16];
    float ext[3], scale;
};
static_assert(sizeof(S2bParams) == 264, "S2bParams is 264 bytes on both sides");

__device__ __forceinline__ uint64_t s2b_splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct S2bShared {
    int hist[256];
    int wsum[4];
    int bin, below;
    int count[3];       // rows the rule keeps, rows `prob > -1` keeps, rows the rule keeps with gt_mask > 0
    int fill;
};

struct S2bRow {
    uint64_t key;       // ord << 32 | e
    bool rule, all, fg;
};

// what steps 1, 3 and 4 need of row e, recomputed wherever it is asked for
__device__ __forceinline__ S2bRow s2b_row(const float2 *__restrict__ rows, uint32_t e, uint64_t base, int flags, int shift, double gt0, double gt2) {
    const float2 xy = rows[(size_t)e * 3], zr = rows[(size_t)e * 3 + 1], pg = rows[(size_t)e * 3 + 2];
    const uint64_t h = s2b_splitmix64(base + e);
    const bool train = (flags & S2B_TRAIN) != 0;
    const bool fl = train && (uint32_t)(h >> 32) < S2B_FLIP;
    const float prob = fl ? -pg.x : pg.x;
    const float gtm = train ? (fl ? -pg.y : pg.y) : prob;
    S2bRow r;
    r.key = train ? (((uint64_t)((uint32_t)h >> shift) << 32) | e) : (uint64_t)e;
    r.all = !train || prob > -1.0f;
    r.rule = r.all;
    if (flags & S2B_DROP) {
        const double x = (double)xy.x, z = (double)zr.x;
        const bool sx = (flags & S2B_X_GT) ? x > gt0 : x < gt0;
        const bool sz = (flags & S2B_Z_GT) ? z > gt2 : z < gt2;
        const bool in_x = prob > 0.0f && sx, in_z = prob > 0.0f && sz;
        r.rule = (flags & S2B_OR) ? (in_x || in_z) : (in_x && in_z);
        if (flags & S2B_NEG) r.rule = r.rule || prob < 0.0f;
    }
    r.fg = r.rule && gtm > 0.0f;
    return r;
}

// column l of rows . m^T as train_rcnn._apply4 writes it
__device__ __forceinline__ float s2b_col(const float *__restrict__ m, int l, float p0, float p1, float p2, float p3) {
    return ((p0 * m[l * 4] + p1 * m[l * 4 + 1]) + p2 * m[l * 4 + 2]) + p3 * m[l * 4 + 3];
}

__global__ __launch_bounds__(S2B_NT) void stage2_batch_kernel(const S2bParams *__restrict__ params, const float *__restrict__ rows_all,
                                                              const int32_t *__restrict__ offsets, int records, long total_rows, int key_bits,
                                                              float *__restrict__ out_pts, float *__restrict__ out_reflect,
                                                              float *__restrict__ out_mask, int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint64_t s_keys[S2B_NP];
    __shared__ S2bShared s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const S2bParams &pr = params[b];
    const int rec = pr.record, flags = pr.flags;

    // the record's slice of the packed rows; offsets that do not describe one: nothing of the sample is touched
    int off = 0, n = 0;
    bool ok = rec >= 0 && rec < records;
    if (ok) {
        off = offsets[rec];
        const int end = offsets[rec + 1];
        n = end - off;
        ok = off >= 0 && end > off && (long)end <= total_rows;
    }
    if (status && tid == 0) status[b] = ok ? S2B_OK : S2B_BAD_OFFSETS;
    if (!ok) return;
    const float2 *rows = reinterpret_cast<const float2 *>(rows_all) + (size_t)off * 3;
    const uint64_t base = s2b_splitmix64(pr.seed + 0x9E3779B97F4A7C15ull);
    const int shift = 32 - key_bits;
    const double gt0 = pr.gt0, gt2 = pr.gt2;

    // 1. the counts
    if (tid < 3) s.count[tid] = 0;
    if (tid == 3) s.fill = 0;
    __syncthreads();
    for (int i0 = tid - lane; i0 < n; i0 += S2B_NT) {       // wave-uniform trip count: the ballots see whole waves
        const int i = i0 + lane;
        S2bRow r;
        r.rule = r.all = r.fg = false;
        if (i < n) r = s2b_row(rows, (uint32_t)i, base, flags, shift, gt0, gt2);
        const uint64_t mr = __ballot(r.rule), ma = __ballot(r.all), mf = __ballot(r.fg);
        if (lane == 0) {
            if (mr) atomicAdd(&s.count[0], (int)__builtin_popcountll(mr));
            if (ma) atomicAdd(&s.count[1], (int)__builtin_popcountll(ma));
            if (mf) atomicAdd(&s.count[2], (int)__builtin_popcountll(mf));
        }
    }
    __syncthreads();

    // 2. the fall-back and the number of output rows
    const bool by_rule = s.count[2] > 0;
    const int K = by_rule ? s.count[0] : s.count[1];
    int m = K < S2B_NP ? K : S2B_NP;
    if (m == S2B_NP) m = pr.cut < 1 ? 1 : (pr.cut < S2B_NP ? pr.cut : S2B_NP);
    float *opts = out_pts + (size_t)b * S2B_NP * 3, *orefl = out_reflect + (size_t)b * S2B_NP, *omask = out_mask + (size_t)b * S2B_NP;
    if (m <= 0) {           // every prob a NaN: the host route has no rows to repeat either
        for (int j = tid; j < S2B_NP; j += S2B_NT) {
            opts[j * 3] = opts[j * 3 + 1] = opts[j * 3 + 2] = 0.f;
            orefl[j] = omask[j] = 0.f;
        }
        return;
    }

    // 3. the m-th smallest composite among the kept rows (every thread ends with the same value)
    uint64_t cut = ~0ull;
    if (K > m) {
        uint64_t prefix = 0;
        int k = m;
        for (int pass = 7; pass >= 0; --pass) {
            s.hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += S2B_NT) {
                const S2bRow r = s2b_row(rows, (uint32_t)i, base, flags, shift, gt0, gt2);
                if (!(by_rule ? r.rule : r.all)) continue;
                const bool in = pass == 7 || (r.key >> (8 * pass + 8)) == (prefix >> (8 * pass + 8));
                if (in) atomicAdd(&s.hist[(int)((r.key >> (8 * pass)) & 255)], 1);
            }
            __syncthreads();
            const int v = s.hist[tid];
            int incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            if (lane == 63) s.wsum[w] = incl;
            __syncthreads();
            for (int q = 0; q < w; ++q) incl += s.wsum[q];
            const int excl = incl - v;
            if (excl < k && k <= incl) {
                s.bin = tid;
                s.below = excl;
            }
            __syncthreads();
            prefix |= (uint64_t)s.bin << (8 * pass);
            k -= s.below;
        }
        cut = prefix;
    }

    // 4. the kept keys into LDS (any place: the sort follows), padded to a power of two
    int P2 = 2;
    while (P2 < m) P2 <<= 1;
    for (int i0 = tid - lane; i0 < n; i0 += S2B_NT) {
        const int i = i0 + lane;
        bool keep = false;
        uint64_t key = 0;
        if (i < n) {
            const S2bRow r = s2b_row(rows, (uint32_t)i, base, flags, shift, gt0, gt2);
            keep = (by_rule ? r.rule : r.all) && r.key <= cut;
            key = r.key;
        }
        const uint64_t mk = __ballot(keep);
        if (mk == 0) continue;
        const int first = (int)__builtin_ctzll(mk);
        int at = 0;
        if (lane == first) at = atomicAdd(&s.fill, (int)__builtin_popcountll(mk));
        at = __builtin_amdgcn_readlane(at, first) + (int)__builtin_popcountll(mk & ((1ull << lane) - 1));
        if (keep && at < m) s_keys[at] = key;
    }
    for (int j = m + tid; j < P2; j += S2B_NT) s_keys[j] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= P2; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (tid < (P2 >> 1)) {
                const int lo = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), hi = lo | j;
                const uint64_t a = s_keys[lo], c = s_keys[hi];
                if ((a > c) == ((lo & kk) == 0)) {
                    s_keys[lo] = c;
                    s_keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }

    // 5. the rows
    const bool train = (flags & S2B_TRAIN) != 0, xflip = (flags & S2B_XFLIP) != 0;
    const double cx = pr.cx, cz = pr.cz;
    const float e0 = pr.ext[0], e1 = pr.ext[1], e2 = pr.ext[2], scale = pr.scale;
    for (int j = tid; j < S2B_NP; j += S2B_NT) {
        uint32_t e = (uint32_t)s_keys[j % m];
        if (e >= (uint32_t)n) e = 0;        // cannot happen: the m kept keys are row numbers below n
        const float2 xy = rows[(size_t)e * 3], zr = rows[(size_t)e * 3 + 1], pg = rows[(size_t)e * 3 + 2];
        const uint64_t h = s2b_splitmix64(base + e);
        const bool fl = train && (uint32_t)(h >> 32) < S2B_FLIP;
        double xd = (double)xy.x;
        if (xflip) xd = -xd;
        float p0 = (float)(xd - cx), p1 = (float)((double)xy.y - S2B_GROUND_Y), p2 = (float)((double)zr.x - cz), p3 = 1.0f;
        float q0 = s2b_col(pr.revive0, 0, p0, p1, p2, p3), q1 = s2b_col(pr.revive0, 1, p0, p1, p2, p3);
        float q2 = s2b_col(pr.revive0, 2, p0, p1, p2, p3), q3 = s2b_col(pr.revive0, 3, p0, p1, p2, p3);
        q0 = q0 * e1;
        q1 = q1 * e0;
        q2 = q2 * e2;
        p0 = s2b_col(pr.revive1, 0, q0, q1, q2, q3);
        p1 = s2b_col(pr.revive1, 1, q0, q1, q2, q3);
        p2 = s2b_col(pr.revive1, 2, q0, q1, q2, q3);
        p3 = s2b_col(pr.revive1, 3, q0, q1, q2, q3);
        p0 = p0 * scale;
        p1 = p1 * scale;
        p2 = p2 * scale;
        opts[j * 3] = s2b_col(pr.rot, 0, p0, p1, p2, p3);
        opts[j * 3 + 1] = s2b_col(pr.rot, 1, p0, p1, p2, p3);
        opts[j * 3 + 2] = s2b_col(pr.rot, 2, p0, p1, p2, p3);
        orefl[j] = zr.y;
        omask[j] = fl ? -pg.x : pg.x;
    }
}

}  // namespace ws3d

extern "C" int ws3d_stage2_batch_param_bytes(void) { return (int)sizeof(ws3d::S2bParams); }

extern "C" int ws3d_stage2_batch(int samples, const void *params, const float *rows, const int32_t *offsets, int records, long total_rows,
                                 int key_bits, float *cur_box_point, float *cur_box_reflect, float *train_mask, int32_t *status,
                                 ws3d_stream_t stream) {
    using namespace ws3d;
    if (samples < 0 || records < 0 || total_rows < 0 || total_rows > 0x7fffffffL || key_bits < 1 || key_bits > 32) {
        set_error("ws3d_stage2_batch: invalid argument (samples=%d records=%d total_rows=%ld key_bits=%d)", samples, records, total_rows, key_bits);
        return WS3D_E_INVALID;
    }
    if (samples == 0) return WS3D_OK;
    if (!params || !rows || !offsets || !cur_box_point || !cur_box_reflect || !train_mask) {
        set_error("ws3d_stage2_batch: invalid argument (null pointer)");
        return WS3D_E_INVALID;
    }
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(rows)) & 7) {
        set_error("ws3d_stage2_batch: invalid argument (params and rows must be 8-byte aligned)");
        return WS3D_E_INVALID;
    }
    hipLaunchKernelGGL(stage2_batch_kernel, dim3(samples), dim3(S2B_NT), 0, as_stream(stream), static_cast<const S2bParams *>(params), rows, offsets,
                       records, total_rows, key_bits, cur_box_point, cur_box_reflect, train_mask, status);
    return check_launch("ws3d_stage2_batch");
}
