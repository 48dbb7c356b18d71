// rpn_targets.hip -- the Stage-1 training targets and the RPN loss on the device (include/ws3d_ops.h):
//   ws3d_rpn_center_labels  generate_gaussian_training_labels (lib/datasets/kitti_rcnn_dataset.py:529-573), a padded batch per call
//   ws3d_rpn_loss           get_rpn_loss (lib/net/train_functions.py:163-228) on SigmoidFocalClassificationLoss and get_rpn_reg_loss
//                           (lib/utils/loss_utils.py:25-156): every component, the foreground count and the gradient of the total
// The contracts are ws3d_amd.losses.gaussian_center_labels and ws3d_amd.losses.rpn_loss(gaussian_center=True); conventions are those of
// stage2_loss.hip (row terms in float64 from the fp32 inputs, means as sum / max(count, 1), float64 sums in a fixed order, no atomics).
#include <climits>
#include <math.h>

#include "common.h"

namespace ws3d {

// ------------------------------------------------------------------------------------------------ labels
// One thread per point, grid (ceil(N / 256), B); the scene's centres go through LDS in chunks of LABEL_CHUNK (every lane reads the same
// address: a broadcast), so any count works.  Every operation of the distance is a separate correctly rounded fp32 operation in
// numpy's order: the point's own height scaled, (dx^2 + yh^2) + dz^2, sqrtf (hipcc keeps fp32 sqrt correctly rounded by default;
// __fsqrt_rn of this toolchain's headers is the native, NOT correctly rounded instruction).  min_k clip(d_k - status, 0, 100) =
// clip(min_k d_k - status, 0, 100): fp32 subtraction and the clip are monotone, so one running minimum serves near, close and target.
// Labels 16.9-18.4 m from the nearest centre are fp32 denormals and count as foreground downstream: nothing here flushes them (the
// library is built with fp32 denormals on, the gfx9 default).
constexpr int LABEL_T = 256, LABEL_CHUNK = 64;

__global__ __launch_bounds__(LABEL_T) void rpn_center_labels_kernel(int n, int kmax, int pts_stride, float gauss_height, float gauss_status,
                                                                    double gauss_cov, const float *__restrict__ pts,
                                                                    const float *__restrict__ centres, const int32_t *__restrict__ count,
                                                                    float *__restrict__ cls_label, float *__restrict__ reg_label) {
    __shared__ float2 xz_s[LABEL_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int i = blockIdx.x * LABEL_T + tid;
    const int nb = min(max(count[b], 0), kmax);  // workgroup-uniform; a count outside 0..Kmax cannot carry a read past the scene's centres
    // a lane past the scene loads the last point (clamped, never branched) and stores nothing
    const float *p = pts + ((size_t)b * n + min(i, n - 1)) * pts_stride;
    const float px = p[0], py = p[1], pz = p[2];
    const float yh = py * gauss_height;
    const float yh2 = yh * yh;
    const float *c = centres + (size_t)b * kmax * 3;
    float best = INFINITY, tx = 0.f, tz = 0.f;
    for (int k0 = 0; k0 < nb; k0 += LABEL_CHUNK) {
        const int kn = min(LABEL_CHUNK, nb - k0);
        if (tid < kn) xz_s[tid] = make_float2(c[(size_t)(k0 + tid) * 3], c[(size_t)(k0 + tid) * 3 + 2]);  // a centre's y is never read
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            const float2 q = xz_s[k];
            const float dx = px - q.x, dz = pz - q.y;
            const float d = sqrtf((dx * dx + yh2) + dz * dz);
            if (d < best || (k0 + k) == 0) { best = d; tx = q.x; tz = q.y; }  // the FIRST minimum, as argmin (centre 0 when none is finite)
        }
        __syncthreads();
    }
    if (i >= n) return;
    float cls = 0.f, rx = 0.f, rz = 0.f;
    if (nb > 0) {
        const float near = fminf(100.0f, fminf(fmaxf(best - gauss_status, 0.0f), 100.0f));
        cls = (float)exp(-0.5 * ((double)near * (double)near) / gauss_cov);
        if (best < 4.0f) { rx = tx - px; rz = tz - pz; }
    }
    const size_t o = (size_t)b * n + i;
    cls_label[o] = cls;
    reg_label[o * 3] = rx; reg_label[o * 3 + 1] = 0.f; reg_label[o * 3 + 2] = rz;
}

// ------------------------------------------------------------------------------------------------ loss
// Three launches on the caller's stream, nothing read back:
//   1. rpn_loss_counts_kernel  workgroup g sums the labels and counts the foreground rows (label > 0) of rows [4096 g, 4096 g + 4096)
//   2. rpn_loss_rows_kernel    workgroup g owns rows [128 g, 128 g + 128): it folds the partial counts (every workgroup the same fold, so
//                              every workgroup holds the same totals), evaluates its rows, writes their gradient -- of the TOTAL loss,
//                              already normalised -- and leaves its seven partial sums at workspace slot g
//   3. rpn_loss_fold_kernel    one workgroup folds the partial sums and writes vals / counts
// Every fold is "thread t adds slots t, t + T, ... in ascending order, then a halving tree": the result depends on the number of rows
// only, never on which workgroup ran when -- a call is bit-reproducible, and the workspace carries no state from one call to the next.
//
// A row's terms are float64 from its fp32 inputs, with the roundings the contract itself makes in fp32 whatever the dtype of the
// logits, because it forms them from `label.float()` and from `bin_label.float()`:
//   neg = fp32(1 - label), the weight fp32(fp32(label + neg) / fp32(max(sum label, 1))), alpha_t = fp32(fp32(label * alpha) +
//   fp32(neg * (1 - alpha))), and the centre of the labelled bin fp32(fp32(bin * bin_size) + fp32(bin_size / 2)).
// The gradient is autograd's: through the focal modulating factor too, d clamp(x, 0) = [x >= 0], d |x| = sign(x).
constexpr int RL_T = 128;                       // rows (= threads) per workgroup of the row kernel: 128 * 16 * bins bytes of LDS, 64 KiB at 32 bins
constexpr int RL_CT = 256, RL_CROWS = 4096;     // the counting kernel: 256 threads, 16 rows each
constexpr int RL_FT = 256;                      // the final fold
constexpr int RL_SUMS = 7, RL_SLOT = 8;         // partial sums per workgroup of the row kernel / doubles per workspace slot
constexpr int RL_MAX_BINS = 32;
enum { S_CLS, S_POS, S_NEG, S_XBIN, S_ZBIN, S_XRES, S_ZRES };

typedef float rl_f4 __attribute__((ext_vector_type(4)));

struct RpnLossArgs {
    int rows, bins;
    double loc_scope, bin_size, alpha, gamma, w_cls, w_reg;
};

__host__ __device__ static inline long rl_count_slots(long rows) { return (rows + RL_CROWS - 1) / RL_CROWS; }
__host__ __device__ static inline long rl_row_slots(long rows) { return (rows + RL_T - 1) / RL_T; }

// halving tree over red[0..T); every thread returns the total
template <int T>
__device__ __forceinline__ double tree_sum(double *red, double v) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int half = T / 2; half > 0; half >>= 1) {
        if (t < half) red[t] = red[t] + red[t + half];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// sum of v[i * stride], i < n, in the fixed order described above
template <int T>
__device__ __forceinline__ double fold_slots(const double *__restrict__ v, long n, int stride, double *red) {
    double a = 0.0;
    for (long i = threadIdx.x; i < n; i += T) a += v[i * stride];
    return tree_sum<T>(red, a);
}

// foreground = label > 0 on the bits, so that no denormal mode can turn a denormal label into background
__device__ __forceinline__ bool is_fg(float label) { return __float_as_uint(label) - 1u < 0x7f800000u; }

__global__ __launch_bounds__(RL_CT) void rpn_loss_counts_kernel(int rows, const float *__restrict__ cls_label, double *__restrict__ cnt) {
    __shared__ double red[RL_CT];
    const long base = (long)blockIdx.x * RL_CROWS;
    double s = 0.0, f = 0.0;
#pragma unroll 4
    for (int j = 0; j < RL_CROWS / RL_CT; ++j) {
        const long r = base + j * RL_CT + threadIdx.x;
        if (r < rows) {
            const float l = cls_label[r];
            s += (double)l;
            f += is_fg(l) ? 1.0 : 0.0;
        }
    }
    s = tree_sum<RL_CT>(red, s);
    f = tree_sum<RL_CT>(red, f);
    if (threadIdx.x == 0) { cnt[2 * blockIdx.x] = s; cnt[2 * blockIdx.x + 1] = f; }
}

__device__ __forceinline__ double rl_smooth_l1(double d) { const double a = fabs(d); return a < 1.0 ? 0.5 * d * d : a - 0.5; }
__device__ __forceinline__ double rl_smooth_l1_grad(double d) { return fabs(d) < 1.0 ? d : (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0)); }

// One axis of a foreground row held in LDS: bin cross entropy over g[lo .. lo + bins), smooth-L1 on the residual column of the labelled
// bin (g[2 bins + lo + bin]); the row's entries are replaced by their gradient (scale = loss weight / foreground rows).
__device__ __forceinline__ void rl_axis(float *g, int lo, const RpnLossArgs &a, float offset, double scale, double &ce, double &res) {
    const double shift = fmin(fmax((double)offset + a.loc_scope, 0.0), a.loc_scope * 2 - 1e-3);
    int bin = (int)floor(shift / a.bin_size);
    bin = bin < 0 ? 0 : (bin >= a.bins ? a.bins - 1 : bin);                       // (inside the row whatever the configuration)
    const float centre = (float)bin * (float)a.bin_size + (float)(a.bin_size / 2);  // fp32, see above
    const double res_label = (shift - (double)centre) / (a.bin_size / 2);
    double m = (double)g[lo];
    for (int k = 1; k < a.bins; ++k) m = fmax(m, (double)g[lo + k]);
    double z = 0.0;
    for (int k = 0; k < a.bins; ++k) z += exp((double)g[lo + k] - m);
    ce = log(z) + m - (double)g[lo + bin];
    const double d = (double)g[2 * a.bins + lo + bin] - res_label;
    res = rl_smooth_l1(d);
    for (int k = 0; k < a.bins; ++k) {
        g[lo + k] = (float)(scale * (exp((double)g[lo + k] - m) / z - (k == bin ? 1.0 : 0.0)));
        g[2 * a.bins + lo + k] = k == bin ? (float)(scale * rl_smooth_l1_grad(d)) : 0.f;
    }
}

__global__ __launch_bounds__(RL_T) void rpn_loss_rows_kernel(RpnLossArgs a, const float *__restrict__ rpn_cls, const float *__restrict__ rpn_reg,
                                                             const float *__restrict__ cls_label, const float *__restrict__ reg_label,
                                                             const double *__restrict__ cnt, double *__restrict__ part,
                                                             float *__restrict__ grad_cls, float *__restrict__ grad_reg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rl_lds[];
    float *tile = reinterpret_cast<float *>(rl_lds);      // [RL_T rows][4 bins]
    double *red = reinterpret_cast<double *>(rl_lds);     // the folds, before and after the tile's life
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int width = 4 * a.bins;

    const long cslots = rl_count_slots(a.rows);
    const double sum_label = fold_slots<RL_T>(cnt, cslots, 2, red);
    const double n_fg = fmax(fold_slots<RL_T>(cnt + 1, cslots, 2, red), 1.0);
    const float denom = fmaxf((float)sum_label, 1.0f);

    const long r = (long)blockIdx.x * RL_T + t;
    const bool live = r < a.rows;
    const float label = live ? cls_label[r] : 0.f;
    const bool fg = live && is_fg(label);
    double acc[RL_SUMS];
#pragma unroll
    for (int k = 0; k < RL_SUMS; ++k) acc[k] = 0.0;

    if (live) {     // the focal term
        const float neg = (float)(1.0 - (double)label);
        const float weight = (label + neg) / denom;
        const float alpha_t = label * (float)a.alpha + neg * (float)(1.0 - a.alpha);
        const double x = (double)rpn_cls[r], td = (double)label, nd = (double)neg;
        const double e = exp(-fabs(x));
        const double ce = (fmax(x, 0.0) - x * td) + log1p(e);
        const double p = 1.0 / (1.0 + exp(-x)), q = 1.0 - p;
        const double base = 1.0 - (td * p + nd * q);
        double mod, dmod;                                           // the modulating factor base^gamma and its derivative in base
        if (a.gamma == 2.0) { mod = base * base; dmod = 2.0 * base; }
        else if (a.gamma == 0.0) { mod = 1.0; dmod = 0.0; }
        else { mod = pow(base, a.gamma); dmod = a.gamma * pow(base, a.gamma - 1.0); }
        const double aw = (double)alpha_t * (double)weight;
        const double per = mod * (double)alpha_t * ce * (double)weight;
        const double dce = ((x >= 0.0 ? 1.0 : 0.0) - td) - (x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0)) * e / (1.0 + e);
        const double dbase = (nd - td) * p * q;
        grad_cls[r] = (float)(a.w_cls * (aw * (dmod * dbase * ce + mod * dce)));
        acc[S_CLS] = per; acc[S_POS] = per * td; acc[S_NEG] = per * nd;
    }

    // The regression rows.  A wave moves its 64 rows (64 * bins contiguous 16-byte pieces) into LDS with 16-byte accesses, a lane works
    // on its own row there, and the wave moves the rows out again as the gradient.  A wave without a foreground row reads nothing and
    // stores zeros.
    const bool any = __ballot(fg) != 0;
    const size_t piece0 = ((size_t)blockIdx.x * RL_T + (size_t)wave * 64) * a.bins, pieces = (size_t)a.rows * a.bins;
    rl_f4 *tile4 = reinterpret_cast<rl_f4 *>(tile) + (size_t)wave * 64 * a.bins;
    if (any) {
        const rl_f4 *in4 = reinterpret_cast<const rl_f4 *>(rpn_reg);
        for (int i = lane; i < 64 * a.bins; i += 64)
            if (piece0 + i < pieces) tile4[i] = in4[piece0 + i];
    }
    __syncthreads();
    if (any) {
        float *g = tile + (size_t)t * width;
        if (fg) {
            const float *off = reg_label + (size_t)r * 3;
            const double scale = a.w_reg / n_fg;
            rl_axis(g, 0, a, off[0], scale, acc[S_XBIN], acc[S_XRES]);
            rl_axis(g, a.bins, a, off[2], scale, acc[S_ZBIN], acc[S_ZRES]);
        } else {
            for (int k = 0; k < width; ++k) g[k] = 0.f;
        }
    }
    __syncthreads();
    {
        rl_f4 *out4 = reinterpret_cast<rl_f4 *>(grad_reg);
        const rl_f4 zero = {0.f, 0.f, 0.f, 0.f};
        for (int i = lane; i < 64 * a.bins; i += 64)
            if (piece0 + i < pieces) out4[piece0 + i] = any ? tile4[i] : zero;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RL_SUMS; ++k) {
        const double s = tree_sum<RL_T>(red, acc[k]);
        if (t == 0) part[(size_t)blockIdx.x * RL_SLOT + k] = s;
    }
}

__global__ __launch_bounds__(RL_FT) void rpn_loss_fold_kernel(RpnLossArgs a, const double *__restrict__ cnt, const double *__restrict__ part,
                                                              float *__restrict__ vals, int32_t *__restrict__ counts) {
    __shared__ double red[RL_FT];
    const double f = fold_slots<RL_FT>(cnt + 1, rl_count_slots(a.rows), 2, red);
    const long slots = rl_row_slots(a.rows);
    double s[RL_SUMS];
#pragma unroll
    for (int k = 0; k < RL_SUMS; ++k) s[k] = fold_slots<RL_FT>(part + k, slots, RL_SLOT, red);
    if (threadIdx.x == 0) {
        const double n_fg = fmax(f, 1.0);
        const double x_bin = s[S_XBIN] / n_fg, z_bin = s[S_ZBIN] / n_fg, x_res = s[S_XRES] / n_fg, z_res = s[S_ZRES] / n_fg;
        const double loss_reg = (x_bin + z_bin) + (x_res + z_res);      // the reference's order
        vals[0] = (float)(s[S_CLS] * a.w_cls + loss_reg * a.w_reg);
        vals[1] = (float)s[S_CLS]; vals[2] = (float)loss_reg; vals[3] = (float)s[S_POS]; vals[4] = (float)s[S_NEG];
        vals[5] = (float)x_bin; vals[6] = (float)z_bin; vals[7] = (float)x_res; vals[8] = (float)z_res;
        counts[0] = (int32_t)f;
    }
}

}  // namespace ws3d

using namespace ws3d;

extern "C" int ws3d_rpn_center_labels(int batch, int n, int kmax, int pts_stride, float gauss_height, float gauss_status, double gauss_cov,
                                      const float *pts, const float *centres, const int32_t *count, float *cls_label, float *reg_label,
                                      ws3d_stream_t stream) {
    if (batch < 0 || n < 0 || kmax < 0 || pts_stride < 3 || !(gauss_cov > 0.0)) {
        set_error("ws3d_rpn_center_labels: invalid argument (B=%d N=%d Kmax=%d stride=%d cov=%g)", batch, n, kmax, pts_stride, gauss_cov);
        return WS3D_E_INVALID;
    }
    if (batch == 0 || n == 0) return WS3D_OK;
    if (!pts || !count || !cls_label || !reg_label || (kmax > 0 && !centres)) {
        set_error("ws3d_rpn_center_labels: invalid argument (a required pointer is NULL)");
        return WS3D_E_INVALID;
    }
    if (batch > 65535 || (long)n + LABEL_T > INT_MAX) {     // grid.y, int point indices
        set_error("ws3d_rpn_center_labels: B=%d N=%d in one call are not supported", batch, n);
        return WS3D_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(rpn_center_labels_kernel, dim3((n + LABEL_T - 1) / LABEL_T, batch), dim3(LABEL_T), 0, as_stream(stream), n, kmax, pts_stride,
                       gauss_height, gauss_status, gauss_cov, pts, centres, count, cls_label, reg_label);
    return check_launch("ws3d_rpn_center_labels");
}

extern "C" size_t ws3d_rpn_loss_workspace_bytes(int rows) {
    const long r = rows > 0 ? rows : 0;
    return (size_t)(2 * rl_count_slots(r) + RL_SLOT * rl_row_slots(r) + 2) * sizeof(double);
}

extern "C" int ws3d_rpn_loss(int rows, int bins, double loc_scope, double loc_bin_size, double alpha, double gamma, double weight_cls,
                             double weight_reg, const float *rpn_cls, const float *rpn_reg, const float *cls_label, const float *reg_label,
                             float *vals, int32_t *counts, float *grad_cls, float *grad_reg, void *workspace, size_t workspace_bytes,
                             ws3d_stream_t stream) {
    if (rows < 0 || bins <= 0 || bins > RL_MAX_BINS || !(loc_bin_size > 0.0) ||
        (rows > 0 && (!rpn_cls || !rpn_reg || !cls_label || !reg_label || !vals || !counts || !grad_cls || !grad_reg || !workspace))) {
        set_error("ws3d_rpn_loss: invalid argument (rows=%d bins=%d (1..%d) loc_bin_size=%g, or a required pointer is NULL)", rows, bins, RL_MAX_BINS,
                  loc_bin_size);
        return WS3D_E_INVALID;
    }
    if (rows == 0) return WS3D_OK;
    if (((uintptr_t)rpn_reg | (uintptr_t)grad_reg) & 15 || (uintptr_t)workspace & 7) {
        set_error("ws3d_rpn_loss: invalid argument (rpn_reg and grad_reg must be 16-byte aligned, the workspace 8-byte aligned)");
        return WS3D_E_INVALID;
    }
    if (workspace_bytes < ws3d_rpn_loss_workspace_bytes(rows)) {
        set_error("ws3d_rpn_loss: workspace of %zu bytes, %zu needed", workspace_bytes, ws3d_rpn_loss_workspace_bytes(rows));
        return WS3D_E_WORKSPACE;
    }
    const RpnLossArgs a = {rows, bins, loc_scope, loc_bin_size, alpha, gamma, weight_cls, weight_reg};
    double *cnt = static_cast<double *>(workspace), *part = cnt + 2 * rl_count_slots(rows);
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(rpn_loss_counts_kernel, dim3((unsigned)rl_count_slots(rows)), dim3(RL_CT), 0, s, rows, cls_label, cnt);
    hipLaunchKernelGGL(rpn_loss_rows_kernel, dim3((unsigned)rl_row_slots(rows)), dim3(RL_T), (size_t)RL_T * 16 * bins, s, a, rpn_cls, rpn_reg, cls_label,
                       reg_label, cnt, part, grad_cls, grad_reg);
    hipLaunchKernelGGL(rpn_loss_fold_kernel, dim3(1), dim3(RL_FT), 0, s, a, cnt, part, vals, counts);
    return check_launch("ws3d_rpn_loss");
}
