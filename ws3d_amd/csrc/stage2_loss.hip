// stage2_loss.hip -- the two Stage-2 training losses, value and gradient in one launch each (include/ws3d_ops.h):
//   ws3d_stage2_rcnn_loss  get_rcnn_loss (lib/net/train_functions.py:230-392) + get_rcnn_reg_loss (lib/utils/loss_utils.py:151-338)
//   ws3d_stage2_ioun_loss  get_ioun_loss (train_functions.py:394-516)
// A translation unit of its own: tests/test_stage2.py pins the kernels of stage2.hip by name.
#include <math.h>

#include "common.h"
#include "bev_overlap.h"

namespace ws3d {

// ------------------------------------------------------------------------------------------------ losses
// One workgroup of LOSS_T threads per loss.  Pass 1: thread t walks rows t, t + LOSS_T, ... in ascending order and adds each row's
// terms to its own float64 partial sums; the partials meet in LDS ([sum][thread]: conflict-free) and are folded by a halving tree --
// a fixed order, no atomics, so a call is bit-reproducible.  Every thread then reads the totals, and pass 2 walks the same rows again
// and writes the gradient of the TOTAL loss, normalised by the counts pass 1 found; nothing goes back to the host.
// A row's terms are evaluated in float64 from its fp32 inputs (a few dozen operations per row: free at this size), so a component
// differs from the reference's float64 run by the order of the float64 sums and the final rounding to fp32 only -- except for two
// things that are fp32 by contract, and carry fp32 error into the terms that read them:
//   * the 3-D IoU is paired_iou (bev_overlap.h), fp32, bit for bit what ws3d_boxes_iou3d_paired returns;
//   * binary cross entropy keeps the library's fp32 behaviour at saturation: where sigmoid rounds to 0 or 1 in fp32 the log is
//     clamped to -100 and the gradient through the sigmoid is 0.
// A selection that is empty in the reference (no foreground row, no IoU above 0.5, no non-zero gt box) gives exact zeros: every
// mean is sum / max(count, 1) over a sum that received no term.
constexpr int LOSS_T = 128;
constexpr int LOSS_MAX_SUMS = 12;

struct LossLds {
    float vx[16 * LOSS_T], vy[16 * LOSS_T], va[16 * LOSS_T];
    double red[LOSS_MAX_SUMS][LOSS_T];
};

template <int NS>
__device__ __forceinline__ void loss_reduce(LossLds &s, double (&acc)[NS]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; ++k) s.red[k][t] = acc[k];
    __syncthreads();
    for (int half = LOSS_T / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int k = 0; k < NS; ++k) s.red[k][t] = s.red[k][t] + s.red[k][t + half];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = s.red[k][0];
}

__device__ __forceinline__ double smooth_l1(double d) { const double a = fabs(d); return a < 1.0 ? 0.5 * d * d : a - 0.5; }
__device__ __forceinline__ double smooth_l1_grad(double d) { return fabs(d) < 1.0 ? d : (d > 0.0 ? 1.0 : -1.0); }
__device__ __forceinline__ double py_mod_d(double a, double b) {
    double r = fmod(a, b);
    if (r != 0.0 && ((r < 0.0) != (b < 0.0))) r += b;
    return r;
}
__device__ __forceinline__ double at_least_one(double n) { return n < 1.0 ? 1.0 : n; }

// heading label of loss_utils.py:295-301: bin in [0, head_bins), residual normalised by half a bin
__device__ __forceinline__ int ry_label(double ry, int head_bins, double &res_norm) {
    const double two_pi = 2.0 * M_PI, apc = two_pi / head_bins;
    const double shift = py_mod_d(py_mod_d(ry, two_pi) + apc / 2, two_pi);
    int bin = (int)floor(shift / apc);
    res_norm = (shift - ((double)bin * apc + apc / 2)) / (apc / 2);
    return bin < 0 ? 0 : (bin >= head_bins ? head_bins - 1 : bin);       // (a NaN heading: any bin inside the row)
}

// corner c of a box (kitti_utils.py:104-131): x = +-l/2, y = 0 | -h, z = +-w/2, turned by ry about y, plus the centre
__device__ __forceinline__ void box_corner(const double *b, double cosa, double sina, int c, double &x, double &y, double &z) {
    const double xc = ((c & 3) < 2 ? 0.5 : -0.5) * b[5];
    const double yc = c < 4 ? 0.0 : -b[3];
    const double zc = (((c & 3) == 0 || (c & 3) == 3) ? 0.5 : -0.5) * b[4];
    x = cosa * xc + sina * zc + b[0];
    y = yc + b[1];
    z = -sina * xc + cosa * zc + b[2];
}

struct RcnnLossArgs {
    int rows, nb, hb;
    float loc_scope, h, w, l;
};

// per row: sigmoid and the two clamped logs with fp32 saturation -> bce; dq = d bce / d logit
__device__ __forceinline__ double bce_row(float logit, double y, double &dq) {
    const double p = 1.0 / (1.0 + exp(-(double)logit));
    const float pf = (float)p;
    const double lp = pf == 0.f ? -100.0 : fmax(log(p), -100.0);
    const double lq = pf == 1.f ? -100.0 : fmax(log1p(-p), -100.0);
    const double pq = (pf == 0.f || pf == 1.f) ? 0.0 : p * (1.0 - p);
    dq = (p - y) / fmax(pq, 1e-12) * pq;         // binary_cross_entropy's backward (EPS 1e-12), then sigmoid's
    return -(y * lp + (1.0 - y) * lq);
}

__global__ __launch_bounds__(LOSS_T) void stage2_rcnn_loss_kernel(RcnnLossArgs a, const float *__restrict__ rcnn_cls,
                                                                  const float *__restrict__ rcnn_reg, const float *__restrict__ pred,
                                                                  const float *__restrict__ gt, const float *__restrict__ cls,
                                                                  float *__restrict__ vals, int32_t *__restrict__ counts,
                                                                  float *__restrict__ grad_cls, float *__restrict__ grad_reg) {
    __shared__ LossLds s;
    const int t = threadIdx.x;
    const int width = 4 * a.nb + 1 + 2 * a.hb + 3;
    const int cx = 2 * a.nb, cz = 3 * a.nb, cy = 4 * a.nb, cbin = cy + 1, cres = cbin + a.hb, csz = cres + a.hb;
    const double anchor[3] = {(double)a.h, (double)a.w, (double)a.l};
    enum { S_X, S_Z, S_Y, S_CE, S_RES, S_SIZE, S_CORNER, S_BCE, N_FG, N_IOU, N_VALID, N_BG, NS };
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;

    for (int r = t; r < a.rows; r += LOSS_T) {
        const float *g = rcnn_reg + (long)r * width, *b = gt + (long)r * 7, *p = pred + (long)r * 7;
        const float label = cls[r];
        if (label >= 0.f) {
            double dq;
            acc[S_BCE] += bce_row(rcnn_cls[r], (double)label, dq);
            acc[N_VALID] += 1.0;
        }
        if (label == 0.f) acc[N_BG] += 1.0;
        if (!(label > 0.f)) continue;
        acc[N_FG] += 1.0;
        acc[S_X] += smooth_l1((double)g[cx] - (double)b[0] / (double)a.loc_scope);
        acc[S_Z] += smooth_l1((double)g[cz] - (double)b[2] / (double)a.loc_scope);
        const double dy = (double)g[cy] - (double)b[1];
        acc[S_Y] += dy * dy;
        double res_norm;
        const int bin = ry_label((double)b[6], a.hb, res_norm);
        double m = (double)g[cbin];
        for (int k = 1; k < a.hb; ++k) m = fmax(m, (double)g[cbin + k]);
        double z = 0.0;
        for (int k = 0; k < a.hb; ++k) z += exp((double)g[cbin + k] - m);
        acc[S_CE] += log(z) + m - (double)g[cbin + bin];
        acc[S_RES] += smooth_l1((double)g[cres + bin] - res_norm);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[S_SIZE] += smooth_l1((double)g[csz + k] - ((double)b[3 + k] - anchor[k]) / anchor[k]);
        const PairIou iou = paired_iou<LOSS_T>(p, b, s.vx + t, s.vy + t, s.va + t);
        if (iou.iou3d > 0.5f) {
            acc[N_IOU] += 1.0;
            double pb[7], gb[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) { pb[k] = (double)p[k]; gb[k] = (double)b[k]; }
            const double pc = cos(pb[6]), ps = sin(pb[6]), gc = cos(gb[6]), gs = sin(gb[6]);
            const double fc = cos(gb[6] + M_PI), fs = sin(gb[6] + M_PI);
            for (int c = 0; c < 8; ++c) {
                double px, py, pz, qx, qy, qz, fx, fy, fz;
                box_corner(pb, pc, ps, c, px, py, pz);
                box_corner(gb, gc, gs, c, qx, qy, qz);
                box_corner(gb, fc, fs, c, fx, fy, fz);
                const double d0 = sqrt((px - qx) * (px - qx) + (py - qy) * (py - qy) + (pz - qz) * (pz - qz));
                const double d1 = sqrt((px - fx) * (px - fx) + (py - fy) * (py - fy) + (pz - fz) * (pz - fz));
                acc[S_CORNER] += smooth_l1(fmin(d0, d1));
            }
        }
    }
    loss_reduce<NS>(s, acc);

    const double n_fg = at_least_one(acc[N_FG]), n_valid = at_least_one(acc[N_VALID]);
    if (t == 0) {
        const double loss_cls = acc[S_BCE] / n_valid;
        const double loc = ((acc[S_X] / n_fg + acc[S_Z] / n_fg) + acc[S_Y] / n_fg) * 20.0;
        const double angle = acc[S_CE] / n_fg + acc[S_RES] / n_fg;
        const double size = acc[S_SIZE] / (n_fg * 3.0) * 300.0;
        const double corner = acc[S_CORNER] / (at_least_one(acc[N_IOU]) * 8.0) * 10.0;
        const double reg = loc + angle + size;
        vals[0] = (float)loss_cls; vals[1] = (float)loc; vals[2] = (float)angle; vals[3] = (float)size; vals[4] = (float)corner;
        vals[5] = (float)reg; vals[6] = (float)(loss_cls + reg + corner); vals[7] = 0.f;
        counts[0] = (int32_t)acc[N_FG]; counts[1] = (int32_t)acc[N_IOU]; counts[2] = (int32_t)acc[N_VALID]; counts[3] = (int32_t)acc[N_BG];
    }

    for (int r = t; r < a.rows; r += LOSS_T) {
        const float *g = rcnn_reg + (long)r * width, *b = gt + (long)r * 7;
        float *o = grad_reg + (long)r * width;
        const float label = cls[r];
        double dq = 0.0;
        if (label >= 0.f) bce_row(rcnn_cls[r], (double)label, dq);
        grad_cls[r] = label >= 0.f ? (float)(dq / n_valid) : 0.f;
        for (int k = 0; k < width; ++k) o[k] = 0.f;
        if (!(label > 0.f)) continue;
        o[cx] = (float)(20.0 * smooth_l1_grad((double)g[cx] - (double)b[0] / (double)a.loc_scope) / n_fg);
        o[cz] = (float)(20.0 * smooth_l1_grad((double)g[cz] - (double)b[2] / (double)a.loc_scope) / n_fg);
        o[cy] = (float)(20.0 * 2.0 * ((double)g[cy] - (double)b[1]) / n_fg);
        double res_norm;
        const int bin = ry_label((double)b[6], a.hb, res_norm);
        double m = (double)g[cbin];
        for (int k = 1; k < a.hb; ++k) m = fmax(m, (double)g[cbin + k]);
        double z = 0.0;
        for (int k = 0; k < a.hb; ++k) z += exp((double)g[cbin + k] - m);
        for (int k = 0; k < a.hb; ++k) o[cbin + k] = (float)((exp((double)g[cbin + k] - m) / z - (k == bin ? 1.0 : 0.0)) / n_fg);
        o[cres + bin] = (float)(smooth_l1_grad((double)g[cres + bin] - res_norm) / n_fg);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[csz + k] = (float)(300.0 * smooth_l1_grad((double)g[csz + k] - ((double)b[3 + k] - anchor[k]) / anchor[k]) / (n_fg * 3.0));
    }
}

__global__ __launch_bounds__(LOSS_T) void stage2_ioun_loss_kernel(int rows, const float *__restrict__ rcnn_iou, const float *__restrict__ rcnn_ref,
                                                                  const float *__restrict__ pred, const float *__restrict__ refined,
                                                                  const float *__restrict__ gt, const float *__restrict__ cls,
                                                                  float *__restrict__ vals, int32_t *__restrict__ counts,
                                                                  float *__restrict__ grad_iou, float *__restrict__ grad_ref) {
    __shared__ LossLds s;
    const int t = threadIdx.x;
    enum { S_LOC, S_SIZ, S_ANG, S_IOU, N_FG, N_VALID, NS };
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;

    // a row's regression residuals: d[0:3] location, d[3:6] size, d[6] heading (train_functions.py:431-448)
    auto residuals = [&](int r, double *d) {
        const float *f = rcnn_ref + (long)r * 7, *b = gt + (long)r * 7, *p = pred + (long)r * 7;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d[k] = (double)f[k] - ((double)b[k] - (double)p[k]) / (double)p[3 + k];
            d[3 + k] = (double)f[3 + k] - ((double)b[3 + k] - (double)p[3 + k]) / (double)p[3 + k];
        }
        d[6] = (double)f[6] - (py_mod_d((double)b[6], M_PI) - py_mod_d((double)p[6], M_PI));
    };
    // "range MSE" rows.  The reference selects gt.sum(-1) != 0, whose outcome for entries that cancel depends on the library's
    // summation order; here a row counts when ANY entry is non-zero (a NaN entry included) -- the same rows whenever no box cancels
    // to exactly zero, and no order to depend on.  stage2_losses' torch route uses the same rule.
    auto valid_row = [&](int r) {
        const float *b = gt + (long)r * 7;
        bool any = false;
#pragma unroll
        for (int k = 0; k < 7; ++k) any = any || b[k] != 0.f;
        return any;
    };

    for (int r = t; r < rows; r += LOSS_T) {
        if (valid_row(r)) {
            const PairIou iou = paired_iou<LOSS_T>(refined + (long)r * 7, gt + (long)r * 7, s.vx + t, s.vy + t, s.va + t);
            const double e = (double)rcnn_iou[r] - (double)iou.iou3d * (double)iou.iou3d;
            acc[S_IOU] += e * e;
            acc[N_VALID] += 1.0;
            grad_iou[r] = (float)e;             // parked for pass 2 (same thread, same row): the rotated overlap runs once per row
        }
        if (!(cls[r] > 0.f)) continue;
        double d[7];
        residuals(r, d);
        acc[N_FG] += 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[S_LOC] += smooth_l1(d[k]); acc[S_SIZ] += smooth_l1(d[3 + k]); }
        acc[S_ANG] += smooth_l1(d[6]);
    }
    loss_reduce<NS>(s, acc);

    const double n_fg = at_least_one(acc[N_FG]), n_valid = at_least_one(acc[N_VALID]);
    if (t == 0) {
        const double loc = acc[S_LOC] / (n_fg * 3.0) * 300.0, siz = acc[S_SIZ] / (n_fg * 3.0) * 300.0, ang = acc[S_ANG] / n_fg * 20.0;
        const double l_iou = acc[S_IOU] / n_valid * 100.0;
        const double reg = loc + siz + ang;
        vals[0] = (float)loc; vals[1] = (float)siz; vals[2] = (float)ang; vals[3] = (float)l_iou; vals[4] = (float)reg;
        vals[5] = (float)(l_iou + reg); vals[6] = 0.f; vals[7] = 0.f;
        counts[0] = (int32_t)acc[N_FG]; counts[1] = (int32_t)acc[N_VALID]; counts[2] = 0; counts[3] = 0;
    }

    for (int r = t; r < rows; r += LOSS_T) {
        // pass 1 parked e = rcnn_iou - iou3d^2 rounded to fp32 (|e| <= a few units: 2^-24 relative, below the fp32 result's own rounding)
        grad_iou[r] = valid_row(r) ? (float)(100.0 * 2.0 * (double)grad_iou[r] / n_valid) : 0.f;
        float *o = grad_ref + (long)r * 7;
        if (cls[r] > 0.f) {
            double d[7];
            residuals(r, d);
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = (float)(300.0 * smooth_l1_grad(d[k]) / (n_fg * 3.0));
            o[6] = (float)(20.0 * smooth_l1_grad(d[6]) / n_fg);
        } else {
#pragma unroll
            for (int k = 0; k < 7; ++k) o[k] = 0.f;
        }
    }
}

}  // namespace ws3d

using namespace ws3d;

extern "C" int ws3d_stage2_rcnn_loss(int rows, int loc_bins, int head_bins, float loc_scope, float h, float w, float l, const float *rcnn_cls,
                                     const float *rcnn_reg, const float *pred_boxes3d, const float *gt_boxes, const float *cls, float *vals,
                                     int32_t *counts, float *grad_cls, float *grad_reg, ws3d_stream_t stream) {
    if (rows < 0 || loc_bins <= 0 || head_bins <= 0 || !vals || !counts ||
        (rows > 0 && (!rcnn_cls || !rcnn_reg || !pred_boxes3d || !gt_boxes || !cls || !grad_cls || !grad_reg))) {
        set_error("ws3d_stage2_rcnn_loss: invalid argument (rows=%d loc_bins=%d head_bins=%d)", rows, loc_bins, head_bins);
        return WS3D_E_INVALID;
    }
    const RcnnLossArgs a = {rows, loc_bins, head_bins, loc_scope, h, w, l};
    hipLaunchKernelGGL(stage2_rcnn_loss_kernel, dim3(1), dim3(LOSS_T), 0, as_stream(stream), a, rcnn_cls, rcnn_reg, pred_boxes3d, gt_boxes, cls,
                       vals, counts, grad_cls, grad_reg);
    return check_launch("ws3d_stage2_rcnn_loss");
}

extern "C" int ws3d_stage2_ioun_loss(int rows, const float *rcnn_iou, const float *rcnn_ref, const float *pred_boxes3d, const float *refined_box,
                                     const float *gt_boxes, const float *cls, float *vals, int32_t *counts, float *grad_iou, float *grad_ref,
                                     ws3d_stream_t stream) {
    if (rows < 0 || !vals || !counts ||
        (rows > 0 && (!rcnn_iou || !rcnn_ref || !pred_boxes3d || !refined_box || !gt_boxes || !cls || !grad_iou || !grad_ref))) {
        set_error("ws3d_stage2_ioun_loss: invalid argument (rows=%d)", rows);
        return WS3D_E_INVALID;
    }
    hipLaunchKernelGGL(stage2_ioun_loss_kernel, dim3(1), dim3(LOSS_T), 0, as_stream(stream), rows, rcnn_iou, rcnn_ref, pred_boxes3d, refined_box,
                       gt_boxes, cls, vals, counts, grad_iou, grad_ref);
    return check_launch("ws3d_stage2_ioun_loss");
}
