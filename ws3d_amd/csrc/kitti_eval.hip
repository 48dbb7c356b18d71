// kitti_eval.hip -- the two hot loops of the KITTI object evaluator for gfx950.  Replaces the reference's
// tools/kitti_object_eval_python: the numba.cuda rotated-box overlap (rotate_iou.py:16-329), the numba CPU
// image / 3-D overlaps (eval.py:84-145) and the per-(frame, threshold) matching (compute_statistics_jit /
// fused_compute_statistics, eval.py:155-333).
//
// Overlaps: the reference computes a full cross-frame matrix per group of ~75 frames (calculate_iou_partly,
// eval.py:335-410) and keeps only the diagonal per-frame blocks.  Here one launch computes exactly those
// blocks for every frame: workgroup (frame, slice), thread = one (detection, ground truth) pair, output
// block (n_dt x n_gt) row-major at out_off[frame].  The rotated intersection keeps the reference's
// expression order in fp32 (library built with -ffp-contract=off; sin / cos = double libm rounded to float,
// DESIGN.md section 4); its <= 16-point polygon and the insertion sort live in LDS in [vertex][thread]
// order, so nothing is a dynamically indexed private array (no scratch).  Pairs whose centres are farther
// apart than the sum of their half-diagonals (with a margin) have no intersection point in the reference
// either: their area is set to 0 without the 16 edge tests.
//
// Matching: one wave per (frame, threshold) task.  Lanes own detections j = lane + 64 c, the "assigned"
// flags are one bit per chunk in a lane register (<= 64 chunks: <= 4096 detections per frame), the gt loop
// is sequential as in the reference, and the per-gt choice is a wave argmax of (key, -index):
//   collection  (compute_fp=False): key = score             -> highest score, first index on ties
//   counting    (compute_fp=True):  key = overlap (ignored_det == 0) or -1 (ignored_det == 1)
//                                   -> highest overlap among ignored_det == 0, first on ties; else the
//                                      first ignored_det == 1 candidate
// which is what the reference's sequential if / elif chain selects.  Per-task (tp, fp, fn, similarity) go
// to a workspace and a second kernel sums them per threshold in frame order: exact counts, a similarity
// that is the same from run to run, no float atomics.
#include <math.h>

#include "common.h"

namespace ws3d {

constexpr int KE_OV_THREADS = 128;   // overlap kernel: threads per workgroup (LDS polygon: 24 KiB)
constexpr int KE_MAX_PTS = 16;       // intersection points kept per pair (the reference's array holds 8)
constexpr int KE_MATCH_WAVES = 4;    // matching kernel: waves (tasks) per workgroup
constexpr int KE_MAX_CHUNKS = 64;    // 64 chunks of 64 detections = one uint64 of assigned flags per lane

struct Quad { float x[4], y[4]; };

// rbbox_to_corners (rotate_iou.py:233-256): box (cx, cy, dx, dy, angle)
__device__ __forceinline__ Quad rbox_corners(float cx, float cy, float xd, float yd, float angle) {
    const float a_cos = cosf_cr(angle), a_sin = sinf_cr(angle);
    const float hx = -xd / 2, hy = -yd / 2, gx = xd / 2, gy = yd / 2;
    const float px[4] = {hx, hx, gx, gx};
    const float py[4] = {hy, gy, gy, hy};
    Quad q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        q.x[i] = a_cos * px[i] + a_sin * py[i] + cx;
        q.y[i] = -a_sin * px[i] + a_cos * py[i] + cy;
    }
    return q;
}

// point_in_quadrilateral (rotate_iou.py:177-192)
__device__ __forceinline__ bool point_in_quad(float pt_x, float pt_y, const Quad &c) {
    const float ab0 = c.x[1] - c.x[0], ab1 = c.y[1] - c.y[0];
    const float ad0 = c.x[3] - c.x[0], ad1 = c.y[3] - c.y[0];
    const float ap0 = pt_x - c.x[0], ap1 = pt_y - c.y[0];
    const float abab = ab0 * ab0 + ab1 * ab1;
    const float abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1;
    const float adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}

// line_segment_intersection (rotate_iou.py:75-120): edge i of p1 against edge j of p2
__device__ __forceinline__ bool segment_cross(const Quad &p1, const Quad &p2, int i, int j, float &ox, float &oy) {
    const int i1 = (i + 1) & 3, j1 = (j + 1) & 3;
    const float Ax = p1.x[i], Ay = p1.y[i], Bx = p1.x[i1], By = p1.y[i1];
    const float Cx = p2.x[j], Cy = p2.y[j], Dx_ = p2.x[j1], Dy_ = p2.y[j1];
    const float BA0 = Bx - Ax, BA1 = By - Ay;
    const float DA0 = Dx_ - Ax, CA0 = Cx - Ax;
    const float DA1 = Dy_ - Ay, CA1 = Cy - Ay;
    const bool acd = DA1 * CA0 > CA1 * DA0;
    const bool bcd = (Dy_ - By) * (Cx - Bx) > (Cy - By) * (Dx_ - Bx);
    if (acd == bcd) return false;
    const bool abc = CA1 * BA0 > BA1 * CA0;
    const bool abd = DA1 * BA0 > BA1 * DA0;
    if (abc == abd) return false;
    const float DC0 = Dx_ - Cx, DC1 = Dy_ - Cy;
    const float ABBA = Ax * By - Bx * Ay;
    const float CDDC = Cx * Dy_ - Dx_ * Cy;
    const float DH = BA1 * DC0 - BA0 * DC1;
    const float Dx = ABBA * DC0 - BA0 * CDDC;
    const float Dy = ABBA * DC1 - BA1 * CDDC;
    ox = Dx / DH;
    oy = Dy / DH;
    return true;
}

// inter (rotate_iou.py:259-274) = quadrilateral_intersection + sort_vertex_in_convex_polygon + area.
// px / py / pk: this thread's column of the LDS polygon ([vertex * KE_OV_THREADS + thread]).
__device__ float rbox_inter(const float *b1, const float *b2, float *px, float *py, float *pk) {
    const Quad c1 = rbox_corners(b1[0], b1[1], b1[2], b1[3], b1[4]);
    const Quad c2 = rbox_corners(b2[0], b2[1], b2[2], b2[3], b2[4]);
    int n = 0;
    auto push = [&](float x, float y) {
        if (n < KE_MAX_PTS) {
            px[n * KE_OV_THREADS] = x;
            py[n * KE_OV_THREADS] = y;
            ++n;
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // quadrilateral_intersection (:195-214)
        if (point_in_quad(c1.x[i], c1.y[i], c2)) push(c1.x[i], c1.y[i]);
        if (point_in_quad(c2.x[i], c2.y[i], c1)) push(c2.x[i], c2.y[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float ox, oy;
            if (segment_cross(c1, c2, i, j, ox, oy)) push(ox, oy);
        }
    }
    if (n <= 0) return 0.0f;
    // sort_vertex_in_convex_polygon (:34-72)
    float cx = 0.0f, cy = 0.0f;
    for (int i = 0; i < n; ++i) {
        cx += px[i * KE_OV_THREADS];
        cy += py[i * KE_OV_THREADS];
    }
    cx /= (float)n;
    cy /= (float)n;
    for (int i = 0; i < n; ++i) {
        float v0 = px[i * KE_OV_THREADS] - cx, v1 = py[i * KE_OV_THREADS] - cy;
        const float d = sqrtf(v0 * v0 + v1 * v1);
        v0 = v0 / d;
        v1 = v1 / d;
        if (v1 < 0) v0 = -2 - v0;
        pk[i * KE_OV_THREADS] = v0;
    }
    for (int i = 1; i < n; ++i) {
        if (pk[(i - 1) * KE_OV_THREADS] > pk[i * KE_OV_THREADS]) {
            const float temp = pk[i * KE_OV_THREADS], tx = px[i * KE_OV_THREADS], ty = py[i * KE_OV_THREADS];
            int j = i;
            while (j > 0 && pk[(j - 1) * KE_OV_THREADS] > temp) {
                pk[j * KE_OV_THREADS] = pk[(j - 1) * KE_OV_THREADS];
                px[j * KE_OV_THREADS] = px[(j - 1) * KE_OV_THREADS];
                py[j * KE_OV_THREADS] = py[(j - 1) * KE_OV_THREADS];
                --j;
            }
            pk[j * KE_OV_THREADS] = temp;
            px[j * KE_OV_THREADS] = tx;
            py[j * KE_OV_THREADS] = ty;
        }
    }
    // area (:23-30): fan of triangles around vertex 0, trangle_area = cross / 2
    const float ax = px[0], ay = py[0];
    float area_val = 0.0f;
    for (int i = 0; i + 2 < n; ++i) {
        const float bx = px[(i + 1) * KE_OV_THREADS], by = py[(i + 1) * KE_OV_THREADS];
        const float qx = px[(i + 2) * KE_OV_THREADS], qy = py[(i + 2) * KE_OV_THREADS];
        area_val += fabsf(((ax - qx) * (by - qy) - (ay - qy) * (bx - qx)) / 2.0f);
    }
    return area_val;
}

// the intersection area of query box q and box b (inter(rbox1=q, rbox2=b), rotate_iou.py:282), 0 without
// the edge tests when the circumscribed circles are clearly apart
__device__ __forceinline__ float rbox_area(const float *q, const float *b, float *px, float *py, float *pk) {
    const float dx = q[0] - b[0], dy = q[1] - b[1];
    const float rq = 0.5f * sqrtf(q[2] * q[2] + q[3] * q[3]), rb = 0.5f * sqrtf(b[2] * b[2] + b[3] * b[3]);
    const float reach = (rq + rb) * 1.001f + 1e-3f;
    if (dx * dx + dy * dy > reach * reach) return 0.0f;
    return rbox_inter(q, b, px, py, pk);
}

// devRotateIoUEval (rotate_iou.py:277-288), rbox1 = the query box
__device__ __forceinline__ float rbox_iou(const float *q, const float *b, int criterion, float *px, float *py, float *pk) {
    const float area1 = q[2] * q[3];
    const float area2 = b[2] * b[3];
    const float area_inter = rbox_area(q, b, px, py, pk);
    if (criterion == -1) return area_inter / (area1 + area2 - area_inter);
    if (criterion == 0) return area_inter / area1;
    if (criterion == 1) return area_inter / area2;
    return area_inter;
}

__device__ __forceinline__ double pymin(double a, double b) { return b < a ? b : a; }   // Python's min(a, b)
__device__ __forceinline__ double pymax(double a, double b) { return b > a ? b : a; }   // Python's max(a, b)

// image_box_overlap (eval.py:84-111) for one (box n, query k) pair, in double and in source order
__device__ __forceinline__ double image_overlap(const double *b, const double *q, int criterion) {
    const double qbox_area = (q[2] - q[0]) * (q[3] - q[1]);
    const double iw = pymin(b[2], q[2]) - pymax(b[0], q[0]);
    if (!(iw > 0)) return 0.0;
    const double ih = pymin(b[3], q[3]) - pymax(b[1], q[1]);
    if (!(ih > 0)) return 0.0;
    double ua;
    if (criterion == -1) ua = (b[2] - b[0]) * (b[3] - b[1]) + qbox_area - iw * ih;
    else if (criterion == 0) ua = (b[2] - b[0]) * (b[3] - b[1]);
    else if (criterion == 1) ua = qbox_area;
    else ua = 1.0;
    return iw * ih / ua;
}

// Per-frame blocks: out[out_off[f] + j * n_gt + i] = overlap(detection j, ground truth i) of frame f.
// METRIC 0: dt / gt boxes (n, 4) image boxes; 1: (n, 5) BEV (x, z, l, w, ry); 2: (n, 7) (x, y, z, l, h, w, ry).
template <int METRIC>
__global__ void __launch_bounds__(KE_OV_THREADS) kitti_overlap_kernel(int frames, int criterion, const int32_t *__restrict__ gt_off,
                                                                     const int32_t *__restrict__ dt_off, const int64_t *__restrict__ out_off,
                                                                     const double *__restrict__ dt_boxes, const double *__restrict__ gt_boxes,
                                                                     double *__restrict__ out) {
    constexpr int W = METRIC == 0 ? 4 : (METRIC == 1 ? 5 : 7);
    __shared__ float poly[METRIC == 0 ? 1 : 3 * KE_MAX_PTS * KE_OV_THREADS];
    float *px = poly + threadIdx.x, *py = px + KE_MAX_PTS * KE_OV_THREADS, *pk = py + KE_MAX_PTS * KE_OV_THREADS;
    {
        const int f = blockIdx.x;
        const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
        const int d0 = dt_off[f], nd = dt_off[f + 1] - d0;
        const long pairs = (long)ng * nd;
        double *o = out + out_off[f];
        for (long p = (long)blockIdx.y * KE_OV_THREADS + threadIdx.x; p < pairs; p += (long)gridDim.y * KE_OV_THREADS) {
            const int j = (int)(p / ng), i = (int)(p - (long)j * ng);
            const double *db = dt_boxes + (long)(d0 + j) * W;
            const double *gb = gt_boxes + (long)(g0 + i) * W;
            if constexpr (METRIC == 0) {
                o[p] = image_overlap(db, gb, criterion);   // boxes = detections, query = ground truths (eval.py:468, :356)
            } else if constexpr (METRIC == 1) {
                const float q[5] = {(float)gb[0], (float)gb[1], (float)gb[2], (float)gb[3], (float)gb[4]};
                const float b[5] = {(float)db[0], (float)db[1], (float)db[2], (float)db[3], (float)db[4]};
                o[p] = (double)rbox_iou(q, b, criterion, px, py, pk);
            } else {
                // d3_box_overlap (eval.py:148-152): BEV columns [0, 2, 3, 5, 6], criterion 2, then the height part (:119-145)
                const float q[5] = {(float)gb[0], (float)gb[2], (float)gb[3], (float)gb[5], (float)gb[6]};
                const float b[5] = {(float)db[0], (float)db[2], (float)db[3], (float)db[5], (float)db[6]};
                float rinc = rbox_area(q, b, px, py, pk);
                if (rinc > 0) {
                    const double iw = pymin(db[1], gb[1]) - pymax(db[1] - db[4], gb[1] - gb[4]);
                    if (iw > 0) {
                        const double area1 = db[3] * db[4] * db[5];
                        const double area2 = gb[3] * gb[4] * gb[5];
                        const double inc = iw * (double)rinc;
                        double ua;
                        if (criterion == -1) ua = area1 + area2 - inc;
                        else if (criterion == 0) ua = area1;
                        else if (criterion == 1) ua = area2;
                        else ua = inc;
                        rinc = (float)(inc / ua);
                    } else {
                        rinc = 0.0f;
                    }
                }
                o[p] = (double)rinc;
            }
        }
    }
}

__device__ __forceinline__ void wave_argmax(double &key, int &idx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ok = __shfl_xor(key, off, WS3D_WAVE);
        const int oi = __shfl_xor(idx, off, WS3D_WAVE);
        if (ok > key || (ok == key && oi < idx)) {
            key = ok;
            idx = oi;
        }
    }
}

__device__ __forceinline__ int wave_count(bool pred) { return __popcll(__ballot(pred)); }

constexpr int KE_NONE = 0x7fffffff;
constexpr double KE_NO_DETECTION = -10000000.0;   // NO_DETECTION (eval.py:180)

// compute_statistics_jit (eval.py:155-273), one wave per task.  COUNT = false: collection (thresh 0, compute_fp False),
// task = frame, writes tp_flag / tp_score per ground truth.  COUNT = true: task = frame * num_thresh + t, writes
// (tp, fp, fn) to cnt[(t * frames + frame) * 3 + .] and the similarity to sim[t * frames + frame].
template <bool COUNT>
__global__ void __launch_bounds__(KE_MATCH_WAVES *WS3D_WAVE) kitti_match_kernel(
    int metric, int frames, int num_thresh, const double *__restrict__ thresholds, const int32_t *__restrict__ gt_off,
    const int32_t *__restrict__ dt_off, const int32_t *__restrict__ dc_off, const int64_t *__restrict__ out_off,
    const double *__restrict__ overlaps, const int32_t *__restrict__ ignored_gt, const int32_t *__restrict__ ignored_dt,
    const double *__restrict__ dt_score, const double *__restrict__ dt_alpha, const double *__restrict__ gt_alpha,
    const double *__restrict__ dt_bbox, const double *__restrict__ dc_bbox, double min_overlap, int compute_aos,
    double *__restrict__ tp_score, int32_t *__restrict__ tp_flag, int32_t *__restrict__ cnt, double *__restrict__ sim) {
    const int lane = lane_id();
    const long tasks = COUNT ? (long)frames * num_thresh : (long)frames;
    const long wave0 = (long)blockIdx.x * KE_MATCH_WAVES + (threadIdx.x >> 6);
    for (long task = wave0; task < tasks; task += (long)gridDim.x * KE_MATCH_WAVES) {
        const int f = COUNT ? (int)(task / num_thresh) : (int)task;
        const int t = COUNT ? (int)(task - (long)f * num_thresh) : 0;
        const double thresh = COUNT ? thresholds[t] : 0.0;
        const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
        const int d0 = dt_off[f], nd = dt_off[f + 1] - d0;
        const int chunks = min((nd + WS3D_WAVE - 1) / WS3D_WAVE, KE_MAX_CHUNKS);
        const double *ov = overlaps + out_off[f];
        uint64_t assigned = 0;
        int tp = 0, fn = 0;
        double similarity = 0.0;
        for (int i = 0; i < ng; ++i) {
            const int ig = ignored_gt[g0 + i];
            if (ig == -1) {
                if (!COUNT && lane == 0) tp_flag[g0 + i] = 0;
                continue;
            }
            double key = -INFINITY;
            int idx = KE_NONE;
            for (int c = 0; c < chunks; ++c) {
                const int j = c * WS3D_WAVE + lane;
                if (j >= nd) break;
                const int idt = ignored_dt[d0 + j];
                const double s = dt_score[d0 + j];
                if (idt == -1 || ((assigned >> c) & 1) || (COUNT && s < thresh)) continue;
                const double o = ov[(long)j * ng + i];
                if (!(o > min_overlap)) continue;
                double k;
                if (COUNT) {
                    k = idt == 0 ? o : -1.0;
                } else {
                    if (!(s > KE_NO_DETECTION)) continue;
                    k = s;
                }
                if (k > key) {   // chunks in increasing index order: strict > keeps the first on ties
                    key = k;
                    idx = j;
                }
            }
            wave_argmax(key, idx);
            bool tp_here = false;
            if (idx == KE_NONE) {
                if (ig == 0) ++fn;
            } else {
                const int idt = ignored_dt[d0 + idx];
                if (!(ig == 1 || idt == 1)) {
                    ++tp;
                    tp_here = true;
                    if (COUNT && compute_aos) similarity += (1.0 + cos(gt_alpha[g0 + i] - dt_alpha[d0 + idx])) / 2.0;
                }
                if ((idx & (WS3D_WAVE - 1)) == lane) assigned |= 1ull << (idx / WS3D_WAVE);
            }
            if (!COUNT && lane == 0) {
                tp_flag[g0 + i] = tp_here ? 1 : 0;
                tp_score[g0 + i] = tp_here ? dt_score[d0 + idx] : 0.0;
            }
        }
        if (!COUNT) continue;
        int fp = 0;
        for (int c = 0; c < chunks; ++c) {
            const int j = c * WS3D_WAVE + lane;
            bool counted = false;
            if (j < nd) {
                const int idt = ignored_dt[d0 + j];
                counted = !(((assigned >> c) & 1) || idt == -1 || idt == 1 || dt_score[d0 + j] < thresh);
            }
            fp += wave_count(counted);
        }
        if (metric == 0) {   // detections on DontCare regions are not false positives (eval.py:248-260)
            const int k0 = dc_off[f], nk = dc_off[f + 1] - k0;
            int nstuff = 0;
            for (int k = 0; k < nk; ++k) {
                const double *q = dc_bbox + (long)(k0 + k) * 4;
                for (int c = 0; c < chunks; ++c) {
                    const int j = c * WS3D_WAVE + lane;
                    bool hit = false;
                    if (j < nd && !((assigned >> c) & 1) && ignored_dt[d0 + j] == 0 && !(dt_score[d0 + j] < thresh))
                        hit = image_overlap(dt_bbox + (long)(d0 + j) * 4, q, 0) > min_overlap;
                    if (hit) assigned |= 1ull << c;
                    nstuff += wave_count(hit);
                }
            }
            fp -= nstuff;
        }
        if (lane == 0) {
            int32_t *cp = cnt + ((long)t * frames + f) * 3;
            cp[0] = tp;
            cp[1] = fp;
            cp[2] = fn;
            // similarity is -1 (not added, eval.py:326) only when tp == fp == 0, and then the sum is 0
            sim[(long)t * frames + f] = compute_aos ? similarity : 0.0;
        }
    }
}

// pr[t] = sum over frames, in frame order, of the per-task (tp, fp, fn, similarity): fused_compute_statistics's
// pr[t, :] += ... (eval.py:326-330) without atomics.  One workgroup per threshold.
__global__ void __launch_bounds__(256) kitti_pr_reduce_kernel(int frames, const int32_t *__restrict__ cnt, const double *__restrict__ sim,
                                                              double *__restrict__ pr) {
    __shared__ int32_t sc[256 * 3];
    __shared__ double ss[256];
    const int t = blockIdx.x;
    long tp = 0, fp = 0, fn = 0;
    double s = 0.0;
    for (int base = 0; base < frames; base += 256) {
        const int m = min(256, frames - base);
        if ((int)threadIdx.x < m) {
            const int32_t *cp = cnt + ((long)t * frames + base + threadIdx.x) * 3;
            sc[threadIdx.x * 3 + 0] = cp[0];
            sc[threadIdx.x * 3 + 1] = cp[1];
            sc[threadIdx.x * 3 + 2] = cp[2];
            ss[threadIdx.x] = sim[(long)t * frames + base + threadIdx.x];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < m; ++k) {
                tp += sc[k * 3 + 0];
                fp += sc[k * 3 + 1];
                fn += sc[k * 3 + 2];
                s += ss[k];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pr[t * 4 + 0] = (double)tp;
        pr[t * 4 + 1] = (double)fp;
        pr[t * 4 + 2] = (double)fn;
        pr[t * 4 + 3] = s;
    }
}

static size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace ws3d

extern "C" int ws3d_kitti_overlaps(int metric, int criterion, int frames, long max_pairs, const int32_t *gt_off, const int32_t *dt_off,
                                   const int64_t *out_off, const double *dt_boxes, const double *gt_boxes, double *out,
                                   ws3d_stream_t stream) {
    using namespace ws3d;
    if (metric < 0 || metric > 2 || criterion < -1 || criterion > 2 || frames < 0 || max_pairs < 0 ||
        (frames > 0 && (!gt_off || !dt_off || !out_off)) || (max_pairs > 0 && (!dt_boxes || !gt_boxes || !out))) {
        set_error("ws3d_kitti_overlaps: invalid argument (metric=%d criterion=%d frames=%d max_pairs=%ld)", metric, criterion, frames,
                  max_pairs);
        return WS3D_E_INVALID;
    }
    if (frames > (1 << 24)) {   // one workgroup column per frame
        set_error("ws3d_kitti_overlaps: %d frames (at most %d)", frames, 1 << 24);
        return WS3D_E_UNSUPPORTED;
    }
    if (frames == 0 || max_pairs == 0) return WS3D_OK;
    const dim3 grid((unsigned)frames,(unsigned)std::min<long>((max_pairs + KE_OV_THREADS - 1) / KE_OV_THREADS, 1024));
    const hipStream_t s = as_stream(stream);
    if (metric == 0)
        hipLaunchKernelGGL(kitti_overlap_kernel<0>, grid, dim3(KE_OV_THREADS), 0, s, frames, criterion, gt_off, dt_off, out_off, dt_boxes,
                           gt_boxes, out);
    else if (metric == 1)
        hipLaunchKernelGGL(kitti_overlap_kernel<1>, grid, dim3(KE_OV_THREADS), 0, s, frames, criterion, gt_off, dt_off, out_off, dt_boxes,
                           gt_boxes, out);
    else
        hipLaunchKernelGGL(kitti_overlap_kernel<2>, grid, dim3(KE_OV_THREADS), 0, s, frames, criterion, gt_off, dt_off, out_off, dt_boxes,
                           gt_boxes, out);
    return check_launch("ws3d_kitti_overlaps");
}

static unsigned match_grid(long tasks) {
    return (unsigned)std::min<long>((tasks + ws3d::KE_MATCH_WAVES - 1) / ws3d::KE_MATCH_WAVES, 1L << 20);
}

extern "C" int ws3d_kitti_collect_scores(int frames, int max_dt, const int32_t *gt_off, const int32_t *dt_off, const int64_t *out_off,
                                         const double *overlaps, const int32_t *ignored_gt, const int32_t *ignored_dt,
                                         const double *dt_score, double min_overlap, double *tp_score, int32_t *tp_flag,
                                         ws3d_stream_t stream) {
    using namespace ws3d;
    if (frames < 0 || max_dt < 0 || (frames > 0 && (!gt_off || !dt_off || !out_off || !overlaps || !ignored_gt || !ignored_dt ||
                                                     !dt_score || !tp_score || !tp_flag))) {
        set_error("ws3d_kitti_collect_scores: invalid argument (frames=%d max_dt=%d)", frames, max_dt);
        return WS3D_E_INVALID;
    }
    if (max_dt > KE_MAX_CHUNKS * WS3D_WAVE) {
        set_error("ws3d_kitti_collect_scores: %d detections in a frame (at most %d)", max_dt, KE_MAX_CHUNKS * WS3D_WAVE);
        return WS3D_E_UNSUPPORTED;
    }
    if (frames == 0) return WS3D_OK;
    hipLaunchKernelGGL(kitti_match_kernel<false>, dim3(match_grid(frames)), dim3(KE_MATCH_WAVES * WS3D_WAVE), 0, as_stream(stream), 0,
                       frames, 1, (const double *)nullptr, gt_off, dt_off, (const int32_t *)nullptr, out_off, overlaps, ignored_gt,
                       ignored_dt, dt_score, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr,
                       (const double *)nullptr, min_overlap, 0, tp_score, tp_flag, (int32_t *)nullptr, (double *)nullptr);
    return check_launch("ws3d_kitti_collect_scores");
}

extern "C" size_t ws3d_kitti_count_workspace_bytes(int frames, int num_thresh) {
    if (frames <= 0 || num_thresh <= 0) return 0;
    const size_t tasks = (size_t)frames * (size_t)num_thresh;
    return ws3d::align16(tasks * 3 * sizeof(int32_t)) + tasks * sizeof(double);
}

extern "C" int ws3d_kitti_count(int metric, int frames, int max_dt, int num_thresh, const double *thresholds, const int32_t *gt_off,
                                const int32_t *dt_off, const int32_t *dc_off, const int64_t *out_off, const double *overlaps,
                                const int32_t *ignored_gt, const int32_t *ignored_dt, const double *dt_score, const double *dt_alpha,
                                const double *gt_alpha, const double *dt_bbox, const double *dc_bbox, double min_overlap, int compute_aos,
                                void *workspace, size_t workspace_bytes, double *pr, ws3d_stream_t stream) {
    using namespace ws3d;
    const bool work = frames > 0 && num_thresh > 0;
    if (metric < 0 || metric > 2 || frames < 0 || max_dt < 0 || num_thresh < 0 || (num_thresh > 0 && (!thresholds || !pr)) ||
        (work && (!gt_off || !dt_off || !out_off || !overlaps || !ignored_gt || !ignored_dt || !dt_score)) ||
        (work && compute_aos && (!dt_alpha || !gt_alpha)) || (work && metric == 0 && (!dc_off || !dt_bbox || !dc_bbox))) {
        set_error("ws3d_kitti_count: invalid argument (metric=%d frames=%d max_dt=%d num_thresh=%d)", metric, frames, max_dt, num_thresh);
        return WS3D_E_INVALID;
    }
    if (max_dt > KE_MAX_CHUNKS * WS3D_WAVE) {
        set_error("ws3d_kitti_count: %d detections in a frame (at most %d)", max_dt, KE_MAX_CHUNKS * WS3D_WAVE);
        return WS3D_E_UNSUPPORTED;
    }
    if (num_thresh == 0) return WS3D_OK;
    const hipStream_t s = as_stream(stream);
    if (frames == 0) {
        if (hipMemsetAsync(pr, 0, (size_t)num_thresh * 4 * sizeof(double), s) != hipSuccess) {
            set_error("ws3d_kitti_count: hipMemsetAsync failed");
            return WS3D_E_LAUNCH;
        }
        return WS3D_OK;
    }
    const size_t need = ws3d_kitti_count_workspace_bytes(frames, num_thresh);
    if (!workspace || workspace_bytes < need) {
        set_error("ws3d_kitti_count: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return WS3D_E_WORKSPACE;
    }
    const long tasks = (long)frames * num_thresh;
    int32_t *cnt = static_cast<int32_t *>(workspace);
    double *sim = reinterpret_cast<double *>(static_cast<char *>(workspace) + align16((size_t)tasks * 3 * sizeof(int32_t)));
    hipLaunchKernelGGL(kitti_match_kernel<true>, dim3(match_grid(tasks)), dim3(KE_MATCH_WAVES * WS3D_WAVE), 0, s, metric, frames,
                       num_thresh, thresholds, gt_off, dt_off, dc_off, out_off, overlaps, ignored_gt, ignored_dt, dt_score, dt_alpha,
                       gt_alpha, dt_bbox, dc_bbox, min_overlap, compute_aos, (double *)nullptr, (int32_t *)nullptr, cnt, sim);
    int rc = check_launch("ws3d_kitti_count");
    if (rc != WS3D_OK) return rc;
    hipLaunchKernelGGL(kitti_pr_reduce_kernel, dim3(num_thresh), dim3(256), 0, s, frames, cnt, sim, pr);
    return check_launch("ws3d_kitti_count");
}
