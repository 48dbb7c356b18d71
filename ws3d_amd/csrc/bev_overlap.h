// bev_overlap.h -- the rotated-BEV frame of a box and the overlap area of two frames (iou3d_kernel.cu:34-221): the device code
// shared by iou3d.hip (N x M overlap / IoU, NMS masks, the paired 3-D IoU) and stage2_loss.hip (the IoU inside the fused losses).
// Arithmetic: plain IEEE fp32 in source order (-ffp-contract=off), sin/cos/atan2 = double libm rounded to float.
#pragma once
#include "common.h"

namespace ws3d {

struct P2 { float x, y; };

constexpr float IOU_EPS = 1e-8f;  // iou3d_kernel.cu:13

struct BevFrame {
    float x1, y1, x2, y2;   // raw box (iou3d_kernel.cu:111-112)
    float cx, cy;           // centre (:115-116)
    float cosn, sinn;       // cos(-ry), sin(-ry) used by check_in_box2d (:56)
    float area;             // (x2-x1)*(y2-y1) (:217-218)
    float rad;              // half diagonal, for the far-pair reject only
    P2 c[4];                // rotated corners (:124-150)
};
constexpr int FRAME_F = 18;  // floats per frame

__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) {  // :38-40
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__device__ __forceinline__ BevFrame make_bev_frame(const float *box) {
    BevFrame f;
    f.x1 = box[0]; f.y1 = box[1]; f.x2 = box[2]; f.y2 = box[3];
    const float ang = box[4];
    f.cx = (f.x1 + f.x2) / 2;
    f.cy = (f.y1 + f.y2) / 2;
    const float ac = cosf_cr(ang), as = sinf_cr(ang);
    f.cosn = cosf_cr(-ang);
    f.sinn = sinf_cr(-ang);
    f.area = (f.x2 - f.x1) * (f.y2 - f.y1);
    const float hx = (f.x2 - f.x1) * 0.5f, hy = (f.y2 - f.y1) * 0.5f;
    f.rad = sqrtf(hx * hx + hy * hy);
    const float px[4] = {f.x1, f.x2, f.x2, f.x1};
    const float py[4] = {f.y1, f.y1, f.y2, f.y2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // rotate_around_center :98-102
        f.c[k].x = (px[k] - f.cx) * ac + (py[k] - f.cy) * as + f.cx;
        f.c[k].y = -(px[k] - f.cx) * as + (py[k] - f.cy) * ac + f.cy;
    }
    return f;
}

__device__ __forceinline__ void store_frame(float *dst, const BevFrame &f) {
    dst[0] = f.x1; dst[1] = f.y1; dst[2] = f.x2; dst[3] = f.y2; dst[4] = f.cx; dst[5] = f.cy;
    dst[6] = f.cosn; dst[7] = f.sinn; dst[8] = f.area; dst[9] = f.rad;
#pragma unroll
    for (int k = 0; k < 4; ++k) { dst[10 + 2 * k] = f.c[k].x; dst[11 + 2 * k] = f.c[k].y; }
}
__device__ __forceinline__ BevFrame load_frame(const float *src) {
    BevFrame f;
    f.x1 = src[0]; f.y1 = src[1]; f.x2 = src[2]; f.y2 = src[3]; f.cx = src[4]; f.cy = src[5];
    f.cosn = src[6]; f.sinn = src[7]; f.area = src[8]; f.rad = src[9];
#pragma unroll
    for (int k = 0; k < 4; ++k) { f.c[k].x = src[10 + 2 * k]; f.c[k].y = src[11 + 2 * k]; }
    return f;
}

__device__ __forceinline__ bool check_in_box2d(const BevFrame &b, P2 p) {  // :50-65
    const float MARGIN = 1e-5f;
    const float rot_x = (p.x - b.cx) * b.cosn + (p.y - b.cy) * b.sinn + b.cx;
    const float rot_y = -(p.x - b.cx) * b.sinn + (p.y - b.cy) * b.cosn + b.cy;
    return (rot_x > b.x1 - MARGIN && rot_x < b.x2 + MARGIN && rot_y > b.y1 - MARGIN && rot_y < b.y2 + MARGIN);
}

__device__ __forceinline__ bool intersection(P2 p1, P2 p0, P2 q1, P2 q0, P2 &ans) {  // :67-96
    // check_rect_cross(p0, p1, q0, q1) :42-48
    if (!(fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
          fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y)))
        return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > IOU_EPS) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

// far-pair reject: circumscribed circles separated by more than a safety margin => the
// reference finds no edge crossing and no contained corner (cnt == 0) and returns 0.
__device__ __forceinline__ bool far_apart(float acx, float acy, float arad, float bcx, float bcy, float brad) {
    const float dx = acx - bcx, dy = acy - bcy;
    const float rr = arad + brad + 0.01f + 1e-5f * (fabsf(acx) + fabsf(acy) + fabsf(bcx) + fabsf(bcy));
    return dx * dx + dy * dy > rr * rr * 1.0001f;
}

// NMS only needs the BIT iou > thresh, and most pairs that survive the circle test above are nowhere near the threshold (the
// Stage-1 proposals are thousands of car-sized boxes a few decimetres apart under every heading).  Two upper bounds on the
// intersection area of two rectangles, from the frames alone (no corner, no division):
//   (1) along the line through the centres the projections overlap by at most ext = hA(u) + hB(u) - d, across it the
//       intersection is no wider than the narrower box's extent: I <= ext * min(pA, pB)  (all lengths scaled by d: no sqrt);
//   (2) the intersection lies in one strip of A and one strip of B: I <= wA * wB / |sin of the angle between the strips|.
// The reference's polygon is spanned by points ON the boundary of the true intersection (edge crossings, corners inside the
// other box up to its 1e-5 margin): its area is <= I + ~1e-4.  So `bound < T`, T = thresh * (SA + SB) / (1 + thresh), with
// a 2e-3 relative and 1e-3 absolute margin (rounding here is ~1e-6) proves that the reference computes iou <= thresh: the
// bit is clear, exactly.  Degenerate boxes (a non-positive side) and thresh <= 0 never take the shortcut.
__device__ __forceinline__ bool iou_surely_not_above(const float *a, const float *b, float thresh) {
    const float hxa = (a[2] - a[0]) * 0.5f, hya = (a[3] - a[1]) * 0.5f, hxb = (b[2] - b[0]) * 0.5f, hyb = (b[3] - b[1]) * 0.5f;
    if (!(hxa > 0.f && hya > 0.f && hxb > 0.f && hyb > 0.f && thresh > 0.f)) return false;
    const float T = thresh * (a[8] + b[8]) / (1.0f + thresh);
    const float Tm = T * (1.0f - 2e-3f) - 1e-3f;
    if (!(Tm > 0.f)) return false;
    const float ca = a[6], sa = a[7], cb = b[6], sb = b[7];       // e1 = (c, s): the box's x side, e2 = (-s, c)
    // (2) strips
    const float sn = fabsf(ca * sb - sa * cb), cs = fabsf(ca * cb + sa * sb);
    if (4.f * hya * hyb < Tm * sn || 4.f * hxa * hxb < Tm * sn || 4.f * hya * hxb < Tm * cs || 4.f * hxa * hyb < Tm * cs) return true;
    // (1) slab along the centre line, v = cB - cA (not normalised: every length below carries a factor |v|)
    const float vx = b[4] - a[4], vy = b[5] - a[5];
    const float d2 = vx * vx + vy * vy;
    const float va1 = fabsf(vx * ca + vy * sa), va2 = fabsf(vy * ca - vx * sa);     // |v . e1A|, |v . e2A| (= |v_perp . e1A|)
    const float vb1 = fabsf(vx * cb + vy * sb), vb2 = fabsf(vy * cb - vx * sb);
    const float E = hxa * va1 + hya * va2 + hxb * vb1 + hyb * vb2 - d2;             // |v| * (hA(u) + hB(u) - d)
    const float P = fminf(hxa * va2 + hya * va1, hxb * vb2 + hyb * vb1);            // |v| * half the narrower extent across u
    return 2.f * fmaxf(E, 0.f) * P < Tm * d2;
}

// iou3d_kernel.cu:108-212.  vx/vy/va: this lane's polygon scratch in LDS, element v at
// [v * LS] (LS = lanes sharing the scratch; the caller passes pointers offset by its lane id).
template <int LS>
__device__ float box_overlap(const BevFrame &A, const BevFrame &B, float *vx, float *vy, float *va) {
    if (far_apart(A.cx, A.cy, A.rad, B.cx, B.cy, B.rad)) return 0.0f;
    int cnt = 0;
    float pcx = 0.f, pcy = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            P2 ans;
            if (intersection(A.c[(i + 1) & 3], A.c[i], B.c[(j + 1) & 3], B.c[j], ans)) {
                pcx = pcx + ans.x;
                pcy = pcy + ans.y;
                vx[cnt * LS] = ans.x;
                vy[cnt * LS] = ans.y;
                cnt++;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (check_in_box2d(A, B.c[k])) {
            pcx = pcx + B.c[k].x; pcy = pcy + B.c[k].y;
            vx[cnt * LS] = B.c[k].x; vy[cnt * LS] = B.c[k].y;
            cnt++;
        }
        if (check_in_box2d(B, A.c[k])) {
            pcx = pcx + A.c[k].x; pcy = pcy + A.c[k].y;
            vx[cnt * LS] = A.c[k].x; vy[cnt * LS] = A.c[k].y;
            cnt++;
        }
    }
    if (cnt == 0) return 0.0f;  // (0/0 centroid, empty loops, area 0 in the reference)
    pcx /= cnt;
    pcy /= cnt;
    for (int v = 0; v < cnt; ++v) va[v * LS] = atan2f_cr(vy[v * LS] - pcy, vx[v * LS] - pcx);
    // bubble sort with point_cmp = angle(a) > angle(b) (:104-106,188-196)
    for (int j = 0; j < cnt - 1; ++j) {
        for (int i = 0; i < cnt - j - 1; ++i) {
            const float ta = va[i * LS], tb = va[(i + 1) * LS];
            if (ta > tb) {
                va[i * LS] = tb; va[(i + 1) * LS] = ta;
                const float x0 = vx[i * LS], y0 = vy[i * LS];
                vx[i * LS] = vx[(i + 1) * LS]; vy[i * LS] = vy[(i + 1) * LS];
                vx[(i + 1) * LS] = x0; vy[(i + 1) * LS] = y0;
            }
        }
    }
    float area = 0.f;
    const float x0 = vx[0], y0 = vy[0];
    for (int k = 0; k < cnt - 1; ++k) {
        const float ax = vx[k * LS] - x0, ay = vy[k * LS] - y0;
        const float bx = vx[(k + 1) * LS] - x0, by = vy[(k + 1) * LS] - y0;
        area += ax * by - ay * bx;  // cross(a, b) :34-36
    }
    return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_from_overlap(const BevFrame &A, const BevFrame &B, float s_overlap) {
    return s_overlap / fmaxf(A.area + B.area - s_overlap, IOU_EPS);  // :214-221
}

// torch.min / torch.max / torch.clamp(min=) on fp32: a NaN operand comes out as NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float t_min(float a, float b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ float t_max(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ float t_clamp_min(float x, float lo) { return x < lo ? lo : x; }

struct PairIou { float overlap, iou2d, iou3d; };

// One pair of (7,) boxes [x, y_bottom, z, h, w, l, ry]: boxes3d_to_bev_torch (kitti_utils.py:134-147), box_overlap, then the height
// overlap and the two divisions of boxes_iou3d_gpu (iou3d_utils.py:21-56) in torch's fp32 operation order, clamp(min=1e-7) included --
// bit for bit the (i, i) entry of the N x N route.  vx / vy / va: this lane's polygon scratch, as box_overlap takes it.
template <int LS>
__device__ PairIou paired_iou(const float *a, const float *b, float *vx, float *vy, float *va) {
    const float a_hl = a[5] / 2, a_hw = a[4] / 2, b_hl = b[5] / 2, b_hw = b[4] / 2;
    const float bev_a[5] = {a[0] - a_hl, a[2] - a_hw, a[0] + a_hl, a[2] + a_hw, a[6]};
    const float bev_b[5] = {b[0] - b_hl, b[2] - b_hw, b[0] + b_hl, b[2] + b_hw, b[6]};
    PairIou r;
    r.overlap = box_overlap<LS>(make_bev_frame(bev_a), make_bev_frame(bev_b), vx, vy, va);
    const float a_min = a[1] - a[3], b_min = b[1] - b[3];
    const float oh = t_clamp_min(t_min(a[1], b[1]) - t_max(a_min, b_min), 0.f);
    const float s_a = a[4] * a[5], s_b = b[4] * b[5];
    r.iou2d = r.overlap / t_clamp_min(s_a + s_b - r.overlap, 1e-7f);
    const float o3 = r.overlap * oh;
    const float vol_a = a[3] * a[4] * a[5], vol_b = b[3] * b[4] * b[5];
    r.iou3d = o3 / t_clamp_min(vol_a + vol_b - o3, 1e-7f);
    return r;
}

}  // namespace ws3d
