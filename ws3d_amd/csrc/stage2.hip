// stage2.hip -- the per-cloud work of the Stage-2 box network that has no library counterpart (include/ws3d_ops.h):
//   ws3d_stage2_embed   the front of a tower: [canonical transform ->] xyz_up (3 -> 128 -> 128), feature_up (2 -> 128 -> 128),
//                       merge_down (256 -> 128) of a 64-point tile in one kernel (lib/net/rcnn_net.py:253-267, 337-365)
//   ws3d_stage2_boxes   rcnn_reg -> the decoded box and its centre form (rcnn_net.py:293-308)
//   ws3d_stage2_select  the element-wise part of the detection tail (rcnn_net.py:387-390, tools/eval_auto.py:397-436)
// (the training losses ws3d_stage2_rcnn_loss / ws3d_stage2_ioun_loss are in stage2_loss.hip)
#include <math.h>

#include "common.h"
#include "mfma_tile.h"

namespace ws3d {

// ------------------------------------------------------------------------------------------------ embed
// One workgroup of 256 threads = 4 waves per tile of 64 points; tiles may straddle clouds, the tail tile is masked at the store.
//   1. 64 threads read their point, turn it into the box's frame (with a box) and write xyz_out;
//   2. the K = 3 first layer of the xyz branch on the VALU -> a0[128][GP_XS];
//   3. lds_layer: a0 . Wx1 (128 x 128, fp32 matrix cores, W streamed through wbuf) -> cat[0:128];
//   4. the K = 2 first layer of the feature branch on the VALU -> a0;      5. lds_layer: a0 . Wf1 -> cat[128:256];
//   6. lds_layer: cat . Wm (256 x 128) -> feat rows: ONE K loop over both halves, i.e. the sum of the two products
//      u_xyz . Wm[0:128] + u_feat . Wm[128:256] in one accumulator -- the concatenation exists only as two adjacent LDS tiles.
// Every layer: bias, then ReLU.  fp32 matrix instructions (v_mfma_f32_32x32x2_f32), k ascending: the parity bound of the fixture
// (4 x the error of the reference's own fp32 run, ~1e-6 absolute) leaves no room for a split-bf16 product here.
// LDS: a0 33,280 + cat 66,560 + wbuf 16,384 + 1,280 = 117,504 bytes -> ONE workgroup (one wave per SIMD) on a CU; the registers
// would allow more (the compile remark's occupancy, which does not see dynamic LDS, is >= 2 waves per SIMD).
constexpr int EMB_C = 128;
constexpr int EMB_A0 = EMB_C * GP_XS, EMB_CAT = 2 * EMB_C * GP_XS, EMB_WBUF = 2 * GP_KT * 128;
constexpr size_t EMB_LDS = (size_t)(EMB_A0 + EMB_CAT + EMB_WBUF) * sizeof(float);

// Python's float modulo for a positive divisor (torch.remainder)
__device__ __forceinline__ float py_mod(float a, float b) {
    float r = fmodf(a, b);
    if (r != 0.f && ((r < 0.f) != (b < 0.f))) r += b;
    return r;
}

__global__ __launch_bounds__(256) void stage2_embed_kernel(long rows, int pts_per_cloud, const float *__restrict__ pts,
                                                           const float *__restrict__ box_ce, float extend,
                                                           const float *__restrict__ wx0, const float *__restrict__ bx0,
                                                           const float *__restrict__ wx1, const float *__restrict__ bx1,
                                                           const float *__restrict__ wf0, const float *__restrict__ bf0,
                                                           const float *__restrict__ wf1, const float *__restrict__ bf1,
                                                           const float *__restrict__ wm, const float *__restrict__ bm,
                                                           float *__restrict__ xyz_out, float *__restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) float smem_embed[];
    __shared__ float in5[5][64];
    float *a0 = smem_embed, *cat = a0 + EMB_A0, *wbuf = cat + EMB_CAT;
    const Wave w;
    const long row0 = (long)blockIdx.x * 64;

    if (w.tid < 64) {
        const long r = row0 + w.tid;
        float x = 0.f, y = 0.f, z = 0.f, f0 = 0.f, f1 = 0.f;
        if (r < rows) {
            const float *p = pts + r * 5;
            x = p[0]; y = p[1]; z = p[2]; f0 = p[3]; f1 = p[4];
            if (box_ce) {
                // rcnn_net.py:338-351 in its order: centre, Rot_y(-ry) (einsum row . Rot^T), half extents l, h, w, the 1.2 x box
                const float *b = box_ce + (r / pts_per_cloud) * 7;
                x = x - b[0]; y = y - b[1]; z = z - b[2];
                const float a = -b[6], c = cosf_cr(a), s = sinf_cr(a);
                float cx = x * c + z * s;
                float cz = x * (-s) + z * c;
                cx = cx / (b[5] / 2.f);
                float cy = y / (b[3] / 2.f);
                cz = cz / (b[4] / 2.f);
                const float m = gp_nanmax(gp_nanmax(fabsf(cx), fabsf(cy)), fabsf(cz));
                const bool outside = m > extend;
                x = outside ? 0.f : cx; y = outside ? 0.f : cy; z = outside ? 0.f : cz;
            }
            float *o = xyz_out + r * 3;
            o[0] = x; o[1] = y; o[2] = z;
        }
        in5[0][w.tid] = x; in5[1][w.tid] = y; in5[2][w.tid] = z; in5[3][w.tid] = f0; in5[4][w.tid] = f1;
    }
    __syncthreads();

    const int pr = w.tid & 63, pc0 = (w.tid >> 6) * 32;      // the VALU layers: this thread's point, its 32 channels
    {
        const float x = in5[0][pr], y = in5[1][pr], z = in5[2][pr];
        for (int c = pc0; c < pc0 + 32; ++c)
            a0[c * GP_XS + pr] = bias_relu(x * wx0[c] + y * wx0[EMB_C + c] + z * wx0[2 * EMB_C + c], bx0[c], 1);
    }
    lds_layer<2>(w, a0, EMB_C / GP_KT, wx1, EMB_C, EMB_C, wbuf, 0, 1,
                 [&](const floatx16 &acc, int col) { store_act(w, acc, bx1, 1, cat, col); });
    {
        const float f0 = in5[3][pr], f1 = in5[4][pr];
        for (int c = pc0; c < pc0 + 32; ++c) a0[c * GP_XS + pr] = bias_relu(f0 * wf0[c] + f1 * wf0[EMB_C + c], bf0[c], 1);
    }
    lds_layer<2>(w, a0, EMB_C / GP_KT, wf1, EMB_C, EMB_C, wbuf, 0, 1,
                 [&](const floatx16 &acc, int col) { store_act(w, acc, bf1, 1, cat + EMB_C * GP_XS, col); });
    lds_layer<2>(w, cat, 2 * EMB_C / GP_KT, wm, 2 * EMB_C, EMB_C, wbuf, 0, 1,
                 [&](const floatx16 &acc, int col) { store_rows(w, acc, bm, 1, feat, EMB_C, row0 + 32 * w.wm, col, rows); });
}

// ------------------------------------------------------------------------------------------------ boxes
// decode_bbox_target_stage_2 as rcnn_net.py:294-302 calls it (roi centre 0, get_xz_fine = get_ry_fine = False, y by offset), then
// box2center_box; torch's fp32 operation order, python scalars rounded to fp32 the way a tensor-scalar op does.  One thread per row.
__global__ __launch_bounds__(256) void stage2_boxes_kernel(int rows, int nb, int head_bins, float loc_scope, float h, float w, float l,
                                                           const float *__restrict__ reg, float *__restrict__ pred, float *__restrict__ ce) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int width = 4 * nb + 1 + 2 * head_bins + 3;
    const float *g = reg + (long)r * width;
    const float pos_x = g[2 * nb] * loc_scope, pos_z = g[3 * nb] * loc_scope, pos_y = g[4 * nb];
    const float *hb = g + 4 * nb + 1;
    int best = 0;
    float bv = hb[0];
    for (int i = 1; i < head_bins; ++i) {       // torch.argmax: the first maximum; a NaN wins and stays
        const float v = hb[i];
        if (!(bv != bv) && (v > bv || v != v)) { bv = v; best = i; }
    }
    const double apc = (2.0 * M_PI) / head_bins;
    const float two_pi = (float)(2.0 * M_PI);
    const float ry_res = hb[head_bins + best] * (float)(apc / 2.0);
    float ry = py_mod((float)best * (float)apc + ry_res, two_pi);
    if (ry > (float)M_PI) ry = ry - two_pi;
    const float *sz = hb + 2 * head_bins;
    const float bh = sz[0] * h + h, bw = sz[1] * w + w, bl = sz[2] * l + l;
    float *p = pred + (long)r * 7, *c = ce + (long)r * 7;
    p[0] = pos_x + 0.f; p[1] = pos_y; p[2] = pos_z + 0.f; p[3] = bh; p[4] = bw; p[5] = bl; p[6] = ry;
    c[0] = pos_x + 0.f; c[1] = pos_y - bh / 2.f; c[2] = pos_z + 0.f; c[3] = bh; c[4] = bw; c[5] = bl; c[6] = ry;
}

// ------------------------------------------------------------------------------------------------ select
// per slot (b, k): center_box2box, refine_box, ry into (-pi, pi], the shift into the scene's frame, the keep flag and the sort key
struct SelectArgs {
    float cls_thresh, iou_thresh, h_lo, h_hi, w_lo, w_hi, l_lo, l_hi, ground_y;
};

__global__ __launch_bounds__(256) void stage2_select_kernel(int batch, int k_dim, SelectArgs a, const float *__restrict__ box_ce,
                                                            const float *__restrict__ ref, const float *__restrict__ cls,
                                                            const float *__restrict__ iou, const float *__restrict__ center,
                                                            const int32_t *__restrict__ num, float *__restrict__ boxes,
                                                            int32_t *__restrict__ keep, float *__restrict__ key) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)batch * k_dim) return;
    const int b = (int)(i / k_dim), k = (int)(i % k_dim);
    const float *c = box_ce + i * 7, *d = ref + i * 7, *ctr = center + i * 3;
    const float two_pi = (float)(2.0 * M_PI);
    // center_box2box (bbox_transform.py:286-290)
    const float px = c[0], py = c[1] + c[3] / 2.f, pz = c[2], ph = c[3], pw = c[4], pl = c[5], pry = py_mod(c[6], two_pi);
    // refine_box (:298-303): xyz + hwl * ref[0:3], hwl * (1 + ref[3:6]), ry + ref[6]
    float x = px + ph * d[0], y = py + pw * d[1], z = pz + pl * d[2];
    const float h = ph * (1.f + d[3]), wd = pw * (1.f + d[4]), l = pl * (1.f + d[5]);
    float ry = py_mod(pry + d[6], two_pi);
    if (ry > (float)M_PI) ry = ry - two_pi;
    x = x + ctr[0]; z = z + ctr[2]; y = y + a.ground_y;
    const float s = 1.0f / (1.0f + expf(-cls[i]));                 // torch.sigmoid's fp32 expression
    const float q = iou[i];
    const bool kp = s > a.cls_thresh && q > a.iou_thresh && h > a.h_lo && h < a.h_hi && wd > a.w_lo && wd < a.w_hi && l > a.l_lo && l < a.l_hi &&
                    k < num[b];
    float *o = boxes + i * 7;
    o[0] = x; o[1] = y; o[2] = z; o[3] = h; o[4] = wd; o[5] = l; o[6] = ry;
    keep[i] = kp ? 1 : 0;
    key[i] = kp ? q : -1e30f;
}

}  // namespace ws3d

using namespace ws3d;

extern "C" int ws3d_stage2_embed(long rows, int pts_per_cloud, const float *pts, const float *box_ce, float extend, const float *wx0,
                                 const float *bx0, const float *wx1, const float *bx1, const float *wf0, const float *bf0, const float *wf1,
                                 const float *bf1, const float *wm, const float *bm, float *xyz_out, float *feat, ws3d_stream_t stream) {
    if (rows < 0 || pts_per_cloud <= 0 || (rows > 0 && (!pts || !wx0 || !bx0 || !wx1 || !bx1 || !wf0 || !bf0 || !wf1 || !bf1 || !wm || !bm || !xyz_out || !feat))) {
        set_error("ws3d_stage2_embed: invalid argument (rows=%ld pts_per_cloud=%d)", rows, pts_per_cloud);
        return WS3D_E_INVALID;
    }
    if (rows == 0) return WS3D_OK;
    const long tiles = (rows + 63) / 64;
    if (tiles > 0x7fffffffL) { set_error("ws3d_stage2_embed: %ld rows are too many", rows); return WS3D_E_UNSUPPORTED; }
    if (int rc = raise_lds_cap((const void *)stage2_embed_kernel, EMB_LDS, "ws3d_stage2_embed")) return rc;
    hipLaunchKernelGGL(stage2_embed_kernel, dim3((unsigned)tiles), dim3(256), EMB_LDS, as_stream(stream), rows, pts_per_cloud, pts, box_ce, extend,
                       wx0, bx0, wx1, bx1, wf0, bf0, wf1, bf1, wm, bm, xyz_out, feat);
    return check_launch("ws3d_stage2_embed");
}

extern "C" int ws3d_stage2_boxes(int rows, int loc_bins, int head_bins, float loc_scope, float h, float w, float l, const float *rcnn_reg,
                                 float *pred_boxes3d, float *box_ce, ws3d_stream_t stream) {
    if (rows < 0 || loc_bins <= 0 || head_bins <= 0 || (rows > 0 && (!rcnn_reg || !pred_boxes3d || !box_ce))) {
        set_error("ws3d_stage2_boxes: invalid argument (rows=%d loc_bins=%d head_bins=%d)", rows, loc_bins, head_bins);
        return WS3D_E_INVALID;
    }
    if (rows == 0) return WS3D_OK;
    hipLaunchKernelGGL(stage2_boxes_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, as_stream(stream), rows, loc_bins, head_bins, loc_scope,
                       h, w, l, rcnn_reg, pred_boxes3d, box_ce);
    return check_launch("ws3d_stage2_boxes");
}

extern "C" int ws3d_stage2_select(int batch, int slots, float cls_thresh, float iou_thresh, const float *size_window, float ground_y,
                                  const float *box_ce, const float *rcnn_ref, const float *rcnn_cls, const float *rcnn_iou, const float *center,
                                  const int32_t *num, float *boxes, int32_t *keep, float *key, ws3d_stream_t stream) {
    if (batch < 0 || slots < 0 || !size_window ||
        ((long)batch * slots > 0 && (!box_ce || !rcnn_ref || !rcnn_cls || !rcnn_iou || !center || !num || !boxes || !keep || !key))) {
        set_error("ws3d_stage2_select: invalid argument (batch=%d slots=%d)", batch, slots);
        return WS3D_E_INVALID;
    }
    const long n = (long)batch * slots;
    if (n == 0) return WS3D_OK;
    const SelectArgs a = {cls_thresh, iou_thresh, size_window[0], size_window[1], size_window[2], size_window[3], size_window[4], size_window[5], ground_y};
    hipLaunchKernelGGL(stage2_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), batch, slots, a, box_ce, rcnn_ref,
                       rcnn_cls, rcnn_iou, center, num, boxes, keep, key);
    return check_launch("ws3d_stage2_select");
}
