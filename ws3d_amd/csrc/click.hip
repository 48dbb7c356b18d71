// click.hip -- the front of WS3D's click-driven annotation for gfx950 (tools/eval_active.py:187, 198-209, 656-675): a person's BEV
// clicks become (1) a soft foreground score per scene point, the Gaussian of its distance to the nearest click
// (click_gaussian_mask), and (2) the jittered candidate centres, every click on a side x side grid of offsets, in the order the
// reference concatenates them.  The reference does both on the host, scene by scene; here one call serves a padded batch whose
// scenes hold different numbers of clicks, without reading num on the host.
//
// Two element-wise kernels.  Score: one thread per point, the clicks of the scene staged through LDS in chunks of CLICK_CHUNK (every
// lane reads the same LDS address: a broadcast), so K is unbounded; plain stores.  Candidates: one thread per slot.  No allocation,
// no host synchronisation, no atomics; every output element is written.
#include <climits>
#include <cmath>

#include "common.h"

namespace ws3d {

constexpr int CLICK_CHUNK = 256;  // clicks staged per trip = the workgroup's size (ws3d_amd.compat.CLICK_LDS_CHUNK restates it)
constexpr int CLICK_MAX_SIDE = 9;

typedef float ck_f4 __attribute__((ext_vector_type(4)));
typedef ck_f4 ck_f4u __attribute__((aligned(4)));  // 16-byte access, 4-byte aligned

struct ClickOffsets {
    float v[CLICK_MAX_SIDE];
};

__device__ __forceinline__ int click_count(const int32_t *__restrict__ num, int b, int clicks_num) {
    return num ? min(max(num[b], 0), clicks_num) : clicks_num;  // a num outside 0..K cannot carry a read past the scene's clicks
}

// blocks_per_scene workgroups of 256 points per scene.  The order of operations is losses.gaussian_center_labels' (the reference's):
// the point's own height scaled, not a difference; (dx^2 + yh^2) + dz^2; nothing contracted.
__global__ __launch_bounds__(CLICK_CHUNK) void click_score_kernel(int pts_num, int clicks_num, int blocks_per_scene, float gauss_height,
                                                                  float gauss_status, float gauss_cov, const float *__restrict__ pts,
                                                                  const float *__restrict__ clicks, const int32_t *__restrict__ num,
                                                                  float *__restrict__ score) {
    __shared__ float2 xz_s[CLICK_CHUNK];
    const int b = blockIdx.x / blocks_per_scene;
    const int tid = threadIdx.x;
    const int i = (blockIdx.x - b * blocks_per_scene) * CLICK_CHUNK + tid;
    const int nb = click_count(num, b, clicks_num);  // workgroup-uniform: the barriers below are reached by all or by none
    // a lane past the scene loads the last point (clamped, never branched) and stores nothing
    const ck_f4 p = *reinterpret_cast<const ck_f4u *>(pts + ((size_t)b * pts_num + min(i, pts_num - 1)) * 4);
    const float yh = p.y * gauss_height;
    const float yh2 = yh * yh;
    const float *c = clicks + (size_t)b * clicks_num * 3;
    float near = 100.0f;
    for (int k0 = 0; k0 < nb; k0 += CLICK_CHUNK) {
        const int kn = min(CLICK_CHUNK, nb - k0);
        if (tid < kn) xz_s[tid] = make_float2(c[(size_t)(k0 + tid) * 3], c[(size_t)(k0 + tid) * 3 + 2]);  // a click's y is never read
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            const float2 q = xz_s[k];
            const float dx = p.x - q.x, dz = p.z - q.y;
            const float d = sqrtf((dx * dx + yh2) + dz * dz);
            near = fminf(near, fminf(fmaxf(d - gauss_status, 0.0f), 100.0f));
        }
        __syncthreads();
    }
    if (i < pts_num) score[(size_t)b * pts_num + i] = expf(-0.5f * near * near / gauss_cov);
}

// blocks_per_scene workgroups of 256 slots per scene (at least one: slot 0's thread also writes cand_num).  Slot j < side^2 * num[b]:
// grid cell g = j / num[b] (x offset g / side outer, z offset g % side inner), click k = j % num[b] -- whole click lists concatenated.
__global__ __launch_bounds__(256) void click_candidates_kernel(int clicks_num, int side, int blocks_per_scene, ClickOffsets off, float centre_y,
                                                               const float *__restrict__ clicks, const int32_t *__restrict__ num,
                                                               float *__restrict__ cand, int32_t *__restrict__ cand_num) {
    const int b = blockIdx.x / blocks_per_scene;
    const int j = (blockIdx.x - b * blocks_per_scene) * 256 + threadIdx.x;
    const int nb = click_count(num, b, clicks_num);
    const int slots = side * side * clicks_num, real = side * side * nb;
    if (j == 0) cand_num[b] = real;
    if (j >= slots) return;
    float x = 0.f, y = 0.f, z = 0.f;
    if (j < real) {  // nb > 0 here
        const int g = j / nb, k = j - g * nb;
        const int gi = g / side, gj = g - gi * side;
        const float *c = clicks + ((size_t)b * clicks_num + k) * 3;
        float ox = 0.f, oz = 0.f;
#pragma unroll
        for (int m = 0; m < CLICK_MAX_SIDE; ++m) {  // selects, not a dynamic index into the by-value argument (which would go to scratch)
            ox = m == gi ? off.v[m] : ox;
            oz = m == gj ? off.v[m] : oz;
        }
        x = c[0] + ox; y = centre_y; z = c[2] + oz;
    }
    float *o = cand + ((size_t)b * slots + j) * 3;
    o[0] = x; o[1] = y; o[2] = z;
}

}  // namespace ws3d

extern "C" int ws3d_click_prepare(int batch, int pts_num, int clicks_num, int side, const float *offsets, float gauss_height, float gauss_status,
                                  float gauss_cov, float centre_y, const float *pts, const float *clicks, const int32_t *num, float *score,
                                  float *cand, int32_t *cand_num, ws3d_stream_t stream) {
    using namespace ws3d;
    if (batch < 0 || pts_num < 0 || clicks_num < 0 || side < 1 || side > CLICK_MAX_SIDE) {
        set_error("ws3d_click_prepare: invalid argument (B=%d N=%d K=%d side=%d; side must be 1..%d)", batch, pts_num, clicks_num, side, CLICK_MAX_SIDE);
        return WS3D_E_INVALID;
    }
    if (batch == 0) return WS3D_OK;
    if (!offsets || (pts_num > 0 && (!pts || !score)) || (clicks_num > 0 && (!clicks || !cand)) || !cand_num) {
        set_error("ws3d_click_prepare: invalid argument (a required pointer is NULL)");
        return WS3D_E_INVALID;
    }
    const long slots = (long)side * side * clicks_num;
    const long score_bps = ((long)pts_num + CLICK_CHUNK - 1) / CLICK_CHUNK, cand_bps = slots > 0 ? (slots + 255) / 256 : 1;
    if (pts_num > INT_MAX / 2 || slots > INT_MAX / 4 || batch * score_bps > INT_MAX || batch * cand_bps > INT_MAX) {  // int indices, 1-D grids
        set_error("ws3d_click_prepare: B=%d N=%d K=%d side=%d in one call are not supported", batch, pts_num, clicks_num, side);
        return WS3D_E_UNSUPPORTED;
    }
    if (pts_num > 0) {
        hipLaunchKernelGGL(click_score_kernel, dim3((unsigned)(batch * score_bps)), dim3(CLICK_CHUNK), 0, as_stream(stream), pts_num, clicks_num,
                           (int)score_bps, gauss_height, gauss_status, gauss_cov, pts, clicks, num, score);
        if (int rc = check_launch("ws3d_click_prepare")) return rc;
    }
    ClickOffsets off;
    for (int m = 0; m < CLICK_MAX_SIDE; ++m) off.v[m] = m < side ? offsets[m] : 0.f;
    hipLaunchKernelGGL(click_candidates_kernel, dim3((unsigned)(batch * cand_bps)), dim3(256), 0, as_stream(stream), clicks_num, side, (int)cand_bps,
                       off, centre_y, clicks, num, cand, cand_num);
    return check_launch("ws3d_click_prepare");
}
