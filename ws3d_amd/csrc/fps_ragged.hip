// fps_ragged.hip -- furthest point sampling of MANY clouds of different sizes in one launch (ws3d extension; the
// ground-truth database builder samples every object of a chunk of scans at once, ws3d_amd/gt_database.py).
//
// One 256-thread workgroup per cloud.  Cloud i holds the points offsets[i] .. offsets[i+1] of a packed (total,3) array.  As in
// fps.hip the whole cloud and its running minimum distance live in VGPRs for the entire kernel: thread u keeps PPT points, PPT
// chosen PER WORKGROUP from {1,2,4,8,16} by the cloud's own size (a block-uniform switch over instantiations of one device
// function, so a 600-point cloud sweeps 4 slots per lane, not 16).  256 x 16 = 4096 points is what the kernel holds; larger
// clouds are forwarded by the C entry to ws3d_furthest_point_sampling, one launch each on the same stream.  No global scratch.
//
// Bit-equal to ws3d_furthest_point_sampling(1, n_i, m, ...) on each cloud alone: the tie rule depends on the cloud's size through
// bs = opt_n_threads(n_i) and is carried by fps.hip's tie-order POSITION p = bitrev(k mod bs) * S + k / bs (S = ceil(n/bs)):
// thread u owns the contiguous positions [u*PPT, (u+1)*PPT), and "lowest slot, lowest lane, lowest wave wins" is the reference's
// order for any workgroup size.  Distances through sqdist3 (common.h), so every WS3D_DIST_MODE build follows its oracle.
#include <vector>

#include "fps_ragged.h"

namespace ws3d {

__global__ __launch_bounds__(RAGGED_NT) void fps_ragged_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ offsets,
                                                               int32_t *__restrict__ idx, int total, int m, int limit) {
    __shared__ float4 s_cand[2][16];
    __shared__ int s_k[2][16];
    const int c = blockIdx.x;
    const int off = offsets[c];
    const int n = offsets[c + 1] - off;
    // larger clouds belong to the per-cloud kernel (the C entry launches it); anything that does not lie inside the packed array is
    // not touched (the entry validated the host copy of the sizes -- this guards a device array that disagrees with it)
    if (n < 1 || n > limit || n < m || off < 0 || n > total - off) return;
    xyz += (size_t)off * 3;
    idx += (size_t)c * m;
    // bs = opt_n_threads(n) = the largest power of two <= n, capped at 1024 (the entry checked that the launcher's libm expression
    // agrees with this for every n <= limit)
    int log2bs = 31 - __builtin_clz((unsigned)n);
    if (log2bs > 10) log2bs = 10;
    const int bs = 1 << log2bs;
    const int S = (n + bs - 1) / bs;
    const int R = bs * S;                                // tie-order positions, <= 4096 for n <= 4096
    const int ppt = (R + RAGGED_NT - 1) / RAGGED_NT;
    if (threadIdx.x == 0) idx[0] = 0;
    if (ppt <= 1) ragged_cloud<1>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 2) ragged_cloud<2>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 4) ragged_cloud<4>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else if (ppt <= 8) ragged_cloud<8>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    else ragged_cloud<16>(xyz, idx, n, m, bs, log2bs, S, s_cand, s_k);
    // positions -> point indices, off the critical path (thread 0 wrote idx[])
    __syncthreads();
    for (int j = 1 + threadIdx.x; j < m; j += RAGGED_NT) {
        const int p = idx[j];
        const int rb = p / S, sl = p - rb * S;
        idx[j] = ragged_bitrev(rb, log2bs) + sl * bs;
    }
}

}  // namespace ws3d

extern "C" int ws3d_fps_ragged_limit(void) { return ws3d::ragged_limit(); }

extern "C" int ws3d_furthest_point_sampling_ragged(int clouds, const int32_t *offsets, const int32_t *sizes_host, int m, const float *xyz,
                                                   int32_t *idx, ws3d_stream_t stream) {
    using namespace ws3d;
    if (clouds < 0 || m < 0 || (clouds > 0 && (!offsets || !sizes_host || !xyz || (!idx && m > 0)))) {
        set_error("ws3d_furthest_point_sampling_ragged: invalid argument (clouds=%d m=%d)", clouds, m);
        return WS3D_E_INVALID;
    }
    if (clouds == 0) return WS3D_OK;
    long total = 0;
    for (int i = 0; i < clouds; ++i) {
        if (sizes_host[i] < 1 || sizes_host[i] < m) {
            set_error("ws3d_furthest_point_sampling_ragged: invalid argument (cloud %d holds %d points, m=%d)", i, sizes_host[i], m);
            return WS3D_E_INVALID;
        }
        total += sizes_host[i];
    }
    if (total > 0x7fffffffL / 3) {
        set_error("ws3d_furthest_point_sampling_ragged: invalid argument (%ld points exceed the 32-bit offsets)", total);
        return WS3D_E_INVALID;
    }
    if (m == 0) return WS3D_OK;
    const int limit = ragged_limit();
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(fps_ragged_kernel, dim3(clouds), dim3(RAGGED_NT), 0, st, xyz, offsets, idx, (int)total, m, limit);
    if (int rc = check_launch("furthest_point_sampling_ragged")) return rc;
    long off = 0;
    for (int i = 0; i < clouds; ++i) {
        if (sizes_host[i] > limit)
            if (int rc = ws3d_furthest_point_sampling(1, sizes_host[i], m, xyz + off * 3, nullptr, idx + (size_t)i * m, stream)) return rc;
        off += sizes_host[i];
    }
    return WS3D_OK;
}
