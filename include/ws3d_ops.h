/*
 * ws3d_ops.h -- C ABI of libws3d_hip.so: the MI355X (gfx950) replacement for the
 * three CUDA extension modules of hlesmqh/WS3D's PointNet++ / roipool3d / iou3d
 * hot path.
 *
 * The reference has no C ABI: its boundary is three pybind11 modules
 * (pointnet2_cuda, iou3d_cuda, roipool3d_cuda) whose functions take pre-allocated
 * at::Tensor objects.  Every entry point below replaces one of those functions
 * (cited as file:line relative to the reference checkout), with the tensors
 * flattened to plain device pointers + sizes + a stream.  INTEGRATION.md shows the
 * Python (ctypes) binding a reference maintainer adds; ws3d_amd/compat.py is that
 * binding, exporting modules with the reference's exact function names.
 *
 * Conventions
 *   - all pointers are DEVICE pointers to C-contiguous row-major arrays; data are
 *     float32, indices int32 (the reference's dtypes), unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work
 *     is enqueued asynchronously on it; no entry point synchronises the device,
 *     allocates, or frees (scratch comes from caller-provided workspaces sized by
 *     the *_workspace_bytes() queries);
 *   - return value: 0 on success, a negative WS3D_E_* code on failure (never
 *     exit()s, unlike the reference: sampling_gpu.cu:39-43, iou3d.cpp:13-21);
 *     ws3d_last_error() returns a thread-local message for the last failure;
 *   - arithmetic contract (bit-exact index outputs): DESIGN.md section 4.
 */
#ifndef WS3D_OPS_H
#define WS3D_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WS3D_OK 0
#define WS3D_E_INVALID (-1)   /* bad size / null pointer                        */
#define WS3D_E_LAUNCH (-2)    /* hipGetLastError() != hipSuccess after a launch */
#define WS3D_E_WORKSPACE (-3) /* workspace missing or too small                 */
#define WS3D_E_UNSUPPORTED (-4)

#if defined(__GNUC__)
#define WS3D_API __attribute__((visibility("default")))
#else
#define WS3D_API
#endif

typedef void *ws3d_stream_t;

/* bumped whenever an entry point is added or a signature changes (5: ws3d_three_nn_wq, ws3d_roipool3d_ws / ws3d_roipool3d_workspace_bytes, ws3d_furthest_point_sampling_nested_chain, ws3d_ball_query_pairs2; 4: ws3d_pgather_gemm3_compact, ws3d_qinterp_gemm; 3: ws3d_topk_sorted_ws / ws3d_topk_workspace_bytes; 2: launch gates
 * of the SharedMLP kernels, ws3d_sa_mlp3_pool_lists, ws3d_ball_query_pairs, ws3d_three_nn_w; 1: rounds 1-2); ws3d_amd/_lib.py refuses a library whose version differs from the header it was written against */
#define WS3D_ABI_VERSION 6
WS3D_API int ws3d_abi_version(void);
/* Launch-geometry knobs of the persistent kernels (round 6): key 0 = workgroups of ws3d_chain_mlp3, 1 = of ws3d_mlp2_rows, 2 = of
 * ws3d_sa_mlp3_pool_compact, 3 = of ws3d_qinterp_gemm, 4 = of ws3d_compact_mlp_pair kinds 2 / 1 (along x), 5 = waves per 64-centre tile of ws3d_ball_query_pairs2 launches that do not fill the chip (8; anything else: 16); value 0 restores the built-in choice, a negative value only reads.  Returns the
 * previous value (WS3D_E_INVALID for an unknown key).  Speed only: results do not depend on these. Process-wide, not thread-safe. */
WS3D_API int ws3d_tune(int key, int value);
/* Squared-distance convention this library was BUILT with (csrc/common.h WS3D_DIST_MODE; the reference spells
 * dx*dx + dy*dy + dz*dz, sampling_gpu.cu:133 / ball_query_gpu.cu:33 / interpolate_gpu.cu:36, and nvcc's contraction of it
 * cannot be captured without a CUDA device): 0 = fma(dz,dz,fma(dx,dx,dy*dy)) [default], 1 = no contraction,
 * 2 = fma(dz,dz,fma(dy,dy,dx*dx)).  libws3d_hip_dm1.so / _dm2.so are the other builds.                          */
WS3D_API int ws3d_dist_mode(void);
WS3D_API const char *ws3d_last_error(void);
/* name/CU count/LDS bytes of the current device; any pointer may be NULL */
WS3D_API int ws3d_device_info(char *name, int name_len, int *cu_count, int *lds_bytes_per_block);

/* ---------------------------------------------------------------- pointnet2_cuda */

/* furthest_point_sampling_wrapper(b,n,m,xyz,temp,idx)   sampling.cpp:36-46 ->
 * furthest_point_sampling_kernel sampling_gpu.cu:93-253.
 * xyz (b,n,3); temp (b,n) in/out scratch, pre-filled by the caller (1e10,
 * pointnet2_utils.py:26) -- may be NULL (then 1e10 is assumed and nothing is written
 * back); idx (b,m) out.  idx[.,0] = 0.  Tie-break identical to the reference launch
 * geometry (block = opt_n_threads(n), cuda_utils.h:10-14).                          */
WS3D_API int ws3d_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int32_t *idx,
                                 ws3d_stream_t stream);

/* Fused a1+a2 of SURVEY section 8a: FPS that also emits the sampled coordinates
 * new_xyz (b,m,3) = xyz[idx]  (replaces furthest_point_sample + gather_operation +
 * transpose at pointnet2_modules.py:30-35).  new_xyz may be NULL.                  */
WS3D_API int ws3d_furthest_point_sampling_gather(int b, int n, int m, const float *xyz, float *temp,
                                        int32_t *idx, float *new_xyz, ws3d_stream_t stream);

/* ws3d_furthest_point_sampling[_gather] with a caller-provided scratch buffer: for scenes of ws3d_fps_workspace_bytes(b, n) > 0
 * bytes (16384 < n <= 65536; a pure host function, linear in b, a multiple of 16) the scene is counting-sorted once into Z-order
 * buckets of 64 points inside `workspace` and every step updates only the buckets whose bounding box the new sample can reach
 * (fps_pruned.hip: the skip is exact).  idx, temp and new_xyz (may be NULL) equal those of the plain entries bit for bit for ANY
 * input and any initial temp (NULL: 1e10 assumed, nothing written back), ties included.  workspace NULL / too small / not 16-byte
 * aligned, n outside that range, or WS3D_FPS_PRUNED=0 in the environment (read once): this IS ws3d_furthest_point_sampling_gather,
 * return codes included.  Contents undefined on return; nothing is allocated or synchronised.  ws3d extension (ABI 6). */
WS3D_API size_t ws3d_fps_workspace_bytes(int b, int n);
WS3D_API int ws3d_furthest_point_sampling_ws(int b, int n, int m, const float *xyz, float *temp, int32_t *idx,
                                             float *new_xyz /* may be NULL */, void *workspace, size_t workspace_bytes,
                                             ws3d_stream_t stream);

/* FPS + gather of a cloud that is ALREADY in sampling order -- level l+1 of a set-abstraction stack samples the centres
 * level l selected, in the order it selected them (pointnet2_msg.py:56-70) -- where greedy selection returns idx = 0..m-1
 * unless two points tie for a maximum.  Same results as ws3d_furthest_point_sampling_gather for ANY input: the nesting is
 * verified in parallel (every point's running minimum against the picked point's, strictly), and a scene that fails the
 * check is sampled by a literal restatement of sampling_gpu.cu:93-209.  n <= 4096 (else WS3D_E_UNSUPPORTED), m <= n;
 * idx (b,m) and new_xyz (b,m,3) are both required (they double as scratch).  No reference counterpart.               */
WS3D_API int ws3d_furthest_point_sampling_nested(int b, int n, int m, const float *xyz, int32_t *idx, float *new_xyz,
                                        ws3d_stream_t stream);

/* ws3d_furthest_point_sampling_nested for a CHAIN of levels in four launches: level 0 samples m[0] of the n points of xyz (verified in
 * parallel as above), level l > 0 samples m[l] of level l-1's new_xyz (m non-increasing; host array of `levels` <= 5 counts, host arrays of
 * `levels` device pointers idx[l] (b, m[l]) / new_xyz[l] (b, m[l], 3)).  When level 0 verifies, the levels below it are verified with it
 * (their check is a subset of level 0's inequalities on the same floats): one kernel writes their prefixes; a scene that does not verify
 * takes the literal restatement of sampling_gpu.cu:93-209 level by level.  Same outputs as `levels` calls of the entry above.  (round 5) */
WS3D_API int ws3d_furthest_point_sampling_nested_chain(int b, int n, int levels, const int *m, const float *xyz, int32_t *const *idx,
                                                       float *const *new_xyz, ws3d_stream_t stream);

/* Furthest point sampling of `clouds` clouds of DIFFERENT sizes in one launch, one workgroup per cloud, points and running minimum
 * on chip (no scratch).  xyz (total,3) packed; offsets (clouds+1) DEVICE int32 with offsets[0] = 0, cloud i = points offsets[i] ..
 * offsets[i+1]; sizes_host (clouds) a HOST copy of the sizes offsets[i+1] - offsets[i] (validation and forwarding need them without
 * a read-back); idx (clouds,m) out, indices LOCAL to each cloud.  idx[i] is bit-equal to ws3d_furthest_point_sampling(1, n_i, m, ..)
 * on cloud i alone (the tie rule follows the cloud's own opt_n_threads(n_i)).  Clouds above ws3d_fps_ragged_limit() points (4096:
 * 256 threads x 16 points) are forwarded to that entry, one launch each on the same stream (so n_i <= 65536).  clouds == 0 or
 * m == 0: nothing is launched; any n_i < 1 or n_i < m: WS3D_E_INVALID before anything is launched.  No reference counterpart (the
 * reference samples object by object from its dataset, kitti_rcnn_dataset.py:320-331).                                            */
WS3D_API int ws3d_fps_ragged_limit(void);
WS3D_API int ws3d_furthest_point_sampling_ragged(int clouds, const int32_t *offsets, const int32_t *sizes_host, int m, const float *xyz,
                                                 int32_t *idx, ws3d_stream_t stream);

/* gather_points_wrapper(b,c,n,npoints,points,idx,out)   sampling.cpp:11-20 ->
 * sampling_gpu.cu:8-37.  points (b,c,n), idx (b,npoints) -> out (b,c,npoints).     */
WS3D_API int ws3d_gather_points(int b, int c, int n, int npoints, const float *points, const int32_t *idx,
                       float *out, ws3d_stream_t stream);

/* gather_points_grad_wrapper   sampling.cpp:23-33 -> sampling_gpu.cu:46-76.
 * grad_points (b,c,n) must be pre-zeroed by the caller (pointnet2_utils.py:67).    */
WS3D_API int ws3d_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out,
                            const int32_t *idx, float *grad_points, ws3d_stream_t stream);

/* ball_query_wrapper(b,n,m,radius,nsample,new_xyz,xyz,idx)   ball_query.cpp:14-25 ->
 * ball_query_gpu.cu:9-67.  new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample),
 * pre-zeroed by the caller (pointnet2_utils.py:218); rows without a hit are left
 * untouched.  sorted: NULL, or the output of ws3d_sort_points_x for this xyz.       */
WS3D_API int ws3d_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                    const float *xyz, int32_t *idx, const void *sorted, ws3d_stream_t stream);
/* ws3d_ball_query that also writes the rows of centres WITHOUT a hit (as zeros: what the reference's callers see in their
 * zero-initialised idx tensor, pointnet2_utils.py:201), so that idx need not be cleared first.  ws3d extension.           */
WS3D_API int ws3d_ball_query_fill(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                         const float *xyz, int32_t *idx, const void *sorted, ws3d_stream_t stream);
/* ws3d_ball_query_fill + ws3d_compact_pairs in ONE launch: the lists idx (b, m, nsample) and their distinct (centre, source) pairs
 * rowc / rowsrc (b * m * nsample ints each, the first *total valid; *total must be ZERO on entry; compact rows of a centre
 * contiguous, centres in arrival order of their 64-centre workgroups).  Needs the fine-grid buffer of ws3d_sort_points_grid and
 * nsample <= 64 (the kernel that works with one wave per centre), else WS3D_E_UNSUPPORTED.  ws3d extension.                   */
WS3D_API int ws3d_ball_query_pairs(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int32_t *idx,
                          const void *sorted_grid, int32_t *rowc, int32_t *rowsrc, int32_t *total, ws3d_stream_t stream);

/* ws3d_ball_query_pairs for the TWO scales of a set-abstraction level in one launch: same xyz / new_xyz / fine-grid copy, per scale a
 * radius, an nsample (<= 64) and the four outputs of ws3d_ball_query_pairs (every `total` zero on entry).  Same lists and pair tables as
 * two calls; WS3D_E_UNSUPPORTED where the one-wave-per-centre kernel does not cover the call (then call per scale).  (round 5) */
WS3D_API int ws3d_ball_query_pairs2(int b, int n, int m, const float *new_xyz, const float *xyz, const void *sorted_grid,
                                    float radius0, int nsample0, int32_t *idx0, int32_t *rowc0, int32_t *rowsrc0, int32_t *total0,
                                    float radius1, int nsample1, int32_t *idx1, int32_t *rowc1, int32_t *rowsrc1, int32_t *total1,
                                    ws3d_stream_t stream);


/* Optional accelerator for ws3d_ball_query / ws3d_query_and_group (no reference counterpart):
 * a per-scene copy of xyz counting-sorted into uniform x cells (float4 {x,y,z,index} x n, a
 * 16-byte header and a cell-start table per scene; opaque to the caller).  With it each centre
 * scans only the cells overlapping |x - cx| < radius instead of all n points; results are
 * bit-identical.  ws3d_sorted_points_bytes() returns the buffer size, or 0 when the shape is not
 * supported (n > 16384): then pass sorted = NULL.  One binning serves every radius queried
 * against the same xyz.                                                                        */
WS3D_API size_t ws3d_sorted_points_bytes(int b, int n);
WS3D_API int ws3d_sort_points_x(int b, int n, const float *xyz, void *sorted, ws3d_stream_t stream);
/* Same buffer size and layout, but the points are binned into a near-square (x, z) grid (~2 points per
 * cell) instead of x slabs: for ws3d_three_nn ONLY (its search then visits square rings of cells around
 * the query, ~20 candidates instead of an x slab of ~100); not accepted by the ball-query entries.   */
WS3D_API int ws3d_sort_points_xz(int b, int n, const float *xyz, void *sorted, ws3d_stream_t stream);
/* Same buffer size, FINE (x, z) grid (up to 32768 near-square cells, ~0.4 m on a KITTI scene, 16-bit cell offsets): for
 * ws3d_ball_query / ws3d_query_and_group[_nlc] -- a centre scans, per grid row overlapping |z - cz| < r, the cells
 * overlapping |x - cx| < r instead of an x slab spanning all z (~5-30 candidates instead of 50-500 on lidar scenes);
 * results bit-identical to the full scan.  Preferred over ws3d_sort_points_x for the ball-query entries; NOT accepted by
 * ws3d_three_nn.                                                                                                   */
WS3D_API int ws3d_sort_points_grid(int b, int n, const float *xyz, void *sorted, ws3d_stream_t stream);
/* Several binning jobs in ONE launch (round 5): job i bins the (b, n[i], 3) cloud xyz[i] into sorted[i] (ws3d_sorted_points_bytes(b, n[i])
 * bytes each) -- kind[i] 0: as ws3d_sort_points_grid, 1: as ws3d_sort_points_xz; at most 8 jobs, 0 < n[i] <= 16384.  The arrays are host
 * arrays read before the call returns.  Same buffers as one call per job (the levels of a network and both flavours: 6 launches -> 1). */
WS3D_API int ws3d_sort_points_jobs(int b, int njobs, const int *n, const int *kind, const float *const *xyz, void *const *sorted,
                                   ws3d_stream_t stream);

/* group_points_wrapper(b,c,n,npoints,nsample,points,idx,out)   group_points.cpp:25-36
 * -> group_points_gpu.cu:47-86.  points (b,c,n), idx (b,npoints,nsample) ->
 * out (b,c,npoints,nsample).                                                        */
WS3D_API int ws3d_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                      const int32_t *idx, float *out, ws3d_stream_t stream);

/* group_points_grad_wrapper   group_points.cpp:11-22 -> group_points_gpu.cu:8-44.   */
WS3D_API int ws3d_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                           const int32_t *idx, float *grad_points, ws3d_stream_t stream);

/* Fused QueryAndGroup.forward (pointnet2_utils.py:241-264 = ball_query + 2x
 * grouping_operation + centre subtraction + cat).  xyz (b,n,3), new_xyz (b,m,3),
 * features (b,c,n) or NULL (c = 0) -> out (b, (use_xyz?3:0)+c, m, nsample) with
 * channel order [dx,dy,dz, features...].  idx_out (b,m,nsample) may be NULL; when
 * given it receives exactly what ws3d_ball_query would write into a zeroed idx.     */
WS3D_API int ws3d_query_and_group(int b, int n, int m, int c, float radius, int nsample, int use_xyz,
                         const float *xyz, const float *new_xyz, const float *features,
                         int32_t *idx_out, float *out, const void *sorted, ws3d_stream_t stream);

/* three_nn_wrapper(b,n,m,unknown,known,dist2,idx)   interpolate.cpp:14-23 ->
 * interpolate_gpu.cu:9-67.  unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3)
 * SQUARED distances, idx (b,n,3).  sorted_known: NULL (full scan) or the x-binned copy of
 * `known` from ws3d_sort_points_x / ws3d_sort_points_xz(b, m, known, ...) -- same result, the search then only visits
 * the known points whose x is closer than the running third-best distance.            */
WS3D_API int ws3d_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                  int32_t *idx, const void *sorted_known, ws3d_stream_t stream);

/* dist2 (rows,3) SQUARED distances from ws3d_three_nn -> weight (rows,3): the FP module's normalised
 * inverse-distance weights (pointnet2_modules.py:139-142) in one launch.  ws3d extension.            */
WS3D_API int ws3d_three_nn_weights(long rows, const float *dist2, float *weight, ws3d_stream_t stream);
/* ws3d_three_nn with ws3d_three_nn_weights folded into the search kernel's epilogue (same dist2 / idx, weight (b,n,3) as the
 * two-launch form, bit for bit): what the FP modules of ws3d_amd/fastpath.py call.                              */
WS3D_API int ws3d_three_nn_w(int b, int n, int m, const float *unknown, const float *known, float *dist2, int32_t *idx, float *weight,
                             const void *sorted_known, ws3d_stream_t stream);
/* ws3d_three_nn_w with its QUERIES taken in cell order: sorted_unknown = a binned copy of `unknown` (ws3d_sort_points_x / _grid / _xz
 * of the same tensor, any flavour: only its n float4 {x, y, z, bits(index)} per scene are read) or NULL.  Lane i searches for the
 * i-th binned point and writes row bits(index): the rows of dist2 / idx / weight are those of ws3d_three_nn_w bit for bit (a
 * query's result does not depend on the lane that runs it; interpolate_gpu.cu:9-52), the lanes of a wave walk cells of similar
 * density.  Applies to the binned search (sorted_known given, 3 <= m <= 16384); 0 < n <= 16384 when sorted_unknown is given. */
WS3D_API int ws3d_three_nn_wq(int b, int n, int m, const float *unknown, const float *known, float *dist2, int32_t *idx, float *weight,
                              const void *sorted_known, const void *sorted_unknown, ws3d_stream_t stream);
/* Several ws3d_three_nn_wq searches in ONE launch (round 5): job k takes the (b, n[k], 3) queries unknown[k] against the binned known set
 * sorted_known[k] (ws3d_sort_points_xz / _x of a (b, m[k], 3) cloud, 3 <= m[k] <= 4096) and writes dist2[k], idx[k], weight[k] (b, n[k], 3);
 * sorted_unknown (NULL, or per job NULL / a binned copy of the queries: cell order).  At most 4 jobs; host arrays, read before the call
 * returns.  Same rows as one call per job (the FP modules of a network: 3 launches -> 1).                                              */
WS3D_API int ws3d_three_nn_jobs(int b, int njobs, const int *n, const int *m, const float *const *unknown, const void *const *sorted_known,
                                float *const *dist2, int32_t *const *idx, float *const *weight, const void *const *sorted_unknown,
                                ws3d_stream_t stream);

/* The SA module's pool over nsample (pointnet2_modules.py:50, F.max_pool2d(kernel_size=[1, nsample]))
 * with the position of the maximum kept for the backward pass.  x (rows, nsample) -- the contiguous
 * (B,C,npoint,nsample) activation with rows = B*C*npoint -- -> out (rows), arg (rows) u8.  Window
 * scan rule `v > best || isnan(v)`: first position of the maximum, NaN propagates.  nsample <= 255.
 * _grad: grad_x (rows, nsample) = grad_out at arg, 0 elsewhere (every element written).
 * ws3d extension (replaces the library max-pool kernels in the training step).                  */
WS3D_API int ws3d_pool_nsample(long rows, int nsample, const float *x, float *out, uint8_t *arg, ws3d_stream_t stream);
WS3D_API int ws3d_pool_nsample_grad(long rows, int nsample, const float *grad_out, const uint8_t *arg, float *grad_x,
                                    ws3d_stream_t stream);

/* Last SharedMLP layer of a set-abstraction scale fused with the pool over nsample (ws3d extension, replaces
 * addmm + ws3d_rowmax_rows): out[g, 0:o] = act(max over the nsample rows of group g of x_rows . wt + bias).
 * x_rows (rows, k) row-major, wt (k, o) = W^T, rows % 64 == 0, o % 64 == 0, k % 4 == 0, nsample 16 or 32;
 * out (rows/nsample, o) with row stride out_stride.  fp32 matrix cores, fp32 accumulate.
 * WS3D_E_UNSUPPORTED for other shapes (the caller keeps the two-launch path).                       */
WS3D_API int ws3d_gemm_pool(long rows, int nsample, int k_dim, int o_dim, const float *x_rows, const float *wt,
                            const float *bias, int relu, float *out, int out_stride, const int32_t *gate, long gate_limit, ws3d_stream_t stream);

/* First SharedMLP layer of a set-abstraction scale with the grouping fused into the GEMM's A operand (no reference
 * counterpart; replaces QueryAndGroup -> Conv2d(1x1)+BN+ReLU, pointnet2_utils.py:241-264 + pytorch_utils.py:20-32, on
 * channels-last tensors): out (b*m*nsample, o) = relu?([feats[nbr] | xyz[nbr] - new_xyz] @ wt + bias) with feats (b,n,c),
 * xyz (b,n,3), new_xyz (b,m,3), nbr (b,m,nsample) int32 (ws3d_ball_query), wt (c+3, o) row-major with the three xyz rows
 * LAST, on the fp32 matrix cores.  c % 4 == 0, o % 64 == 0, b*m*nsample % 64 == 0, else WS3D_E_UNSUPPORTED.        */
WS3D_API int ws3d_gather_gemm(int b, int n, int m, int nsample, int c_feat, int o_dim, const float *feats, const float *xyz,
                     const float *new_xyz, const int32_t *nbr, const float *wt, const float *bias, int relu, float *out,
                     ws3d_stream_t stream);

/* The first TWO SharedMLP layers of a set-abstraction scale in one kernel (no reference counterpart): layer 1 as
 * ws3d_gather_gemm, its activation tile kept on chip, layer 2 (o1 -> o2) multiplied out of it:
 * out (b*m*nsample, o2) = relu2?(relu1?([f[nbr] | xyz[nbr] - centre] @ w1t + b1) @ w2t + b2).  w1t (c_feat+3, o1) with the
 * three coordinate rows LAST, w2t (o1, o2), both row-major.  o1 in {64, 128, 256}, o2 % 4 == 0, c_feat % 4 == 0,
 * rows % 64 == 0, else WS3D_E_UNSUPPORTED.                                                                             */
WS3D_API int ws3d_gather_gemm2(int b, int n, int m, int nsample, int c_feat, int o1, int o2, const float *feats, const float *xyz,
                      const float *new_xyz, const int32_t *nbr, const float *w1t, const float *b1, int relu1, const float *w2t,
                      const float *b2, int relu2, float *out, ws3d_stream_t stream);

/* Layer 1 of a set-abstraction SharedMLP without its per-pair product: W [f_j ; x_j - c] = W_f f_j + W_x (x_j - c), and
 * P = feats @ W_f (b * n rows, o1 columns at row stride p_stride: ONE GEMM over the points of a scene, by the caller) replaces the
 * product over the b * m * nsample (centre, sample) pairs.  Per pair: gather P's row of the neighbour, add the three-term xyz
 * product (w1x (3, o1): the x, y, z rows of W^T; centred coordinates, as pointnet2_utils.py:255-258) + b1, ReLU.
 *   ws3d_pgather_gemm2: ... then layer 2 (w2t (o1, o2)) as in ws3d_gather_gemm2 -> out (rows, o2); o1 in {64, 128}, m * nsample % 64
 *   ws3d_pgather_rows:  layer 1 alone -> out (rows, o1); o1 % 4, P / w1x / b1 / out 16-byte aligned
 * Same function as ws3d_gather_gemm(2) up to fp32 summation order.  ws3d extension, used by ws3d_amd/fastpath.py.          */
WS3D_API int ws3d_pgather_gemm2(int b, int n, int m, int nsample, int o1, int o2, const float *pmat, int p_stride, const float *xyz,
                       const float *new_xyz, const int32_t *nbr, const float *w1x, const float *b1, int relu1,
                       const float *w2t, const float *b2, int relu2, float *out, const int32_t *gate, long gate_limit, ws3d_stream_t stream);
WS3D_API int ws3d_pgather_rows(int b, int n, int m, int nsample, int o1, const float *pmat, int p_stride, const float *xyz, const float *new_xyz,
                      const int32_t *nbr, const float *w1x, const float *b1, int relu1, float *out, ws3d_stream_t stream);

/* First layer of a feature-propagation module without its product over the interpolated channels: interpolation is linear,
 * so Q = known_feats @ W_a (b * m rows, o columns, by the caller: a product over the KNOWN points) is interpolated instead of the
 * features:  out[r, :] = relu?( w0 Q[i0] + w1 Q[i1] + w2 Q[i2] + lin[r, :] )  with lin = skip @ W_b + bias (rows, o) from the
 * caller, or, lin == NULL and c1 <= 4 skip channels, skip (rows, c1) @ wb (c1, o) + bias evaluated inside.  idx / weight
 * (b, n, 3) as three_interpolate's (interpolate.cpp:37-56).  o % 4 == 0, float pointers 16-byte aligned.  Same function as
 * ws3d_interp_gemm up to fp32 summation order.  ws3d extension, used by ws3d_amd/fastpath.py.                              */
WS3D_API int ws3d_qinterp_rows(int b, int n, int m, int o, const float *q, const int32_t *idx, const float *weight, const float *lin,
                      const float *skip, int c1, const float *wb, const float *bias, int relu, float *out, ws3d_stream_t stream);

/* Launch gates (device-side dispatch between the compact and the dense form of a SharedMLP; ABI version 2).  Both forms are exact;
 * which one is faster depends on how full the ball-query lists are (break-even ~55 % distinct rows), a number that only exists
 * on the device and changes per batch -- a captured hipGraph cannot branch on the host.  So the caller launches BOTH forms and
 * every kernel of a form reads the pair total in its prologue:
 *   compact kernels (ws3d_pgather_gemm2_compact, ws3d_gemm_pool_compact, ws3d_pgather_gemm3_compact, ws3d_sa_mlp3_pool_compact): `limit` -- run iff *total <= limit
 *                  (limit < 0: always);
 *   dense kernels   (ws3d_pgather_gemm2, ws3d_gemm_pool, ws3d_sa_mlp3_pool_lists): `gate`, `gate_limit` -- run iff *gate > gate_limit
 *                  (gate == NULL: always), gate = the `total` word of ws3d_compact_pairs.
 * The form that does not run costs one launch whose workgroups return at once.  Exactly one of the two writes the result; with
 * the same limit on both sides the decision is consistent whatever the total.                                                 */

/* Compact (centre, sample) pairs.  A ball-query list holds its hits in ascending order, padded with the first one
 * (ball_query_gpu.cu:29-44); a padded row repeats row 0 of its centre in every SharedMLP layer and cannot change the maximum over
 * nsample, so the layers may run over the DISTINCT pairs only -- bit-identical results.
 *   ws3d_compact_pairs_count: cnt[c] = number of distinct neighbours of centre c (centres = b * m rows of nbr (centres, nsample))
 *   ws3d_compact_pairs_rows:  with incl = the INCLUSIVE prefix sum of cnt (by the caller): rowc[t] / rowsrc[t] = centre / source
 *                             point of compact row t, *total = incl[centres - 1]; rowc, rowsrc hold centres * nsample ints
 *   ws3d_pgather_gemm2_compact: ws3d_pgather_gemm2 over the compact rows (o1 in {64, 128, 256}) -> out (total rows, o2); launched for max_rows rows,
 *                             workgroups beyond *total return at once
 *   ws3d_gemm_pool_compact:   last layer + ReLU + max over each centre's rows by integer atomic max into out[centre, 0:o_dim]
 *                             (row stride out_stride), which the caller ZEROES first; the layer must end in a ReLU
 *   ws3d_pgather_gemm3_compact: the two above in ONE kernel (o1 in {64, 128}, o3 % 128 == 0, layer 2's tile kept in LDS: WS3D_E_UNSUPPORTED
 *                             beyond 159 KB): out[centre, 0:o3] by integer atomic max, bit-identical to the two-kernel form
 * ws3d extensions, used by ws3d_amd/fastpath.py.                                                                          */
 /* ws3d_compact_pairs: count + placement in ONE launch (*total must be ZERO on entry; the order of the compact rows is then arrival
 *  order of the 256-centre workgroups -- undefined, and irrelevant to every consumer above) */
WS3D_API int ws3d_compact_pairs(long centres, int nsample, const int32_t *nbr, int32_t *rowc, int32_t *rowsrc, int32_t *total, ws3d_stream_t stream);
WS3D_API int ws3d_compact_pairs_count(long centres, int nsample, const int32_t *nbr, int32_t *cnt, ws3d_stream_t stream);
WS3D_API int ws3d_compact_pairs_rows(long centres, int nsample, const int32_t *nbr, const int32_t *cnt, const int32_t *incl, int32_t *rowc,
                            int32_t *rowsrc, int32_t *total, ws3d_stream_t stream);
WS3D_API int ws3d_pgather_gemm2_compact(int b, int n, int m, long max_rows, int o1, int o2, const float *pmat, int p_stride, const float *xyz,
                               const float *new_xyz, const int32_t *rowc, const int32_t *rowsrc, const int32_t *total, const float *w1x,
                               const float *b1, int relu1, const float *w2t, const float *b2, int relu2, float *out, long limit, ws3d_stream_t stream);
WS3D_API int ws3d_pgather_gemm3_compact(int b, int n, int m, long max_rows, int o1, int o2, int o3, const float *pmat, int p_stride, const float *xyz,
                               const float *new_xyz, const int32_t *rowc, const int32_t *rowsrc, const int32_t *total, const float *w1x,
                               const float *b1, int relu1, const float *w2t, const float *b2, int relu2, const float *w3t, const float *b3,
                               float *out, int out_stride, long limit, ws3d_stream_t stream);
WS3D_API int ws3d_gemm_pool_compact(long max_rows, int k_dim, int o_dim, const float *x_rows, const int32_t *rowc, const int32_t *total,
                           const float *wt, const float *bias, float *out, int out_stride, long limit, ws3d_stream_t stream);
/* The two scales of a set-abstraction level in ONE launch (round 5).  Each block restates the arguments of the single-scale entries:
 * kind 3 = ws3d_pgather_gemm3_compact on both blocks, kind 2 = ws3d_pgather_gemm2_compact (its rows go to `mid`, (max_rows, o2)),
 * kind 1 = ws3d_gemm_pool_compact (x_rows = mid, k = o2, o = o3, wt = w3t, bias = b3).  Both blocks must name the same o1 (kinds 3, 2);
 * pmat already points at the scale's first column.  Same results as the two single-scale launches.                                 */
typedef struct ws3d_compact_mlp_args {
    int b, n, m;
    long max_rows;
    int o1, o2, o3;
    const float *pmat;
    int p_stride;
    const float *xyz, *new_xyz;
    const int32_t *rowc, *rowsrc, *total;
    const float *w1x, *b1;
    int relu1;
    const float *w2t, *b2;
    int relu2;
    const float *w3t, *b3;
    float *mid;
    float *out;
    int out_stride;
    long limit;
} ws3d_compact_mlp_args;
WS3D_API int ws3d_compact_mlp_pair(int kind, const ws3d_compact_mlp_args *scale0, const ws3d_compact_mlp_args *scale1, ws3d_stream_t stream);
/* The same function as kind 3 (three layers + pool of one or two scales over their compact rows; scale1 may be NULL) on the round-6
 * kernel (csrc/chain_mlp.hip, ABI 6): a wave owns 32 rows from the gather to the pooled atomics, the activations stay in registers
 * between the layers (transposed products + v_permlane32_swap), the weights of both scales are resident in LDS, 32-row tiles are handed
 * out by ticket counters.  blob0 / blob1: the scales' weights packed by ws3d_chain_mlp3_pack (once per weight set,
 * ws3d_chain_mlp3_blob_floats(o2) floats, 16-byte aligned); ticket: ws3d_chain_mlp3_ticket_ints() int32, ZERO on entry, consumed.
 * Covered: o1 = 64, o2 <= 96, o3 = 128, 16-byte aligned P rows (SA2 of the Stage-1 network: pointnet2_msg.py's MLPS[1]); anything else
 * WS3D_E_UNSUPPORTED, nothing launched.  workgroups: 0 = one per compute unit.  Pooled rows bit-identical to
 * ws3d_pgather_gemm3_compact's (the same fmaf chains in the same k order). */
WS3D_API int ws3d_chain_mlp3_ticket_ints(void);
WS3D_API size_t ws3d_chain_mlp3_blob_floats(int o2);
WS3D_API int ws3d_chain_mlp3_pack(const ws3d_compact_mlp_args *scale, float *blob, ws3d_stream_t stream);
WS3D_API int ws3d_chain_mlp3(const ws3d_compact_mlp_args *scale0, const ws3d_compact_mlp_args *scale1, const float *blob0, const float *blob1,
                             int32_t *ticket, int workgroups, ws3d_stream_t stream);

/* ws3d_sa_mlp3_pool over compact pairs (see ws3d_compact_pairs_*): the first level's three-layer SharedMLP (16-16-32 or 32-32-64,
 * every layer with bias + ReLU) on rows [x_j - c, f_j] built here from xyz (b, n, 3), new_xyz (b, m, 3) and the ONE feature
 * channel feat (b, n); max over each centre's rows by integer atomic max into out[centre, 0:c3] (row stride out_stride), which
 * the caller ZEROES.  Other widths return WS3D_E_UNSUPPORTED.  ws3d extension, used by ws3d_amd/fastpath.py.               */
WS3D_API int ws3d_sa_mlp3_pool_compact(int b, int n, int m, long max_rows, int c1, int c2, int c3, const float *xyz, const float *new_xyz,
                              const float *feat, const int32_t *rowc, const int32_t *rowsrc, const int32_t *total, const float *w1t,
                              const float *b1, const float *w2t, const float *b2, const float *w3t, const float *b3, float *out,
                              int out_stride, long limit, ws3d_stream_t stream);

/* The same three layers + pool over ALL rows of the neighbour lists nbr (b, m, nsample), rows built here like above (no grouped
 * tensor), the pool over registers and STORED (no atomics, out need not be zeroed): replaces ws3d_query_and_group_nlc +
 * ws3d_sa_mlp3_pool, bit-identical to it and to the compact form.  nsample 16 | 32, widths 16-16-32 | 32-32-64.              */
WS3D_API int ws3d_sa_mlp3_pool_lists(int b, int n, int m, int nsample, int c1, int c2, int c3, const float *xyz, const float *new_xyz,
                            const float *feat, const int32_t *nbr, const float *w1t, const float *b1, const float *w2t, const float *b2,
                            const float *w3t, const float *b3, int relu3, float *out, int out_stride, const int32_t *gate, long gate_limit,
                            ws3d_stream_t stream);

/* First layer of a feature-propagation module with three_interpolate and the skip concatenation fused into the GEMM's A
 * operand (no reference counterpart; replaces three_interpolate -> torch.cat -> Conv2d(1x1)+BN+ReLU,
 * pointnet2_modules.py:138-155, on channels-last tensors): out (b*n, o) = relu?([w0 f[i0] + w1 f[i1] + w2 f[i2] | u] @ wt +
 * bias) with f = known_feats (b,m,c2), u = unknown_feats (b,n,c1) or NULL (c1 = 0), idx / weight (b,n,3) from ws3d_three_nn
 * + ws3d_three_nn_weights, wt (c2+c1, o) row-major.  c2 % 4 == 0, o % 64 == 0, b*n % 64 == 0, else WS3D_E_UNSUPPORTED. */
WS3D_API int ws3d_interp_gemm(int b, int n, int m, int c2, int c1, int o_dim, const float *known_feats, const float *unknown_feats,
                     const int32_t *idx, const float *weight, const float *wt, const float *bias, int relu, float *out,
                     ws3d_stream_t stream);

/* Weight gradient of a 1x1 convolution on channels-first tensors (the Conv1d / Conv2d of every SharedMLP
 * block, pytorch_utils.py:35-101): grad_w (o, c) = sum_b sum_l grad_out[b, o, l] * x[b, c, l].  fp32 matrix
 * cores, the (scene, l-range) slices of the sum are added in a fixed order: bit-reproducible (the library's
 * split-K kernels use atomics).  workspace: ws3d_conv1x1_wgrad_workspace_bytes(b, o, c, l) bytes.  ws3d extension. */
WS3D_API size_t ws3d_conv1x1_wgrad_workspace_bytes(int b, int o, int c, long l);
WS3D_API int ws3d_conv1x1_wgrad(int b, int o, int c, long l, const float *grad_out, const float *x, float *grad_w,
                                void *workspace, size_t workspace_bytes, ws3d_stream_t stream);

/* Training-mode BatchNorm (+ ReLU) of a channels-first activation x (b, c, l) -- the norm + activation
 * of every conv -> BatchNorm -> ReLU block of the reference (pytorch_utils.py:35-101, nn.BatchNorm1d/2d
 * in train() mode followed by nn.ReLU).  fwd: batch statistics per channel over b*l values (biased
 * variance for the normalisation, unbiased for running_var), y = relu(((x-mean)*invstd)*gamma+beta),
 * running_mean/var (nullable) updated with `momentum`, *num_batches_tracked (nullable, one int64 on
 * the device) incremented, save_mean/save_invstd (c) kept for bwd.
 * bwd: dx (b,c,l), dgamma (c), dbeta (c) from dy; the ReLU mask is re-derived from x.  relu = 0: plain
 * BatchNorm.  Reductions run in a fixed order (fp64 partials): bit-reproducible run to run.
 * workspace: ws3d_bn_workspace_bytes(b, c, l) bytes, 8-byte aligned.  ws3d extension (replaces the
 * library BatchNorm + ReLU kernels in the training step).                                        */
WS3D_API size_t ws3d_bn_workspace_bytes(int b, int c, long l);
WS3D_API int ws3d_bn_relu_train_fwd(int b, int c, long l, const float *x, const float *gamma, const float *beta, float eps,
                                    float momentum, int relu, float *running_mean, float *running_var,
                                    int64_t *num_batches_tracked, float *y, float *save_mean, float *save_invstd,
                                    void *workspace, size_t workspace_bytes, ws3d_stream_t stream);
WS3D_API int ws3d_bn_relu_train_bwd(int b, int c, long l, const float *x, const float *dy, const float *gamma,
                                    const float *beta, const float *save_mean, const float *save_invstd, int relu, float *dx,
                                    float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, ws3d_stream_t stream);

/* three_interpolate_wrapper(b,c,m,n,points,idx,weight,out)   interpolate.cpp:26-39 ->
 * interpolate_gpu.cu:77-117.  points (b,c,m), idx/weight (b,n,3) -> out (b,c,n).    */
WS3D_API int ws3d_three_interpolate(int b, int c, int m, int n, const float *points, const int32_t *idx,
                           const float *weight, float *out, ws3d_stream_t stream);

/* three_interpolate_grad_wrapper(b,c,n,m,grad_out,idx,weight,grad_points)
 * interpolate.cpp:41-53 -> interpolate_gpu.cu:120-160.  grad_points pre-zeroed.     */
WS3D_API int ws3d_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out,
                                const int32_t *idx, const float *weight, float *grad_points,
                                ws3d_stream_t stream);

/* Deterministic backward.  Same results as the *_grad entry points above up to the
 * summation order, which is FIXED here: every gradient element is the sum of its contributions in
 * ascending slot order (slot = m*nsample+s, or point*3+k), i.e. bit-identical to the sequential
 * loop `for slot: dst[idx[slot]] += v[slot]` and to itself from run to run (the reference's float
 * atomicAdd scatter is neither).  grad_points is fully written (no pre-zeroing needed).
 * workspace: ws3d_scatter_workspace_bytes(b, c, n_targets, slots_per_scene) bytes of device memory,
 * n_targets = n (group/gather) or m (three_interpolate), slots_per_scene = npoints*nsample or n*3.
 * gather_points_grad == group_points_grad_det with nsample = 1.                                  */
WS3D_API size_t ws3d_scatter_workspace_bytes(int b, int c, int n_targets, long slots_per_scene);
WS3D_API int ws3d_group_points_grad_det(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                                        const int32_t *idx, float *grad_points, void *workspace,
                                        size_t workspace_bytes, ws3d_stream_t stream);
WS3D_API int ws3d_three_interpolate_grad_det(int b, int c, int n, int m, const float *grad_out, const int32_t *idx,
                                             const float *weight, float *grad_points, void *workspace,
                                             size_t workspace_bytes, ws3d_stream_t stream);

/* y[b,o,l] = relu?(y[b,o,l] + bias[o]) in place, one pass: the epilogue of the SharedMLP
 * (1x1 conv + eval-mode BatchNorm folded into one GEMM, pytorch_utils.py:20-101).  ws3d extension. */
WS3D_API int ws3d_bias_act_inplace(int b, int o_ch, long l, int relu, float *y, const float *bias,
                                   ws3d_stream_t stream);

/* out[b,o,m] = relu?(max_s y[b,o,m,s] + bias[o]) (bias may be NULL): the set-abstraction pool
 * F.max_pool2d(new_features, kernel_size=[1, nsample]) (pointnet2_modules.py:51-58) fused with
 * the last SharedMLP layer's bias + ReLU, which commute with the max exactly.  ws3d extension. */
WS3D_API int ws3d_rowmax_bias_act(int b, int o_ch, long m, int s, int relu, const float *y, const float *bias,
                                  float *out, ws3d_stream_t stream);

/* Channels-last ("nlc") variants for a row-major SharedMLP chain (ws3d extension, ws3d_amd/fastpath.py):
 * features are (b, points, C) instead of the reference's (b, C, points); idx / xyz arguments and
 * every index result are identical to the channels-first entry points.
 *   ws3d_query_and_group_nlc : out (b, m, nsample, 3*use_xyz + c), row = [dx, dy, dz, features...]
 *   ws3d_three_interpolate_nlc: out row p = sum_k weight[p,k] * feats[idx[p,k], :], row stride out_stride
 *   ws3d_rowmax_rows          : out row r = max over rows r*ns .. r*ns+ns-1 of y (rows, o_ch)        */
WS3D_API int ws3d_query_and_group_nlc(int b, int n, int m, int c, float radius, int nsample, int use_xyz,
                                      const float *xyz, const float *new_xyz, const float *features_nlc,
                                      int32_t *idx_out, float *out_nlc, const void *sorted, ws3d_stream_t stream);
WS3D_API int ws3d_three_interpolate_nlc(int b, int c, int m, int n, const float *feats_nlc, const int32_t *idx,
                                        const float *weight, float *out_nlc, int out_stride, ws3d_stream_t stream);
WS3D_API int ws3d_rowmax_rows(long rows_out, int ns, int o_ch, const float *y, float *out, int out_stride,
                              ws3d_stream_t stream);

/* First SA level fused: x_rows4 (rows, 4) grouped columns [dx,dy,dz,f] -> three pointwise layers
 * (W^T row-major (in, out), BN folded; ReLU after layers 1, 2 and, if relu3, 3) -> max over each
 * group of nsample consecutive rows -> out (rows/nsample, c3) with row stride out_stride.  Widths
 * (c1,c2,c3) x nsample in {(16,16,32),(32,32,64)} x {16,32}; WS3D_E_UNSUPPORTED otherwise (the
 * caller then runs the GEMM chain).  ws3d extension, used by ws3d_amd/fastpath.py.               */
WS3D_API int ws3d_sa_mlp3_pool(long rows, int nsample, int c1, int c2, int c3, const float *x_rows4,
                               const float *w1t, const float *b1, const float *w2t, const float *b2,
                               const float *w3t, const float *b3, int relu3, float *out, int out_stride,
                               ws3d_stream_t stream);

/* Two pointwise layers on rows in one kernel, 128 -> 128 -> o2 (o2 <= 64; the RPN's classification and regression heads):
 * out (rows, o2) = relu2?(relu1?(x @ w1t + b1) @ w2t + b2), w1t (128, 128) and w2t (128, o2) row-major, biases may be NULL.
 * The (rows, 128) activation between the layers stays in registers (fp32 matrix cores).  rows % 32 == 0; other shapes
 * return WS3D_E_UNSUPPORTED (the caller runs two GEMMs).  ticket: one device int, ZERO on entry (consumed: it counts the
 * 32-row tiles handed out), or NULL for a static split of the rows over the workgroups -- slower when other streams hold
 * compute units.  ws3d extension, used by ws3d_amd/fastpath.py.                                                        */
WS3D_API int ws3d_mlp2_rows(long rows, int k_dim, int o1, int o2, const float *x_rows, const float *w1t, const float *b1, int relu1,
                   const float *w2t, const float *b2, int relu2, float *out, int *ticket, ws3d_stream_t stream);

/* The RPN's two heads in ONE launch on the bf16 matrix cores at fp32 accuracy (split product: DESIGN.md section 4):
 *   out_cls (rows, 1)  = relu2?(relu1?(x @ W1c + b1c) @ W2c + b2c),   out_reg (rows, o2) likewise with the regression head's weights,
 * x (rows, 128) row-major, rows % 32 == 0.  Each head's weights are packed once per weight set by ws3d_rpn_heads_pack into a device
 * blob of ws3d_rpn_heads_blob_bytes(o2) bytes (16-byte aligned; 0 = o2 not covered: 1 .. 64; the regression head takes o2 >= 2); w1t (128, 128)
 * and w2t (128, o2) as ws3d_mlp2_rows takes them, biases may be NULL.  heads: 1 = the classification head only (blob_cls, o2 = 1),
 * 2 = the regression head only, 3 = both in one launch.  ticket_cls / ticket_reg: one device int each, ZERO on entry (consumed).
 * workgroups: of the whole launch, 0 = one per CU.  Deterministic: the outputs do not depend on the order the tickets hand out the
 * tiles.  Other shapes return WS3D_E_UNSUPPORTED (the caller runs ws3d_mlp2_rows).  ws3d extension, used by ws3d_amd/fastpath.py. */
WS3D_API size_t ws3d_rpn_heads_blob_bytes(int o2);
WS3D_API int ws3d_rpn_heads_pack(int o2, const float *w1t, const float *b1, int relu1, const float *w2t, const float *b2, int relu2, void *blob,
                        ws3d_stream_t stream);
WS3D_API int ws3d_rpn_heads(long rows, const float *x_rows, int heads, const void *blob_cls, float *out_cls, int *ticket_cls, int o2_reg,
                   const void *blob_reg, float *out_reg, int *ticket_reg, int workgroups, ws3d_stream_t stream);

/* A plain row GEMM on the bf16 matrix cores at fp32 accuracy (split product: DESIGN.md section 4 item 8; csrc/gemm_rows.hip):
 *   out (rows, n_dim) = relu?( a (rows, k_dim) @ wt (k_dim, n_dim) + bias ),   a, wt, out fp32 row-major and contiguous, bias may be NULL.
 * wt is split ONCE per weight set by ws3d_gemm_rows_pack into a device image of ws3d_gemm_rows_pack_bytes(k_dim, n_dim) bytes (16-byte
 * aligned; 0 = shape not covered): three bf16 planes in the order the kernel's operand reads take them.  a is split inside the kernel.
 * No split-K and no atomics: every output element is summed by one wave in ascending k, so the launch geometry changes no bit.
 * Cover: rows % 64 == 0, k_dim % 32 == 0, n_dim % 64 == 0 (both <= 4096), a / pack / out / bias 16-byte aligned; anything else returns
 * WS3D_E_UNSUPPORTED with nothing launched (the caller runs the library GEMM).  ws3d extension, used by ws3d_amd/fastpath.py.        */
WS3D_API size_t ws3d_gemm_rows_pack_bytes(int k_dim, int n_dim);
WS3D_API int ws3d_gemm_rows_pack(int k_dim, int n_dim, const float *wt, void *pack, ws3d_stream_t stream);
WS3D_API int ws3d_gemm_rows_split(long rows, int k_dim, int n_dim, const float *a, const void *pack, const float *bias, int relu, float *out,
                         ws3d_stream_t stream);

/* Both layers of a two-layer feature-propagation module in one kernel (round 4): the first layer's rows are built in the A operand of the
 * second layer's product exactly as ws3d_qinterp_rows builds them,
 *   x = relu1?( w0 Q[i0] + w1 Q[i1] + w2 Q[i2] + (lin (b*n, c)  |  skip (b*n, c1 <= 4) @ wb (c1, c) + b1) ),   out (b*n, o) = relu2?( x @ w2t (c, o) + b2 )
 * q (b, m, c) = known_feats @ W_a; idx / weight (b, n, 3).  b*n % 64, c % 16, o % 128; otherwise WS3D_E_UNSUPPORTED (the caller runs
 * ws3d_qinterp_rows + a GEMM).  ws3d extension, used by ws3d_amd/fastpath.py.                                                          */
WS3D_API int ws3d_qinterp_gemm(int b, int n, int m, int c, int o_dim, const float *q, const int32_t *idx, const float *weight, const float *lin,
                      const float *skip, int c1, const float *wb, const float *b1, int relu1, const float *w2t, const float *b2, int relu2,
                      float *out, ws3d_stream_t stream);

/* -------------------------------------------------------------------- iou3d_cuda */

/* boxes_overlap_bev_gpu(boxes_a,boxes_b,ans)   iou3d.cpp:31-50 -> iou3d_kernel.cu:
 * 108-234,354-363.  boxes (N,5) [x1,y1,x2,y2,ry] -> ans (num_a,num_b) overlap area. */
WS3D_API int ws3d_boxes_overlap_bev(int num_a, const float *boxes_a, int num_b, const float *boxes_b,
                           float *ans, ws3d_stream_t stream);

/* boxes_iou_bev_gpu   iou3d.cpp:52-71 -> iou3d_kernel.cu:214-248,365-371.           */
WS3D_API int ws3d_boxes_iou_bev(int num_a, const float *boxes_a, int num_b, const float *boxes_b,
                       float *ans, ws3d_stream_t stream);

/* Additive to ABI 6.  The DIAGONAL of boxes_iou3d_gpu (lib/utils/iou3d/iou3d_utils.py:21-56) for n pairs boxes_a[i], boxes_b[i], each
 * (n,7) [x, y_bottom, z, h, w, l, ry]: overlap_bev[i], iou2d[i], iou3d[i], each (n).  One thread per pair on the device code of
 * ws3d_boxes_overlap_bev; the BEV corners, the height overlap and the two divisions (clamp(min=1e-7) included) are evaluated in the
 * kernel in torch's fp32 operation order, so all three outputs are bit for bit entry (i, i) of the n x n route -- n rotated
 * intersections instead of n * n.                                                                                                  */
WS3D_API int ws3d_boxes_iou3d_paired(int n, const float *boxes_a, const float *boxes_b, float *overlap_bev, float *iou2d, float *iou3d,
                                     ws3d_stream_t stream);

/* The K12/K13 mask alone (iou3d_kernel.cu:250-292 / 306-348): mask (n, ceil(n/64))
 * uint64, bit t of word c of row i = iou(box_i, box_{64c+t}) > thresh (diagonal
 * block: only t > i%64).  Words of blocks c < i/64 (never read by the sweep,
 * iou3d.cpp:108) are written as 0 unless full_grid != 0, in which case they are
 * computed like the reference grid does.  normal != 0 selects the axis-aligned IoU.  */
WS3D_API int ws3d_nms_mask(int boxes_num, const float *boxes, float thresh, int normal, int full_grid,
                  uint64_t *mask, ws3d_stream_t stream);

/* nms_gpu / nms_normal_gpu(boxes, keep, thresh) -> num_to_keep   iou3d.cpp:73-170.
 * boxes (n,5) already score-sorted (iou3d_utils.py:67-69).  The reference copies the
 * mask to the host and sweeps there; here mask kernel + greedy sweep both run on the
 * device: keep (n) int64 DEVICE, num_keep (1) int32 DEVICE -- no D2H, no sync.
 * max_keep > 0 stops the sweep after that many survivors (the first max_keep entries of
 * the reference's keep list; its callers slice [:RPN_POST_NMS_TOP_N]); <= 0 = all.
 * workspace: ws3d_nms_workspace_bytes(n) bytes of device memory.                     */
WS3D_API size_t ws3d_nms_workspace_bytes(int boxes_num);
WS3D_API int ws3d_nms(int boxes_num, const float *boxes, float thresh, int normal, int max_keep,
                      void *workspace, size_t workspace_bytes, int64_t *keep, int32_t *num_keep,
                      ws3d_stream_t stream);

/* The same for a batch of scenes in ONE launch pair: boxes (batch,n,5), keep (batch,n),
 * num_keep (batch); workspace >= batch * ws3d_nms_workspace_bytes(n).                      */
WS3D_API int ws3d_nms_batched(int batch, int boxes_num, const float *boxes, float thresh, int normal,
                              int max_keep, void *workspace, size_t workspace_bytes, int64_t *keep,
                              int32_t *num_keep, ws3d_stream_t stream);

/* ------------------------------------------------ Stage-1 proposal stage */

/* Greedy radius NMS of centre proposals, replacing the reference's Python loops
 * (generate_box_dataset.py:127-140, tools/eval_auto.py:270-284: one host sync per candidate).
 * centers (batch,n,2) = (x,z) per scene, sorted by descending score; candidate i is kept iff
 * distance_2 (lib/utils/distance.py:3, fp32) to every kept centre is > radius.  Outputs and
 * workspace as ws3d_nms_batched (workspace >= batch * ws3d_nms_workspace_bytes(n)).          */
WS3D_API int ws3d_radius_nms_batched(int batch, int n, const float *centers, float radius, int max_keep,
                                     void *workspace, size_t workspace_bytes, int64_t *keep,
                                     int32_t *num_keep, ws3d_stream_t stream);

/* Sorted top-k per scene (ws3d extension): scores (b, n), n <= 16384 -> the k largest in
 * descending order, out_scores (b, k) and out_idx (b, k) int64; equal scores in ascending index
 * order, NaN first (torch.topk's convention).                                                       */
WS3D_API int ws3d_topk_sorted(int b, int n, int k, const float *scores, float *out_scores, int64_t *out_idx,
                              ws3d_stream_t stream);
/* The same result with the sort of a scene spread over several workgroups (2048-key segments sorted side by side, then ranked
 * against each other): workspace >= ws3d_topk_workspace_bytes(b, n) bytes of device memory, 16-byte aligned; with a NULL / short
 * workspace, or n <= 2048 (ws3d_topk_workspace_bytes returns 0), it IS ws3d_topk_sorted.  At 16384 scores x 8 scenes: 107 -> ~25 us. */
WS3D_API size_t ws3d_topk_workspace_bytes(int b, int n);
WS3D_API int ws3d_topk_sorted_ws(int b, int n, int k, const float *scores, float *out_scores, int64_t *out_idx, void *workspace,
                                 size_t workspace_bytes, ws3d_stream_t stream);
/* The same two sorts over sigmoid(logits[i]) = 1 / (1 + exp(-x)) in fp32, torch.sigmoid's expression, evaluated while the keys are
 * loaded (round 5): the proposal stage then needs no score tensor and no sigmoid launch; out_scores holds the sigmoid values. */
WS3D_API int ws3d_topk_sorted_sigmoid(int b, int n, int k, const float *logits, float *out_scores, int64_t *out_idx, ws3d_stream_t stream);
WS3D_API int ws3d_topk_sorted_sigmoid_ws(int b, int n, int k, const float *logits, float *out_scores, int64_t *out_idx, void *workspace,
                                         size_t workspace_bytes, ws3d_stream_t stream);

/* Proposal decode (ws3d extension): xyz (b,n,3), rpn_reg (b,n,4*bins) -> boxes (b,n,7)
 * = [x + dx, y + h/2, z + dz, h, w, l, ry] with (dx, dz) = decode_center_target
 * (lib/utils/bbox_transform.py:24-61) and ry the per-index synthetic heading of
 * ws3d_amd.stage1.synthetic_orientation; bit-identical to the torch composition.          */
WS3D_API int ws3d_decode_center_boxes(int b, int n, int bins, float loc_scope, float loc_bin_size, float h, float w,
                                      float l, const float *xyz, const float *rpn_reg, float *boxes,
                                      ws3d_stream_t stream);

/* Glue of the on-device proposal stage (no reference counterpart: the reference does these steps in Python around its ops,
 * kitti_utils.py:134-160, roipool3d_utils.py:19, generate_box_dataset.py:92-140).
 * ws3d_gather_boxes_bev: box (b,n,7), order (b,top) int64 -> box_sorted (b,top,7) = box[order] and bev (b,top,5) =
 * [x - l/2, z - w/2, x + l/2, z + w/2, ry] (boxes3d_to_bev).                                                        */
WS3D_API int ws3d_gather_boxes_bev(int b, int n, int top, const float *box, const int64_t *order, float *box_sorted, float *bev,
                          ws3d_stream_t stream);
/* ws3d_decode_center_boxes + ws3d_gather_boxes_bev in one launch (round 5): only the `top` points that order (b, top) names are decoded
 * (same arithmetic, bit-identical rows), written in that order with their BEV rectangles; no (b, n, 7) tensor of every point's box. */
WS3D_API int ws3d_decode_gather_boxes_bev(int b, int n, int top, int bins, float loc_scope, float loc_bin_size, float h, float w, float l,
                                          const float *xyz, const float *rpn_reg, const int64_t *order, float *box_sorted, float *bev,
                                          ws3d_stream_t stream);
/* ws3d_select_proposals: keep (b,keep_stride) int64 / num (b) int32 from ws3d_nms_batched on score-sorted boxes -> the
 * first min(num, k) survivors as boxes_out (b,k,7) and scores_out (b,k), zero-padded (row * 0 for the padding, as the
 * torch composition does), count (b) int64, and (optional) pooled_boxes (b,k,7) = enlarge_box3d(boxes_out, extra_width). */
WS3D_API int ws3d_select_proposals(int b, int top, int keep_stride, int k, const float *box_sorted, const float *scores_sorted,
                          const int64_t *keep, const int32_t *num, float extra_width, float *boxes_out, float *scores_out,
                          int64_t *count, float *pooled_boxes, ws3d_stream_t stream);
/* ... and additionally packed (b, k, 8) rows = box + score (or NULL): what the multi-GPU gather sends (ws3d_amd/dist.py), written here
 * instead of by a concatenation launch (round 5). */
WS3D_API int ws3d_select_proposals_packed(int b, int top, int keep_stride, int k, const float *box_sorted, const float *scores_sorted,
                                          const int64_t *keep, const int32_t *num, float extra_width, float *boxes_out, float *scores_out,
                                          int64_t *count, float *pooled_boxes, float *packed, ws3d_stream_t stream);
/* ... the packed rows written straight into the multi-GPU exchange's send buffer (round 6, ABI 6): scene i's k rows of 8 floats at
 * send + i * send_stride, the scene's count as the float behind them (send_stride >= k * 8 + 1 floats; counts < 2^24 are exact), so
 * that the step's one all-gather (ws3d_amd/dist.py ProposalExchange; replaces nn.DataParallel's gather, tools/train_rpn.py:175-176)
 * sends a buffer no other launch packs. */
WS3D_API int ws3d_select_proposals_send(int b, int top, int keep_stride, int k, const float *box_sorted, const float *scores_sorted,
                                        const int64_t *keep, const int32_t *num, float extra_width, float *boxes_out, float *scores_out,
                                        int64_t *count, float *pooled_boxes, float *send, long send_stride, ws3d_stream_t stream);
/* The step's prologue in one launch (round 5): the (rows, c) input rows, c >= 3, split into xyz (rows, 3) and feats (rows, c - 3), and
 * clear_bytes bytes at `clear` zeroed (16-byte aligned and a multiple of 16; 0: nothing) -- the pass's zero-initialised scratch. */
WS3D_API int ws3d_split_points_clear(long rows, int c, const float *pc, float *xyz, float *feats, void *clear, size_t clear_bytes,
                                     ws3d_stream_t stream);

/* ---------------------------------------------------------------- roipool3d_cuda */

/* forward(xyz,boxes3d,pts_feature,pooled_features,pooled_empty_flag)
 * roipool3d.cpp:48-79 -> roipool3dLauncher roipool3d_kernel.cu:209-237 (K14-K16);
 * forward_slow (roipool3d.cpp:15-44) has identical results.
 * xyz (B,N,3), boxes3d (B,M,7) [x,y_bottom,z,h,w,l,ry] (already enlarged by the
 * caller, roipool3d_utils.py:19), pts_feature (B,N,C) -> pooled_features
 * (B,M,S,3+C) and pooled_empty_flag (B,M) int32, BOTH pre-zeroed by the caller
 * (roipool3d_utils.py:21-23): rows of empty boxes are left untouched.
 * pts_idx (B,M,S) int32 may be NULL; when given it receives the selected point
 * indices (the reference's internal pts_idx scratch; zeros for empty boxes).
 * No B*N*M scratch, no allocation: selection and copy are fused per box.             */
WS3D_API int ws3d_roipool3d(int batch_size, int pts_num, int boxes_num, int feature_in_len,
                   int sampled_pts_num, const float *xyz, const float *boxes3d,
                   const float *pts_feature, float *pooled_features, int32_t *pooled_empty_flag,
                   int32_t *pts_idx, ws3d_stream_t stream);
/* Same result, but EVERY element of pooled_features / pooled_empty_flag (/ pts_idx) is written: no
 * pre-zeroing by the caller (the wrapper's zero-fill is a 214 MB memset per 8 scenes at the C3 shapes;
 * here only the rows of empty boxes are zeroed, by the workgroup that found the box empty).        */
WS3D_API int ws3d_roipool3d_fill(int batch_size, int pts_num, int boxes_num, int feature_in_len,
                   int sampled_pts_num, const float *xyz, const float *boxes3d,
                   const float *pts_feature, float *pooled_features, int32_t *pooled_empty_flag,
                   int32_t *pts_idx, ws3d_stream_t stream);

/* ws3d_roipool3d / ws3d_roipool3d_fill (fill != 0) with a caller-provided scratch buffer: for scenes of
 * ws3d_roipool3d_workspace_bytes(batch, pts_num) > 0 bytes (16384 <= pts_num <= 262144) the scene is counting-sorted once into an
 * (x, z) grid inside `workspace` and every box tests only the cells under its footprint (roipool3d.hip: roi_bin_kernel +
 * roipool3d_binned_kernel; the first-S-by-point-index rule of roipool3d_kernel.cu:97-160 is kept by a radix select on the index).
 * Same outputs as ws3d_roipool3d bit for bit; workspace NULL / too small / not applicable: the scanning kernels run.
 * 16-byte aligned, contents undefined on return; nothing is allocated or synchronised.  ws3d extension (round 5, ABI 5). */
WS3D_API size_t ws3d_roipool3d_workspace_bytes(int batch_size, int pts_num);
WS3D_API int ws3d_roipool3d_ws(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num, const float *xyz,
                               const float *boxes3d, const float *pts_feature, float *pooled_features, int32_t *pooled_empty_flag,
                               int32_t *pts_idx, int fill, void *workspace, size_t workspace_bytes, ws3d_stream_t stream);


/* Device twin of pts_in_boxes3d_cpu (roipool3d.cpp:97-124): pts (N,3), boxes3d (M,7)
 * -> flag (M,N) int64 in {0,1}.                                                      */
WS3D_API int ws3d_pts_in_boxes3d(int boxes_num, int pts_num, const float *pts, const float *boxes3d,
                        int64_t *flag, ws3d_stream_t stream);

/* ------------------------------------------------- Stage-2 instance clouds (no reference op: Python loops) */

/* The cut between Stage 1 and Stage 2.  In the reference every centre kept by the radius NMS becomes an instance cloud: the scene
 * points whose (x, z) distance to the centre is below 4.0 m, in scene order, shifted to the centre, with reflectance and a per-point
 * score channel (generate_box_dataset.py:197-229, 293-307 stores them; tools/eval_auto.py:286-292, 323-372 feeds each to rcnn_forward;
 * lib/datasets/kitti_boxplace_dataset.py:327-342 brings a stored cloud to 512 rows).  Both drivers use an (N x K) distance matrix and
 * a Python loop over the centres with boolean-mask indexing; here one launch serves a batch.  Additive to ABI 6.
 *   pts (B,N,4) x, y, z, reflectance; score (B,N) sigmoid of rpn_cls; feats (B,N,C) channels-last or NULL with C = 0 (C % 4 == 0,
 *   16-byte aligned); centres (B,K,3) -- the caller chooses the y it is shifted by: 0 reproduces generate_box_dataset.py:226, 1.65
 *   tools/eval_auto.py:323; num (B) int32 valid centre slots per scene or NULL (all K).
 *   member: sqrtf(dx*dx + dz*dz) < radius, dx = cx - px, dz = cz - pz, nothing contracted (lib/utils/distance.py:3); NaN = outside.
 *   row of a member: (px - cx, py - cy, pz - cz, reflectance, m), m = score (mask_mode 0, generate_box_dataset.py:222) or
 *   (score > mask_thresh ? 1 : 0) - 0.5 (mask_mode 1, tools/eval_auto.py:345, 367); members in ascending point index.
 * Fixed form: cloud (B,K,S,5), cloud_feats (B,K,S,C) (with features), count (B,K) int32 = the TRUE number of members (not capped at S),
 * pts_idx (B,K,S) int32 or NULL.  With t = min(count, S): row j < t is the j-th member, row j >= t repeats row j mod t
 * (kitti_boxplace_dataset.py:327-337).  count == 0 and every slot k >= num[b]: all-zero rows, count 0, pts_idx 0.  EVERY output element
 * is written (the ws3d_roipool3d_fill convention).  No allocation, no host synchronisation, no atomics; capturable.
 * B or K == 0: nothing to do; N == 0: the zeros are written.  S * 24 bytes of LDS: S <= 6400.                                        */
WS3D_API int ws3d_instance_clouds(int batch, int pts_num, int centres_num, int feat_len, int sampled_pts_num, float radius, int mask_mode,
                                  float mask_thresh, const float *pts, const float *score, const float *feats, const float *centres,
                                  const int32_t *num, float *cloud, float *cloud_feats, int32_t *count, int32_t *pts_idx,
                                  ws3d_stream_t stream);
/* Ragged form, what generate_box_dataset.py:220-229 stores and tools/eval_auto.py:341-372 feeds.  ws3d_instance_clouds_count writes
 * count (B,K) int32 (0 for slots k >= num[b]); the caller forms offsets (B*K + 1) int64, the exclusive prefix sum in (b, k) order, and
 * allocates; ws3d_instance_clouds_emit writes rows (total,5), row_feats (total,C) (with features) and row_idx (total) int32 or NULL:
 * centre (b, k)'s members at offsets[b*K + k] ... in ascending point index.  A row that would fall at or past offsets[b*K + k + 1]
 * is dropped, so offsets that no longer match the inputs cannot make the launch write outside a centre's range.                      */
WS3D_API int ws3d_instance_clouds_count(int batch, int pts_num, int centres_num, float radius, const float *pts, const float *centres,
                                        const int32_t *num, int32_t *count, ws3d_stream_t stream);
WS3D_API int ws3d_instance_clouds_emit(int batch, int pts_num, int centres_num, int feat_len, float radius, int mask_mode, float mask_thresh,
                                       const float *pts, const float *score, const float *feats, const float *centres, const int32_t *num,
                                       const int64_t *offsets, float *rows, float *row_feats, int32_t *row_idx, ws3d_stream_t stream);

/* ------------------------------------------------- click-driven annotation (no reference op: host numpy / torch) */

/* The front of tools/eval_active.py (:187, 198-209, 656-675) for a padded batch: BEV clicks -> a soft foreground score per scene
 * point and the jittered candidate centres that ws3d_instance_clouds then cuts around.  Additive to ABI 6.
 *   pts (B,N,4); clicks (B,K,3), a click's y is never read; num (B) int32 clicks per scene or NULL (all K), clamped to 0..K;
 *   offsets: side floats in HOST memory, 1 <= side <= 9, the jitter grid's steps (the reference: 0.1 * (m - 2), m = 0..4).
 *   score (B,N) = click_gaussian_mask (:656-675) in fp32, nothing contracted: yh = py * gauss_height; per click k < num[b]
 *   d = sqrtf((dx*dx + yh*yh) + dz*dz) with dx = px - cx, dz = pz - cz, t = clamp(d - gauss_status, 0, 100); near = min over k
 *   starting from 100; score = expf(-0.5f * near * near / gauss_cov).  A scene without clicks scores expf(-5000 / gauss_cov)
 *   everywhere, exactly 0 for the reference's gauss_cov = 1.5.
 *   cand (B, side*side*K, 3) in the reference's order (:202-209, whole click lists concatenated, x offset outer, z offset inner):
 *   slot j < side*side*num[b], g = j / num[b], k = j % num[b]: (cx_k + offsets[g / side], centre_y, cz_k + offsets[g % side]),
 *   fp32 additions; slots at or past side*side*num[b] are all zero.  cand_num (B) int32 = side*side*num[b].
 * EVERY output element is written.  No allocation, no host synchronisation, no atomics; two launches, capturable.  B == 0: nothing to
 * do; K == 0: score and cand_num are written (zeros for gauss_cov = 1.5); N == 0: only cand / cand_num are written.  Non-finite
 * inputs give unspecified values.                                                                                                    */
WS3D_API int ws3d_click_prepare(int batch, int pts_num, int clicks_num, int side, const float *offsets, float gauss_height, float gauss_status,
                                float gauss_cov, float centre_y, const float *pts, const float *clicks, const int32_t *num, float *score,
                                float *cand, int32_t *cand_num, ws3d_stream_t stream);

/* ------------------------------------------------- KITTI evaluation (kitti_object_eval_python) */

/* Frames are CSR ranges: gt_off / dt_off (frames + 1) int32 offsets of each frame's ground truths / detections, out_off (frames + 1)
 * int64 offset of each frame's (n_dt x n_gt) overlap block (row = detection, as eval_class's calculate_iou_partly(dt_annos, gt_annos),
 * eval.py:468).  All data float64 unless stated.  Additive to ABI 6: no existing entry changed.                                       */

/* Per-frame overlap blocks, every frame in one launch: replaces calculate_iou_partly (eval.py:335-410), whose cross-frame matrix per
 * group of frames is only read on its diagonal blocks.  out[out_off[f] + j * n_gt + i] = overlap(detection j, ground truth i):
 *   metric 0  boxes (n, 4) image boxes: image_box_overlap (eval.py:84-111) in double, criterion -1 / 0 / 1 / 2;
 *   metric 1  boxes (n, 5) (x, z, l, w, ry) rounded to fp32: rotate_iou_gpu_eval / devRotateIoUEval (rotate_iou.py:16-329) in fp32,
 *             the ground truth as the query box rbox1, criterion -1 / 0 / 1 / 2;
 *   metric 2  boxes (n, 7) (x, y, z, l, h, w, ry): d3_box_overlap (eval.py:119-152), the fp32 BEV intersection of columns
 *             [0, 2, 3, 5, 6] and the height / volume part in double, stored rounded to fp32.
 * max_pairs >= max over frames of n_dt * n_gt (any value >= it; 0 = nothing to do).  Any box count per frame, 0 included.           */
WS3D_API int ws3d_kitti_overlaps(int metric, int criterion, int frames, long max_pairs, const int32_t *gt_off, const int32_t *dt_off,
                                 const int64_t *out_off, const double *dt_boxes, const double *gt_boxes, double *out,
                                 ws3d_stream_t stream);

/* The collection pass of eval_class (eval.py:480-494): compute_statistics_jit (eval.py:155-273) with thresh = 0, compute_fp = False
 * for every frame.  ignored_gt / ignored_dt int32 per box (clean_data, eval.py:28-81), dt_score per detection; out per ground truth:
 * tp_flag int32 = 1 where it was matched as a true positive, tp_score = that detection's score (0 elsewhere).  The reference's
 * thresholds list is tp_score[tp_flag == 1] in (frame, ground truth) order.  max_dt >= the largest n_dt (at most 4096).             */
WS3D_API int ws3d_kitti_collect_scores(int frames, int max_dt, const int32_t *gt_off, const int32_t *dt_off, const int64_t *out_off,
                                       const double *overlaps, const int32_t *ignored_gt, const int32_t *ignored_dt,
                                       const double *dt_score, double min_overlap, double *tp_score, int32_t *tp_flag,
                                       ws3d_stream_t stream);

/* The counting pass: fused_compute_statistics (eval.py:285-333) over num_thresh score thresholds for every frame, compute_fp = True,
 * with the DontCare suppression of metric 0 (dc_off (frames + 1) int32, dc_bbox (n_dc, 4)) and, if compute_aos, the orientation
 * similarity (dt_alpha / gt_alpha).  pr (num_thresh, 4) = tp, fp, fn, similarity summed over the frames in frame order (exact
 * counts, reproducible sums: no atomics).  workspace >= ws3d_kitti_count_workspace_bytes(frames, num_thresh) bytes of device memory. */
WS3D_API size_t ws3d_kitti_count_workspace_bytes(int frames, int num_thresh);
WS3D_API int ws3d_kitti_count(int metric, int frames, int max_dt, int num_thresh, const double *thresholds, const int32_t *gt_off,
                              const int32_t *dt_off, const int32_t *dc_off, const int64_t *out_off, const double *overlaps,
                              const int32_t *ignored_gt, const int32_t *ignored_dt, const double *dt_score, const double *dt_alpha,
                              const double *gt_alpha, const double *dt_bbox, const double *dc_bbox, double min_overlap, int compute_aos,
                              void *workspace, size_t workspace_bytes, double *pr, ws3d_stream_t stream);

/* ------------------------------------------------- Stage-2 box network (lib/net/rcnn_net.py, tools/eval_auto.py) */

/* Additive to ABI 6: no existing entry changed.
 * The front of a tower of RCNNNet for rows = R * pts_per_cloud points in one launch: replaces rcnn_net.py:253-267 (xyz_up_layer,
 * feature_up_layer, cat, merge_down_layer) and, with box_ce, rcnn_net.py:337-365 (the IoU-net's canonical transform + the can_* layers).
 *   pts (rows, 5) = [x, y, z, reflectance, mask]; box_ce (R, 7) = [x, y_centre, z, h, w, l, ry] or NULL;
 *   wx0 (3, 128), wx1 (128, 128), wf0 (2, 128), wf1 (128, 128), wm (256, 128): the layers' W^T (row = input channel), b* (128);
 *   xyz_out (rows, 3): with a box, the point minus the centre, turned by -ry about y, divided by (l/2, h/2, w/2), all three set to 0 where the
 *   largest |coordinate| exceeds `extend` (fp32, the reference's operation order); without one, a copy.  feat (rows, 128), channels last:
 *   relu(wm^T [relu(wx1^T relu(wx0^T xyz_out + bx0) + bx1) ; relu(wf1^T relu(wf0^T [reflectance, mask] + bf0) + bf1)] + bm).
 * 128 x 128 and 256 x 128 layers on the fp32 matrix cores, k ascending.  Any rows >= 0; tiles of 64 rows may straddle clouds.          */
WS3D_API int ws3d_stage2_embed(long rows, int pts_per_cloud, const float *pts, const float *box_ce, float extend, const float *wx0,
                               const float *bx0, const float *wx1, const float *bx1, const float *wf0, const float *bf0, const float *wf1,
                               const float *bf1, const float *wm, const float *bm, float *xyz_out, float *feat, ws3d_stream_t stream);
/* rcnn_reg (rows, 4 * loc_bins + 1 + 2 * head_bins + 3) -> pred_boxes3d (rows, 7) = decode_bbox_target_stage_2 as rcnn_net.py:293-302 calls
 * it (lib/utils/bbox_transform.py:64-179 with a zero roi, get_xz_fine = get_ry_fine = False, y by offset: x = reg[2 loc_bins] * loc_scope,
 * z = reg[3 loc_bins] * loc_scope, the FIRST maximal heading bin, sizes reg * (h, w, l) + (h, w, l)) and box_ce (rows, 7) = box2center_box
 * of it (bbox_transform.py:292-296: y - h / 2).                                                                                          */
WS3D_API int ws3d_stage2_boxes(int rows, int loc_bins, int head_bins, float loc_scope, float h, float w, float l, const float *rcnn_reg,
                               float *pred_boxes3d, float *box_ce, ws3d_stream_t stream);
/* The element-wise part of the detection tail for (batch, slots) clouds: center_box2box + refine_box (rcnn_net.py:387-390,
 * bbox_transform.py:286-303), ry wrapped into (-pi, pi], x and z shifted by center (batch, slots, 3), y by ground_y (eval_auto.py:397-403);
 * keep (int32 0 / 1) = sigmoid(rcnn_cls) > cls_thresh && rcnn_iou > iou_thresh && the size window size_window[6] = h_lo, h_hi, w_lo, w_hi,
 * l_lo, l_hi (HOST pointer; all bounds exclusive, eval_auto.py:426-436) && slot < num[scene]; key = rcnn_iou where kept, -1e30 elsewhere:
 * the per-scene sort keys of the sweep of eval_auto.py:597-609.  boxes (batch, slots, 7) is written for every slot.                     */
WS3D_API int ws3d_stage2_select(int batch, int slots, float cls_thresh, float iou_thresh, const float *size_window, float ground_y,
                                const float *box_ce, const float *rcnn_ref, const float *rcnn_cls, const float *rcnn_iou, const float *center,
                                const int32_t *num, float *boxes, int32_t *keep, float *key, ws3d_stream_t stream);

/* Additive to ABI 6: no existing entry changed.  Stage 2 on WHOLE instance clouds of different sizes (csrc/stage2_ragged.hip), the form
 * tools/eval_auto.py:286-403 evaluates in: cloud i owns the packed rows offsets[i] .. offsets[i+1]; offsets (clouds + 1) DEVICE int32,
 * ascending, offsets[0] = 0; sizes_host (clouds) a HOST copy of the sizes, every one >= 1 (else WS3D_E_INVALID before any launch).
 *
 * ws3d_stage2_canonical_ragged: pts (rows, 5) = [x, y, z, reflectance, mask], box_ce (clouds, 7) -> pts_out (rows, 5): the canonical
 * transform of ws3d_stage2_embed with the box of the row's OWN cloud (found by a search over offsets per row: nothing depends on clouds
 * being aligned to tiles), same fp32 operations in the same order; reflectance and mask copied.  ws3d_stage2_embed(pts_out, NULL) is
 * bit-equal to ws3d_stage2_embed(pts_i, box_i) on each cloud alone.  rows must equal offsets[clouds].                              */
WS3D_API int ws3d_stage2_canonical_ragged(int rows, int clouds, const int32_t *offsets, const float *pts, const float *box_ce, float extend,
                                          float *pts_out, ws3d_stream_t stream);
/* ws3d_furthest_point_sampling_ragged that also writes new_xyz (clouds, m, 3) = xyz[offsets[i] + idx[i]] and accepts m > n_i: the result
 * is then what sampling_gpu.cu:93-209 gives with block = opt_n_threads(n_i) -- once the distinct points are used up the running minima
 * are all 0 and the tie rule returns index 0.  idx (clouds, m) local to each cloud, bit-equal to ws3d_furthest_point_sampling on cloud i
 * alone for every n_i >= 1.  Clouds above ws3d_fps_ragged_limit() points are forwarded to ws3d_furthest_point_sampling_gather, one
 * launch each on the same stream.                                                                                                    */
WS3D_API int ws3d_furthest_point_sampling_ragged_gather(int clouds, const int32_t *offsets, const int32_t *sizes_host, int m, const float *xyz,
                                                        int32_t *idx, float *new_xyz, ws3d_stream_t stream);
/* ball_query_kernel_fast (ball_query_gpu.cu:9-45) per cloud: xyz (total, 3) packed, new_xyz (clouds, m, 3) -> idx (clouds, m, nsample):
 * the cloud's points in ascending index, d2 < radius * radius strictly, the first hit fills all nsample slots, stop at nsample, a centre
 * without a hit keeps 0.  global_rows = 1 adds offsets[i] to every entry (the padding zeros included), so the lists index the packed
 * array.  nsample <= 64 (else WS3D_E_UNSUPPORTED).  Every element of idx is written; no atomics, allocation or host synchronisation.  */
WS3D_API int ws3d_ball_query_ragged(int clouds, const int32_t *offsets, int m, float radius, int nsample, const float *xyz, const float *new_xyz,
                                    int global_rows, int32_t *idx, ws3d_stream_t stream);

/* The Stage-2 training losses (lib/net/train_functions.py:230-516, lib/utils/loss_utils.py:151-338 with LOC_XZ_FINE = LOC_Y_BY_BIN =
 * get_ry_fine = False), value AND gradient in one launch of one workgroup each: no host branch on fg_sum / iou_sum, no read-back, no
 * atomics, sums folded in a fixed order (a call is bit-reproducible).  Row terms in float64 from the fp32 inputs; the paired 3-D IoU
 * inside is the device function of ws3d_boxes_iou3d_paired.  An empty selection (no foreground row, ...) contributes an exact 0.
 *
 * ws3d_stage2_rcnn_loss: rcnn_cls (rows), rcnn_reg (rows, 4 loc_bins + 1 + 2 head_bins + 3), pred_boxes3d / gt_boxes (rows, 7)
 * [x, y_bottom, z, h, w, l, ry], cls (rows) labels (> 0 foreground, 0 background, < 0 ignored by the classification term) ->
 *   vals (8) = rcnn_loss_cls, 20 loc, angle, 300 size, 10 corner, rcnn_loss_reg = loc + angle + size, rcnn_loss = cls + reg + corner, 0
 *   counts (4) int32 = fg_sum, iou_sum (foreground rows with iou3d(pred, gt) > 0.5), rows with cls >= 0, rows with cls == 0
 *   grad_cls (rows), grad_reg (rows, width) = d rcnn_loss / d rcnn_cls, d rcnn_reg (pred_boxes3d is a constant: the corner term has a
 *   value and no gradient, as in the reference, which detaches it).                                                                  */
WS3D_API int ws3d_stage2_rcnn_loss(int rows, int loc_bins, int head_bins, float loc_scope, float h, float w, float l, const float *rcnn_cls,
                                   const float *rcnn_reg, const float *pred_boxes3d, const float *gt_boxes, const float *cls, float *vals,
                                   int32_t *counts, float *grad_cls, float *grad_reg, ws3d_stream_t stream);
/* ws3d_stage2_ioun_loss: rcnn_iou (rows), rcnn_ref (rows, 7), pred_boxes3d / refined_box / gt_boxes (rows, 7), cls (rows) ->
 *   vals (8) = 300 loc, 300 size, 20 angle, loss_iou = 100 mse(rcnn_iou, iou3d(refined_box, gt)^2) over the rows whose gt box has a
 *   non-zero entry (the reference: whose entries do not SUM to 0 -- the same rows unless a box cancels to exactly zero, which would
 *   depend on the summation order; 0 when there is none: the reference's mean over an empty selection is NaN), loss_reg, rcnn_loss_iou = loss_iou + loss_reg, 0, 0
 *   counts (4) int32 = fg_sum, rows with a non-zero gt box, 0, 0
 *   grad_iou (rows), grad_ref (rows, 7) = d rcnn_loss_iou / d rcnn_iou, d rcnn_ref.                                                  */
WS3D_API int ws3d_stage2_ioun_loss(int rows, const float *rcnn_iou, const float *rcnn_ref, const float *pred_boxes3d, const float *refined_box,
                                   const float *gt_boxes, const float *cls, float *vals, int32_t *counts, float *grad_iou, float *grad_ref,
                                   ws3d_stream_t stream);

/* The Stage-1 training targets for a padded batch: generate_gaussian_training_labels (lib/datasets/kitti_rcnn_dataset.py:529-573), which
 * the reference runs per scene on the host.  pts (batch, n, >= 3) with pts_stride floats from one point to the next (x, y, z lead),
 * centres (batch, kmax, 3), count (batch) int32: the first count[b] centres of scene b are real, the others are never read (a count
 * outside 0..kmax is clamped) -> cls_label (batch, n) = exp(-0.5 near^2 / gauss_cov) with near = clip(min_k d_k - gauss_status, 0, 100),
 * d_k = sqrt(((px - cx)^2 + (py * gauss_height)^2) + (pz - cz)^2) in correctly rounded fp32 operations, the exponential in float64 and
 * rounded once (labels beyond ~17 m are fp32 denormals, kept: they count as foreground); reg_label (batch, n, 3) = (cx - px, 0, cz - pz)
 * of the FIRST nearest centre where d < 4, zeros elsewhere.  count[b] == 0: zeros.  One launch, no workspace.                          */
WS3D_API int ws3d_rpn_center_labels(int batch, int n, int kmax, int pts_stride, float gauss_height, float gauss_status, double gauss_cov,
                                    const float *pts, const float *centres, const int32_t *count, float *cls_label, float *reg_label,
                                    ws3d_stream_t stream);
/* The Stage-1 loss, get_rpn_loss (lib/net/train_functions.py:163-228) with SigmoidFocalClassificationLoss on soft targets and
 * get_rpn_reg_loss (lib/utils/loss_utils.py:25-156), value AND gradient, no host branch on fg_sum and no read-back.
 * rpn_cls (rows), rpn_reg (rows, 4 bins) laid out [x_bin | z_bin | x_res | z_res], cls_label (rows), reg_label (rows, 3) ->
 *   vals (9) = rpn_loss = weight_cls * rpn_loss_cls + weight_reg * rpn_loss_reg, rpn_loss_cls, rpn_loss_reg = (x_bin + z_bin) + (x_res +
 *              z_res), rpn_loss_cls_pos, rpn_loss_cls_neg, loss_x_bin, loss_z_bin, loss_x_res, loss_z_res
 *   counts (1) int32 = foreground rows (cls_label > 0)
 *   grad_cls (rows), grad_reg (rows, 4 bins) = d rpn_loss / d rpn_cls, d rpn_reg, written in full (zeros on the other rows).
 * The focal weights are 1 / max(sum cls_label, 1); the regression terms are means over the foreground rows, sum / max(count, 1): no
 * foreground row gives an exact 0.  Row terms in float64 from the fp32 inputs, float64 sums in a fixed order over per-workgroup
 * partials, no atomics: a call is bit-reproducible and the workspace (ws3d_rpn_loss_workspace_bytes(rows), 8-byte aligned) carries
 * nothing from call to call.  bins in 1..32; rpn_reg and grad_reg 16-byte aligned.  Three launches on `stream`.                       */
WS3D_API size_t ws3d_rpn_loss_workspace_bytes(int rows);
WS3D_API int ws3d_rpn_loss(int rows, int bins, double loc_scope, double loc_bin_size, double alpha, double gamma, double weight_cls,
                           double weight_reg, const float *rpn_cls, const float *rpn_reg, const float *cls_label, const float *reg_label,
                           float *vals, int32_t *counts, float *grad_cls, float *grad_reg, void *workspace, size_t workspace_bytes,
                           ws3d_stream_t stream);

/* Raw KITTI scans -> pts_input on the device: the projection, frustum / range filter and npoints-row sample that
 * kitti_io.rpn_input_from_scan does per scene on the host (get_rpn_sample, lib/datasets/kitti_rcnn_dataset.py:399-452), for a ragged
 * batch in one call with no read-back.  ANOTHER random stream than the reference's (counter-based, keyed by (seed, scene_key)) and no
 * sort by lidar z: DESIGN.md "Scan preparation on the device" states the contract, ws3d_amd/scan_prepare.py restates it bit for bit.
 *   offsets (scenes + 1) int32: scene b holds the raw points offsets[b] .. offsets[b+1] of raw (total_points, 4) [x, y, z, refl]
 *   (16-byte aligned); max_scan_points: the largest scan of the call; calib (scenes, 24): T (4 x 3) = V2C^T . R0^T, then P2 (3 x 4);
 *   img_hw (scenes, 2) int32 = height, width; scope: HOST pointer to x0 x1 y0 y1 z0 z1 or NULL (no range filter); scene_key (scenes)
 *   int64; key_bits 1..32 (32 in production; fewer bits force ties) ->
 *   pts_input (scenes, npoints, 4) = [r_0, r_1, r_2, refl - 0.5f] (16-byte aligned), src_index (scenes, npoints) = the raw index of
 *   each row, valid_count (scenes) = V, status (scenes): 0 ok; 1 no valid point; 2 more than npoints points beyond 40 m; 3 offsets
 *   that do not describe a slice of raw.  A scene with a non-zero status gets zero rows and src_index -1 and leaves the others alone.
 * WS3D_E_UNSUPPORTED: npoints above ws3d_scan_prepare_limit(), npoints * max_scan_points above 2^32 or more than 65535 scenes.
 * workspace: ws3d_scan_prepare_workspace_bytes(scenes, total_points) bytes, 4-byte aligned.  Two launches on `stream`.            */
WS3D_API int ws3d_scan_prepare_limit(void);
WS3D_API size_t ws3d_scan_prepare_workspace_bytes(int scenes, long total_points);
WS3D_API int ws3d_scan_prepare(int scenes, const int32_t *offsets, long total_points, int max_scan_points, const float *raw, const float *calib,
                               const int32_t *img_hw, const float *scope, int npoints, uint64_t seed, const int64_t *scene_key, int key_bits,
                               float *pts_input, int32_t *src_index, int32_t *valid_count, int32_t *status, void *workspace,
                               size_t workspace_bytes, ws3d_stream_t stream);

/* Additive to ABI 6: no existing entry changed.  Stage-2 training batches from box records that lie on the device
 * (csrc/stage2_batch.hip): what train_rcnn.BoxDataset.sample -> collate -> prepare_batch do per cloud on the host, for a batch in ONE
 * launch with one workgroup per sample and no read-back.  ANOTHER random stream than BoxDataset's for the per-point draws (mask
 * flips and shuffle: a counter-based hash of (sample_seed, row number)); every floating-point draw is made by the caller.  DESIGN.md
 * 5.13a "Stage-2 batches on the device" states the contract, ws3d_amd/stage2_batch.py restates it bit for bit and builds the blocks.
 *   params (samples) blocks of ws3d_stage2_batch_param_bytes() bytes each, on the device, 8-byte aligned:
 *     double gt0, gt2 (the box centre the region drop-out compares x and z with), cx, cz (recentring offsets);
 *     uint64 sample_seed; int32 record, flags, cut, pad; float revive_matrix[0] (16), revive_matrix[1] (16), Rot_y (16),
 *     ext_noise (3), noise_scale.  flags: 1 TRAIN mode, 2 drop-out on, 4 / 8 its x / z side is '>', 16 OR of the sides (else AND),
 *     32 rows with prob < 0 are kept as well, 64 x flip.  cut: the rows kept of a cloud that fills all 512 (512, 128 or 32).
 *   rows (total_rows, 6) = [x, y, z, reflect, prob -+ 0.5, gt_mask - 0.5], 8-byte aligned; offsets (records + 1) int32: record r
 *   holds the rows offsets[r] .. offsets[r+1]; key_bits 1..32 (32 in production; fewer bits force ties in the shuffle keys) ->
 *   cur_box_point (samples, 512, 3), cur_box_reflect (samples, 512), train_mask (samples, 512); status (samples) or NULL: 0 ok,
 *   3 a record index or offsets that do not describe a non-empty slice of rows -- such a sample's outputs are not touched.
 * WS3D_E_INVALID: a negative count, total_rows above 2^31 - 1, key_bits out of range, a null or misaligned pointer; nothing launched. */
WS3D_API int ws3d_stage2_batch_param_bytes(void);
WS3D_API int ws3d_stage2_batch(int samples, const void *params, const float *rows, const int32_t *offsets, int records, long total_rows,
                               int key_bits, float *cur_box_point, float *cur_box_reflect, float *train_mask, int32_t *status,
                               ws3d_stream_t stream);

/* ------------------------------------------------- test hooks */

/* What ws3d_roipool3d / _fill / _ws would launch for these sizes under this process's WS3D_ROI_* knobs, without launching it:
 * 1000 * family + 100 * G + CR -- family 0: roipool3d_kernel<G, CR> (G boxes per workgroup), 1: roipool3d_pipe_kernel<G, CR> (G boxes
 * per pass), 2: roi_bin_kernel + roipool3d_binned_kernel<CR> (G = 1); CR: rows per LDS stretch of the copy, 0 = the direct copy.
 * 0: nothing to launch (no scene or no box); the launcher's negative error code where it would refuse the sizes.
 * aligned16: pts_feature and pooled_features are 16-byte aligned; workspace_bytes: what ws3d_roipool3d_ws is given (0: none).
 * The launcher decides through the same function.  No HIP call.  (tests/test_roipool_plan.py) */
WS3D_API int ws3d_roipool3d_plan(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num, int aligned16,
                                 size_t workspace_bytes);

/* What ws3d_ball_query / _fill / _pairs / _pairs2 / ws3d_query_and_group / _nlc would launch for these sizes, without launching it.
 * fused: the query_and_group entries (c feature channels, nlc: channels-last); flavour: what the sort entry points noted for the
 * binned copy (1: ws3d_sort_points_grid / a "grid" job, 0: any other binned copy, -1: none); pairs: the compact pairs are wanted;
 * scales: 1, or 2 for ws3d_ball_query_pairs2 (nsample = the longer of its two lists); wide_nw: the value of ws3d_tune key 5.
 * plan[0..7] = family (0: ball_query_kernel, 1: ball_query_sorted_kernel, 2: ball_query_grid_kernel, 3: ball_query_grid_coop_kernel),
 * bits of a list index in LDS (16 | 32), FUSED, waves per workgroup, workgroups per tile of 64 centres (grid z), dynamic LDS bytes,
 * grid x, grid y; all zero when there is nothing to launch (b == 0 or m == 0) or the sizes are refused.  Returns WS3D_OK or the
 * launcher's error code.  The launchers decide through the same function.  No HIP call.  (tests/test_ballquery_plan.py) */
WS3D_API int ws3d_ball_query_plan(int b, int n, int m, int c, int nsample, int fused, int nlc, int flavour, int pairs, int scales, int wide_nw,
                                  int32_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* WS3D_OPS_H */
