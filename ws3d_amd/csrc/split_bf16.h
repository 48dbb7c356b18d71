// split_bf16.h -- the split-bf16 product: an fp32 matrix product on the bf16 matrix cores at fp32 accuracy,
// the arithmetic shared by rpn_heads.hip and gemm_rows.hip.
//
// Every fp32 operand is written as three bf16 pieces, x = x1 + x2 + x3 (+ a remainder below 2^-24 |x|), and the six largest of
// the nine partial products of a k-step are summed on v_mfma_f32_32x32x16_bf16 (32 cycles per k = 16; a bf16 x bf16 product is exact
// in the fp32 accumulator) into ONE fp32 accumulator, smallest first: a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1.  The dropped terms
// a2 b3, a3 b2, a3 b3 are below 2^-16 |a b| x 2^-8 each.  6 / 16 of the time v_mfma_f32_32x32x2_f32 takes per product.
// The pieces, their order and the dropped terms are the contract: a kernel chooses its geometry, not these.
#pragma once
#include "common.h"

namespace ws3d {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));        // one lane's eight k of a v_mfma_f32_32x32x16_bf16 operand

// x = p1 + p2 + p3 (+ a remainder below 2^-24 |x|): each piece is the bf16 nearest to what the pieces before it left; every
// subtraction is exact in fp32.  +-Inf gives (Inf, NaN, NaN), NaN three NaNs.
__device__ __forceinline__ void split3(float x, __bf16 &p1, __bf16 &p2, __bf16 &p3) {
    p1 = (__bf16)x;
    const float r1 = x - (float)p1;
    p2 = (__bf16)r1;
    const float r2 = r1 - (float)p2;
    p3 = (__bf16)r2;
}

__device__ __forceinline__ void split8(const float *v, bf16x8 &q1, bf16x8 &q2, bf16x8 &q3) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __bf16 p1, p2, p3;
        split3(v[j], p1, p2, p3);
        q1[j] = p1; q2[j] = p2; q3[j] = p3;
    }
}

// The six products of one k-step for NC accumulator chains that share the A operand's pieces (a1 largest); b1 .. b3 and acc hold
// one entry per chain.  Every accumulator is summed in the order above; with NC > 1 the chains are interleaved product by product,
// so that consecutive matrix instructions do not depend on each other.
template <int NC>
__device__ __forceinline__ void split_mfma6(const bf16x8 &a1, const bf16x8 &a2, const bf16x8 &a3, const bf16x8 *b1, const bf16x8 *b2,
                                            const bf16x8 *b3, floatx16 *acc) {
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1[m], acc[m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2[m], acc[m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3[m], acc[m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1[m], acc[m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2[m], acc[m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[m], acc[m], 0, 0, 0);
}

// ReLU that keeps a NaN (fmaxf(NaN, 0) = 0 would turn a non-finite row into a finite output)
__device__ __forceinline__ float relu_keep_nan(float y) { return y < 0.f ? 0.f : y; }

}  // namespace ws3d
