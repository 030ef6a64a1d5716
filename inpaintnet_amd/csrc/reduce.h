// The reduction orders of the helper kernels, stated once.  Device-only, no state.
//
// THE DETERMINISM CONTRACT.  Several kernels promise "no float atomics, every sum in a fixed order, the same bits from call to call"
// (the free-bits keep bits, the MMD / attribute / IWAE / weighted cross-entropy values, the Adam bit fixtures, "ce_w with every option
// off gives ce_kernel's bits").  The order those promises rest on is the one written here and nowhere else:
//   wave_sum / wave_max / wave_min   the xor butterfly over a wave's 64 lanes, o = 32, 16, 8, 4, 2, 1: lane L combines with lane L ^ o.
//                                    Every lane ends with the same bits.  wave_max skips a NaN (fmaxf / fmax).
//   sum4                             four partials in index order, ((p[0] + p[1]) + p[2]) + p[3] -- a workgroup's four waves in wave order.
//   block_sum                        wave_sum, lane 0 of each of the four waves files its value, a barrier, sum4 on every thread.
//   wave_max_dpp                     the maximum alone through DPP row operations and four readlanes (a maximum has no order to keep).
// Changing any of these changes recorded bits: tests/golden/adam_bits, the keep bits of tests/test_gpu_kl_fb.py and the equalities of
// tests/test_gpu_ce_w_kernels.py hold the kernels to them.
//
// Sums that are NOT these and keep their own text, because their order differs and is part of somebody's bits too:
//   - the pairwise (p0 + p1) + (p2 + p3) over four waves of reparam_kl_kernel (latent.hip) and nll_rows_kernel (iw.hip);
//   - the 16-lane trees of decode_chain.hip (a row of an MFMA tile, not a wave);
//   - the value+index butterfly of arnn_gen.hip's argmax_wave (two registers travel together);
//   - table_grad_kernel's __shfl_down tree and its four-wave sum over a strided LDS table (pointwise.hip);
//   - the eight- and sixteen-term trees inside the pair kernels (mmd.hip, attr.hip): a thread's own registers, no lanes involved;
//   - gemv_rows_kernel's butterfly in gemm.hip: the same order, but calling wave_sum there moves its instructions.
#pragma once
#include <hip/hip_runtime.h>

template <class T>
__device__ __forceinline__ T wave_sum(T v) {                       // float, double, int, long long
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {             // fmax: a NaN is skipped (a caller that cares looks for NaNs itself)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// maximum over the 64 lanes of the wave without LDS (exact, wave-uniform): two quad permutes, the two mirrors of a 16-lane row, then the four rows through SGPRs
__device__ __forceinline__ float wave_max_dpp(float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0xB1, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x4E, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x141, 0xF, 0xF, false)));  // row_half_mirror
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x140, 0xF, 0xF, false)));  // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// four partials in index order; the second form: column j of a [4][N] table
template <class T>
__device__ __forceinline__ T sum4(const T* p) { return ((p[0] + p[1]) + p[2]) + p[3]; }
template <class T, int N>
__device__ __forceinline__ T sum4(const T (&p)[4][N], int j) { return ((p[0][j] + p[1][j]) + p[2][j]) + p[3][j]; }

// the sum of the workgroup's 256 values on every thread: the wave tree, then the four waves in wave order (part4: four T of LDS)
template <class T>
__device__ __forceinline__ T block_sum(T v, T* part4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part4[threadIdx.x >> 6] = v;
    __syncthreads();
    return sum4(part4);
}

// argmax_first, np.argmax's rule (the one arnn_gen.hip follows): a NaN is the maximum, the lowest index wins among equals.  `m` is
// the row's maximum as fmaxf leaves it (NaN skipped).  A lane folds the candidates of its elements into ONE key, so that one wave
// minimum decides: a NaN at v -> v, an element equal to m -> kAmEq + v (V < 2^30), anything else -> kAmNone; am_index() of the
// minimum is the row's argmax (every row has a candidate: its maximum, or a NaN).
constexpr int kAmEq = 0x40000000, kAmNone = 0x7fffffff;
__device__ __forceinline__ int am_key(float x, float m, int v) { return x != x ? v : (x == m ? kAmEq + v : kAmNone); }
__device__ __forceinline__ int am_index(int key) { return key & (kAmEq - 1); }
