// Temperature sampling of one token in numpy's order, for the generation of AnticipationRNN
// (AnticipationRNN/anticipation_rnn_gauss_reg_model.py:655-667: preds = softmax(T * logits); np.random.choice(V, p=preds)).
// np.random.choice draws ONE random_sample() double u per call and returns searchsorted(cumsum(p) / sum(p), u, 'right'): the first
// v whose inclusive prefix exceeds u.  Here e_v = exp(s_v - max s) in f32 (s = T x, the reference's f32 softmax numerator), the
// prefix over v in f64 (a wave scan over 64 lanes x NV chunks: DPP shifts inside the 16-lane rows, the row totals by readlane), and
// token = the first v with prefix_v > u * S, S = the total, by ballot and ctz.  The result is wave-uniform.
#pragma once
#include <hip/hip_runtime.h>

namespace sample {

template <int CTRL>
__device__ __forceinline__ double dpp_d(double x) {                    // lanes whose source lies outside the row read 0
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double readlane_d(double x, int l) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// inclusive prefix sum over the 64 lanes of the wave
__device__ __forceinline__ double wave_scan(double x, int lane) {
    x += dpp_d<0x111>(x);                                              // row_shr:1
    x += dpp_d<0x112>(x);                                              // row_shr:2
    x += dpp_d<0x114>(x);                                              // row_shr:4
    x += dpp_d<0x118>(x);                                              // row_shr:8
    const double r0 = readlane_d(x, 15), r1 = readlane_d(x, 31), r2 = readlane_d(x, 47);
    const int row = lane >> 4;
    return x + (row == 0 ? 0.0 : row == 1 ? r0 : row == 2 ? r0 + r1 : (r0 + r1) + r2);
}

// s[j] = T x_v of v = lane + 64 j (-inf for v >= V), no NaN among them; m = max_v s_v (wave-uniform); u = the tick's uniform.
// -> the first v with prefix_v > u S, or -1 where the rule does not apply (m or S not finite, u outside [0, 1)): the caller then
// takes the argmax rule.  The result lies in [0, V) or is -1.
template <int NV>
__device__ __forceinline__ int pick(const float (&s)[NV], float m, double u, int V, int lane) {
    if (!(m > -INFINITY && m < INFINITY) || !(u >= 0.0 && u < 1.0)) return -1;
    double pre[NV];
    double carry = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const double e = lane + 64 * j < V ? (double)expf(s[j] - m) : 0.0;
        const double x = wave_scan(e, lane);
        pre[j] = carry + x;
        carry += readlane_d(x, 63);
    }
    if (!(carry > 0.0 && carry < INFINITY)) return -1;
    const double thr = u * carry;
    int tok = -1;
#pragma unroll
    for (int j = NV - 1; j >= 0; --j) {
        const unsigned long long b = __ballot(lane + 64 * j < V && pre[j] > thr);
        if (b) tok = 64 * j + __builtin_ctzll(b);
    }
    return tok;
}

}  // namespace sample
