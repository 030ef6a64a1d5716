// The importance-weighted log-likelihood of a measure (the IWAE bound): the rule stands in iw.h, the reasons in DESIGN.md section 26.
// Three launches, each one read of its data, no float atomics, every sum in an order that depends on the shape (and, for iw_draw, on
// which of its two paths runs) alone: two calls on the same inputs give the same bits.
//   iw_draw_kernel   one wavefront per row r = b * Kc + j: z[r,:] and logr[r]
//   nll_rows_kernel  one workgroup of four waves per measure row: the row's T cross-entropy terms, ce_kernel's arithmetic per term
//   iw_finish_kernel one wavefront per measure: the log-mean-exp over its K samples and what comes out of the same pass, in double
#include <cmath>
#include "common.h"
#include "iw.h"
#include "prof.h"
#include "reduce.h"

namespace {

constexpr int kIwBlock = 256;                    // four waves: four rows of iw_draw, one row of nll_rows, four measures of iw_finish
constexpr int kIwWaves = kIwBlock / 64;
constexpr long kIwMaxRows = 1L << 24;

// One element of a row: z = mu + eps * exp(ls), reparam_kl_kernel's expression with the same expf; the element's term of logr.
__device__ __forceinline__ float iw_elem(float m, float l, float e, float& zo) {
    const float s = expf(l);
    const float z = m + e * s;
    zo = z;
    return 0.5f * e * e - 0.5f * z * z + l;
}

// VEC = 4: Z % 4 == 0 and every row of every operand 16-byte aligned -- a lane takes d = 4 lane .. 4 lane + 3, then 256 further on.
// VEC = 1: a lane takes d = lane, lane + 64, ...  Either way a lane adds its terms in ascending d, then the xor tree adds the lanes.
template <int VEC>
__global__ void __launch_bounds__(kIwBlock)
iw_draw_kernel(const float* __restrict__ mu, const float* __restrict__ ls, const float* __restrict__ eps, long eps_stride_b,
               float* __restrict__ z, float* __restrict__ logr, long rows, int Kc, int Z) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * kIwWaves + (threadIdx.x >> 6);
    if (r >= rows) return;                                           // (a whole wave leaves: no barrier follows)
    const long b = r / Kc;
    const int j = (int)(r - b * Kc);
    const float* __restrict__ m = mu + b * Z;
    const float* __restrict__ l = ls + b * Z;
    const float* __restrict__ e = eps + b * eps_stride_b + (long)j * Z;
    float* __restrict__ zo = z + r * Z;
    float acc = 0.f;
    if constexpr (VEC == 4) {
        for (int d = 4 * lane; d < Z; d += 256) {
            const f32x4 mv = *reinterpret_cast<const f32x4*>(m + d), lv = *reinterpret_cast<const f32x4*>(l + d);
            const f32x4 ev = *reinterpret_cast<const f32x4*>(e + d);
            f32x4 zv;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float zi;
                acc += iw_elem(mv[i], lv[i], ev[i], zi);
                zv[i] = zi;
            }
            *reinterpret_cast<f32x4*>(zo + d) = zv;
        }
    } else {
        for (int d = lane; d < Z; d += 64) {
            float zi;
            acc += iw_elem(m[d], l[d], e[d], zi);
            zo[d] = zi;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) logr[r] = acc;
}

// Workgroup r: wave w takes ticks w, w + 4, ...; per tick ce_kernel's arithmetic (the maximum, expf(x - m) added per lane in ascending
// v, the xor tree, lse = m + logf(se), the term lse - x[target]); lane 0 adds its wave's terms in ascending tick order, the four waves
// meet in LDS as (p0 + p1) + (p2 + p3).  A target outside [0, V) makes the row NaN and is never used as an index.
__global__ void __launch_bounds__(kIwBlock)
nll_rows_kernel(const float* __restrict__ W, long ld_w, const long long* __restrict__ tgt, const float* __restrict__ logr,
                float* __restrict__ nll, float* __restrict__ logw, long ld_out, int group, int T, int V) {
    __shared__ float part[kIwWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = blockIdx.x;
    float acc = 0.f;
    for (int t = wave; t < T; t += kIwWaves) {
        const float* __restrict__ w = W + (r * T + t) * ld_w;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, w[v]);
        m = wave_max(m);
        float se = 0.f;
        for (int v = lane; v < V; v += 64) se += expf(w[v] - m);
        se = wave_sum(se);
        const float lse = m + logf(se);
        if (lane == 0) {
            const long long tg = tgt[r * T + t];
            acc += (tg >= 0 && tg < V) ? lse - w[tg] : __builtin_nanf("");
        }
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float n = (part[0] + part[1]) + (part[2] + part[3]);
        const long at = (r / group) * ld_out + r % group;
        if (nll) nll[at] = n;
        if (logw) logw[at] = (logr ? logr[r] : 0.f) - n;
    }
}

// Wave = measure b; lanes stride over K; everything in double on the widened floats.  Pass 1: the maximum (and whether a NaN is in the
// row: fmax skips them).  Pass 2: s1, s2, sum logw, sum nll per lane in ascending k, then the xor tree.
__global__ void __launch_bounds__(kIwBlock)
iw_finish_kernel(const float* __restrict__ logw, const float* __restrict__ nll, long ld, long B, int K, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long b = (long)blockIdx.x * kIwWaves + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* __restrict__ lw = logw + b * ld;
    const float* __restrict__ nl = nll + b * ld;
    double m = -INFINITY;
    bool nan = false;
    for (int k = lane; k < K; k += 64) {
        const double x = (double)lw[k];
        nan |= x != x;
        m = fmax(m, x);
    }
    m = wave_max(m);
    nan = __any(nan);
    double s1 = 0.0, s2 = 0.0, sw = 0.0, sn = 0.0;
    for (int k = lane; k < K; k += 64) {
        const double x = (double)lw[k], d = x - m;
        s1 += exp(d);
        s2 += exp(2.0 * d);
        sw += x;
        sn += (double)nl[k];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    sw = wave_sum(sw);
    sn = wave_sum(sn);
    if (lane == 0) {
        const double kd = (double)K;
        double iwae = m + log(s1 / kd), elbo = sw / kd, ess = (s1 * s1) / s2;
        if (nan) {
            iwae = elbo = ess = __builtin_nan("");
        } else if (m == -INFINITY) {                                 // every sample has zero weight
            iwae = elbo = -INFINITY;
            ess = 0.0;
        }
        double* __restrict__ o = out + 5 * b;
        o[0] = iwae;
        o[1] = elbo;
        o[2] = ess;
        o[3] = sn / kd;
        o[4] = -(sw + sn) / kd;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int iw_draw_launch(const float* mu, const float* ls, const float* eps, long eps_stride_b, float* z, float* logr, long B, int Kc, int Z,
                   hipStream_t s) {
    if (!mu || !ls || !eps || !z || !logr || B < 1 || Kc < 1 || Z < 1 || B > kIwMaxRows / Kc) return -1;
    if (eps_stride_b < (long)Kc * Z) return -1;
    const long rows = B * Kc;
    const bool vec = Z % 4 == 0 && eps_stride_b % 4 == 0 && aligned16(mu) && aligned16(ls) && aligned16(eps) && aligned16(z);
    const dim3 grid((unsigned)((rows + kIwWaves - 1) / kIwWaves));
    ProfScope prof(PROF_HBM, 0.0, s, "iw_draw", 4.0 * (2.0 * (double)rows * Z + 2.0 * (double)B * Z + (double)rows));
    if (vec)
        hipLaunchKernelGGL(iw_draw_kernel<4>, grid, dim3(kIwBlock), 0, s, mu, ls, eps, eps_stride_b, z, logr, rows, Kc, Z);
    else
        hipLaunchKernelGGL(iw_draw_kernel<1>, grid, dim3(kIwBlock), 0, s, mu, ls, eps, eps_stride_b, z, logr, rows, Kc, Z);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int nll_rows_launch(const float* weights, long ld_w, const long long* targets, const float* logr, float* nll, float* logw, long ld_out,
                    long R, int group, int T, int V, hipStream_t s) {
    if (!weights || !targets || (!nll && !logw) || R < 1 || R > kIwMaxRows || group < 1 || T < 1 || V < 1) return -1;
    if (ld_w < V || R % group != 0 || ld_out < group) return -1;
    ProfScope prof(PROF_HBM, 0.0, s, "nll_rows", 4.0 * (double)R * T * V + 8.0 * (double)R * T + 12.0 * (double)R);
    hipLaunchKernelGGL(nll_rows_kernel, dim3((unsigned)R), dim3(kIwBlock), 0, s, weights, ld_w, targets, logr, nll, logw, ld_out, group,
                       T, V);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int iw_finish_launch(const float* logw, const float* nll, long ld, long B, int K, double* out, hipStream_t s) {
    if (!logw || !nll || !out || B < 1 || B > kIwMaxRows || K < 1 || ld < K) return -1;
    ProfScope prof(PROF_HBM, 0.0, s, "iw_finish", 8.0 * (double)B * K + 40.0 * (double)B);
    hipLaunchKernelGGL(iw_finish_kernel, dim3((unsigned)((B + kIwWaves - 1) / kIwWaves)), dim3(kIwBlock), 0, s, logw, nll, ld, B, K,
                       out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
