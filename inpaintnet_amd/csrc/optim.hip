// The optimizer step over the flat arena and, in front of it, the norm of the gradient arena; the step-flag export and the epoch
// statistics that take the step's skip decision.  Grid-stride, 16 bytes per lane; the workgroup sums are reduce.h's block_sum.
#include <cmath>
#include "common.h"
#include "optim.h"
#include "prof.h"
#include "chain.h"
#include "pw_launch.h"
#include "reduce.h"

namespace {

// ---- the optimizer step and, in front of it, the norm of the gradient arena.  grad_sqnorm_kernel leaves kSqnormParts f64 partial sums
// of squares; adamw_kernel, the ONE step kernel behind every inet_adam_step* entry point, adds them up itself (clip rule, below).
constexpr int kSqnormParts = 1024;               // workgroups of grad_sqnorm_kernel = doubles of its output
constexpr int kSqnormBlock = 256;

// partials[b] = the squares of workgroup b's grid-stride share of g, in f64.  EVERY workgroup stores (one without elements: 0.0), with a
// plain store: nothing to zero in front, no atomics, no hand-off between workgroups -- the consumer is the next launch.
__global__ void __launch_bounds__(kSqnormBlock) grad_sqnorm_kernel(const float* __restrict__ g, long n, double* __restrict__ partials) {
    __shared__ double part[4];
    const long n4 = n >> 2;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    const long stride = (long)gridDim.x * blockDim.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;                   // one chain per element slot of the 16-byte load
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // four loads in flight per lane: the grid holds 4 MB per pass, the HBM pipe wants more than that outstanding
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 x0 = g4[i], x1 = g4[i + stride], x2 = g4[i + 2 * stride], x3 = g4[i + 3 * stride];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x4 x = k == 0 ? x0 : k == 1 ? x1 : k == 2 ? x2 : x3;
            a0 = fma((double)x[0], (double)x[0], a0);
            a1 = fma((double)x[1], (double)x[1], a1);
            a2 = fma((double)x[2], (double)x[2], a2);
            a3 = fma((double)x[3], (double)x[3], a3);
        }
    }
    for (; i < n4; i += stride) {
        const f32x4 x = g4[i];
        a0 = fma((double)x[0], (double)x[0], a0);
        a1 = fma((double)x[1], (double)x[1], a1);
        a2 = fma((double)x[2], (double)x[2], a2);
        a3 = fma((double)x[3], (double)x[3], a3);
    }
    // tail, as the step kernel's
    for (long t = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) a0 = fma((double)g[t], (double)g[t], a0);
    const double s = block_sum((a0 + a1) + (a2 + a3), part);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- the optimizer step: torch.optim.Adam / AdamW (2.x single-tensor form) over the flat arena, optionally
// behind global-norm clipping, with decoupled weight decay and with EMA shadow weights.  One kernel; the rule, stated once.
//
// Skip and report.  A chain kernel gave up waiting for its group (chain.h): the gradients of the step are not valid, so the step leaves
// every arena as it is.  Which word decides: `step_flag` when the caller passes one -- the flags of ALL ranks summed with the gradients
// (inet_step_flag_export + the all-reduce), so that every rank of a data-parallel job takes the same decision --, else this process's own
// device word.  `report` (nullable; host-mapped words the caller owns and zeroed) tells the host what was decided (encoder.py:111-116,
// decoder.py:424-429): [0] = 1 the kernel ran, [1] = 1 the flag skipped the step, [2] = 1 a parameter left the finite range, [3] = 1
// SOME rank's prologue kernels met a token outside the vocabulary (step_flag[1] = the ranks' exported token words: every rank raises the
// reference's check_index ValueError at the same step).  WITHOUT partials only these four words are ever stored to: a record of four
// words is enough.  With partials the record has eight: [4] = 1 clipped, [5] = 1 dropped for a non-finite gradient, [6] = the bits of
// (float)norm (also on a skip), [7] stays 0.
//
// Clipping (partials given: what grad_sqnorm_kernel left for the gradient arena g[0..n); 0 < max_norm <= +inf; section 18):
//   1. S = sum (double)g_i * (double)g_i: every square exact in f64, the sum in f64 in a FIXED order that depends on n only.  Every
//      workgroup sums the kSqnormParts partials itself, in the SAME order (lane-strided reads, the same tree), so that all of them derive
//      norm, c, scale and the decision bit for bit alike.  norm = |gscale| * sqrt(S) in f64.
//   2. nonfinite = !isfinite(norm)  (a finite f32 arena cannot overflow the f64 sum: true iff some element is inf or NaN).
//   3. c = max_norm / (norm + 1e-6) in f64 (torch's clip_grad_norm_ coefficient); scale = c < 1 ? (float)c : 1.0f;
//      clipped = c < 1.  max_norm = +inf never clips.
//   4. the chain / step flag says skip: the step is skipped, nonfinite and clipped are reported as 0.
//   5. else nonfinite: every arena stays untouched, report[5] = 1, report[1] and report[2] stay 0 (not a chain failure).
//   6. else the step below with gs = the ONE f32 product gscale * scale.
// Without partials gs = gscale, max_norm is ignored and only the flag skips.
//
// Decay and EMA (section 19).  weight_decay >= 0; a nullable decay mask (bit i & 31 of word i >> 5 set: element i decays; null: every
// element decays); a nullable arena ema[0..n) and ema_decay in [0, 1).  The launcher rounds the factors ONCE, on the host:
// lr_over_bc1 = (float)(lr / (1 - b1^step)), inv_sqrt_bc2 = (float)(1 / sqrt(1 - b2^step)), decay = (float)(1.0 - (double)lr *
// (double)weight_decay) -- exactly 1.0f for weight_decay == 0 --, omd = (float)(1.0 - (double)ema_decay).  A skipped or dropped step
// leaves p, m, v AND ema bit for bit untouched.
//
// The applied step, per element, every operation in f32 and every rounding spelled out -- contraction is OFF in the kernel and each fused
// operation is written as an fmaf, so the bits do not depend on what a compiler would contract (tests/test_gpu_adam_bits.py holds them to
// a recording):
//   gr    = g * gs
//   m     = fmaf(1 - b1, gr, b1 * m)
//   v     = fmaf(b2, v, gr * ((1 - b2) * gr))        in the 16-byte body;
//           b2 * v + gr * ((1 - b2) * gr)            in the scalar tail: BOTH products rounded, then the sum.  An oddity, and part of the
//                                                    recorded bits: the last n & 3 elements round v once more than the rest
//   denom = fmaf(sqrtf(v), inv_sqrt_bc2, eps)        (torch: sqrt(v) / sqrt(bc2) + eps)
//   p1    = decays(i) ? p * decay : p                (torch's _single_tensor_adamw order, param.mul_(1 - lr * wd) first; the product is
//                                                    rounded on its own, never fused into what follows: p * 1.0f is p)
//   p     = fmaf(-lr_over_bc1, m / denom, p1);       report[2] tests this p
//   ema   = fmaf(ema_decay, ema, omd * p)            (ema given; the product rounded on its own: ema_decay == 0 gives ema == p)
//
// The grid is grid_for(n / 4 + 1, 256, 4096) workgroups of kSqnormBlock threads, grid-stride over 16-byte groups, then the n & 3 elements
// of the tail.  EMA / MASK: whether `ema` / `mask` are given -- compile-time, so that the plain form carries neither loads nor
// registers of the other three.  Four consecutive elements never straddle a mask word: the body reads ONE word per 16 bytes.
template <bool EMA, bool MASK>
__global__ void __launch_bounds__(kSqnormBlock)
adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
             float lr_over_bc1, float inv_sqrt_bc2, float b1, float b2, float eps, float gscale, float max_norm,
             const double* __restrict__ partials, float decay, const unsigned* __restrict__ mask, float* __restrict__ ema,
             float ema_decay, float omd, const unsigned* __restrict__ abort_word, const float* __restrict__ step_flag,
             unsigned* __restrict__ report) {
#pragma clang fp contract(off)
    __shared__ double part[4];
    const bool skip = step_flag ? (*step_flag != 0.f)
                                : (abort_word && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u);
    bool nonfinite = false, clipped = false;
    double norm = 0.0, c = 1.0;
    if (partials) {                                  // uniform over the grid: steps 1-3 of the clip rule
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < kSqnormParts / kSqnormBlock; ++k) acc += partials[threadIdx.x + k * kSqnormBlock];
        const double S = block_sum(acc, part);
        norm = fabs((double)gscale) * sqrt(S);
        nonfinite = !skip && !(fabs(norm) <= 1.7976931348623157e308);          // NaN or +inf
        c = (double)max_norm / (norm + 1e-6);
        clipped = !skip && !nonfinite && c < 1.0;
    }
    if (report && blockIdx.x == 0 && threadIdx.x == 0) {
        __hip_atomic_store(report + 0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (skip) __hip_atomic_store(report + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (step_flag && step_flag[1] != 0.f) __hip_atomic_store(report + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (partials) {
            if (clipped) __hip_atomic_store(report + 4, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (nonfinite) __hip_atomic_store(report + 5, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(report + 6, __float_as_uint((float)norm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (skip || nonfinite) return;
    const float gs = partials ? gscale * (clipped ? (float)c : 1.0f) : gscale;
    const float omb1 = 1.f - b1, omb2 = 1.f - b2;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    bool bad = false;
    const long n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    f32x4* e4 = reinterpret_cast<f32x4*>(ema);
    for (long i = tid; i < n4; i += stride) {
        f32x4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i], ee;
        if (EMA) ee = e4[i];
        unsigned bits = 0xfu;
        if (MASK) bits = mask[i >> 3] >> (((unsigned)i & 7u) << 2);            // elements 4i .. 4i+3: word (4i) >> 5, bit (4i) & 31
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gr = gg[e] * gs;
            mm[e] = fmaf(omb1, gr, b1 * mm[e]);
            vv[e] = fmaf(b2, vv[e], gr * (omb2 * gr));
            const float denom = fmaf(sqrtf(vv[e]), inv_sqrt_bc2, eps);
            const float p1 = (!MASK || ((bits >> e) & 1u)) ? pp[e] * decay : pp[e];
            pp[e] = fmaf(-lr_over_bc1, mm[e] / denom, p1);
            bad |= !(fabsf(pp[e]) <= 3.402823466e38f);          // NaN or +-inf
            if (EMA) ee[e] = fmaf(ema_decay, ee[e], omd * pp[e]);
        }
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (EMA) e4[i] = ee;
    }
    for (long i = (n4 << 2) + tid; i < n; i += stride) {          // tail: the mask per element; v's sum rounds both products
        const float gr = g[i] * gs;
        const float mm = fmaf(omb1, gr, b1 * m[i]);
        const float vv = b2 * v[i] + gr * (omb2 * gr);
        m[i] = mm; v[i] = vv;
        const float p1 = (!MASK || ((mask[i >> 5] >> ((unsigned)i & 31u)) & 1u)) ? p[i] * decay : p[i];
        const float pn = fmaf(-lr_over_bc1, mm / fmaf(sqrtf(vv), inv_sqrt_bc2, eps), p1);
        p[i] = pn;
        bad |= !(fabsf(pn) <= 3.402823466e38f);
        if (EMA) ema[i] = fmaf(ema_decay, ema[i], omd * pn);
    }
    if (bad && report) __hip_atomic_store(report + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// dst[0] = 1 if a chain launch of this process has timed out since the last reset, else 0: the word a data-parallel caller sums
// over ranks together with the gradients (inet_step_flag_export)
// dst[1] = 1 if a prologue kernel of this process has met a token outside the vocabulary since the last reset (the host-mapped
// word behind inet_token_status): decoder.py:36-45's ValueError, raised by all ranks together
__global__ void step_flag_export_kernel(const unsigned* abort_word, const unsigned* tok_word, float* dst) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        dst[0] = (abort_word && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ? 1.f : 0.f;
        dst[1] = (tok_word && __hip_atomic_load(tok_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) ? 1.f : 0.f;
    }
}

}  // namespace

int pw_sqnorm_parts() { return kSqnormParts; }
int pw_grad_sqnorm(const float* g, long n, double* partials, hipStream_t s) {
    ProfScope prof(PROF_HBM, 0.0, s, "grad_sqnorm", 4.0 * (double)n);         // one read of the arena
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(kSqnormParts), dim3(kSqnormBlock), 0, s, g, n, partials);
    return ok();
}
template <bool EMA, bool MASK>
static void launch_adam_step(const PwAdamStep& a, float lr_over_bc1, float inv_sqrt_bc2, float decay, float omd, hipStream_t s) {
    hipLaunchKernelGGL((adamw_kernel<EMA, MASK>), dim3(grid_for(a.n / 4 + 1, 256, 4096)), dim3(kSqnormBlock), 0, s, a.p, a.g, a.m, a.v,
                       a.n, lr_over_bc1, inv_sqrt_bc2, a.b1, a.b2, a.eps, a.gscale, a.max_norm, a.partials, decay, a.mask, a.ema,
                       a.ema_decay, omd, (const unsigned*)chain_dev_status(), a.step_flag, a.report);
}
int pw_adam_step(const PwAdamStep& a, hipStream_t s) {
    const double bc1 = 1.0 - pow((double)a.b1, a.step), bc2 = 1.0 - pow((double)a.b2, a.step);
    // the factors of the rule, rounded ONCE here: what the kernel multiplies by does not depend on how it was compiled
    const float l1 = (float)(a.lr / bc1), is2 = (float)(1.0 / sqrt(bc2));
    const float decay = (float)(1.0 - (double)a.lr * (double)a.weight_decay), omd = (float)(1.0 - (double)a.ema_decay);
    // the label says what the launch does: "w" with decay or an EMA, "_clip" behind the partials
    const bool w = a.weight_decay > 0.f || a.ema;
    // read p,g,m,v; write p,m,v + a bit per element of the mask + one read and one write of the EMA arena + the partials
    ProfScope prof(PROF_HBM, 0.0, s, w ? (a.partials ? "adamw_clip" : "adamw") : (a.partials ? "adam_clip" : "adam"),
                   28.0 * (double)a.n + (a.mask ? (double)a.n / 8.0 : 0.0) + (a.ema ? 8.0 * (double)a.n : 0.0) +
                       (a.partials ? 8.0 * kSqnormParts : 0.0));
    if (a.ema) { if (a.mask) launch_adam_step<true, true>(a, l1, is2, decay, omd, s); else launch_adam_step<true, false>(a, l1, is2, decay, omd, s); }
    else       { if (a.mask) launch_adam_step<false, true>(a, l1, is2, decay, omd, s); else launch_adam_step<false, false>(a, l1, is2, decay, omd, s); }
    return ok();
}
int pw_step_flag_export(float* dst, hipStream_t s) {
    hipLaunchKernelGGL(step_flag_export_kernel, dim3(1), dim3(64), 0, s, (const unsigned*)chain_dev_status(),
                       (const unsigned*)token_host_status(), dst);
    return ok();
}

// sums[0..2] += (loss, accuracy, 1) unless a chain launch of this process has timed out since the last reset: the statistics of
// steps whose results are not valid (and that the optimizer kernel skipped) stay out of the epoch means
__global__ void epoch_stats_add_kernel(float* sums, const float* loss, const float* acc, const unsigned* abort_word,
                                       const float* step_flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    // the same decision as the optimizer kernel of the step (adamw_kernel): the ranks' summed flag if the caller has one
    if (step_flag ? (*step_flag != 0.f)
                  : (abort_word && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) return;
    sums[0] += loss[0];
    if (acc) sums[1] += acc[0];
    sums[2] += 1.f;
}
int pw_epoch_stats_add(float* sums, const float* loss, const float* acc, hipStream_t s, const float* step_flag) {
    hipLaunchKernelGGL(epoch_stats_add_kernel, dim3(1), dim3(64), 0, s, sums, loss, acc, (const unsigned*)chain_dev_status(),
                       step_flag);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
