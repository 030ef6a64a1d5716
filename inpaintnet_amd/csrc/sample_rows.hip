// The sampling row kernels outside the fused decode launches -- the multinomial draw and the four levels of sample.h's rule
// (temperature, truncated, constrained, forced), one wavefront per row -- and the counter-based dropout mask that shares the
// generator.  The four row kernels stay unfolded (DESIGN.md section 16 records why folding them failed).
#include <algorithm>
#include <cstdio>
#include "common.h"
#include "sample_rows.h"
#include "prof.h"
#include "pw_launch.h"
#include "reduce.h"
#include "sample.h"

namespace {

// Counter-based dropout mask: out = keep ? 1/(1-p) : 0, keep ~ Bernoulli(1-p).
// splitmix64-style hash of (seed, stream offset + element index): reproducible,
// rank-offsettable, no state.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__global__ void dropout_mask_kernel(float* __restrict__ out, long n, float p, uint64_t seed, uint64_t offset) {
    const float scale = 1.f / (1.f - p);
    const uint32_t thr = (uint32_t)((double)p * 4294967296.0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const uint64_t h = mix64(mix64(seed) ^ (offset + (uint64_t)i));
        out[i] = ((uint32_t)(h >> 32) >= thr) ? scale : 0.f;
    }
}

// samples[row*stride] ~ Multinomial(softmax(W[row,:]))  (decoder.py:506-509, sampling = 'multinomial'): one wavefront per
// row, inverse-CDF draw with one counter-based uniform per row (seed, offset + row): reproducible, rank-offsettable.
__global__ void sample_multinomial_kernel(const float* __restrict__ W, long ld_w, int rows, int V,
                                          long long* __restrict__ out, long stride, uint64_t seed, uint64_t offset) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int row = wave; row < rows; row += nwaves) {
        const float* w = W + (long)row * ld_w;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, w[v]);
        m = wave_max(m);
        float tot = 0.f;
        for (int v = lane; v < V; v += 64) tot += expf(w[v] - m);
        tot = wave_sum(tot);
        const uint64_t h = mix64(mix64(seed) ^ (offset + (uint64_t)row));
        const float target = (float)((uint32_t)(h >> 40)) * (1.f / 16777216.f) * tot;     // u in [0, 1) times the total mass
        // `tot` was summed lane-strided and across the wave, the prefix below runs in index order: the two can differ in the last
        // bits, so for u close to 1 no prefix need exceed the target.  The draw then is the LAST TOKEN WITH MASS (the inverse CDF at
        // u -> 1), not index V - 1, whose mass may be zero.  (The maximum has e = 1, so there is one; a row of NaN keeps V - 1.)
        float base = 0.f;
        int pick, last = V - 1;
        bool found = false;
        for (int v0 = 0; v0 < V && !found; v0 += 64) {
            const int v = v0 + lane;
            const float e = v < V ? expf(w[v] - m) : 0.f;
            const unsigned long long mass = __ballot(e > 0.f);
            if (mass) last = v0 + 63 - __builtin_clzll(mass);
            float incl = e;                                     // inclusive prefix sum over the 64 lanes
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            // e > 0: the lanes' prefixes are summed in different tree orders, so behind the last token with mass a lane's prefix can
            // come out an ulp ABOVE its neighbour's and cross the target where no lane with mass did
            const unsigned long long hit = __ballot(v < V && e > 0.f && base + incl > target);
            if (hit) { pick = v0 + __ffsll((long long)hit) - 1; found = true; }
            base += __shfl(incl, 63, 64);
        }
        if (!found) pick = last;
        if (lane == 0) out[(long)row * stride] = pick;
    }
}

// samples[row*stride] = the token sample.h's rule draws from softmax(temp * W[row,:]) with the uniform uniforms[row*u_stride] (the
// decoder's temperature sampling outside decode_b1.hip's launch; the same rule): one wavefront per row, V <= 64 NV.  Where the rule
// does not apply (a NaN among temp * W, a non-finite maximum or total, a uniform outside [0, 1)) the row takes argmax_first.
template <int NV>
__global__ void sample_temperature_kernel(const float* __restrict__ W, long ld_w, int rows, int V, float temp,
                                          const double* __restrict__ uniforms, long u_stride, long long* __restrict__ out, long stride) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int row = wave; row < rows; row += nwaves) {
        const float* w = W + (long)row * ld_w;
        const double u = uniforms[(long)row * u_stride];
        float x[NV], sv[NV], m = -INFINITY, ms = -INFINITY;
        bool nan = false;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = lane + 64 * j;
            x[j] = v < V ? w[v] : -INFINITY;
            sv[j] = v < V ? x[j] * temp : -INFINITY;
            nan |= sv[j] != sv[j];
            m = fmaxf(m, x[j]);
            ms = fmaxf(ms, sv[j]);
        }
        double S;                                              // (not read: the temperature draw has no logp)
        int tok = __ballot(nan) ? -1 : sample::pick<NV>(sv, wave_max(ms), u, V, lane, S);
        if (tok < 0) {
            m = wave_max(m);
            int am = kAmNone;
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (lane + 64 * j < V) am = min(am, am_key(x[j], m, lane + 64 * j));
            tok = am_index(wave_min(am));
        }
        if (lane == 0) out[(long)row * stride] = tok;
    }
}

// The same draw behind sample.h's top-k / nucleus truncation (sample::truncate in front of sample::pick: the decoder's truncated
// sampling outside decode_b1.hip's launch; the same rule), and logp[row*lp_stride] (nullable) = the drawn token's log-probability
// under the truncated distribution, NaN for a row that took argmax_first.  One wavefront per row, V <= 64 NV.
template <int NV>
__global__ void sample_truncated_kernel(const float* __restrict__ W, long ld_w, int rows, int V, float temp,
                                        const double* __restrict__ uniforms, long u_stride, int top_k, double top_p,
                                        long long* __restrict__ out, long stride, float* __restrict__ logp, long lp_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int row = wave; row < rows; row += nwaves) {
        const float* w = W + (long)row * ld_w;
        const double u = uniforms[(long)row * u_stride];
        float x[NV], sv[NV], m = -INFINITY, ms = -INFINITY;
        bool nan = false;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = lane + 64 * j;
            x[j] = v < V ? w[v] : -INFINITY;
            sv[j] = v < V ? x[j] * temp : -INFINITY;
            nan |= sv[j] != sv[j];
            m = fmaxf(m, x[j]);
            ms = fmaxf(ms, sv[j]);
        }
        int tok = -1;
        float lp = __builtin_nanf("");
        if (!__ballot(nan)) {
            ms = wave_max(ms);
            double S;
            sample::truncate<NV>(sv, ms, top_k, top_p, V, lane);
            tok = sample::pick<NV>(sv, ms, u, V, lane, S);
            if (tok >= 0) lp = sample::logp_of(sample::logp_gap<NV>(sv, ms, tok), S);
        }
        if (tok < 0) {
            m = wave_max(m);
            int am = kAmNone;
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (lane + 64 * j < V) am = min(am, am_key(x[j], m, lane + 64 * j));
            tok = am_index(wave_min(am));
        }
        if (lane == 0) {
            out[(long)row * stride] = tok;
            if (logp) logp[(long)row * lp_stride] = lp;
        }
    }
}

// The truncated draw behind sample.h's per-tick token constraints (the tick-by-tick path of a constrained decoder call; the same rule):
// allow + row * allow_stride = the row's ceil(V / 64) mask words (<= 8), read by every lane through a wave-uniform address.  An empty mask
// counts as all ones (sample::mask_words).  A row outside the rule takes argmax_first over its ALLOWED tokens -- the banned entries count
// as -inf and are no candidates, so the token is an allowed one whatever the logits hold -- with logp NaN.  One wavefront per row, V <= 64 NV.
template <int NV>
__global__ void sample_constrained_kernel(const float* __restrict__ W, long ld_w, int rows, int V, float temp,
                                          const double* __restrict__ uniforms, long u_stride, int top_k, double top_p,
                                          long long* __restrict__ out, long stride, float* __restrict__ logp, long lp_stride,
                                          const unsigned long long* __restrict__ allow, long allow_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int nw = (V + 63) / 64;
    for (int row = wave; row < rows; row += nwaves) {
        const float* w = W + (long)row * ld_w;
        const double u = uniforms[(long)row * u_stride];
        unsigned long long aw[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) aw[j] = j < nw ? allow[(long)row * allow_stride + j] : 0ull;
        sample::mask_words<NV>(aw, V);
        float x[NV], sv[NV], m = -INFINITY;
        bool nan = false;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = lane + 64 * j;
            x[j] = v < V ? w[v] : -INFINITY;
            sv[j] = v < V ? x[j] * temp : -INFINITY;
            nan |= sv[j] != sv[j];
            if (!sample::allowed(aw[j], lane)) x[j] = -INFINITY;
            m = fmaxf(m, x[j]);
        }
        int tok = -1;
        float lp = __builtin_nanf("");
        if (!__ballot(nan)) {
            const float ms = wave_max(sample::mask_scores<NV>(sv, aw, lane));
            double S;
            sample::truncate<NV>(sv, ms, top_k, top_p, V, lane);
            tok = sample::pick<NV>(sv, ms, u, V, lane, S);
            if (tok >= 0) lp = sample::logp_of(sample::logp_gap<NV>(sv, ms, tok), S);
        }
        if (tok < 0) {
            m = wave_max(m);
            int am = kAmNone;
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (sample::allowed(aw[j], lane)) am = min(am, am_key(x[j], m, lane + 64 * j));
            tok = am_index(wave_min(am));
        }
        if (lane == 0) {
            out[(long)row * stride] = tok;
            if (logp) logp[(long)row * lp_stride] = lp;
        }
    }
}

// The constrained draw behind sample.h's forced tokens (the tick-by-tick path of a forced decoder call; the same rule): forced[row *
// forced_stride] = the row's forced token, a value outside [0, V) = a free row, which is sample_constrained_kernel's row.  A forced row runs
// the same mask, truncation and pick (u = 0.0, for the kept total S alone), returns f whatever the mask, the truncation or the logits hold,
// and reports logp = (s_f - m) - log S: -inf where f is banned or truncated away, NaN where the rule does not apply.  A null `allow` counts
// as all ones.  One wavefront per row, V <= 64 NV.
template <int NV>
__global__ void sample_forced_kernel(const float* __restrict__ W, long ld_w, int rows, int V, float temp,
                                     const double* __restrict__ uniforms, long u_stride, int top_k, double top_p,
                                     long long* __restrict__ out, long stride, float* __restrict__ logp, long lp_stride,
                                     const unsigned long long* __restrict__ allow, long allow_stride,
                                     const int* __restrict__ forced, long forced_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int nw = (V + 63) / 64;
    for (int row = wave; row < rows; row += nwaves) {
        const float* w = W + (long)row * ld_w;
        const int f = forced[(long)row * forced_stride];
        const bool isf = sample::is_forced(f, V);
        const double u = isf ? 0.0 : uniforms[(long)row * u_stride];
        unsigned long long aw[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) aw[j] = j < nw ? (allow ? allow[(long)row * allow_stride + j] : ~0ull) : 0ull;
        sample::mask_words<NV>(aw, V);
        float x[NV], sv[NV], m = -INFINITY;
        bool nan = false;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = lane + 64 * j;
            x[j] = v < V ? w[v] : -INFINITY;
            sv[j] = v < V ? x[j] * temp : -INFINITY;
            nan |= sv[j] != sv[j];
            if (!sample::allowed(aw[j], lane)) x[j] = -INFINITY;
            m = fmaxf(m, x[j]);
        }
        int tok = -1;
        float lp = __builtin_nanf("");
        if (!__ballot(nan)) {
            const float ms = wave_max(sample::mask_scores<NV>(sv, aw, lane));
            double S;
            sample::truncate<NV>(sv, ms, top_k, top_p, V, lane);
            tok = sample::pick<NV>(sv, ms, u, V, lane, S);
            if (tok >= 0) lp = sample::logp_of(sample::logp_gap<NV>(sv, ms, isf ? f : tok), S);
        }
        if (isf) tok = f;
        if (tok < 0) {
            m = wave_max(m);
            int am = kAmNone;
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (sample::allowed(aw[j], lane)) am = min(am, am_key(x[j], m, lane + 64 * j));
            tok = am_index(wave_min(am));
        }
        if (lane == 0) {
            out[(long)row * stride] = tok;
            if (logp) logp[(long)row * lp_stride] = lp;
        }
    }
}

}  // namespace

int pw_dropout_mask(float* out, long n, float p, uint64_t seed, uint64_t offset, hipStream_t s) {
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(n)), dim3(256), 0, s, out, n, p, seed, offset);
    return ok();
}
int pw_sample_multinomial(const float* W, long ld_w, int rows, int V, long long* out, long stride, uint64_t seed,
                          uint64_t offset, hipStream_t s) {
    hipLaunchKernelGGL(sample_multinomial_kernel, dim3(grid_for((long)rows * 64, 256, 1024)), dim3(256), 0, s, W, ld_w, rows, V,
                       out, stride, seed, offset);
    return ok();
}
int pw_sample(const float* W, long ld_w, int rows, int V, long long* out, long stride, const sample::Request& r, int floor_level,
              hipStream_t s) {
    if (!r.uniforms || r.logits || !r.ok(V)) return -1;
    const int level = std::max(std::min(floor_level, 2), r.level(V));      // (a floor above 2 would read a null mask or forced array)
    char label[48];
    if (level == 1) std::snprintf(label, sizeof label, "sample_temperature B%d V%d", rows, V);
    else std::snprintf(label, sizeof label, "%ssample B%d V%d", sample::prefix(level), rows, V);
    // per row: the logits, the uniform and the token; from level 2 the log-probability, the mask words where given, at level 4 the forced word
    ProfScope prof(PROF_HBM, 0.0, s, label, (double)rows * (4.0 * V + 16.0 + (level >= 2 ? 4.0 : 0.0) + (level >= 4 ? 4.0 : 0.0) +
                                                            (r.allow ? 8.0 * sample::Request::words(V) : 0.0)));
    const dim3 grid(grid_for((long)rows * 64, 256, 1024));
    const float temp = r.temperature;
#define PW_ST(NV)                                                                                                                         \
    do { switch (level) {                                                                                                                 \
        case 1: hipLaunchKernelGGL(sample_temperature_kernel<NV>, grid, dim3(256), 0, s, W, ld_w, rows, V, temp, r.uniforms, r.ld_u, out,   \
                                   stride); break;                                                                                        \
        case 2: hipLaunchKernelGGL(sample_truncated_kernel<NV>, grid, dim3(256), 0, s, W, ld_w, rows, V, temp, r.uniforms, r.ld_u, r.top_k, \
                                   r.top_p, out, stride, r.logp, r.ld_logp); break;                                                       \
        case 3: hipLaunchKernelGGL(sample_constrained_kernel<NV>, grid, dim3(256), 0, s, W, ld_w, rows, V, temp, r.uniforms, r.ld_u,       \
                                   r.top_k, r.top_p, out, stride, r.logp, r.ld_logp, r.allow, r.ld_allow); break;                         \
        default: hipLaunchKernelGGL(sample_forced_kernel<NV>, grid, dim3(256), 0, s, W, ld_w, rows, V, temp, r.uniforms, r.ld_u, r.top_k,  \
                                    r.top_p, out, stride, r.logp, r.ld_logp, r.allow, r.ld_allow, r.forced, r.ld_forced);                 \
    } } while (0)
    if (V <= 64) PW_ST(1); else if (V <= 128) PW_ST(2); else if (V <= 256) PW_ST(4); else PW_ST(8);
#undef PW_ST
    return ok();
}
