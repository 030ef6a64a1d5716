// Temperature sampling of one token in numpy's order, for the generation of AnticipationRNN
// (AnticipationRNN/anticipation_rnn_gauss_reg_model.py:655-667: preds = softmax(T * logits); np.random.choice(V, p=preds)).
// np.random.choice draws ONE random_sample() double u per call and returns searchsorted(cumsum(p) / sum(p), u, 'right'): the first
// v whose inclusive prefix exceeds u.  Here e_v = exp(s_v - max s) in f32 (s = T x, the reference's f32 softmax numerator), the
// prefix over v in f64 (a wave scan over 64 lanes x NV chunks: DPP shifts inside the 16-lane rows, the row totals by readlane), and
// token = the first v with prefix_v > u * S, S = the total, by ballot and ctz.  The result is wave-uniform.
// Below, in this order: pick(), truncate(), the mask and forced-token helpers, draw() -- the device rule of one (row, tick), one build per
// level -- and, host side, Request: what a CALL asks of the draw, carried as one value from the C-ABI entries to the launch sites of
// vae.hip, decode_b1.hip, arnn_gen.hip and sample_rows.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "common.h"
#include "reduce.h"

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
// takes the argmax rule.  The result lies in [0, V) or is -1.  S = the total the threshold was taken of (the kept total behind
// truncate(); 0 with -1): what logp_of() needs -- a caller that does not read it lets it die.
template <int NV>
__device__ __forceinline__ int pick(const float (&s)[NV], float m, double u, int V, int lane, double& S) {
    S = 0.0;
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
    S = carry;
    const double thr = u * carry;
    int tok = -1;
#pragma unroll
    for (int j = NV - 1; j >= 0; --j) {
        const unsigned long long b = __ballot(lane + 64 * j < V && pre[j] > thr);
        if (b) tok = 64 * j + __builtin_ctzll(b);
    }
    return tok;
}

// TOP-K / NUCLEUS TRUNCATION in front of pick().  Order the tokens by (s_v descending, v ascending); K = top_k if 1 <= top_k < V, else V;
// A_i = the f64 sum of e_v = expf(s_v - m) over the first i tokens of the order; n = the smallest i <= K with A_i >= top_p A_K (top_p
// >= 1: n = K, nothing evaluated); the first n tokens are kept.  A token with r tokens in front of it is kept iff r < K and A_r < top_p
// A_K (A is monotone, A_0 = 0 < top_p A_K: the top-ranked token always stays, so m stays the maximum).  Dropped tokens get s = -inf:
// e = 0 in pick(), which then is the rule on the truncated distribution.
// How: passes over the V tokens w in index order, s_w by readlane with a wave-uniform lane, every lane looking at its own tokens v.
// Top-k: count the w that rank in front of v -- exact integer counts of f32 comparisons, so ties (every zero logit ties with every
// other) fall lowest index first with nothing to round -- and keep the ballot of rank < K.  Nucleus: A_K = the wave's f64 sum of e over
// that ballot, then per 64-token chunk of v a second pass that adds up e_w (f64) of the w in front of v.  What stays live between the
// passes are ballots (scalar registers); per lane a pass holds NV counters or ONE f64 sum next to s.  V x (a readlane + NV x (2
// compares, an add)) for top-k, V x NV x (readlane, expf, 2 compares, an f64 add) for the nucleus: linear in V with no sort.  (Measured
// against ONE pass that keeps e, the counters and the f64 sums per lane and reads e_w by a second readlane: that one is slower in the
// decode kernel, +4.1 against +2.7 us per tick for top-k and +6.5 against +6.1 for the nucleus at b = 1 -- DESIGN.md section 11.)  A
// radix descent over the 32 key bits with a masked f64 wave sum per bit would cost 32 x (NV selects + an f64 wave reduction of ~25
// DPP / readlane steps), more than these passes for the decoder's V <= 128.
// s[j] of v >= V must be -inf and no s may be NaN (as for pick()); m not finite: nothing is done (pick() refuses it).
template <int NV>
__device__ __forceinline__ void truncate(float (&s)[NV], float m, int top_k, double top_p, int V, int lane) {
    const int K = (top_k >= 1 && top_k < V) ? top_k : V;
    const bool nucleus = top_p < 1.0;
    if ((K == V && !nucleus) || !(m > -INFINITY && m < INFINITY)) return;
    unsigned long long keep[NV];                                            // ballots: token lane + 64 j stays
#pragma unroll
    for (int j = 0; j < NV; ++j) keep[j] = __ballot(lane + 64 * j < V);
    if (K < V) {
        int rank[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) rank[j] = 0;
#pragma unroll
        for (int jw = 0; jw < NV; ++jw) {
            const int n = V - 64 * jw < 64 ? V - 64 * jw : 64;              // (wave-uniform; <= 0 beyond the vocabulary)
            for (int l = 0; l < n; ++l) {
                const float sw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s[jw]), l));
                const int w = 64 * jw + l;
#pragma unroll
                for (int j = 0; j < NV; ++j) rank[j] += (sw > s[j] || (sw == s[j] && w < lane + 64 * j)) ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) keep[j] &= __ballot(rank[j] < K);
    }
    if (nucleus) {
        double ak = 0.0;                                                    // A_K: the mass of what top-k kept
#pragma unroll
        for (int j = 0; j < NV; ++j)
            ak += readlane_d(wave_scan(((keep[j] >> lane) & 1) ? (double)expf(s[j] - m) : 0.0, lane), 63);
        const double thr = top_p * ak;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double before = 0.0;                                            // A_r of token v = lane + 64 j: the mass ranked in front of it
#pragma unroll
            for (int jw = 0; jw < NV; ++jw) {
                const int n = V - 64 * jw < 64 ? V - 64 * jw : 64;
                for (int l = 0; l < n; ++l) {
                    const float sw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s[jw]), l));
                    const double ew = (double)expf(sw - m);                 // (wave-uniform; the value pick() sums)
                    before += (sw > s[j] || (sw == s[j] && 64 * jw + l < lane + 64 * j)) ? ew : 0.0;
                }
            }
            // (a token in front of a kept one is kept: `before` of a token inside the top K is a sum over the top K alone)
            keep[j] &= __ballot(before < thr);
        }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (!((keep[j] >> lane) & 1)) s[j] = -INFINITY;
}

// PER-TICK TOKEN CONSTRAINTS in front of truncate() / pick() (DESIGN.md section 13 has the same text).
//
// Mask layout.  `allow` is an array of 64-bit words [rows][T][NW], with NW = ceil(V / 64).  Token v is allowed iff bit v % 64 of word
// v / 64 is set.  Bits at or above V are ignored.  A null `allow` means no constraint.
//
// For one (row, tick), with logits x[0..V), temperature T, uniform u, top_k and top_p:
//  0. Empty mask.  A mask with no bit set in [0, V) counts as all ones for that tick.  The Python surfaces refuse such a tick with
//     ValueError before any launch.
//  1. Scores.  s_v = T x_v in f32.  The NaN test of section 10 runs over all V values of s, as today.  The mask therefore does not change
//     which ticks fall back.  Then s_v = -inf for every banned v, and m = the maximum over the allowed tokens.
//  2. Truncation and draw.  Steps 2-7 of section 11 run unchanged on these s, with V and K = top_k unchanged.  Banned tokens tie at -inf
//     and rank last.  Their e = expf(-inf - m) is 0, so they add no mass and cannot be the first prefix above u S.  A top_k above the
//     number of allowed tokens keeps all of them.  logp is taken under the masked and truncated distribution.
//  3. Fallback.  Where the rule does not apply (a NaN among s, m or S not finite, u outside [0, 1) or NaN), the tick takes today's argmax
//     rule on the logits with every banned entry replaced by -inf.  The decode kernel may use its padding value -1 instead, which lies
//     below every post-ReLU logit.  logp is NaN there.  The token is still an allowed one.
//
// The mask words of one (row, tick) are wave-uniform (every lane holds all NV of them; scalar registers where the address is uniform).
// mask_words(): step 0 -- the words with the bits at or above V cleared, or the words of the full vocabulary where none is left.
template <int NV>
__device__ __forceinline__ void mask_words(unsigned long long (&aw)[NV], int V) {
    unsigned long long any = 0ull;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int n = V - 64 * j;                                           // tokens of this word
        const unsigned long long valid = n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1ull;
        aw[j] &= valid;
        any |= aw[j];
    }
    if (!any) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int n = V - 64 * j;
            aw[j] = n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1ull;
        }
    }
}
__device__ __forceinline__ bool allowed(unsigned long long word, int lane) { return (word >> lane) & 1ull; }
// mask_scores(): step 1 behind the NaN test -- s = -inf for the banned lanes (aw from mask_words()); returns THIS LANE's maximum over
// its allowed tokens (-inf without one): the caller reduces it over the wave with the reduction it has, and that is m.
template <int NV>
__device__ __forceinline__ float mask_scores(float (&s)[NV], const unsigned long long (&aw)[NV], int lane) {
    float ms = -INFINITY;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (!allowed(aw[j], lane)) s[j] = -INFINITY;
        ms = fmaxf(ms, s[j]);
    }
    return ms;
}

// FORCED TOKENS behind the per-tick constraints (DESIGN.md section 15 has the same text).
//
// Layout.
//  - `forced` is an array of `int32` `[rows][T]`.
//  - A value `f` with `0 <= f < V` forces that tick.
//  - Every other value makes the tick free.  The Python surfaces write -1 for a free tick.
//  - A null `forced` means no tick is forced.
//
// At a free tick nothing changes.  Section 13's rule runs as it does today.
//
// At a forced tick with token `f`:
//  1. Scores and truncation.
//     - Steps 0-2 of section 13 run unchanged on the tick's logits: s = T x in f32, the NaN test, the mask, m, and the top-k / nucleus
//       truncation.
//     - S is the kept total.
//     - The tick's uniform is not used.  The rule is evaluated as with u = 0, so a uniform outside [0, 1) or NaN at a forced tick causes
//       no fallback.
//  2. Token.
//     - The token is `f`.  It is reported in `samples` and fed back into tick t + 1.
//     - This holds whether or not `f` is allowed or kept, and it holds on a fallback tick too.
//  3. Log-probability.  logp = (s_f - m) - log S as f32.
//     - It is exactly -inf when `f` is banned or truncated away (s_f = -inf).
//     - It is NaN where the rule does not apply: a NaN among s, or m or S not finite.
//
// Consequences.  The tests hold each of these exactly.
//  (a) No forced tick.  A null `forced`, or one with no value in [0, V), gives inet_vae_decoder_sample_cx bit for bit in tokens, logits
//      and logp.
//  (b) Replay.  Force, at every tick, the tokens that a sampled, truncated or constrained call returned.  The replay uses the same
//      temperature, top_k, top_p and mask, and any uniforms at all.  It returns that call's logits and logp bit for bit, with NaN where
//      that call had NaN.
//  (c) A banned forced token is still returned and fed back.  Its logp is -inf.
//  (d) One-bit mask.  A forced tick whose mask has the single bit `f` set has logp exactly 0.0f.
//  (e) Free ticks of a partly forced call follow section 13's rule on the trajectory behind the forced tokens.
//
// How: the callers run mask_scores(), truncate() and pick() (u = 0.0 at a forced tick, for S) as at a free tick, then take tok = f and
// logp_gap(s, m, f).  The forced word of one (row, tick) is wave-uniform like the mask words.
__device__ __forceinline__ bool is_forced(int f, int V) { return (unsigned)f < (unsigned)V; }

// The log-probability of the drawn token under the (truncated) distribution pick() drew from is (s_tok - m) - log(S), stored as f32, in
// two halves: logp_gap() = s_tok - m (f32; tok in [0, V) from pick(); wave-uniform) where the draw is made, logp_of() where there are
// registers for an f64 logarithm -- decode_b1.hip's pick has none to spare and takes the logarithms behind its last tick.
template <int NV>
__device__ __forceinline__ float logp_gap(const float (&s)[NV], float m, int tok) {
    float st = m;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if ((tok >> 6) == j) st = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s[j]), tok & 63));
    return st - m;
}
__device__ __forceinline__ float logp_of(float gap, double S) { return (float)((double)gap - log(S)); }

// THE DRAW of one (row, tick): the rule above as one function, in builds of one LEVEL each -- 1 = temperature, 2 = truncated, 3 = masked,
// 4 = forced; every step stands behind its level, so a lower build carries nothing of a higher one.
//  x[j] = the logit of v = lane + 64 j (anything for v >= V); u = the tick's uniform; aw = the tick's mask words behind mask_words()
//  (level 3 up; below it any array), f = the tick's forced word (level 4).
//  -> the token; gap = s_tok - m (logp_gap()); S = the kept total.  Where the rule does not apply: -1, gap NaN and S = 1 -- the caller
//  then takes ITS argmax rule (they differ: the decode kernel's padding -1, AnticipationRNN's NaN-aware order over the allowed entries,
//  reduce.h's am_key in sample_rows.hip).  A forced tick returns f, never -1, with gap NaN and S = 1 where the rule does not apply.
// s_v = T x_v is ONE rounded f32 product that the NaN test and expf(s_v - m) both read.
template <int NV, int LEVEL, int NA>
__device__ __forceinline__ int draw(const float (&x)[NV], float temp, double u, int V, int lane, int top_k, double top_p,
                                    const unsigned long long (&aw)[NA], int f, float& gap, double& S) {
    static_assert(LEVEL >= 1 && LEVEL <= 4 && (LEVEL < 3 || NA == NV), "one mask word per 64 tokens from the masked build up");
    const bool forced = LEVEL >= 4 && is_forced(f, V);
    float s[NV], ms = -INFINITY;
    bool nan = false;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        s[j] = lane + 64 * j < V ? x[j] * temp : -INFINITY;
        nan |= s[j] != s[j];
        if constexpr (LEVEL < 3) ms = fmaxf(ms, s[j]);
    }
    gap = __builtin_nanf("");
    S = 1.0;
    if (__ballot(nan)) return forced ? f : -1;
    if constexpr (LEVEL >= 3) ms = mask_scores<NV>(s, aw, lane);
    ms = wave_max_dpp(ms);
    if constexpr (LEVEL >= 2) truncate<NV>(s, ms, top_k, top_p, V, lane);
    int tok = pick<NV>(s, ms, forced ? 0.0 : u, V, lane, S);
    if (tok >= 0) {
        if (forced) tok = f;
        gap = logp_gap<NV>(s, ms, tok);
    } else S = 1.0;
    return forced ? f : tok;
}

// The prefix of a level's launch labels.
constexpr const char* prefix(int level) {
    return level == 4 ? "force_" : level == 3 ? "cons_" : level == 2 ? "trunc_" : level == 1 ? "sample_" : "";
}

// THE REQUEST of a call, host side: everything a caller may ask of the draw, as ONE value from the C-ABI entry (api.hip builds it and asks
// ok()) to the place a kernel-argument struct is filled, which reads it field by field.  The default value is the argmax call.  Arrays are
// per (row, tick): row r of `x` starts at x + r * ld_x, tick t behind it (logits: t * V floats, allow: t * ceil(V / 64) words).
struct Request {
    const double* uniforms = nullptr;            // one uniform per (row, tick); null: the argmax rule, and nothing below may be set
    float temperature = 1.f;                     // the logits' factor in front of the softmax
    int top_k = 0; double top_p = 1.0;           // truncate(): top_k <= 0 or >= V: off; top_p in (0, 1], 1: off
    float* logp = nullptr;                       // the drawn tokens' log-probabilities, or null
    float* logits = nullptr;                     // [.., V] what each tick drew from (AnticipationRNN alone), or null
    const unsigned long long* allow = nullptr;   // [.., ceil(V / 64)] the allowed tokens' words, or null: no constraint
    const int* forced = nullptr;                 // the forced tokens, or null: no tick is forced
    long ld_u = 0, ld_logp = 0, ld_logits = 0, ld_allow = 0, ld_forced = 0;   // the row strides, in elements

    // the strides of contiguous [rows][T] arrays
    Request& dense(int T, int V) {
        ld_u = ld_logp = ld_forced = T; ld_logits = (long)T * V; ld_allow = (long)T * words(V);
        return *this;
    }
    static constexpr int words(int V) { return (V + 63) / 64; }
    template <class P> static P* at(P* p, long off) { return p ? p + off : nullptr; }
    // the request of the rows from r0 on / of the ticks from t on: every array moved, null stays null
    Request rows(long r0) const {
        Request q = *this;
        q.uniforms = at(uniforms, r0 * ld_u); q.logp = at(logp, r0 * ld_logp); q.logits = at(logits, r0 * ld_logits);
        q.allow = at(allow, r0 * ld_allow); q.forced = at(forced, r0 * ld_forced);
        return q;
    }
    Request tick(long t, int V) const {
        Request q = *this;
        q.uniforms = at(uniforms, t); q.logp = at(logp, t); q.logits = at(logits, t * V);
        q.allow = at(allow, t * words(V)); q.forced = at(forced, t);
        return q;
    }
    // a truncating call: truncation on, or something only the truncating kernels read or write
    bool truncating(int V) const { return (top_k >= 1 && top_k < V) || top_p < 1.0 || logp || logits || allow || forced; }
    // 0 = argmax (no uniforms), 1 = temperature, 2 = truncated, 3 = masked, 4 = forced: draw()'s LEVEL
    int level(int V) const { return !uniforms ? 0 : forced ? 4 : allow ? 3 : truncating(V) ? 2 : 1; }
    // what every entry refuses: a top_p outside (0, 1] (a NaN too), anything asked of an argmax call, a temperature that is not finite,
    // more tokens than the widest build holds
    bool ok(int V) const {
        if (!(top_p > 0.0 && top_p <= 1.0)) return false;
        if (!uniforms) return top_k <= 0 && top_p == 1.0 && !logp && !logits && !allow && !forced;
        return std::isfinite(temperature) && V <= 512;
    }
};

}  // namespace sample
