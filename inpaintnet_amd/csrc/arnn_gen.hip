// AnticipationRNN's token generation (arnn_gen.h): the free-running token pass as ONE persistent launch (round 5), and the per-tick
// launches behind it for every other shape.
//
// The reference's free-running forward (AnticipationRNN/anticipation_rnn_gauss_reg_model.py:190-259) feeds the argmax of BATCH
// ELEMENT 0 back to the whole batch (:253-256): the L tokens depend on that one row, and producing them is strictly sequential --
// per tick  [embedding of the previous token | constraint output of the tick] -> LSTM 0 -> LSTM 1 -> ReLU(linear_1) -> note head ->
// argmax.  Round 4 queued that as four small launches per tick (arnn_ticks at the end of this file): 14.3 us per tick = 4 x 3.6 us per dependent
// launch, 5.5 ms of the 14.4 ms free-running training step.  Here 13 workgroups of 512 threads stay resident for the whole
// sequence, every one with its weights in REGISTERS (a 256 x 256 f32 slice: 128 VGPRs per thread, see "Threads and products"
// below), and 1-KB vectors move between them as 8-byte {value, tick} granules (one relaxed agent-scope 64-bit store / polled load
// per element: MI355X_MICROARCH.md "handoff-1to1", form R2 -- the tag travels with the value, nothing to order):
//
//   C   (1)      W1 = linear_1, W2 = note head.  Per tick: L0's gates = pre[t] + T0[tok] + hh0 (all precomputed or received:
//                NO product on this edge), L0's cell, publish h0_t; wait for h1_t; u = ReLU(W1 h1 + b1); logits = W2 u + b2;
//                argmax (numpy order: NaN is the maximum, lowest index among equals) -> tok_t
//   A_k (4)      W_hh0 rows of units 64k..64k+63: hh0 for tick t+1 = W_hh0 h0_t           (off the critical path)
//   Bi_k (4)     W_ih1 rows of units 64k..: gates of L1 = W_ih1 h0_t + b_ih1 + hh1, L1's cell, publish h1_t
//   Bh_k (4)     W_hh1 rows: hh1 for tick t+1 = W_hh1 h1_t + b_hh1                        (off the critical path)
//
// so a tick is TWO hand-offs on its critical path (C -> Bi -> C) with one 256 x 256 product behind each, instead of four
// launches: the input-side product of layer 0 does not depend on the sequence (pre[t] = W_ih0[:, E:] oc_t + b_ih0 + b_hh0 for all
// ticks and T0[v] = W_ih0[:, :E] emb[v] for every token are made by one small launch in front), and both recurrent products are
// started the moment their state exists and arrive before they are needed (their granules are REQUESTED a phase early and looked at
// late: a granule read is a ~0.8 us round trip through the memory side).  The gate summands hh0 / hh1 have ONE reader per granule
// (the cell thread of the unit) and are single-buffered: their writer's next write needs the whole next state, which the reader
// publishes behind its read.  The state vectors h0 / h1 have FIVE readers (the four recurrent-side workgroups and the next stage)
// while their writer's next write waits only for the summands of its own unit, from ONE of the four: they alternate between two
// slots by tag parity -- the overwrite of h_t happens at h_{t+2}, which needs hh_{t+2} of the unit, which needs ALL of h_{t+1},
// whose every unit needed hh_{t+1} from its own recurrent-side workgroup: all four have read h_t by then.  (With one slot a
// recurrent-side workgroup a tick late found tag t + 2 where it looked for t + 1 and ran into its bound: ADVICE r05.)
// Measured (tools/arnn_token_pass.py, INET_ARNN_GEN_STAMPS=1; profiles/r05_arnn_token_pass.txt): 4.0 us per tick = 0.74 + 0.89 us
// for the two hand-offs, 0.4 us per 256 x 256 product, 0.25 each for the head's product and the argmax, the rest barriers and the
// cells: 384 ticks in 1.5 ms (round 4: 5.5).
// Shapes: H = U = 256 (the reference's configuration), V <= 128; anything else keeps the per-tick launches.  Every spin is bounded.
// The sampling build (SAMPLE = true: ConstraintModelGaussianReg.generate, anticipation_rnn_gauss_reg_model.py:570-679) draws each token
// from softmax(T * logits) with a host-drawn uniform (sample.h) instead of the argmax, and runs up to 8 independent rows ("teams" of 13
// workgroups, each with its own exchange) in the workgroups that the argmax build leaves idle.
// The truncating build (TRUNC = true, V <= 64: inet_arnn_sample_ex) puts sample.h's top-k / nucleus truncation in front of that draw,
// reports the drawn tokens' log-probabilities (the logarithms are taken behind the last tick) and, where asked, every tick's logits;
// head_b1_kernel<NI, 2> does the same for the per-tick launches.  A call without truncation, logp or logits runs the sampling build.
// The masked build (MASK = true, V <= 64: inet_arnn_sample_cx) puts sample.h's per-tick token constraints in front of the truncation;
// head_b1_kernel<NI, 3> does the same for the per-tick launches.  A call without a mask runs the kernels it ran before.
// The forced build (FORCE = true, V <= 64: inet_arnn_sample_fx) puts sample.h's forced tokens behind the constraints: a forced tick returns
// and feeds back its token and reports that token's log-probability; head_b1_kernel<NI, 4> does the same for the per-tick launches.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <optional>
#include "chain.h"
#define INET_GRANULE_KID chain::K_ARNN_GEN
#include "granule.h"
#include "prof.h"
#include "arnn_gen.h"
#include "pointwise.h"
#include "reduce.h"
#include "sample.h"

namespace {
using namespace granule;

constexpr int GH = 256, G4 = 4 * GH;
constexpr int kExXcc = 4 * GH + 2 * G4;          // granules behind the exchange: the workgroups' XCC ids (granule::same_xcd)
constexpr long kExGranules = kExXcc + 16;         // 8-byte granules of the exchange (of one team)

struct GenArgs {
    int L, V, E, K0, stride, near;                   // K0 = E + Hc: row stride of W_ih0; stride: block b works iff b % stride == 0, role b / stride
    const float* emb; const float* W_ih0;
    const float* W_hh0; const float* W_ih1; const float* b_ih1; const float* W_hh1; const float* b_hh1;
    const float* W1; const float* b1; const float* W2; const float* b2;
    const float* pre; const float* T0;           // [L][4H], [V][4H]
    const float* hc_init; const long long* first_tok; long long* tokens;
    unsigned long long* ex;                      // granules: h0 [2][256] | h1 [2][256] | hh0 [1024] | hh1 [1024]  (h: slot = tag & 1)
    unsigned long long* stamps;                  // diagnostics (INET_ARNN_GEN_STAMPS=1): [C, Bi_0][L][8] wall-clock ticks (10 ns), or null
    chain::Status status;
    // sampling build: `rows` independent teams of 13 workgroups (pre, hc_init, uniforms, tokens and the exchange per team; T0
    // shared), the head draws token t from softmax(temp * logits) with the uniform uniforms[team][t] (sample.h)
    int rows; float temp; const double* uniforms;
    // truncating build (TRUNC: sample.h's truncation in front of the draw): logp [rows][L] or null, logits [rows][L][V] or null
    int top_k; double top_p; float* logp; float* logits;
    // masked build (MASK: sample.h's token constraints in front of the truncation): the allowed tokens' words [rows][L][ceil(V / 64)]
    const unsigned long long* allow;
    // forced build (FORCE: sample.h's forced tokens behind the constraints): the forced words [rows][L], a value in [0, V) forces its tick
    const int* forced;
};
#define GEN_STAMP(who, t, i) do { if (a.stamps && tid == 0) a.stamps[((long)(who) * a.L + (t)) * 8 + (i)] = wall_clock64(); } while (0)

// Threads and products.  512 threads per workgroup; thread (q4, e) = (tid >> 3, tid & 7) holds the k eighth e (32 values) of FOUR
// rows in 128 VGPRs and reads its eighth of the vector from LDS: 8 x ds_read_b128 feed 128 FMAs.  (A broadcast LDS read still
// costs the LDS its 4 cycles per wave instruction: one row per thread -- 64 reads per 256 FMAs -- kept the LDS busy for twice the
// FMA time, 0.9 us per product; here the LDS is busy half of it.)  The eight partial sums of a row meet by three DPP adds inside
// the 8-lane group, no LDS, no barrier.  In the LSTM roles the four rows are the four gates of ONE unit, so the cell is computed
// where the sums land.  The vector's eighths sit 36 floats apart in LDS: eight distinct 16-byte reads of a wave instruction then
// fall into eight different bank quads.
constexpr int NT = 512, EK = GH / 8, XP = EK + 4, XS = 8 * XP;
__device__ __forceinline__ int xs_index(int k) { return (k >> 5) * XP + (k & 31); }

__device__ __forceinline__ void load_rows(float (&w)[4][EK], const float* __restrict__ W, const int (&row)[4], int e) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < EK; k += 4) {
            const f32x4 v = ld4u(W + (long)row[i] * GH + EK * e + k);
            w[i][k] = v[0]; w[i][k + 1] = v[1]; w[i][k + 2] = v[2]; w[i][k + 3] = v[3];
        }
}
// y[i] = row i . x for the thread's four rows: partial sums over its eighth, then the 8-lane group's total in every lane of the group
__device__ __forceinline__ void dot4(const float (&w)[4][EK], const float* xe, float (&y)[4]) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < EK; k += 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(xe + k);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i) fmac(a[i], w[i][k + kk], x[kk]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float s = a[i];
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x141, 0xF, 0xF, true));   // row_half_mirror: the other quad
        y[i] = s;
    }
}

// a recurrent-side product off the critical path: y_t = W x_{t-1} (+ b) for the ticks 0 .. L-1, x_{-1} = the initial state
__device__ __forceinline__ void recurrent_role(const GenArgs& a, int k, const float* __restrict__ W, const float* __restrict__ bias,
                                               const float* x_init, const unsigned long long* xin, unsigned long long* yout,
                                               float (*xs)[XS], volatile int* bad, bool near) {
    const int tid = threadIdx.x, j = tid >> 3, e = tid & 7;
    const int row[4] = {64 * k + j, GH + 64 * k + j, 2 * GH + 64 * k + j, 3 * GH + 64 * k + j};      // the four gates of unit 64 k + j
    float w[4][EK];
    load_rows(w, W, row, e);
    const int myrow = row[e & 3];                              // lanes 0 .. 3 of the group publish one gate each
    const float b = bias ? bias[myrow] : 0.f;
    for (int t = 0; t < a.L; ++t) {
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        if (t == 0) {
            if (x_init) {
                if (tid < GH) xs[0][xs_index(tid)] = x_init[tid];
                lds_barrier();
                dot4(w, xs[0] + XP * e, y);
            }
        } else {
            if (tid < GH) {
                float x;
                if (!get_1(xin + (t & 1) * GH + tid, (unsigned)t, a.status, x)) *bad = 1;
                xs[t & 1][xs_index(tid)] = x;
            }
            lds_barrier();
            if (*bad) break;
            dot4(w, xs[t & 1] + XP * e, y);
        }
        if (e < 4) put(yout + myrow, (e == 0 ? y[0] : e == 1 ? y[1] : e == 2 ? y[2] : y[3]) + b, (unsigned)t + 1u, near);
    }
}

// SAMPLE = false: the argmax head (the free-running forward's token pass); true: the sampling head and teams (generate)
// TRUNC (the truncating build of the sampling build; behind SAMPLE so that every build without it keeps its parameters): top-k / nucleus
// truncation in front of the draw, the drawn token's log-probability and the tick's logits.  Every wave of C draws for itself; the
// waves 4 .. 7 own no unit of layer 0 and reach the next tick's first barrier early (it waits for h1: Bi's product and two hand-offs),
// so wave 6 stores the logits and wave 7 files the tick's (S, s_tok - m) there.  The f64 logarithm inside the tick spills (256 VGPRs, 2
// spilled next to the 160 weight registers), as it did in decode_b1.hip: the workgroup takes all logarithms behind the last tick, one
// tick per thread, where the weights' registers are free.  The terms are filed in the first three floats of the tick's own row of
// `pre`: the row's 256 readers are this workgroup's unit threads, which consumed it in front of the tick's first barrier.
// MASK (the masked build of the truncating build: inet_arnn_sample_cx; sample.h has the rule): the tick's word of allowed tokens bans
// tokens behind the NaN test and in front of the truncation.  The word arrives like the tick's uniform: requested a tick early through a
// wave-uniform address, so every wave of C holds it in scalar registers and the token stays a function of the logits, u, the word and
// kernel arguments -- the same in all eight waves.  The note head is not ReLU'd: a tick outside the rule takes the argmax rule over its
// ALLOWED logits alone (the banned ones count as -inf and are no candidates, a NaN at a banned place is no NaN), so its token is an
// allowed one whatever the logits hold.  The logits the call returns stay the unmasked ones.  One word per tick: V <= 64, as the
// truncating build.
// FORCE (the forced build of the masked build: inet_arnn_sample_fx; sample.h has the rule): the tick's forced word arrives like the mask
// word -- requested a tick early through a wave-uniform address, held in scalar registers by every wave of C -- so the token stays a
// function of the logits, u, the mask word, the forced word and kernel arguments.  A forced tick runs the tick's steps with u = 0.0 for S
// alone, then takes tok = f and the gap of f: -inf where f is banned or truncated away.  On a fallback tick f skips the argmax block.  A
// forced call without a mask (a null `allow`: a kernel argument, wave-uniform) takes a word of all ones, which mask_words() trims.
template <int NV, bool SAMPLE, bool TRUNC = false, bool MASK = false, bool FORCE = false>
__global__ __launch_bounds__(NT) void arnn_token_pass_kernel(GenArgs a) {
    static_assert(SAMPLE || !TRUNC, "the truncating build is a sampling build");
    static_assert(TRUNC || !MASK, "the masked build is a truncating build");
    static_assert(MASK || !FORCE, "the forced build is a masked build");
    static_assert(!MASK || NV == 1, "the masked build reads ONE word per tick: NW = ceil(V / 64) = NV = 1");
    __shared__ __attribute__((aligned(16))) float xs[2][XS];
    __shared__ __attribute__((aligned(16))) float us[GH];
    __shared__ float ps[8][64 * NV];
    __shared__ int bad_s, near_s;
    // sampling build: team r = the blocks b = r (mod 8) with role b / 8 under stride 8 (one XCD per team under round-robin
    // dispatch), the contiguous blocks [13 r, 13 r + 13) under stride 1.  (Written so that the argmax build compiles to the same
    // code as before the teams: team 0, its pointers a's own.)
    if (!SAMPLE && blockIdx.x % a.stride) return;
    const int team = SAMPLE ? (a.stride == 1 ? (int)blockIdx.x / 13 : (int)blockIdx.x % a.stride) : 0;
    const int role = SAMPLE ? (a.stride == 1 ? (int)blockIdx.x % 13 : (int)blockIdx.x / a.stride) : (int)(blockIdx.x / a.stride);
    if (SAMPLE && team >= a.rows) return;
    unsigned long long* const ex = a.ex + team * kExGranules;
    const float* const pre = a.pre + (long)team * a.L * G4;
    const float* const hc_init = SAMPLE && a.hc_init ? a.hc_init + team * 4 * GH : a.hc_init;
    long long* const tokens = a.tokens + (long)team * a.L;
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    unsigned long long* const e_h0 = ex;
    unsigned long long* const e_h1 = ex + 2 * GH;
    unsigned long long* const e_hh0 = ex + 4 * GH;
    unsigned long long* const e_hh1 = ex + 4 * GH + G4;
    volatile int* const bad = &bad_s;
    if (tid == 0) bad_s = 0;
    __syncthreads();
    // all 13 workgroups on one XCD (mode 3 asks; the answer is the hardware's): granules as plain stores (granule.h)
    const bool near = a.near && same_xcd(ex + kExXcc, role, 13, a.status, &near_s);

    if (role >= 1 && role <= 4) {
        recurrent_role(a, role - 1, a.W_hh0, nullptr, hc_init, e_h0, e_hh0, xs, bad, near);  // (b_hh0 sits in pre)
    } else if (role >= 9) {
        recurrent_role(a, role - 9, a.W_hh1, a.b_hh1, hc_init ? hc_init + 2 * GH : nullptr, e_h1, e_hh1, xs, bad, near);
    } else if (role >= 5) {
        // ---- Bi_k: layer 1's input-side product and its cell: thread (unit j, eighth e) holds the four gate rows of its unit, the
        // sums land in every lane of the 8-lane group, lane e = 0 computes the cell -- no LDS, no barrier behind the product ----
        const int k = role - 5, j = tid >> 3, e = tid & 7;
        const int row[4] = {64 * k + j, GH + 64 * k + j, 2 * GH + 64 * k + j, 3 * GH + 64 * k + j};
        const bool cell = e == 0;
        float w[4][EK];
        load_rows(w, a.W_ih1, row, e);
        float bb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bb[i] = a.b_ih1[row[i]];
        float c1 = (cell && hc_init) ? hc_init[3 * GH + 64 * k + j] : 0.f;
        for (int t = 0; t < a.L; ++t) {
            // the recurrent summands of this tick were started a tick ago: they are here before h0_t is
            float hh[4] = {0.f, 0.f, 0.f, 0.f};
            unsigned long long hw[4];
            if (k == 0) GEN_STAMP(1, t, 0);
            if (cell && !get_n<4>(e_hh1 + 64 * k + j, GH, (unsigned)t + 1u, a.status, hh, hw)) *bad = 1;
            if (k == 0) GEN_STAMP(1, t, 1);
            if (tid < GH) {
                float x;
                if (!get_1(e_h0 + ((t + 1) & 1) * GH + tid, (unsigned)t + 1u, a.status, x)) *bad = 1;
                xs[t & 1][xs_index(tid)] = x;
            }
            if (k == 0) GEN_STAMP(1, t, 2);
            lds_barrier();
            if (*bad) break;
            if (k == 0) GEN_STAMP(1, t, 3);
            float y[4];
            dot4(w, xs[t & 1] + XP * e, y);
            if (k == 0) GEN_STAMP(1, t, 4);
            if (cell) {
                const float ig = sigmoid_f(y[0] + bb[0] + hh[0]), fg = sigmoid_f(y[1] + bb[1] + hh[1]);
                const float gv = tanh_f(y[2] + bb[2] + hh[2]), og = sigmoid_f(y[3] + bb[3] + hh[3]);
                c1 = fg * c1 + ig * gv;
                put(e_h1 + ((t + 1) & 1) * GH + 64 * k + j, og * tanh_f(c1), (unsigned)t + 1u, near);
            }
            if (k == 0) GEN_STAMP(1, t, 5);
        }
    } else {
        // ---- C: layer 0's cell (no product: its three summands arrive), linear_1, the note head, argmax ----
        const int rq = tid >> 3, e = tid & 7;
        const int row[4] = {4 * rq, 4 * rq + 1, 4 * rq + 2, 4 * rq + 3};
        float w1[4][EK];
        load_rows(w1, a.W1, row, e);
        float w2[NV][32];                                      // rows lane + 64 j of the head, k eighth q
        float b2[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = min(lane + 64 * j, a.V - 1);
            b2[j] = a.b2[v];
#pragma unroll
            for (int i = 0; i < 32; i += 4) {
                const f32x4 x = ld4u(a.W2 + (long)v * GH + 32 * q + i);
                w2[j][i] = x[0]; w2[j][i + 1] = x[1]; w2[j][i + 2] = x[2]; w2[j][i + 3] = x[3];
            }
        }
        const float b1 = a.b1[4 * rq + (e & 3)];               // lanes 0 .. 3 of the group write one row of u each
        const bool unit = tid < GH;                            // threads 0 .. 255 also own one unit of layer 0
        float c0 = (unit && hc_init) ? hc_init[GH + tid] : 0.f;
        long long tok = a.first_tok ? *a.first_tok : 0;
        float pr[4] = {0.f, 0.f, 0.f, 0.f}, hh[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned long long hw[4];
        const double* const urow = SAMPLE ? a.uniforms + (long)team * a.L : nullptr;
        double u = 0.0, u_next = SAMPLE ? urow[0] : 0.0;       // (the next tick's uniform is requested a tick early)
        [[maybe_unused]] const unsigned long long* const arow = MASK ? a.allow + (long)team * a.L * NV : nullptr;
        [[maybe_unused]] unsigned long long aw[NV] = {}, aw_next[NV] = {};   // (masked build: ... and its words of allowed tokens)
        [[maybe_unused]] const bool masked = !FORCE || a.allow;             // (forced build: a call without a mask has words of all ones)
        if constexpr (MASK) {
#pragma unroll
            for (int j = 0; j < NV; ++j) aw_next[j] = masked ? arow[j] : ~0ull;
        }
        [[maybe_unused]] const int* const frow = FORCE ? a.forced + (long)team * a.L : nullptr;
        [[maybe_unused]] int fw = -1, fw_next = -1;           // (forced build: ... and its forced word)
        if constexpr (FORCE) fw_next = frow[0];
        if (unit) {
#pragma unroll
            for (int g = 0; g < 4; ++g) pr[g] = pre[g * GH + tid];
            if (!get_n<4>(e_hh0 + tid, GH, 1u, a.status, hh, hw)) *bad = 1;
        }
        [[maybe_unused]] int done = 0;                        // (truncating build: the ticks finished)
        [[maybe_unused]] float* const lrow = TRUNC && a.logits ? a.logits + (long)team * a.L * a.V : nullptr;
        [[maybe_unused]] float* const terms = TRUNC && a.logp ? const_cast<float*>(pre) : nullptr;
        for (int t = 0; t < a.L; ++t) {
            const bool more = t + 1 < a.L;
            if constexpr (SAMPLE) {
                u = u_next;
                if (more) u_next = urow[t + 1];
            }
            if constexpr (MASK) {
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    aw[j] = aw_next[j];
                    if (more && masked) aw_next[j] = arow[(long)(t + 1) * NV + j];
                }
            }
            if constexpr (FORCE) {
                fw = fw_next;
                if (more) fw_next = frow[t + 1];
            }
            GEN_STAMP(0, t, 0);
            if (unit) {
                float gate[4];
                if (t == 0) {                                  // the token in front of the first tick may lie outside the head's range
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float s = 0.f;
                        for (int e = 0; e < a.E; ++e) s = fmaf(a.emb[tok * a.E + e], a.W_ih0[(long)(g * GH + tid) * a.K0 + e], s);
                        gate[g] = pr[g] + s + hh[g];
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) gate[g] = pr[g] + a.T0[tok * G4 + g * GH + tid] + hh[g];
                }
                const float ig = sigmoid_f(gate[0]), fg = sigmoid_f(gate[1]), gv = tanh_f(gate[2]), og = sigmoid_f(gate[3]);
                c0 = fg * c0 + ig * gv;
                put(e_h0 + ((t + 1) & 1) * GH + tid, og * tanh_f(c0), (unsigned)t + 1u, near);
                GEN_STAMP(0, t, 1);
                if (more) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) pr[g] = pre[(long)(t + 1) * G4 + g * GH + tid];
                }
                float x;
                if (!get_1(e_h1 + ((t + 1) & 1) * GH + tid, (unsigned)t + 1u, a.status, x)) *bad = 1;
                GEN_STAMP(0, t, 2);
                xs[0][xs_index(tid)] = x;
            }
            lds_barrier();
            if (*bad) break;
            GEN_STAMP(0, t, 3);
            // the next tick's recurrent summands left A_k about when h1_t left Bi_k: request them now, look at them behind the head
            if (unit && more) {
#pragma unroll
                for (int g = 0; g < 4; ++g) hw[g] = peek(e_hh0 + g * GH + tid);
            }
            float y[4];
            dot4(w1, xs[0] + XP * e, y);
            if (e < 4) us[4 * rq + e] = fmaxf((e == 0 ? y[0] : e == 1 ? y[1] : e == 2 ? y[2] : y[3]) + b1, 0.f);
            lds_barrier();
            GEN_STAMP(0, t, 4);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                float p0 = 0.f, p1 = 0.f;
#pragma unroll
                for (int i = 0; i < 32; i += 4) {
                    const f32x4 u4 = *reinterpret_cast<const f32x4*>(us + 32 * q + i);
                    fmac(p0, w2[j][i], u4[0]); fmac(p1, w2[j][i + 1], u4[1]); fmac(p0, w2[j][i + 2], u4[2]); fmac(p1, w2[j][i + 3], u4[3]);
                }
                ps[q][lane + 64 * j] = p0 + p1;
            }
            lds_barrier();
            GEN_STAMP(0, t, 5);
            // every wave takes the argmax for itself (wave-uniform result, no fourth barrier): the maximum by DPP, its lowest index by
            // ballot; a NaN is the maximum (np.argmax), the lowest NaN wins
            {
                float lg[NV];
                unsigned long long nanm[NV];
                float m = -INFINITY;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int v = lane + 64 * j;
                    float x = b2[j];
#pragma unroll
                    for (int qq = 0; qq < 8; ++qq) x += ps[qq][v];
                    lg[j] = v < a.V ? x : -INFINITY;
                    nanm[j] = __ballot(lg[j] != lg[j]);
                    m = fmaxf(m, lg[j]);                        // (fmaxf skips a NaN)
                }
                m = wave_max_dpp(m);
                int bi = -1;
                if constexpr (SAMPLE) {
                    // the sampling head (sample.h): a NaN logit, a non-finite total or a uniform outside [0, 1) keep the argmax rule.
                    // The steps of sample::draw stand here in the pass's own order, not as one call: through draw() the masked build
                    // ran 3 % slower and the V > 64 sampling build 0.2 % -- a change to the rule is made here too,
                    // and the forced step (u = 0.0 for S, then tok = f and the gap of f) exists in both places
                    float sv[NV], ms = -INFINITY;
                    bool nan = false;
                    [[maybe_unused]] const bool forced = FORCE && sample::is_forced(fw, a.V);
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        sv[j] = lane + 64 * j < a.V ? lg[j] * a.temp : -INFINITY;
                        nan |= sv[j] != sv[j];
                        ms = fmaxf(ms, sv[j]);
                    }
                    double tot = 0.0;
                    if constexpr (TRUNC) {
                        // (one wave: plain vector stores of what every wave holds)
                        if (lrow && q == 6) {
                            float* const row = lrow + (long)t * a.V;
#pragma unroll
                            for (int j = 0; j < NV; ++j)
                                if (lane + 64 * j < a.V) row[lane + 64 * j] = lg[j];
                        }
                        float gap = 0.f;
                        if constexpr (MASK) sample::mask_words<NV>(aw, a.V);
                        if (!__ballot(nan)) {
                            if constexpr (MASK) ms = sample::mask_scores<NV>(sv, aw, lane);
                            const float mw = wave_max_dpp(ms);
                            sample::truncate<NV>(sv, mw, a.top_k, a.top_p, a.V, lane);
                            bi = sample::pick<NV>(sv, mw, FORCE && forced ? 0.0 : u, a.V, lane, tot);
                            if constexpr (FORCE) { if (forced && bi >= 0) bi = fw; }
                            if (bi >= 0) gap = sample::logp_gap<NV>(sv, mw, bi);
                        }
                        // (a tick that falls back to the argmax rule below files S = NaN: its logp comes out NaN)
                        if (terms && tid == NT - 64) {
                            float* const term = terms + (long)t * G4;
                            *reinterpret_cast<double*>(term) = bi >= 0 ? tot : (double)__builtin_nanf("");
                            term[2] = gap;
                        }
                        if constexpr (FORCE) { if (forced) bi = fw; }    // (on a fallback tick too: f skips the argmax block)
                    } else {
                        if (!__ballot(nan)) bi = sample::pick<NV>(sv, wave_max_dpp(ms), u, a.V, lane, tot);
                    }
                }
                if (bi < 0) {
                    if constexpr (MASK) {                       // the argmax rule over the allowed logits alone (the logits are stored by now)
                        m = -INFINITY;
#pragma unroll
                        for (int j = 0; j < NV; ++j) {
                            if (!sample::allowed(aw[j], lane)) lg[j] = -INFINITY;
                            nanm[j] = __ballot(lg[j] != lg[j]);
                            m = fmaxf(m, lg[j]);
                        }
                        m = wave_max_dpp(m);
                    }
#pragma unroll
                    for (int j = NV - 1; j >= 0; --j) {
                        const unsigned long long eq = __ballot(lg[j] == m) & (MASK ? aw[j] : ~0ull);   // (allowed logits all -inf: the lowest allowed)
                        if (eq) bi = 64 * j + __builtin_ctzll(eq);
                    }
#pragma unroll
                    for (int j = NV - 1; j >= 0; --j)
                        if (nanm[j]) bi = 64 * j + __builtin_ctzll(nanm[j]);
                    // (NaN in the lower half beats one in the upper: the loops run downwards and the lower overwrites)
                    bool anynan = false;
#pragma unroll
                    for (int j = 0; j < NV; ++j) anynan |= nanm[j] != 0;
                    if (!anynan && bi < 0) bi = 0;
                }
                tok = (bi >= 0 && bi < a.V) ? bi : 0;
                if (tid == 0) tokens[t] = tok;
            }
            GEN_STAMP(0, t, 6);
            if (unit && more && !get_n<4>(e_hh0 + tid, GH, (unsigned)t + 2u, a.status, hh, hw, false)) *bad = 1;
            GEN_STAMP(0, t, 7);
            if constexpr (TRUNC) done = t + 1;
        }
        if constexpr (TRUNC) {
            // ... behind the last tick: the logarithms, one tick per thread (a tick that a timed-out launch never reached: NaN)
            if (a.logp) {
                __syncthreads();
                for (int t = tid; t < a.L; t += NT) {
                    const float* const term = pre + (long)t * G4;
                    a.logp[(long)team * a.L + t] =
                        t < done ? sample::logp_of(term[2], *reinterpret_cast<const double*>(term)) : __builtin_nanf("");
                }
            }
        }
    }
    __syncthreads();
    if (bad_s && tid == 0) chain::raise_timeout(a.status);
}

// pre[t][r] = sum_k oc[t][k] W_ih0[r][E + k] + b_ih0[r] + b_hh0[r]  (tiles of 16 ticks x 64 gate rows), and
// T0[v][r] = sum_e emb[v][e] W_ih0[r][e]                              (the blocks behind them, 256 outputs each);
// `rows` rows of pre (the sampling build's teams): row i from oc0 + i * oc_bstride into pre + i * L * 4H
struct PrepArgs {
    int L, V, E, Hc, K0, nb_pre, rows;
    const float* oc0; long oc_stride, oc_bstride;
    const float* emb; const float* W_ih0; const float* b_ih0; const float* b_hh0;
    float* pre; float* T0;
};
__global__ __launch_bounds__(256) void arnn_gen_prep_kernel(PrepArgs a) {
    __shared__ float Ws[64 * 65];
    __shared__ float Os[16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, tg = tid >> 6;
    if ((int)blockIdx.x >= a.nb_pre * a.rows) {
        const long o = (long)(blockIdx.x - a.nb_pre * a.rows) * 256 + tid;
        if (o < (long)a.V * G4) {
            const int v = (int)(o / G4), r = (int)(o % G4);
            float s = 0.f;
            for (int e = 0; e < a.E; ++e) s = fmaf(a.emb[(long)v * a.E + e], a.W_ih0[(long)r * a.K0 + e], s);
            a.T0[o] = s;
        }
        return;
    }
    const int row = blockIdx.x / a.nb_pre, bb = blockIdx.x % a.nb_pre;
    const int rb = bb % (G4 / 64), tb = bb / (G4 / 64);
    const float* const oc0 = a.oc0 + row * a.oc_bstride;
    float* const pre = a.pre + (long)row * a.L * G4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.Hc; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + 256 * i, kk = e & 63, row = e >> 6;
            Ws[kk * 65 + row] = k0 + kk < a.Hc ? a.W_ih0[(long)(rb * 64 + row) * a.K0 + a.E + k0 + kk] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, kk = e & 63, tk = e >> 6, t = tb * 16 + tk;
            Os[tk * 64 + kk] = (t < a.L && k0 + kk < a.Hc) ? oc0[(long)t * a.oc_stride + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 64; ++kk) {
            const float w = Ws[kk * 65 + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(w, Os[(4 * tg + i) * 64 + kk], acc[i]);
        }
    }
    const int r = rb * 64 + lane;
    const float b = a.b_ih0[r] + a.b_hh0[r];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = tb * 16 + 4 * tg + i;
        if (t < a.L) pre[(long)t * G4 + r] = acc[i] + b;
    }
}

int g_mode = -1;                                 // 0 = the per-tick launches, 1 = persistent kernel on 13 consecutive workgroups,
                                                 // 2 = on every 8th workgroup of 104: one XCD under the round-robin dispatch observed
                                                 // today (speed only, 4.0 vs 4.2 us per tick; correct under any placement),
                                                 // 3 (default) = 2 + plain granule stores once the workgroups have FOUND themselves on
                                                 // one XCD (granule.h: 3.6 -> 3.2 us per tick; agent-scope stores otherwise);
                                                 // 4 = test hook: 3's request on consecutive workgroup ids (the check must say no)
int mode() {
    if (g_mode < 0) {
        const char* v = std::getenv("INET_ARNN_GEN");
        g_mode = v ? std::atoi(v) : 3;
        if (g_mode < 0 || g_mode > 4) g_mode = 3;
    }
    return g_mode;
}
constexpr long kExFloats = 2 * kExGranules + 64; // ... as floats, + the launch's status word (64 floats behind them)

bool arnn_token_pass_ok(const ArnnGenNet& n) {
    return mode() != 0 && chain_enabled() && n.H == GH && n.U == GH && n.V >= 1 && n.V <= 128;
}

// The truncating build exists for V <= 64 alone: with two logit chunks per lane (<2, true, true>, 64 < V <= 128) it can only be had
// with spills (256 VGPRs, 40 spilled, 148 bytes of scratch -- the argmax and sampling builds of that shape spill 36 and 41), so it is
// not built and a truncated call with V > 64 takes the per-tick launches.
bool arnn_token_trunc_ok(const ArnnGenNet& n) { return arnn_token_pass_ok(n) && n.V <= 64; }
// The masked build (<1, true, true, true>) fits where the truncating build does: one word of allowed tokens per tick.
bool arnn_token_cons_ok(const ArnnGenNet& n) { return arnn_token_trunc_ok(n); }
// The forced build (<1, true, true, true, true>) fits where the masked build does: one forced word per tick in scalar registers.
bool arnn_token_force_ok(const ArnnGenNet& n) { return arnn_token_cons_ok(n); }

// tables | exchange + status | stamps (2 x L x 8 64-bit words, written only under INET_ARNN_GEN_STAMPS=1: tools/arnn_token_pass.py)
size_t arnn_token_pass_ws_floats(int L, int V) { return (size_t)L * G4 + (size_t)V * G4 + (size_t)kExFloats + 64 + (size_t)32 * L; }
long arnn_token_pass_stamps_offset(int L, int V) { return (long)L * G4 + (long)V * G4 + kExFloats + 64; }

// the prep launch of `rows` rows (row i from oc0 + i * oc_bstride) and the pass behind it, as far as the network and the workspace decide
PrepArgs prep_args(const ArnnGenNet& n, int L, int rows, const float* oc0, long oc_stride, long oc_bstride, float* pre, float* T0) {
    PrepArgs p{};
    p.L = L; p.V = n.V; p.E = n.E; p.Hc = n.Hc; p.K0 = n.E + n.Hc;
    p.nb_pre = (G4 / 64) * ((L + 15) / 16); p.rows = rows;
    p.oc0 = oc0; p.oc_stride = oc_stride; p.oc_bstride = oc_bstride;
    p.emb = n.emb; p.W_ih0 = n.W_ih0; p.b_ih0 = n.b_ih0; p.b_hh0 = n.b_hh0; p.pre = pre; p.T0 = T0;
    return p;
}
GenArgs gen_args(const ArnnGenNet& n, int L, const float* pre, const float* T0, unsigned long long* ex, unsigned* status) {
    GenArgs a{};
    a.L = L; a.V = n.V; a.E = n.E; a.K0 = n.E + n.Hc;
    // (mode 4: test hook -- XCD-local stores REQUESTED on consecutive ids: the workgroups must find out that they do not share an XCD)
    a.stride = (mode() == 2 || mode() == 3) ? 8 : 1; a.near = mode() >= 3;
    a.emb = n.emb; a.W_ih0 = n.W_ih0; a.W_hh0 = n.W_hh0; a.W_ih1 = n.W_ih1; a.b_ih1 = n.b_ih1; a.W_hh1 = n.W_hh1; a.b_hh1 = n.b_hh1;
    a.W1 = n.W1; a.b1 = n.b1; a.W2 = n.W2; a.b2 = n.b2; a.pre = pre; a.T0 = T0;
    a.ex = ex; a.status = chain_status_for(status);
    return a;
}

int arnn_token_pass(const ArnnGenNet& n, int L, const float* oc0, long oc_stride, const float* hc_init, const long long* first_tok,
                    long long* tokens, float* ws, hipStream_t s) {
    const int V = n.V;
    float* pre = ws;
    float* T0 = pre + (size_t)L * G4;
    // (the exchange starts on a 16-float boundary behind the tables: L * 4H and V * 4H are multiples of 1024)
    unsigned long long* ex = reinterpret_cast<unsigned long long*>(T0 + (size_t)V * G4);
    unsigned* status = reinterpret_cast<unsigned*>(ex + kExGranules);
    if (hipMemsetAsync(ex, 0, (size_t)kExFloats * sizeof(float), s) != hipSuccess) return -2;
    const PrepArgs p = prep_args(n, L, 1, oc0, oc_stride, 0, pre, T0);
    const int nb_t0 = (int)(((long)V * G4 + 255) / 256);
    hipLaunchKernelGGL(arnn_gen_prep_kernel, dim3(p.nb_pre + nb_t0), dim3(256), 0, s, p);
    GenArgs a = gen_args(n, L, pre, T0, ex, status);
    a.hc_init = hc_init; a.first_tok = first_tok; a.tokens = tokens;
    static const bool stamps = [] { const char* v = std::getenv("INET_ARNN_GEN_STAMPS"); return v && v[0] == '1'; }();
    a.stamps = stamps ? reinterpret_cast<unsigned long long*>(ws + arnn_token_pass_stamps_offset(L, V)) : nullptr;
    char label[64];
    std::snprintf(label, sizeof label, "arnn_token_pass L%d V%d", L, V);
    // per tick: four 1024 x 256 products (one of them, the input side of layer 0, in the prep launch), linear_1, the head
    ProfScope prof(PROF_GRU_FWD, 2.0 * L * (3.0 * G4 * GH + (double)GH * GH + (double)V * GH), s, label,
                   4.0 * (3.0 * G4 * GH + (double)GH * GH + (double)V * GH + (double)(L + V) * G4));
    const dim3 grid(13 * a.stride);
    if (V <= 64) hipLaunchKernelGGL((arnn_token_pass_kernel<1, false>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((arnn_token_pass_kernel<2, false>), grid, dim3(NT), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- the sampling build: R independent rows, up to 8 teams of 13 workgroups per launch ----
// teams per launch: at most 8 (the stride-8 placement has 8 residues), and 13 x teams workgroups inside the chain capacity
int sample_teams(int R) {
    const int cap = chain_capacity() / 13;
    return std::max(1, std::min(std::min(R, 8), cap));
}

// pre [teams][L][4H] | T0 [V][4H] | exchange [teams][kExGranules] granules + the status word (64 floats) + 64
size_t arnn_token_sample_ws_floats(int R, int L, int V) {
    const size_t n = (size_t)sample_teams(R);
    return n * L * G4 + (size_t)V * G4 + n * 2 * kExGranules + 64 + 64;
}

// rq ([R][L] arrays, uniforms given), one build per level of the request, the labels of a level from 2 up with its prefix:
// 2 = the truncating build (V <= 64: arnn_token_trunc_ok); 3 = the masked build (arnn_token_cons_ok), [R][L][1] words of allowed tokens;
// 4 = the forced build (arnn_token_force_ok), [R][L] forced words, allow nullable
int arnn_token_sample(const ArnnGenNet& net, int R, int L, const float* oc0, long oc_stride, long oc_bstride, const float* hc_init,
                      long long* tokens, float* ws, hipStream_t s, const sample::Request& rq) {
    const int V = net.V, n = sample_teams(R);
    float* pre = ws;
    float* T0 = pre + (size_t)n * L * G4;
    unsigned long long* ex = reinterpret_cast<unsigned long long*>(T0 + (size_t)V * G4);
    const int nb_t0 = (int)(((long)V * G4 + 255) / 256);
    char label[64];
    const int level = rq.level(V);
    std::snprintf(label, sizeof label, "%sarnn_token_sample R%d L%d V%d", level >= 2 ? sample::prefix(level) : "", R, L, V);
    for (int r0 = 0; r0 < R; r0 += n) {                          // R > teams: successive launches of up to `n` rows
        const int rows = std::min(n, R - r0);
        unsigned* status = reinterpret_cast<unsigned*>(ex + rows * kExGranules);
        if (hipMemsetAsync(ex, 0, ((size_t)rows * 2 * kExGranules + 64) * sizeof(float), s) != hipSuccess) return -2;
        const PrepArgs p = prep_args(net, L, rows, oc0 + (long)r0 * oc_bstride, oc_stride, oc_bstride, pre, T0);
        hipLaunchKernelGGL(arnn_gen_prep_kernel, dim3(p.nb_pre * rows + (r0 == 0 ? nb_t0 : 0)), dim3(256), 0, s, p);
        GenArgs a = gen_args(net, L, pre, T0, ex, status);
        a.hc_init = hc_init ? hc_init + (long)r0 * 4 * GH : nullptr; a.tokens = tokens + (long)r0 * L;
        const sample::Request q = rq.rows(r0);                   // (this launch's rows)
        a.rows = rows; a.temp = q.temperature; a.uniforms = q.uniforms;
        a.top_k = q.top_k; a.top_p = q.top_p;
        a.logp = q.logp; a.logits = q.logits; a.allow = q.allow; a.forced = q.forced;
        ProfScope prof(PROF_GRU_FWD, 2.0 * rows * L * (3.0 * G4 * GH + (double)GH * GH + (double)V * GH), s, label,
                       4.0 * (3.0 * G4 * GH + (double)GH * GH + (double)V * GH + (double)(rows * L + V) * G4));
        const dim3 grid(a.stride == 8 ? 13 * 8 : 13 * rows);
        if (level == 4) hipLaunchKernelGGL((arnn_token_pass_kernel<1, true, true, true, true>), grid, dim3(NT), 0, s, a);   // (arnn_token_force_ok)
        else if (level == 3) hipLaunchKernelGGL((arnn_token_pass_kernel<1, true, true, true>), grid, dim3(NT), 0, s, a);   // (V <= 64: arnn_token_cons_ok)
        else if (level == 2) hipLaunchKernelGGL((arnn_token_pass_kernel<1, true, true>), grid, dim3(NT), 0, s, a);    // (V <= 64: arnn_token_trunc_ok)
        else if (V <= 64) hipLaunchKernelGGL((arnn_token_pass_kernel<1, true>), grid, dim3(NT), 0, s, a);
        else hipLaunchKernelGGL((arnn_token_pass_kernel<2, true>), grid, dim3(NT), 0, s, a);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}
}  // namespace

void arnn_gen_set_mode(int m) { g_mode = (m < 0 || m > 4) ? 3 : m; }

// ---- The per-tick launches: every shape the persistent pass does not take (and mode 0) ---------------------------------------------
// L ticks of ONE row -- per tick: input = [embedding of the previous token | constraint output of the tick], two LSTM cells,
// linear_1 + ReLU, the note head, argmax or draw -- as 4 small launches per tick queued from here (no host round trip: the token
// stays on the device).  (The free-running pass needs batch element 0 alone, see the head of this file; with its tokens the caller
// runs the whole batch through the batched, teacher-forced-shaped kernels: 195 -> 14 ms per training step.)
namespace {
// dot products of ONE row against weight rows, lanes striding over k: every load of a wave is issued before the first multiply (NI =
// ceil(K / 64) is a template bound: a runtime k loop waits for each 64-wide slice in turn -- 7 us per launch instead of 2)
template <int NI>
__device__ __forceinline__ void load_x(float (&xv)[NI], const float* pa, int Ka, const float* pb, int K, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int k = lane + 64 * i;
        xv[i] = k < Ka ? pa[k] : (k < K ? pb[k - Ka] : 0.f);
    }
}
template <int NI>
__device__ __forceinline__ float dot_row(const float* __restrict__ Wrow, const float (&xv)[NI], int K, int lane) {
    float wv[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) { const int k = lane + 64 * i; wv[i] = k < K ? Wrow[k] : 0.f; }
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) a = fmaf(wv[i], xv[i], a);
    return a;
}

// One LSTM cell for ONE row, both products in the launch: gates = W_ih [xa | xb] + b_ih + W_hh h_prev + b_hh.  One wave per hidden
// unit (its four gate rows), four units per workgroup.  xa = the embedding row of *tok (tok null: token 0) when `emb` is given.
template <int NI, int NH>
__global__ __launch_bounds__(256) void lstm_cell_b1_kernel(const float* __restrict__ emb, const long long* __restrict__ tok,
                                                           const float* __restrict__ xa, int Ka, const float* __restrict__ xb, int Kb,
                                                           const float* __restrict__ W_ih, const float* __restrict__ b_ih,
                                                           const float* __restrict__ h_prev, const float* __restrict__ c_prev,
                                                           const float* __restrict__ W_hh, const float* __restrict__ b_hh,
                                                           float* __restrict__ h_new, float* __restrict__ c_new, int H) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + w;
    const int K = Ka + Kb;
    const float* pa = emb ? emb + (tok ? *tok : 0) * Ka : xa;
    float xv[NI], hv[NH];
    load_x<NI>(xv, pa, Ka, xb, K, lane);
    load_x<NH>(hv, h_prev, H, nullptr, H, lane);
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        pre[g] = dot_row<NI>(W_ih + (long)(g * H + j) * K, xv, K, lane) + dot_row<NH>(W_hh + (long)(g * H + j) * H, hv, H, lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) pre[g] = wave_sum(pre[g]);
    if (lane == 0) {
        const float i = sigmoid_f(pre[0] + b_ih[j] + b_hh[j]);
        const float f = sigmoid_f(pre[1] + b_ih[H + j] + b_hh[H + j]);
        const float g = tanh_f(pre[2] + b_ih[2 * H + j] + b_hh[2 * H + j]);
        const float o = sigmoid_f(pre[3] + b_ih[3 * H + j] + b_hh[3 * H + j]);
        const float c = f * c_prev[j] + i * g;
        c_new[j] = c;
        h_new[j] = o * tanh_f(c);
    }
}

// y[j] = ReLU(W[j,:] . x + b[j]) for ONE row: a wave per output
template <int NI>
__global__ __launch_bounds__(256) void relu_linear_b1_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                             const float* __restrict__ b, float* __restrict__ y, int N, int K) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + w;
    if (j >= N) return;
    float xv[NI];
    load_x<NI>(xv, x, K, nullptr, K, lane);
    const float v = wave_sum(dot_row<NI>(W + (long)j * K, xv, K, lane));
    if (lane == 0) y[j] = fmaxf(v + b[j], 0.f);
}

// does (b2, i2) come before (best, bi) in numpy's argmax order?  NaN > everything, ties to the lower index
__device__ __forceinline__ bool argmax_better(float b2, int i2, float best, int bi) {
    const bool n2 = b2 != b2, n1 = best != best;
    if (n2 || n1) return n2 && (!n1 || i2 < bi);
    return b2 > best || (b2 == best && i2 < bi);
}

// np.argmax order over the ALLOWED entries of lg[0 .. V) (anticipation_rnn_gauss_reg_model.py:253) by one wave: a NaN is the maximum, the
// lowest index wins among equals -- an all-NaN or all -inf row yields a token INSIDE the vocabulary (the next tick gathers the embedding
// row by it).  aw: the words of sample::mask_words (at least one bit set; no mask: all ones); a banned entry is no candidate whatever it
// holds -- a NaN there does not win --, so the token is an allowed one
__device__ __forceinline__ int argmax_wave(const float* lg, const unsigned long long (&aw)[4], int V, int lane) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = lane + 64 * j;
        if (v < V && sample::allowed(aw[j], lane) && argmax_better(lg[v], v, best, bi)) { best = lg[v]; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float b2 = __shfl_xor(best, o, 64);
        const int i2 = __shfl_xor(bi, o, 64);
        if (argmax_better(b2, i2, best, bi)) { best = b2; bi = i2; }
    }
    return bi;
}

// The head of one tick, V <= 256: ONE workgroup of 16 waves; a wave's rows (V = 48: three) are all requested before the first sum, the
// logits W[v,:] . x + b[v] meet in LDS and the first wave takes the token, in one build per LEVEL that reads its own level's arguments alone:
//  0: token = the argmax, lowest index on ties.
//  1: token = a draw from softmax(temp * logits) with the uniform *u (sample.h: numpy's np.random.choice order,
//     anticipation_rnn_gauss_reg_model.py:655-667); a NaN logit, a non-finite total or a uniform outside [0, 1) keep the argmax rule.
//  2: ... behind sample.h's top-k / nucleus truncation: *logp (nullable) receives the drawn token's log-probability under the truncated
//     distribution (NaN where the tick takes the argmax rule) and logits [V] (nullable) the tick's logits, from the LDS array the draw reads.
//  3: ... behind sample.h's token constraints: allow = the tick's ceil(V / 64) words of allowed tokens (<= 4), read by wave 0 through a
//     wave-uniform address.  A tick outside the rule takes the argmax over its allowed logits.  The logits stored are the unmasked ones.
//  4: ... behind sample.h's forced tokens: *forced = the tick's forced word, read by wave 0 through a wave-uniform address; a value in
//     [0, V) is the token whatever the logits, the mask and the uniform hold.  A null allow: words of all ones.
template <int NI, int LEVEL>
__global__ __launch_bounds__(1024) void head_b1_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                       const float* __restrict__ b, long long* __restrict__ tok, int V, int K,
                                                       float temp, const double* __restrict__ u, int top_k, double top_p,
                                                       float* __restrict__ logp, float* __restrict__ logits,
                                                       const unsigned long long* __restrict__ allow,
                                                       const int* __restrict__ forced) {
    __shared__ float lg[256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float xv[NI];
    load_x<NI>(xv, x, K, nullptr, K, lane);
    float part[16];                                            // rows w, w + 16, ...: V <= 256
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int v = w + 16 * r;
        part[r] = v < V ? dot_row<NI>(W + (long)v * K, xv, K, lane) : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int v = w + 16 * r;
        if (v < V) {                                           // (wave-uniform)
            const float a = wave_sum(part[r]);
            if (lane == 0) lg[v] = a + b[v];
        }
    }
    __syncthreads();
    if constexpr (LEVEL >= 2) {
        if (w == 1 && logits)
            for (int v = lane; v < V; v += 64) logits[v] = lg[v];
    }
    if (w == 0) {
        const int nw = (V + 63) / 64;
        unsigned long long aw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)                            // (below level 3: constants, and v < V bounds the argmax)
            aw[j] = LEVEL < 3 ? ~0ull : j < nw ? (LEVEL >= 4 && !allow ? ~0ull : allow[j]) : 0ull;
        if constexpr (LEVEL >= 3) sample::mask_words<4>(aw, V);
        int bi = -1;
        if constexpr (LEVEL >= 1) {
            float xs[4], gap;
            double tot;
#pragma unroll
            for (int j = 0; j < 4; ++j) xs[j] = lane + 64 * j < V ? lg[lane + 64 * j] : -INFINITY;
            const int f = LEVEL >= 4 && forced ? *forced : -1;
            bi = sample::draw<4, LEVEL>(xs, temp, *u, V, lane, top_k, top_p, aw, f, gap, tot);
            if constexpr (LEVEL >= 2) { if (logp && lane == 0) *logp = bi >= 0 ? sample::logp_of(gap, tot) : gap; }
        }
        if (bi < 0) bi = argmax_wave(lg, aw, V, lane);
        if (lane == 0) *tok = bi >= 0 && bi < V ? bi : 0;
    }
}

// the template bounds of the one-row kernels (ops.arnn_generate_ok in Python)
bool arnn_ticks_ok(const ArnnGenNet& n) { return n.E + n.Hc <= 320 && n.H <= 256 && n.U <= 256 && n.V <= 256; }
size_t arnn_ticks_ws_floats(const ArnnGenNet& n) { return (size_t)(n.E + n.Hc) + 4 * (size_t)n.H + 8 * (size_t)n.H + n.U + n.V + 64; }

// L ticks of one row from the state hc_init [layer][h | c][H] (null: zeros; inpainting: the state after the prefix) and the token
// *first_tok (null: 0), the head of the request's level: rq = the ROW's request ([L] arrays; no uniforms: the argmax head).  From level 2
// up one label (trunc_ / cons_ / force_arnn_ticks ...) goes around the row's launches; a call below files nothing.
int arnn_ticks(const ArnnGenNet& n, int L, const float* oc, long oc_stride, const float* hc_init, const long long* first_tok,
               long long* tokens, float* ws, hipStream_t s, const sample::Request& rq) {
    const int H = n.H;
    const int level = rq.level(n.V);
    std::optional<ProfScope> prof;
    if (level >= 2) {
        char label[64];
        std::snprintf(label, sizeof label, "%sarnn_ticks L%d V%d", sample::prefix(level), L, n.V);
        prof.emplace(PROF_GRU_FWD, 2.0 * L * ((double)4 * H * (n.E + n.Hc + 3.0 * H) + (double)n.U * H + (double)n.V * n.U), s, label);
    }
    float* hc = ws;                                            // [layer][h|c][ping-pong][H]
    float* u = hc + 8 * H;
    if (pw_zero(hc, 8L * H, s) != 0) return -2;
    auto H_ = [&](int l, int p) { return hc + ((l * 2 + 0) * 2 + p) * H; };
    auto C_ = [&](int l, int p) { return hc + ((l * 2 + 1) * 2 + p) * H; };
    if (hc_init)
        for (int l = 0; l < 2; ++l)
            if (pw_copy_bytes(H_(l, 0), hc_init + (2 * l) * H, H * sizeof(float), s) != 0 ||
                pw_copy_bytes(C_(l, 0), hc_init + (2 * l + 1) * H, H * sizeof(float), s) != 0) return -2;
    for (int t = 0, p = 0; t < L; ++t, p ^= 1) {
        hipLaunchKernelGGL((lstm_cell_b1_kernel<5, 4>), dim3(H / 4), dim3(256), 0, s, n.emb, t ? tokens + t - 1 : first_tok,
                           (const float*)nullptr, n.E, oc + (long)t * oc_stride, n.Hc, n.W_ih0, n.b_ih0, (const float*)H_(0, p),
                           (const float*)C_(0, p), n.W_hh0, n.b_hh0, H_(0, p ^ 1), C_(0, p ^ 1), H);
        hipLaunchKernelGGL((lstm_cell_b1_kernel<4, 4>), dim3(H / 4), dim3(256), 0, s, (const float*)nullptr, (const long long*)nullptr,
                           (const float*)H_(0, p ^ 1), H, (const float*)nullptr, 0, n.W_ih1, n.b_ih1, (const float*)H_(1, p),
                           (const float*)C_(1, p), n.W_hh1, n.b_hh1, H_(1, p ^ 1), C_(1, p ^ 1), H);
        hipLaunchKernelGGL((relu_linear_b1_kernel<4>), dim3((n.U + 3) / 4), dim3(256), 0, s, (const float*)H_(1, p ^ 1), n.W1, n.b1, u,
                           n.U, H);
        const sample::Request q = rq.tick(t, n.V);
#define HEAD_B1(LEVEL)                                                                                                          \
    hipLaunchKernelGGL((head_b1_kernel<4, LEVEL>), dim3(1), dim3(1024), 0, s, (const float*)u, n.W2, n.b2, tokens + t, n.V, n.U,       \
                       q.temperature, q.uniforms, q.top_k, q.top_p, q.logp, q.logits, q.allow, q.forced)
        switch (level) {
            case 0: HEAD_B1(0); break;
            case 1: HEAD_B1(1); break;
            case 2: HEAD_B1(2); break;
            case 3: HEAD_B1(3); break;
            default: HEAD_B1(4);
        }
#undef HEAD_B1
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // namespace

// ---- The entry points: the persistent pass where it applies (the reference's configuration), the ticks otherwise ------------------
size_t arnn_generate_ws_floats(const ArnnGenNet& n, int L) {
    return std::max(arnn_ticks_ws_floats(n), arnn_token_pass_ok(n) ? arnn_token_pass_ws_floats(L, n.V) : (size_t)0);
}
size_t arnn_sample_ws_floats(const ArnnGenNet& n, int R, int L) {
    return std::max(arnn_ticks_ws_floats(n), arnn_token_pass_ok(n) ? arnn_token_sample_ws_floats(R, L, n.V) : (size_t)0);
}

int arnn_generate(const ArnnGenNet& n, int L, const float* oc0, long oc_stride, const float* hc_init, const long long* first_tok,
                  long long* tokens, float* ws, hipStream_t s) {
    if (arnn_token_pass_ok(n)) return arnn_token_pass(n, L, oc0, oc_stride, hc_init, first_tok, tokens, ws, s);   // 14.3 -> ~3.5 us per tick
    if (!arnn_ticks_ok(n)) return -1;
    return arnn_ticks(n, L, oc0, oc_stride, hc_init, first_tok, tokens, ws, s, sample::Request{});
}

int arnn_sample(const ArnnGenNet& n, int R, int L, const float* oc0, long oc_stride, long oc_bstride, const float* hc_init,
                long long* tokens, float* ws, hipStream_t s, const sample::Request& rq) {
    // each level has its build of the token pass, and the builds have bounds of their own (V <= 64 from level 2 up): never a kernel that
    // ignores what the request asks for
    const int level = rq.level(n.V);
    if (level < 1 || !rq.ok(n.V)) return -1;
    if (level == 4 ? arnn_token_force_ok(n) : level == 3 ? arnn_token_cons_ok(n) : level == 2 ? arnn_token_trunc_ok(n) : arnn_token_pass_ok(n))
        return arnn_token_sample(n, R, L, oc0, oc_stride, oc_bstride, hc_init, tokens, ws, s, rq);    // up to 8 rows per launch
    if (!arnn_ticks_ok(n)) return -1;
    int rc = 0;
    for (int r = 0; r < R && rc == 0; ++r)                     // the rows one after the other
        rc = arnn_ticks(n, L, oc0 + (long)r * oc_bstride, oc_stride, hc_init ? hc_init + (long)r * 4 * n.H : nullptr, nullptr,
                        tokens + (long)r * L, ws, s, rq.rows(r));
    return rc;
}
