// AnticipationRNN's token generation (arnn_gen.hip): the generation network's weights and the two entry points.
#pragma once
#include <hip/hip_runtime.h>
#include "sample.h"

// emb [V', E]; W_ih0 [4H, E + Hc], W_hh0 [4H, H], W_ih1 / W_hh1 [4H, H], b_* [4H]; W1 [U, H], b1 [U]; W2 [V, U], b2 [V]
struct ArnnGenNet {
    int E, Hc, H, U, V;
    const float *emb, *W_ih0, *b_ih0, *W_hh0, *b_hh0, *W_ih1, *b_ih1, *W_hh1, *b_hh1, *W1, *b1, *W2, *b2;
};

// option key 14 / INET_ARNN_GEN: 0 = the per-tick launches always, 1 .. 4 = the persistent pass where it applies
void arnn_gen_set_mode(int m);
// the sequential part of AnticipationRNN's free-running pass: L ticks of batch element 0 -> its argmax tokens.  oc row t at
// oc0 + t * oc_stride; hc_init [2][2][H] or null; first_tok: the token in front of tick 0 (null: 0).  -1: shape out of range.
size_t arnn_generate_ws_floats(const ArnnGenNet& net, int L);
int arnn_generate(const ArnnGenNet& net, int L, const float* oc0, long oc_stride, const float* hc_init, const long long* first_tok,
                  long long* tokens, float* ws, hipStream_t s);
// AnticipationRNN's generate (anticipation_rnn_gauss_reg_model.py:570-679): R independent rows, each L ticks with the token DRAWN from
// softmax(temp * logits) by the uniform uniforms[r][t] (sample.h).  oc row r at oc0 + r * oc_bstride, hc_init [R][2][2][H] or null.
size_t arnn_sample_ws_floats(const ArnnGenNet& net, int R, int L);
// rq: sample.h's Request with [R][L] arrays (logits [R][L][V]: what each tick drew from; allow [R][L][ceil(V / 64)]), uniforms required.
// The request's level picks the kernels: 1 = the sampling build; 2 = the truncating kernels (labels trunc_...: truncation on, or logp /
// logits wanted; logp is NaN where a tick took the argmax rule); 3 = the masked kernels (cons_...), which are truncating ones; 4 = the
// forced kernels (force_...), which are masked ones (allow nullable): a forced value in [0, V) is that tick's token, returned, fed back
// and scored.  -1: a shape out of range, or what rq.ok(V) refuses.
int arnn_sample(const ArnnGenNet& net, int R, int L, const float* oc0, long oc_stride, long oc_bstride, const float* hc_init,
                long long* tokens, float* ws, hipStream_t s, const sample::Request& rq);
