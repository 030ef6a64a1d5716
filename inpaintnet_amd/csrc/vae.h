#pragma once
#include <hip/hip_runtime.h>
#include "../../include/inpaintnet_hip.h"

size_t vae_encoder_ws_bytes(const inet_vae_config& c, int B, int save);
int vae_encoder_fwd(const inet_vae_config& c, int B, const long long* tokens, const float* p, const float* mask,
                    float* mu, float* logsigma, void* ws, int save, hipStream_t s);
int vae_encoder_bwd(const inet_vae_config& c, int B, const long long* tokens, const float* p, float* g,
                    const float* mask, const float* dmu, const float* dls, void* ws, hipStream_t s, int stage = 0);
// stage 0 = the whole backward pass.  1 = the Linear heads and GRU layer 1: afterwards their gradients (two contiguous
// ranges of the arena) are final and a data-parallel all-reduce of them can start; 2 = the rest (layer 0, embedding) on
// the state stage 1 left in `ws`.
size_t vae_decoder_ws_bytes(const inet_vae_config& c, int B, int save);
int vae_decoder_fwd(const inet_vae_config& c, int B, const float* z, const long long* target, int teacher_forced,
                    const float* p, const float* mask_beat, const float* mask_tick, float* weights,
                    long long* samples, void* ws, int save, hipStream_t s, uint64_t multinomial_seed = 0,
                    const double* uniforms = nullptr, float temperature = 1.f, int top_k = 0, double top_p = 1.0,
                    float* logp = nullptr, const unsigned long long* allow = nullptr, const int* forced = nullptr);
// uniforms != null (a free-running call: no target, no seed): temperature sampling by csrc/sample.h's rule, one
// uniform per (row, tick) [B, T] -- inside decode_b1.hip's launch where its planner has a sampling plan, else tick by tick.
// A TRUNCATED call (1 <= top_k < V, top_p < 1, or logp [B, T] != null: the drawn tokens' log-probabilities): sample.h's truncation in
// front of every draw, in the truncating builds of the same launch or tick by tick with pw_sample_truncated.
// A CONSTRAINED call (allow [B, T, ceil(V / 64)] != null: sample.h's words of allowed tokens per (row, tick)) is a truncated call with the
// mask in front of the truncation: the masked builds of the same launch, or tick by tick with pw_sample_constrained.
// A FORCED call (forced [B, T] != null: sample.h's forced token per (row, tick), a value outside [0, V) = a free tick) is a constrained call,
// with or without a mask, whose forced ticks return and feed back the given token and report its log-probability: the forced builds of the
// same launch, or tick by tick with pw_sample_forced.
int vae_decoder_bwd(const inet_vae_config& c, int B, const float* dweights, const float* weights,
                    const long long* tokens_in, const float* p, float* g, const float* mask_beat,
                    const float* mask_tick, float* dz, void* ws, hipStream_t s);
int vae_ws_field(const inet_vae_config& c, int B, int which, const char* name, long long* offset_floats, long long* count);
