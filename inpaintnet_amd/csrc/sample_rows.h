// Host-side launchers of the sampling row kernels (sample_rows.hip) and of the counter-based dropout mask that shares their generator.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

int pw_sample_multinomial(const float* W, long ld_w, int rows, int V, long long* out, long stride, uint64_t seed,
                          uint64_t offset, hipStream_t s);
// out[row*stride] = sample.h's token of the row W[row,:] for the request r: a row here is what r calls a row, so r's strides step from
// row to row (uniforms required, logits not written).  ONE of the four row kernels runs -- temperature, truncated, constrained, forced --:
// the one of level max(floor_level, r.level(V)).  floor_level is 1 or 2: an entry that promises the truncating kernel passes 2, so that
// inet_sample_truncated with truncation off and no logp still runs it under its trunc_ label; vae.hip's tick loop passes the call's level.
// Levels 3 and 4 come from r's mask and forced array alone (level 4 without a mask: words of all ones).  A row outside the rule takes
// argmax_first over its allowed tokens, logp NaN.  -1: what r.ok(V) refuses.
namespace sample { struct Request; }
int pw_sample(const float* W, long ld_w, int rows, int V, long long* out, long stride, const sample::Request& r, int floor_level,
              hipStream_t s);
int pw_dropout_mask(float* out, long n, float p, uint64_t seed, uint64_t offset, hipStream_t s);
