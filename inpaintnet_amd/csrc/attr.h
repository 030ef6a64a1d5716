// Attribute-regularised latent dimensions (AR-VAE, Pati & Lerch 2020) on the MeasureVAE (attr.hip): the four
// per-measure attributes of the reference's dataset, and the pairwise loss that ties an attribute to a latent dimension.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int kAttrColumns = 4;                  // num_notes, note_range, rhy_entropy, beat_strength
constexpr int kAttrMaxT = 96;                    // ticks of a measure the extractor stages in LDS (the model's T is 24)
constexpr int kAttrMaxA = 8;                     // regularised dimensions of one call

struct AttrDims { int d[kAttrMaxA]; };

// tokens [B, T] int64 -> out [B, 4].  -1: a bad argument (before any launch); -2: the launch failed.
int attr_measure_launch(const long long* tokens, long B, int T, int V, int slur, int rest, int none, const int* midi, int midi_lo,
                        int midi_hi, float* out, hipStream_t s);

// one workspace row (a float sum and three int counts) per attribute and row block of the pair launch
long attr_reg_ws_bytes(long B, int A);
// out[1 + A] = {coeff sum_a L_a, L_0 .. L_{A-1}}; counts[A][3] = {concordant, discordant, attribute-tied} ordered pairs i != j;
// grad (nullable) [B, A] = d out[0] / d z[:, dims[a]].  Two launches (pair, finish), no atomics, every float sum in a fixed order.
int attr_reg_launch(const float* z, long B, int Z, const AttrDims& dims, int A, const float* attrs, float delta, double coeff, float* out,
                    long long* counts, float* grad, void* ws, long ws_bytes, hipStream_t s);
