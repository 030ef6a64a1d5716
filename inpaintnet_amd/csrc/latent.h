// Host-side launchers of the latent kernels (latent.hip): KL + reparameterisation, their backward, and the free-bits family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

int pw_reparam_kl(const float* mu, const float* ls, const float* eps, float* z, float* sigma, long n, float* kl_sum,
                  hipStream_t s);
int pw_latent_bwd(const float* dz, const float* mu, const float* ls, const float* eps, float kscale, const float* kdev,
                  float* dmu, float* dls, long n, hipStream_t s);
// The KL term with a floor (free bits; the rule: latent.hip).  per 0 = 'measure' (a part per row, threshold
// free_nats), 1 = 'dim' (a part per column, threshold rows * free_nats; through a workspace of pw_reparam_kl_fb_ws_bytes).  Two launches.
// parts / keep: rows or Z floats; kl_sum (floored) and kl_raw (plain) are added onto.  z and eps nullable.
long pw_reparam_kl_fb_ws_bytes(long rows, int Z, int per);
int pw_reparam_kl_fb(const float* mu, const float* ls, const float* eps, float* z, long rows, int Z, float free_nats, int per,
                     float* parts, float* keep, float* kl_sum, float* kl_raw, void* ws, long ws_bytes, hipStream_t s);
int pw_latent_bwd_fb(const float* dz, const float* mu, const float* ls, const float* eps, float kscale, const float* kdev,
                     const float* keep, int per, float* dmu, float* dls, long rows, int Z, hipStream_t s);
