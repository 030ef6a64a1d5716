// The importance-weighted log-likelihood of a measure (the IWAE bound, Burda et al. 2016) in three launches (iw.hip, DESIGN.md
// section 26).  For a measure x_b (T tokens) with the encoder's mu_b, ls_b (log sigma) [Z] and eps[b,k,:] standard normal, k < K:
//   z[b,k,d]  = mu[b,d] + eps[b,k,d] * exp(ls[b,d])
//   logr[b,k] = log p(z) - log q(z|x) = sum_d ( 0.5 eps^2 - 0.5 z^2 + ls[b,d] )                    (the 2 pi terms cancel)
//   nll[b,k]  = - sum_t log softmax(weights[b,k,t,:])[ x[b,t] ]        (the decoder on z[b,k], x_b's own tokens fed back, eval mode)
//   logw[b,k] = logr[b,k] - nll[b,k]
//   m = max_k logw;  s1 = sum_k exp(logw - m);  s2 = sum_k exp(2 (logw - m))
//   iwae[b] = m + log(s1 / K);  elbo[b] = (sum_k logw) / K;  ess[b] = s1^2 / s2;  rec[b] = (sum_k nll) / K;
//   kl[b] = -(sum_k logr) / K, formed as -(sum_k logw + sum_k nll) / K
// A NaN anywhere in a measure's logw row: iwae, elbo and ess are NaN.  m == -inf: iwae = elbo = -inf, ess = 0.  A +inf in the row:
// whatever IEEE gives (NaN).  No float atomics; every sum in a fixed order: two calls on the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

// z [B*Kc, Z], logr [B*Kc]; row r = b * Kc + j reads mu + b Z, ls + b Z and eps + b * eps_stride_b + j * Z.
int iw_draw_launch(const float* mu, const float* ls, const float* eps, long eps_stride_b, float* z, float* logr, long B, int Kc, int Z,
                   hipStream_t s);
// weights [R*T, V] with row stride ld_w, targets [R, T]; logr (nullable: reads as 0) [R]; nll, logw (nullable, not both) written at
// [(r / group) * ld_out + r % group].  A target outside [0, V): NaN for that row, nothing is read through it.
int nll_rows_launch(const float* weights, long ld_w, const long long* targets, const float* logr, float* nll, float* logw, long ld_out,
                    long R, int group, int T, int V, hipStream_t s);
// logw, nll [B, K] with row stride ld; out [B, 5] doubles = {iwae, elbo, ess, rec, kl}.
int iw_finish_launch(const float* logw, const float* nll, long ld, long B, int K, double* out, hipStream_t s);
