// Host-side launchers of the optimizer kernels (optim.hip): the norm of the gradient arena, the one Adam / AdamW step kernel, and the
// two one-thread kernels that follow a step's skip decision.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The norm of the gradient arena: partials[pw_sqnorm_parts()] = the f64 sums of squares of the fixed grid's shares of g (every entry
// written: nothing to zero in front), what the optimizer step takes as `partials`.
int pw_sqnorm_parts();
int pw_grad_sqnorm(const float* g, long n, double* partials, hipStream_t s);
// The optimizer step, one launch (the rule: optim.hip).  Nullable members switch a part off.
struct PwAdamStep {
    float* p; const float* g; float* m; float* v; long n;
    float lr, b1, b2, eps; int step; float gscale;
    float max_norm; const double* partials;      // global-norm clipping and the non-finite drop; null: neither, max_norm is ignored
    float weight_decay; const unsigned* mask;    // p *= (float)(1 - lr * weight_decay) where the mask says so; null: everywhere
    float* ema; float ema_decay;                 // ema = fmaf(ema_decay, ema, (float)(1 - ema_decay) * p_new); null: none
    const float* step_flag;                      // device float, non-zero = skip (the ranks' summed chain status); null: this process's word
    unsigned* report;                            // host-mapped words zeroed by the caller: four, eight with partials; null: none
};
int pw_adam_step(const PwAdamStep& a, hipStream_t s);
int pw_step_flag_export(float* dst, hipStream_t s);
int pw_epoch_stats_add(float* sums, const float* loss, const float* acc, hipStream_t s, const float* step_flag = nullptr);
