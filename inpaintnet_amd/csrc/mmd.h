// The MMD (InfoVAE / WAE-MMD) latent loss between two samples x, y [B, Z] (mmd.hip).
#pragma once
#include <hip/hip_runtime.h>

enum { MMD_GAUSSIAN = 0, MMD_IMQ = 1 };

// one workspace row (two floats) per workgroup of the pair launch: ceil(B / kMmdRows) row blocks of x, as many of y
long mmd_ws_bytes(long B, int Z);
// out[4] = {coeff (a (S_xx - diag B) + a (S_yy - diag B) - c S_xy), S_xx, S_yy, S_xy}; grad (nullable) [B, Z] = d out[0] / d x.
// Two launches (pair, finish), no float atomics, every sum in a fixed order.  -1: ws too small; -2: a launch failed.
int mmd_launch(const float* x, const float* y, long B, int Z, int kind, float var, double a, double c, double diag, double coeff,
               float* out4, float* grad, void* ws, long ws_bytes, hipStream_t s);
