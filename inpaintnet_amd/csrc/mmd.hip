// The MMD (InfoVAE / WAE-MMD) latent loss between x = z_tilde and y = z_prior, both [B, Z].
//   d(u, v) = sum_z (u_z - v_z)^2;  k = exp(-d / var) (gaussian) or var / (var + d) (imq);  S_xx, S_yy, S_xy = the sums of k over all
//   pairs, diagonals included;  value = coeff (a (S_xx - diag B) + a (S_yy - diag B) - c S_xy);
//   d value / d x_i = coeff (4a sum_j k'(d_ij) (x_i - x_j) - 2c sum_p k'(d_pi) (x_i - y_p)),  k' = -k / var or -k^2 / var.
// Two launches.  mmd_pair: workgroup g < nb owns rows 8g .. 8g + 7 of x and walks the column tiles (256 columns, one per thread) of x,
// then of y: its shares of S_xx and S_xy and, with a gradient, its own 8 gradient rows.  Workgroup nb + g owns the same rows of y
// against y: its share of S_yy.  mmd_finish: one workgroup adds the shares in a fixed order and forms the value.
// A distance is the sum of the squared DIFFERENCES, added in ascending z (never |u|^2 + |v|^2 - 2 u.v): the distance of a row to
// itself is exactly 0, its kernel value exactly 1, so that subtracting the diagonal ('unbiased') is exact.  No float atomic anywhere,
// every sum in an order that depends on (B, Z) alone: two calls on the same inputs give the same bits, in the value and the gradient.
#include <algorithm>
#include "common.h"
#include "mmd.h"
#include "prof.h"
#include "reduce.h"

namespace {

constexpr int kMmdRows = 8;                      // rows of a workgroup's block: B = 256 gives 32 + 32 workgroups
constexpr int kMmdTile = 256;                    // columns of a tile: one per thread
constexpr int kMmdZc = 32;                       // the chunk of Z staged in LDS at a time: any Z >= 1 fits
constexpr int kMmdSpan = 256;                    // latent dimensions whose gradient a workgroup holds in registers at a time (8 per thread)
constexpr int kMmdFinishBlock = 256;

// kernel value and k'(d) of one distance; expf is the device library's (not the hardware approximation __expf)
template <int KIND>
__device__ __forceinline__ void mmd_k(float d, float var, float& k, float& w) {
    if constexpr (KIND == MMD_GAUSSIAN) {
        k = expf(-d / var);
        w = -k / var;
    } else {
        k = var / (var + d);
        w = -(k * k) / var;
    }
}

// A chunk of a column tile on its way to LDS: cols[c][zz] = src[j0 + c][z0 + zz], zeros past B and past Z (a zero pair adds exactly 0
// to a distance).  mmd_fetch issues a thread's 32 loads into registers, mmd_put stores them: the loads of the NEXT chunk are in flight
// while the current one is computed on.  Rows padded to 33 floats: thread c reads cols[c][zz], 64 lanes on 64 different banks.
constexpr int kMmdPre = kMmdTile * kMmdZc / 256;
__device__ __forceinline__ void mmd_fetch(float (&pre)[kMmdPre], const float* __restrict__ src, long B, int Z, long j0, int z0) {
    // thread t loads column t / 32 + 8 i at z0 + t % 32: one address per thread, the step 8 Z between its loads is uniform
    const long j = j0 + threadIdx.x / kMmdZc;
    const int z = z0 + threadIdx.x % kMmdZc;
    const float* __restrict__ p = src + j * Z + z;
    const long left = z < Z ? B - j : 0;                     // columns j + 8 i with 8 i < left exist
#pragma unroll
    for (int i = 0; i < kMmdPre; ++i) pre[i] = (256 / kMmdZc) * i < left ? p[(long)((256 / kMmdZc) * i) * Z] : 0.f;
}
__device__ __forceinline__ void mmd_put(float (*cols)[kMmdZc + 1], const float (&pre)[kMmdPre]) {
#pragma unroll
    for (int i = 0; i < kMmdPre; ++i) {
        const int idx = threadIdx.x + 256 * i;
        cols[idx / kMmdZc][idx % kMmdZc] = pre[i];
    }
}

// Pass 1 of a tile: thread t holds the 8 distances of column j0 + t to the workgroup's rows, each a chain over ascending z; the kernel
// values of a tile are added as ((k0 + k1) + (k2 + k3)) + ((k4 + k5) + (k6 + k7)) and then onto the thread's running share.
// Pass 2 (gradient): the weights k' go to LDS; thread (row r = t / 32, lane zl = t % 32) adds, for each of its latent dimensions
// z = zs + zl + 32 j, the 256 terms k'(d_rc) (x_rz - col_cz) of the tile in four chains (c % 4), combines them (p0 + p1) + (p2 + p3)
// and adds coef * that onto its accumulator -- coef = coeff 4a for the x tiles, -coeff 2c for the y tiles.
template <int KIND>
__global__ void __launch_bounds__(256)
mmd_pair_kernel(const float* __restrict__ x, const float* __restrict__ y, long B, int Z, float var, float ga, float gc,
                float* __restrict__ grad, float* __restrict__ ws, int nb) {
    __shared__ float cols[kMmdTile][kMmdZc + 1];
    __shared__ f32x4 xs[kMmdZc][2];              // xs[zz] = the 8 rows' values at z0 + zz: two 16-byte broadcast reads
    __shared__ f32x4 wl[kMmdRows][kMmdTile / 4];
    __shared__ float red[4];
    const int t = threadIdx.x;
    const bool own_x = (int)blockIdx.x < nb;
    const long i0 = (long)(own_x ? blockIdx.x : blockIdx.x - nb) * kMmdRows;
    const float* __restrict__ rowsrc = own_x ? x : y;
    const bool want_grad = own_x && grad != nullptr;
    const int gr = t >> 5, gz = t & 31;
    const bool grow_ok = i0 + gr < B;
    const int nspan = want_grad ? (Z + kMmdSpan - 1) / kMmdSpan : 1;
    for (int sp = 0; sp < nspan; ++sp) {
        const int zs = sp * kMmdSpan;
        float xr[8], acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int z = zs + gz + 32 * j;
            xr[j] = (want_grad && grow_ok && z < Z) ? rowsrc[(i0 + gr) * Z + z] : 0.f;
            acc[j] = 0.f;
        }
        for (int phase = 0; phase < (own_x ? 2 : 1); ++phase) {
            const float* __restrict__ colsrc = (own_x && phase == 0) ? x : y;
            const float coef = phase == 0 ? ga : -gc;
            float S = 0.f;
            for (long j0 = 0; j0 < B; j0 += kMmdTile) {
                float d[8], pre[kMmdPre], prex;
#pragma unroll
                for (int r = 0; r < 8; ++r) d[r] = 0.f;
                mmd_fetch(pre, colsrc, B, Z, j0, 0);
                prex = (grow_ok && gz < Z) ? rowsrc[(i0 + gr) * Z + gz] : 0.f;
                for (int z0 = 0; z0 < Z; z0 += kMmdZc) {
                    __syncthreads();
                    mmd_put(cols, pre);
                    reinterpret_cast<float*>(xs)[gz * 8 + gr] = prex;
                    __syncthreads();
                    if (z0 + kMmdZc < Z) {
                        mmd_fetch(pre, colsrc, B, Z, j0, z0 + kMmdZc);
                        prex = (grow_ok && z0 + kMmdZc + gz < Z) ? rowsrc[(i0 + gr) * Z + z0 + kMmdZc + gz] : 0.f;
                    }
#pragma unroll 8
                    for (int zz = 0; zz < kMmdZc; ++zz) {
                        const float cv = cols[t][zz];
                        const f32x4 u = xs[zz][0], v = xs[zz][1];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float e = u[r] - cv, f = v[r] - cv;
                            d[r] = fmaf(e, e, d[r]);
                            d[4 + r] = fmaf(f, f, d[4 + r]);
                        }
                    }
                }
                const bool col_ok = j0 + t < B;
                float k[8], w[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    mmd_k<KIND>(d[r], var, k[r], w[r]);
                    if (!(col_ok && i0 + r < B)) { k[r] = 0.f; w[r] = 0.f; }
                }
                S += ((k[0] + k[1]) + (k[2] + k[3])) + ((k[4] + k[5]) + (k[6] + k[7]));
                if (want_grad) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) reinterpret_cast<float*>(wl[r])[t] = w[r];
                    mmd_fetch(pre, colsrc, B, Z, j0, zs);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int z0 = zs + 32 * j;
                        if (z0 < Z) {
                            __syncthreads();
                            mmd_put(cols, pre);
                            __syncthreads();
                            if (j < 7 && z0 + 32 < Z) mmd_fetch(pre, colsrc, B, Z, j0, z0 + 32);
                            const float xv = xr[j];
                            float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll 4
                            for (int c4 = 0; c4 < kMmdTile / 4; ++c4) {
                                const f32x4 wv = wl[gr][c4];
                                p0 = fmaf(wv[0], xv - cols[4 * c4 + 0][gz], p0);
                                p1 = fmaf(wv[1], xv - cols[4 * c4 + 1][gz], p1);
                                p2 = fmaf(wv[2], xv - cols[4 * c4 + 2][gz], p2);
                                p3 = fmaf(wv[3], xv - cols[4 * c4 + 3][gz], p3);
                            }
                            acc[j] = fmaf(coef, (p0 + p1) + (p2 + p3), acc[j]);
                        }
                    }
                }
            }
            if (sp == 0) {                           // the workgroup's share: the xor tree over a wave's lanes, the four waves in order
                S = wave_sum(S);
                if ((t & 63) == 0) red[t >> 6] = S;
                __syncthreads();
                if (t == 0) {
                    ws[2 * (long)blockIdx.x + phase] = sum4(red);
                    if (!own_x) ws[2 * (long)blockIdx.x + 1] = 0.f;
                }
            }
        }
        if (want_grad && grow_ok) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int z = zs + gz + 32 * j;
                if (z < Z) grad[(i0 + gr) * Z + z] = acc[j];
            }
        }
    }
}

// ONE workgroup: thread t adds the shares of workgroups t, t + 256, ... in ascending order, the xor tree adds a wave's lanes, the four
// waves are added in order; one thread forms the value in double from the three float sums and rounds it once.
__global__ void __launch_bounds__(kMmdFinishBlock)
mmd_finish_kernel(const float* __restrict__ ws, int nb, long B, double a, double c, double diag, double coeff, float* __restrict__ out) {
    __shared__ float tot[3][4];
    const int t = threadIdx.x;
    float sxx = 0.f, syy = 0.f, sxy = 0.f;
    for (int g = t; g < nb; g += kMmdFinishBlock) {
        sxx += ws[2 * (long)g];
        sxy += ws[2 * (long)g + 1];
        syy += ws[2 * ((long)nb + g)];
    }
    sxx = wave_sum(sxx);
    syy = wave_sum(syy);
    sxy = wave_sum(sxy);
    if ((t & 63) == 0) { tot[0][t >> 6] = sxx; tot[1][t >> 6] = syy; tot[2][t >> 6] = sxy; }
    __syncthreads();
    if (t == 0) {
        const float Sxx = sum4(tot[0]);
        const float Syy = sum4(tot[1]);
        const float Sxy = sum4(tot[2]);
        const double off = diag * (double)B;
        out[0] = (float)(coeff * (a * ((double)Sxx - off) + a * ((double)Syy - off) - c * (double)Sxy));
        out[1] = Sxx;
        out[2] = Syy;
        out[3] = Sxy;
    }
}

inline long mmd_blocks(long B) { return (B + kMmdRows - 1) / kMmdRows; }

}  // namespace

long mmd_ws_bytes(long B, int Z) {
    if (B < 1 || Z < 1) return -1;
    return 2 * mmd_blocks(B) * 2 * (long)sizeof(float);
}

int mmd_launch(const float* x, const float* y, long B, int Z, int kind, float var, double a, double c, double diag, double coeff,
               float* out4, float* grad, void* ws, long ws_bytes, hipStream_t s) {
    const long need = mmd_ws_bytes(B, Z);
    if (need < 0 || !ws || ws_bytes < need) return -1;
    const int nb = (int)mmd_blocks(B);
    const float ga = (float)(4.0 * coeff * a), gc = (float)(2.0 * coeff * c);
    {
        ProfScope prof(PROF_HBM, 0.0, s, grad ? "mmd_pair_grad" : "mmd_pair", 4.0 * (double)B * Z * (grad ? 3.0 : 2.0));
        if (kind == MMD_GAUSSIAN)
            hipLaunchKernelGGL(mmd_pair_kernel<MMD_GAUSSIAN>, dim3(2 * nb), dim3(256), 0, s, x, y, B, Z, var, ga, gc, grad, (float*)ws, nb);
        else
            hipLaunchKernelGGL(mmd_pair_kernel<MMD_IMQ>, dim3(2 * nb), dim3(256), 0, s, x, y, B, Z, var, ga, gc, grad, (float*)ws, nb);
    }
    if (hipGetLastError() != hipSuccess) return -2;
    ProfScope prof(PROF_HBM, 0.0, s, "mmd_finish", 16.0 * (double)nb + 16.0);
    hipLaunchKernelGGL(mmd_finish_kernel, dim3(1), dim3(kMmdFinishBlock), 0, s, (const float*)ws, nb, B, a, c, diag, coeff, out4);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
