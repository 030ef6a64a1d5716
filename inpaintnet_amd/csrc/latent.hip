// The latent kernels of the MeasureVAE loss: KL + reparameterisation and their backward, and the same with a floor under the KL term
// ("free bits").  Grid-stride and HBM-bound; the wave and workgroup sums are reduce.h's.
#include <algorithm>
#include "common.h"
#include "latent.h"
#include "prof.h"
#include "pw_launch.h"
#include "reduce.h"

namespace {

// z = mu + eps * exp(ls);  kl_sum += sum 0.5(sigma^2 + mu^2 - 1) - ls
__global__ void reparam_kl_kernel(const float* __restrict__ mu, const float* __restrict__ ls,
                                  const float* __restrict__ eps, float* __restrict__ z, float* __restrict__ sigma,
                                  long n, float* __restrict__ kl_sum) {
    float acc = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float l = ls[i], m = mu[i];
        const float s = expf(l);
        if (z) z[i] = m + (eps ? eps[i] : 0.f) * s;
        if (sigma) sigma[i] = s;
        acc += 0.5f * (s * s + m * m - 1.f) - l;
    }
    if (kl_sum) {                                   // one atomic per block: a thousand of them on one address cost ~10 us
        __shared__ float part[4];
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) unsafeAtomicAdd(kl_sum, (part[0] + part[1]) + (part[2] + part[3]));     // pairwise: not reduce.h's sum4
    }
}

// dmu = dz + k*mu ;  dls = dz*eps*sigma + k*(sigma^2 - 1)      (k = kscale [* *kdev]: beta / B times the upstream gradient
// of the KL term, which autograd hands over as a device scalar)
__global__ void latent_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ mu,
                                  const float* __restrict__ ls, const float* __restrict__ eps, float kscale,
                                  const float* __restrict__ kdev, float* __restrict__ dmu, float* __restrict__ dls, long n) {
    if (kdev) kscale *= *kdev;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float s = expf(ls[i]);
        const float g = dz ? dz[i] : 0.f;
        dmu[i] = g + kscale * mu[i];
        dls[i] = g * (eps ? eps[i] : 0.f) * s + kscale * (s * s - 1.f);
    }
}

// ---- the KL term with a floor ("free bits").  KL[b,d] = 0.5(sigma^2 + mu^2 - 1) - ls over [rows, Z] is summed
// into PARTS -- 'measure': part[b] = sum_d, one per row; 'dim': part[d] = sum_b, one per column -- and a part counts with
// max(part, thr): kept = !(part <= thr) (a tie is floored, a NaN part is kept and reaches both sums); kl_sum += sum kept ? part : thr,
// kl_raw += sum part.  Every part is a pure function of (mu, ls, rows, Z, whether the 16-byte path runs): its additions happen in one
// fixed order, no float atomic anywhere -- a part next to the threshold keeps its keep bit from run to run, and so do the two scalars
// their bits.  Two launches per mode: the elementwise pass, then one finishing workgroup.  VEC = 4: Z % 4 == 0 and every pointer
// 16-byte aligned; VEC = 1 otherwise.
constexpr int kFbMeasureGrid = 256;              // workgroups of the 'measure' forward: a wave per row, 1024 rows per pass of the grid
constexpr int kFbDimGrid = 128;                  // workgroups of the 'dim' forward (4 rows each per pass) = rows of its workspace

template <int VEC>
__device__ __forceinline__ void fb_load(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x[k];
    } else {
        v[0] = *p;
    }
}
template <int VEC>
__device__ __forceinline__ void fb_store(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    else *p = v[0];
}
// z (nullable) = m + e * exp(l) for the VEC elements at p; returns their KL terms added onto acc, in element order
template <int VEC>
__device__ __forceinline__ void fb_elements(const float* __restrict__ mu, const float* __restrict__ ls, const float* __restrict__ eps,
                                            float* __restrict__ z, long at, float (&acc)[VEC]) {
    float m[VEC], l[VEC], e[VEC], zz[VEC];
    fb_load<VEC>(mu + at, m);
    fb_load<VEC>(ls + at, l);
    if (eps) fb_load<VEC>(eps + at, e);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float s = expf(l[k]);
        zz[k] = m[k] + (eps ? e[k] : 0.f) * s;
        acc[k] += 0.5f * (s * s + m[k] * m[k] - 1.f) - l[k];
    }
    if (z) fb_store<VEC>(z + at, zz);
}

// 'measure', launch 1 of 2: z and parts[row], one wavefront per row.  Lane L adds its elements L*VEC + k + 64*VEC*j in ascending j (one
// chain per k, then (a0 + a1) + (a2 + a3)), wave_sum's xor tree adds the lanes.  The floor and the two scalars are the finishing launch's.
template <int VEC>
__global__ void __launch_bounds__(256)
reparam_kl_fb_measure_kernel(const float* __restrict__ mu, const float* __restrict__ ls, const float* __restrict__ eps,
                             float* __restrict__ z, long rows, int Z, float* __restrict__ parts) {
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long row = wave; row < rows; row += nwaves) {
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int c = lane * VEC; c < Z; c += 64 * VEC) fb_elements<VEC>(mu, ls, eps, z, row * Z + c, acc);
        float a = acc[0];
        if constexpr (VEC == 4) a = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        a = wave_sum(a);
        if (lane == 0) parts[row] = a;
    }
}

// 'dim', launch 1 of 2: z, and ws[g*Z + c] = workgroup g's share of column c's sum.  A workgroup is 4 row-lanes (its waves) x 64*VEC
// columns; row-lane r of workgroup g adds rows 4g + r + 4*gridDim.x*j in ascending j, the four row-lanes are added in order.  EVERY
// workgroup stores all Z of its entries with plain stores (one without rows: zeros): nothing to zero in front, no atomics -- the
// consumer is the next launch (grad_sqnorm_kernel's pattern).
template <int VEC>
__global__ void __launch_bounds__(256)
reparam_kl_fb_dim_kernel(const float* __restrict__ mu, const float* __restrict__ ls, const float* __restrict__ eps,
                         float* __restrict__ z, long rows, int Z, float* __restrict__ ws) {
    __shared__ float part[4][64 * VEC];
    const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
    for (int c0 = 0; c0 < Z; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        if (c < Z)                                           // (VEC = 4: Z % 4 == 0, so c < Z covers c + 3)
            for (long r = (long)blockIdx.x * 4 + rl; r < rows; r += (long)gridDim.x * 4) fb_elements<VEC>(mu, ls, eps, z, r * Z + c, acc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) part[rl][lane * VEC + k] = acc[k];
        __syncthreads();
        if (rl == 0 && c < Z) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int j = lane * VEC + k;
                ws[(long)blockIdx.x * Z + c + k] = sum4(part, j);
            }
        }
        __syncthreads();
    }
}

// The finishing launch of both modes: ONE workgroup of kFbFinishBlock threads, so that the two scalars are sums in a fixed order too
// (two chains of atomics meet their addends in two different orders: with every part kept kl_sum and kl_raw would differ in the last
// bit from run to run).  ws given ('dim'): part[c] = the G workspace rows of column c -- thread (q, c) adds rows q, q + 4, ... in
// ascending order, the four q are added in order -- and parts[c] is written here; ws null ('measure'): parts[c] is read.  Then the
// floor: keep[c], and per thread the floored and the plain sum of its parts c = t, t + 256, ...; wave_sum, the four waves in order,
// one thread adds onto *kl_sum and *kl_raw.
constexpr int kFbFinishBlock = 1024;
__global__ void __launch_bounds__(kFbFinishBlock)
reparam_kl_fb_finish_kernel(const float* __restrict__ ws, int G, long nparts, float thr, float* __restrict__ parts,
                            float* __restrict__ keep, float* __restrict__ kl_sum, float* __restrict__ kl_raw) {
    __shared__ float part[4][256];
    __shared__ float tot[2][4];
    const int cl = threadIdx.x & 255, q = threadIdx.x >> 8;
    float f = 0.f, r = 0.f;
    for (long c0 = 0; c0 < nparts; c0 += 256) {
        const long c = c0 + cl;
        if (ws) {
            float acc = 0.f;
            if (c < nparts)
                for (int g = q; g < G; g += 4) acc += ws[(long)g * nparts + c];
            part[q][cl] = acc;
            __syncthreads();
        }
        if (q == 0 && c < nparts) {
            float p;
            if (ws) { p = sum4(part, cl); parts[c] = p; }
            else p = parts[c];
            const bool kept = !(p <= thr);
            keep[c] = kept ? 1.f : 0.f;
            f += kept ? p : thr;
            r += p;
        }
        if (ws) __syncthreads();
    }
    if (q == 0) {                                       // threads 0..255: four whole waves
        f = wave_sum(f);
        r = wave_sum(r);
        if ((cl & 63) == 0) { tot[0][cl >> 6] = f; tot[1][cl >> 6] = r; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *kl_sum += sum4(tot[0]);
        *kl_raw += sum4(tot[1]);
    }
}

// latent_bwd_kernel with the keep vector: dmu = dz + kk*mu ; dls = dz*eps*sigma + kk*(sigma^2 - 1), kk = the element's part is kept ?
// k : 0 -- a SELECTION, never a product with the float keep, so that a floored part hands dz on bit for bit and, with every part kept,
// the expressions are latent_bwd_kernel's.  Element i belongs to part i / Z ('measure') or i % Z ('dim'); the pair is carried along
// the grid-stride loop, one division per thread.
__global__ void latent_bwd_fb_kernel(const float* __restrict__ dz, const float* __restrict__ mu, const float* __restrict__ ls,
                                     const float* __restrict__ eps, float kscale, const float* __restrict__ kdev,
                                     const float* __restrict__ keep, int per_dim, float* __restrict__ dmu, float* __restrict__ dls,
                                     long rows, int Z) {
    if (kdev) kscale *= *kdev;
    const long n = rows * Z, stride = (long)gridDim.x * blockDim.x;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long row = i / Z;
    int col = (int)(i - row * Z);
    const long qs = stride / Z;
    const int rs = (int)(stride - qs * Z);
    for (; i < n; i += stride) {
        const float kk = keep[per_dim ? (long)col : row] != 0.f ? kscale : 0.f;
        const float s = expf(ls[i]);
        const float g = dz ? dz[i] : 0.f;
        dmu[i] = g + kk * mu[i];
        dls[i] = g * (eps ? eps[i] : 0.f) * s + kk * (s * s - 1.f);
        col += rs;
        row += qs;
        if (col >= Z) { col -= Z; ++row; }
    }
}

}  // namespace

int pw_reparam_kl(const float* mu, const float* ls, const float* eps, float* z, float* sigma, long n, float* kl_sum,
                  hipStream_t s) {
    hipLaunchKernelGGL(reparam_kl_kernel, dim3(grid_for(n, 256, kl_sum ? 64 : 512)), dim3(256), 0, s, mu, ls, eps, z, sigma, n, kl_sum);
    return ok();
}
int pw_latent_bwd(const float* dz, const float* mu, const float* ls, const float* eps, float kscale, const float* kdev,
                  float* dmu, float* dls, long n, hipStream_t s) {
    hipLaunchKernelGGL(latent_bwd_kernel, dim3(grid_for(n, 256, 512)), dim3(256), 0, s, dz, mu, ls, eps, kscale, kdev, dmu,
                       dls, n);
    return ok();
}
// the 'dim' forward's grid, a function of rows alone: the order of a column's sum depends on nothing else
static int fb_dim_grid(long rows) { return (int)std::min<long>((rows + 3) / 4, kFbDimGrid); }
static bool fb_vec4(int Z, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = (uintptr_t)(Z & 3);
    for (const void* p : ptrs) bits |= (uintptr_t)p & 15;          // (a null pointer is aligned)
    return bits == 0;
}
long pw_reparam_kl_fb_ws_bytes(long rows, int Z, int per) {
    if (rows <= 0 || Z <= 0 || (per != 0 && per != 1)) return -1;
    return per == 1 ? (long)fb_dim_grid(rows) * Z * (long)sizeof(float) : 0;
}
int pw_reparam_kl_fb(const float* mu, const float* ls, const float* eps, float* z, long rows, int Z, float free_nats, int per,
                     float* parts, float* keep, float* kl_sum, float* kl_raw, void* ws, long ws_bytes, hipStream_t s) {
    const long need = pw_reparam_kl_fb_ws_bytes(rows, Z, per);
    if (need < 0 || ws_bytes < need || (need > 0 && !ws)) return -1;
    const bool v4 = fb_vec4(Z, {mu, ls, eps, z});
    const double bytes = 4.0 * (double)rows * Z * (2 + (eps ? 1 : 0) + (z ? 1 : 0));
    const float thr = per == 0 ? free_nats : (float)((double)rows * (double)free_nats);       // 'dim': B * lambda, rounded once
    const int G = fb_dim_grid(rows);
    if (per == 0) {
        ProfScope prof(PROF_HBM, 0.0, s, "reparam_kl_fb_measure", bytes + 4.0 * (double)rows);
        const dim3 grid(grid_for(rows * 64, 256, kFbMeasureGrid));
        if (v4) hipLaunchKernelGGL(reparam_kl_fb_measure_kernel<4>, grid, dim3(256), 0, s, mu, ls, eps, z, rows, Z, parts);
        else    hipLaunchKernelGGL(reparam_kl_fb_measure_kernel<1>, grid, dim3(256), 0, s, mu, ls, eps, z, rows, Z, parts);
    } else {
        ProfScope prof(PROF_HBM, 0.0, s, "reparam_kl_fb_dim", bytes + 4.0 * (double)G * Z);
        if (v4) hipLaunchKernelGGL(reparam_kl_fb_dim_kernel<4>, dim3(G), dim3(256), 0, s, mu, ls, eps, z, rows, Z, (float*)ws);
        else    hipLaunchKernelGGL(reparam_kl_fb_dim_kernel<1>, dim3(G), dim3(256), 0, s, mu, ls, eps, z, rows, Z, (float*)ws);
    }
    if (ok() != 0) return -2;
    const long nparts = per == 0 ? rows : (long)Z;
    ProfScope prof(PROF_HBM, 0.0, s, "reparam_kl_fb_finish", (per == 0 ? 4.0 : 4.0 * G + 4.0) * (double)nparts + 4.0 * (double)nparts);
    hipLaunchKernelGGL(reparam_kl_fb_finish_kernel, dim3(1), dim3(kFbFinishBlock), 0, s, per == 0 ? (const float*)nullptr : (const float*)ws, G,
                       nparts, thr, parts, keep, kl_sum, kl_raw);
    return ok();
}
int pw_latent_bwd_fb(const float* dz, const float* mu, const float* ls, const float* eps, float kscale, const float* kdev,
                     const float* keep, int per, float* dmu, float* dls, long rows, int Z, hipStream_t s) {
    const long n = rows * Z;
    ProfScope prof(PROF_HBM, 0.0, s, "latent_bwd_fb", 4.0 * (double)n * (4 + (dz ? 1 : 0) + (eps ? 1 : 0)));
    hipLaunchKernelGGL(latent_bwd_fb_kernel, dim3(grid_for(n, 256, 512)), dim3(256), 0, s, dz, mu, ls, eps, kscale, kdev, keep, per,
                       dmu, dls, rows, Z);
    return ok();
}
