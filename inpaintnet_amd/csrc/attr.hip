// Attribute-regularised latent dimensions (AR-VAE, Pati & Lerch 2020) on the MeasureVAE.
// attr_measure: tokens [B, T] -> the four attributes of the reference's dataset (folk_dataset.py:607-708), each ONE float operation
//   on ONE exact integer, so that equal attributes are equal bits.  A workgroup stages 64 rows in LDS with one coalesced read, then a
//   thread walks a row.
// attr_pair: for attribute a (blockIdx.y), latent dimension r = dims[a], x_i = z[i, r]:
//   L_a = (1 / B^2) sum_ij |tanh(delta (x_i - x_j)) - sgn(a_i - a_j)|,   value = coeff sum_a L_a,
//   d value / d x_i = (2 coeff delta / B^2) sum_j sgn(t_ij - s_ij) (1 - t_ij^2)   -- t and s are antisymmetric, so the terms (i, j) and
//   (j, i) hand x_i the same amount and a workgroup needs its own rows only.  sgn(0) = 0, as torch's sign and L1Loss's gradient.
//   Workgroup g owns rows 16g .. 16g + 15 and walks the column tiles (256 columns, one per thread): its share of the sum, its counts
//   of concordant / discordant / attribute-tied ordered pairs, and its own 16 gradient elements.
// attr_finish: one workgroup adds the shares in a fixed order.  No atomics anywhere; every float sum in an order that depends on
// (B, A) alone: two calls on the same inputs give the same bits, with or without the gradient.
#include <algorithm>
#include <cmath>
#include "common.h"
#include "attr.h"
#include "prof.h"
#include "reduce.h"

namespace {

constexpr int kAttrMeasureRows = 64;             // rows of a workgroup of the extractor: one thread each after the staging
constexpr int kAttrBadToken = -2;                // what a token outside [0, V) is staged as (-1 is 'the vocabulary has none')
constexpr int kAttrRows = 16;                    // rows of a workgroup's block of the pair launch
constexpr int kAttrTile = 256;                   // columns of a tile: one per thread
constexpr int kAttrFinishBlock = 256;

struct AttrShare { float s; int conc, disc, tied; };

__global__ void __launch_bounds__(256)
attr_measure_kernel(const long long* __restrict__ tokens, long B, int T, int V, int slur, int rest, int none,
                    const int* __restrict__ midi, int midi_span, float* __restrict__ out) {
    __shared__ int tok[kAttrMeasureRows * (kAttrMaxT + 1)];      // row stride T + 1 (odd): 64 threads on 64 rows hit 64 banks
    const long r0 = (long)blockIdx.x * kAttrMeasureRows;
    const int rows = (int)std::min<long>(kAttrMeasureRows, B - r0);
    const int n = rows * T;
    const long long* __restrict__ src = tokens + r0 * T;
    for (int i = threadIdx.x; i < n; i += 256) {
        const long long v = src[i];
        const int row = i / T;
        tok[row * (T + 1) + (i - row * T)] = (v >= 0 && v < V) ? (int)v : kAttrBadToken;
    }
    __syncthreads();
    if ((int)threadIdx.x >= rows) return;
    const int* __restrict__ mine = tok + threadIdx.x * (T + 1);
    int nslur = 0, nrest = 0, n0 = 0, n3 = 0, nother = 0, lo = 0x7fffffff, hi = -1, pos = 0;
    bool bad = false;
    for (int t = 0; t < T; ++t) {
        const int k = mine[t];
        bad |= k == kAttrBadToken;
        const bool is_slur = k == slur, is_rest = k == rest;
        nslur += is_slur;
        nrest += is_rest;
        if (!is_slur) {                          // an onset: the reference's 0/1 vector is 1 wherever the token is not the slur
            n0 += pos == 0;
            n3 += pos == 3;
            nother += pos != 0 && pos != 3;
        }
        if (k >= 0 && !is_slur && !is_rest && k != none) {
            const int m = midi[k];
            if (m >= 0) { lo = std::min(lo, m); hi = std::max(hi, m); }
        }
        pos = pos == 5 ? 0 : pos + 1;
    }
    const int onsets = T - nslur;
    float a0 = (float)(T - nslur - nrest) / (float)T;
    float a1 = (float)(hi >= 0 ? hi - lo : 0) / (float)midi_span;
    float a2 = onsets > 0 ? logf((float)onsets) : 0.f;
    float a3 = (float)(1000 * n0 + 150 * n3 + 8 * nother) / 1000.f;
    if (bad) a0 = a1 = a2 = a3 = __builtin_nanf("");
    float* __restrict__ o = out + (r0 + threadIdx.x) * kAttrColumns;
    o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
}

template <bool GRAD>
__global__ void __launch_bounds__(256)
attr_pair_kernel(const float* __restrict__ z, const float* __restrict__ attrs, long B, int Z, int A, AttrDims dims, float delta,
                 float gcoef, float* __restrict__ grad, AttrShare* __restrict__ ws, int nb) {
#pragma clang fp contract(off)                   // the value's arithmetic is the same instructions in both instantiations
    __shared__ float red[4];
    __shared__ int cred[3][4];
    __shared__ float gred[kAttrRows][4];
    const int t = threadIdx.x;
    const int a = blockIdx.y;
    const int dim = dims.d[a];
    const long i0 = (long)blockIdx.x * kAttrRows;
    const int nrows = (int)std::min<long>(kAttrRows, B - i0);
    float zr[kAttrRows], ar[kAttrRows], g[kAttrRows];
#pragma unroll
    for (int r = 0; r < kAttrRows; ++r) {
        const long i = std::min(i0 + r, B - 1);  // a row past B is read as the last one and never counted
        zr[r] = z[i * Z + dim];
        ar[r] = attrs[i * A + a];
        g[r] = 0.f;
    }
    float S = 0.f;
    int conc = 0, disc = 0, tied = 0;
    for (long j0 = 0; j0 < B; j0 += kAttrTile) {
        const long j = j0 + t;
        const bool col_ok = j < B;
        const float zc = col_ok ? z[j * Z + dim] : 0.f;
        const float ac = col_ok ? attrs[j * A + a] : 0.f;
        float v[kAttrRows];
#pragma unroll
        for (int r = 0; r < kAttrRows; ++r) {
            const bool ok = col_ok && r < nrows;
            const float dz = zr[r] - zc, da = ar[r] - ac;
            const bool up = da > 0.f, dn = da < 0.f;
            const float s = up ? 1.f : (dn ? -1.f : da);         // sgn; a NaN stays a NaN
            const float th = tanhf(delta * dz);
            const float w = th - s;
            v[r] = ok ? fabsf(w) : 0.f;
            if (GRAD) {
                const float sg = w > 0.f ? 1.f : (w < 0.f ? -1.f : w);
                g[r] += ok ? sg * fmaf(-th, th, 1.f) : 0.f;
            }
            const bool off = ok && i0 + r != j;
            const bool zu = dz > 0.f, zd = dz < 0.f;
            conc += off && ((up && zu) || (dn && zd));
            disc += off && ((up && zd) || (dn && zu));
            tied += off && !(up || dn);
        }
        S += (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) +
             (((v[8] + v[9]) + (v[10] + v[11])) + ((v[12] + v[13]) + (v[14] + v[15])));
    }
    // the workgroup's share: the xor tree over a wave's lanes, the four waves in order
    S = wave_sum(S);
    conc = wave_sum(conc);
    disc = wave_sum(disc);
    tied = wave_sum(tied);
    if (GRAD) {
#pragma unroll
        for (int r = 0; r < kAttrRows; ++r) g[r] = wave_sum(g[r]);
    }
    if ((t & 63) == 0) {
        red[t >> 6] = S;
        cred[0][t >> 6] = conc; cred[1][t >> 6] = disc; cred[2][t >> 6] = tied;
        if (GRAD) {
#pragma unroll
            for (int r = 0; r < kAttrRows; ++r) gred[r][t >> 6] = g[r];
        }
    }
    __syncthreads();
    if (t == 0) {
        AttrShare sh;
        sh.s = sum4(red);
        sh.conc = sum4(cred[0]);
        sh.disc = sum4(cred[1]);
        sh.tied = sum4(cred[2]);
        ws[(long)a * nb + blockIdx.x] = sh;
    }
    if (GRAD && t < nrows) grad[(i0 + t) * A + a] = gcoef * sum4(gred[t]);
}

// ONE workgroup, attribute after attribute: thread t adds the shares of row blocks t, t + 256, ... in ascending order, the xor tree
// adds a wave's lanes, the four waves are added in order; one thread forms L_a and the value in double and rounds each once.
__global__ void __launch_bounds__(kAttrFinishBlock)
attr_finish_kernel(const AttrShare* __restrict__ ws, int nb, int A, double inv_b2, double coeff, float* __restrict__ out,
                   long long* __restrict__ counts) {
    __shared__ float tot[4];
    __shared__ long long ctot[3][4];
    const int t = threadIdx.x;
    double total = 0.0;
    for (int a = 0; a < A; ++a) {
        float s = 0.f;
        long long c = 0, d = 0, e = 0;
        for (int g = t; g < nb; g += kAttrFinishBlock) {
            const AttrShare sh = ws[(long)a * nb + g];
            s += sh.s;
            c += sh.conc; d += sh.disc; e += sh.tied;
        }
        s = wave_sum(s);
        c = wave_sum(c);
        d = wave_sum(d);
        e = wave_sum(e);
        __syncthreads();                         // the previous attribute's totals have been read
        if ((t & 63) == 0) { tot[t >> 6] = s; ctot[0][t >> 6] = c; ctot[1][t >> 6] = d; ctot[2][t >> 6] = e; }
        __syncthreads();
        if (t == 0) {
            const float Sa = sum4(tot);
            total += (double)Sa;
            out[1 + a] = (float)((double)Sa * inv_b2);
            for (int k = 0; k < 3; ++k) counts[3 * a + k] = sum4(ctot[k]);
        }
    }
    if (t == 0) out[0] = (float)(coeff * (total * inv_b2));
}

inline long attr_blocks(long B) { return (B + kAttrRows - 1) / kAttrRows; }

}  // namespace

int attr_measure_launch(const long long* tokens, long B, int T, int V, int slur, int rest, int none, const int* midi, int midi_lo,
                        int midi_hi, float* out, hipStream_t s) {
    if (!tokens || !midi || !out || B < 1 || B > (1 << 24) || V < 1 || T < 6 || T > kAttrMaxT || T % 6 != 0) return -1;
    if (slur < -1 || slur >= V || rest < -1 || rest >= V || none < -1 || none >= V || midi_hi <= midi_lo) return -1;
    const long nblk = (B + kAttrMeasureRows - 1) / kAttrMeasureRows;
    ProfScope prof(PROF_HBM, 0.0, s, "measure_attrs", (double)B * (8.0 * T + 4.0 * kAttrColumns));
    hipLaunchKernelGGL(attr_measure_kernel, dim3((unsigned)nblk), dim3(256), 0, s, tokens, B, T, V, slur, rest, none, midi,
                       midi_hi - midi_lo, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

long attr_reg_ws_bytes(long B, int A) {
    if (B < 1 || A < 1 || A > kAttrMaxA) return -1;
    return attr_blocks(B) * A * (long)sizeof(AttrShare);
}

int attr_reg_launch(const float* z, long B, int Z, const AttrDims& dims, int A, const float* attrs, float delta, double coeff, float* out,
                    long long* counts, float* grad, void* ws, long ws_bytes, hipStream_t s) {
    const long need = attr_reg_ws_bytes(B, A);
    if (need < 0 || !ws || ws_bytes < need) return -1;
    const int nb = (int)attr_blocks(B);
    const double inv_b2 = 1.0 / ((double)B * (double)B);
    const float gcoef = (float)(2.0 * coeff * (double)delta * inv_b2);
    {
        ProfScope prof(PROF_HBM, 0.0, s, grad ? "attr_pair_grad" : "attr_pair", 4.0 * (double)B * A * (grad ? 3.0 : 2.0));
        if (grad)
            hipLaunchKernelGGL(attr_pair_kernel<true>, dim3(nb, A), dim3(256), 0, s, z, attrs, B, Z, A, dims, delta, gcoef, grad,
                               (AttrShare*)ws, nb);
        else
            hipLaunchKernelGGL(attr_pair_kernel<false>, dim3(nb, A), dim3(256), 0, s, z, attrs, B, Z, A, dims, delta, gcoef, grad,
                               (AttrShare*)ws, nb);
    }
    if (hipGetLastError() != hipSuccess) return -2;
    ProfScope prof(PROF_HBM, 0.0, s, "attr_finish", 16.0 * (double)nb * A + 4.0 + 28.0 * A);
    hipLaunchKernelGGL(attr_finish_kernel, dim3(1), dim3(kAttrFinishBlock), 0, s, (const AttrShare*)ws, nb, A, inv_b2, coeff, out, counts);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
