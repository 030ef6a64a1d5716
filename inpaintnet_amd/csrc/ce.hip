// The cross-entropy kernels.  ce_kernel: the plain one of the training step -- one wavefront per row, the loss and hit sums through one
// float atomic pair per workgroup.  Behind it the class-weighted, label-smoothed cross-entropy with an ignore index (DESIGN.md
// section 28; the definition is in ce.h), whose bits are pinned to ce_kernel's.  The wave and workgroup sums are reduce.h's.
// ce_count: a flat int64 target array -> counts[V], n_valid, n_bad in integer atomics (a workgroup's histogram in LDS while V fits,
//   one global add per class it met), then the workgroup whose ticket came last forms denom = sum_c w_c counts_c and W = sum_c w_c in
//   double, one thread, in class order: pure functions of the counts.  A target outside [0, V) that is not ignore_index never indexes
//   anything; it is counted in n_bad and sets the token status word.
// ce_w: ce_kernel's decomposition, one wavefront per row, grid-stride -- but the row is read ONCE and kept in registers (V <= 256: up
//   to four values per lane; beyond that it is re-read).  A lane adds its expf terms in ascending class order and the xor tree adds
//   the lanes, as ce_kernel does, so that without weights, smoothing and ignored rows dW and the hit count are ce_kernel's bits.
//   A wave adds its rows' terms in double; a workgroup's four waves are added in order and stored as one partial; the workgroup whose
//   ticket came last adds the partials in ascending order (one per thread, the xor tree, the four waves in order), in double, and
//   writes loss and accuracy.  No float atomic anywhere: the same inputs give the same bits, with or without dW.  The per-class
//   statistics are integer atomics (LDS histogram per workgroup while V fits); the confusion matrix global integer atomics.
#include <algorithm>
#include <cmath>
#include "common.h"
#include "ce.h"
#include "chain.h"
#include "prof.h"
#include "pw_launch.h"
#include "reduce.h"

namespace {

typedef unsigned long long ull;

// One wavefront per row of V logits.  loss_sum += out_scale * (lse - w[target]);
// correct += out_scale * (argmax_first(w) == target); dW = (softmax - onehot) * scale.
__global__ void ce_kernel(const float* __restrict__ W, long ld_w, int rows, int V,
                          const long long* __restrict__ tgt, float* __restrict__ dW, long ld_dw, float scale,
                          float out_scale, float* __restrict__ loss_sum, float* __restrict__ correct,
                          const float* __restrict__ scale_dev, const float* __restrict__ add_term, float add_scale,
                          float* __restrict__ fwd_out, float fwd_scale) {
    // scale_dev: dW is also multiplied by this device scalar (the upstream gradient of the mean loss, read on the device:
    // no elementwise pass over dW afterwards); add_term: *loss_sum also receives add_scale * add_term[0], once (the KL
    // term of the ELBO: loss = CE + beta/B * KL leaves this kernel complete)
    // fwd_out: receives fwd_scale * scale_dev[0] (the gradient handed on to the producer of add_term, e.g. the KL sum)
    if (scale_dev) {
        if (fwd_out && blockIdx.x == 0 && threadIdx.x == 0) *fwd_out = fwd_scale * *scale_dev;
        scale *= *scale_dev;
    }
    if (add_term && loss_sum && blockIdx.x == 0 && threadIdx.x == 0) unsafeAtomicAdd(loss_sum, add_scale * *add_term);
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    float lsum = 0.f, csum = 0.f;
    for (int row = wave; row < rows; row += nwaves) {
        const float* w = W + (long)row * ld_w;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, w[v]);
        m = wave_max(m);
        float se = 0.f;
        int am = kAmNone;
        for (int v = lane; v < V; v += 64) {
            const float x = w[v];
            se += expf(x - m);
            am = min(am, am_key(x, m, v));
        }
        se = wave_sum(se);
        am = am_index(wave_min(am));
        const int tg = (int)tgt[row];
        const float lse = m + logf(se);
        if (lane == 0) {
            lsum += lse - w[tg];
            csum += (am == tg) ? 1.f : 0.f;
        }
        if (dW) {
            float* d = dW + (long)row * ld_dw;
            const float inv = 1.f / se;
            for (int v = lane; v < V; v += 64) d[v] = (expf(w[v] - m) * inv - (v == tg ? 1.f : 0.f)) * scale;
        }
    }
    // lane 0 of every wave holds that wave's partials: combine the 4 waves of the block, one atomic pair per block
    __shared__ float part[2][4];
    if (lane == 0) { part[0][threadIdx.x >> 6] = lsum; part[1][threadIdx.x >> 6] = csum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (loss_sum) unsafeAtomicAdd(loss_sum, sum4(part[0]) * out_scale);
        if (correct) unsafeAtomicAdd(correct, sum4(part[1]) * out_scale);
    }
}

// Words another workgroup reads in the same launch: written through and read past this CU's L1 (agent scope).
__device__ __forceinline__ void ce_put(ull* p, ull v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ ull ce_get(const ull* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One lane, behind a workgroup barrier that every storing wave reached with its stores drained: publish this workgroup's stores and
// take a ticket.  True for the workgroup whose ticket is the last of `n`; it then sees every workgroup's stores.
__device__ __forceinline__ bool ce_last_ticket(ull* ticket, unsigned n) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const ull old = __hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old != (ull)(n - 1)) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return true;
}

__global__ void __launch_bounds__(256)
ce_count_kernel(const long long* __restrict__ tgt, long n, int V, const float* __restrict__ cw, int has_ignore, long long ignore,
                long long* __restrict__ out, unsigned* tok_word) {
    __shared__ int s_cnt[kCeLdsV];
    __shared__ double s_prod[256];
    __shared__ double s_w[256];
    __shared__ long long s_part[2][4];
    __shared__ int s_last;
    const int t = threadIdx.x;
    const bool lds = V <= kCeLdsV;
    ull* __restrict__ counts = reinterpret_cast<ull*>(out + kCeMetaWords);
    ull* meta = reinterpret_cast<ull*>(out);
    if (lds) {
        for (int i = t; i < V; i += 256) s_cnt[i] = 0;
        __syncthreads();
    }
    long long nvalid = 0, nbad = 0;
    for (long i = (long)blockIdx.x * 256 + t; i < n; i += (long)gridDim.x * 256) {
        const long long k = tgt[i];
        if (has_ignore && k == ignore) continue;
        if (k < 0 || k >= V) { ++nbad; continue; }
        ++nvalid;
        if (lds) atomicAdd(&s_cnt[(int)k], 1);
        else atomicAdd(counts + k, 1ull);
    }
    nvalid = wave_sum(nvalid);
    nbad = wave_sum(nbad);
    if ((t & 63) == 0) { s_part[0][t >> 6] = nvalid; s_part[1][t >> 6] = nbad; }
    __syncthreads();
    if (lds) {
        for (int i = t; i < V; i += 256) {
            const int c = s_cnt[i];
            if (c) atomicAdd(counts + i, (ull)c);
        }
    }
    if (t == 0) {
        const long long a = sum4(s_part[0]);
        const long long b = sum4(s_part[1]);
        if (a) atomicAdd(meta + kCeMetaValid, (ull)a);
        if (b) atomicAdd(meta + kCeMetaBad, (ull)b);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // every wave's adds have left before the ticket is taken
    __syncthreads();
    if (t == 0) s_last = ce_last_ticket(meta + kCeMetaCountTicket, gridDim.x) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    // the finishing workgroup: products into LDS 256 classes at a time, one thread adds them in class order
    double denom = 0.0, wsum = 0.0;
    for (int c0 = 0; c0 < V; c0 += 256) {
        const int c = c0 + t;
        if (c < V) {
            const double w = cw ? (double)cw[c] : 1.0;
            s_w[t] = w;
            s_prod[t] = w * (double)(long long)ce_get(counts + c);
        }
        __syncthreads();
        if (t == 0) {
            const int m = min(256, V - c0);
            for (int i = 0; i < m; ++i) { denom += s_prod[i]; wsum += s_w[i]; }
        }
        __syncthreads();
    }
    if (t == 0) {
        out[kCeMetaDenom] = __double_as_longlong(denom);
        out[kCeMetaWsum] = __double_as_longlong(wsum);
        if (tok_word && ce_get(meta + kCeMetaBad) != 0ull)
            __hip_atomic_fetch_add(tok_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

struct CePartial { ull a, b, hits; };            // doubles as bits: the weighted NLL sum, the smoothing sum; the hit count

// NV > 0: the row lives in registers, element v = lane + 64 k in slot k.  NV == 0: V > 256, the row is read again in every pass.
// f(v, x, k) for every element of the row this lane owns, in ascending v.
template <int NV, class F>
__device__ __forceinline__ void ce_each(const float (&x)[NV ? NV : 1], const float* __restrict__ w, int V, int lane, F f) {
    if constexpr (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int v = lane + 64 * k;
            if (v < V) f(v, x[k], k);
        }
    } else {
        for (int v = lane; v < V; v += 64) f(v, w[v], 0);
    }
}

// FULL: class weights or smoothing.  Without them the gradient is (p - onehot) * scale, ce_kernel's expression.
template <int NV, bool FULL>
__global__ void __launch_bounds__(256) ce_w_kernel(CeWArgs a) {
    __shared__ float s_cw[FULL ? kCeLdsV : 1];
    __shared__ int s_stats[3 * kCeLdsV];
    __shared__ double s_red[2][4];
    __shared__ long long s_hits[4];
    __shared__ int s_last;
    const int t = threadIdx.x, lane = t & 63;
    const int V = a.V;
    const bool sums = a.loss || a.acc || a.stats || a.conf;
    const bool cw_lds = FULL && a.cw && V <= kCeLdsV;
    const bool st_lds = a.stats && V <= kCeLdsV;
    const double denom = __longlong_as_double(a.meta[kCeMetaDenom]);
    float scale = denom == 0.0 ? 0.f : (float)(1.0 / denom);
    if (a.scale_dev) {
        if (a.fwd_out && blockIdx.x == 0 && t == 0) *a.fwd_out = a.fwd_scale * *a.scale_dev;
        scale *= *a.scale_dev;
    }
    const bool zero_grad = denom == 0.0;
    if (cw_lds)
        for (int i = t; i < V; i += 256) s_cw[i] = a.cw[i];
    if (st_lds)
        for (int i = t; i < 3 * V; i += 256) s_stats[i] = 0;
    if (cw_lds || st_lds) __syncthreads();
    const float c1 = (float)(1.0 - a.smooth), c2 = (float)(a.smooth / (double)V);
    const float wtot = FULL ? (float)__longlong_as_double(a.meta[kCeMetaWsum]) : 0.f;
    const bool smoothing = FULL && a.smooth > 0.0;
    auto cwv = [&](int c) -> float { return !FULL || !a.cw ? 1.f : (cw_lds ? s_cw[c] : a.cw[c]); };

    const int wave = (blockIdx.x * 256 + t) >> 6, nwaves = gridDim.x * 4;
    double accA = 0.0, accB = 0.0;
    long long hits = 0;
    for (int row = wave; row < a.rows; row += nwaves) {
        const long long tg64 = a.tgt[row];
        const bool valid = tg64 >= 0 && tg64 < V && !(a.has_ignore && tg64 == a.ignore);
        float* __restrict__ d = a.dW ? a.dW + (long)row * a.ld_dw : nullptr;
        if (!valid) {                            // an ignored row: nothing read, nothing counted, an exactly zero gradient
            if (d)
                for (int v = lane; v < V; v += 64) d[v] = 0.f;
            continue;
        }
        const int tg = (int)tg64;
        const float* __restrict__ w = a.W + (long)row * a.ld_w;
        float x[NV ? NV : 1], ex[NV ? NV : 1];
        if constexpr (NV > 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int v = lane + 64 * k;
                x[k] = v < V ? w[v] : -INFINITY;
            }
        }
        float m = -INFINITY;
        ce_each<NV>(x, w, V, lane, [&](int, float xv, int) { m = fmaxf(m, xv); });
        m = wave_max(m);
        float se = 0.f, xt = 0.f;
        int am = kAmNone;
        ce_each<NV>(x, w, V, lane, [&](int v, float xv, int k) {
            const float e = expf(xv - m);
            if constexpr (NV > 0) ex[k] = e;
            se += e;
            am = min(am, am_key(xv, m, v));
            xt = v == tg ? xv : xt;
        });
        se = wave_sum(se);
        am = am_index(wave_min(am));
        xt = __shfl(xt, tg & 63, 64);
        const float lse = m + logf(se);
        const float wt = cwv(tg);
        if (sums) {
            accA += (double)(wt * (lse - xt));
            if (smoothing) {
                float sm = 0.f;
                ce_each<NV>(x, w, V, lane, [&](int v, float xv, int) { sm += cwv(v) * (lse - xv); });
                accB += (double)wave_sum(sm);
            }
            hits += am == tg;
            if (lane == 0) {
                if (a.stats) {
                    if (st_lds) {
                        atomicAdd(&s_stats[3 * tg], 1);
                        if (am == tg) atomicAdd(&s_stats[3 * tg + 1], 1);
                        atomicAdd(&s_stats[3 * am + 2], 1);
                    } else {
                        ull* st = reinterpret_cast<ull*>(a.stats);
                        atomicAdd(st + 3l * tg, 1ull);
                        if (am == tg) atomicAdd(st + 3l * tg + 1, 1ull);
                        atomicAdd(st + 3l * am + 2, 1ull);
                    }
                }
                if (a.conf) atomicAdd(reinterpret_cast<ull*>(a.conf) + (long)tg * V + am, 1ull);
            }
        }
        if (d) {
            if (zero_grad) {
                for (int v = lane; v < V; v += 64) d[v] = 0.f;
            } else {
                const float inv = 1.f / se;
                ce_each<NV>(x, w, V, lane, [&](int v, float xv, int k) {
                    float e;
                    if constexpr (NV > 0) e = ex[k];
                    else e = expf(xv - m);
                    const float hot = v == tg ? 1.f : 0.f;
                    if constexpr (FULL) {
                        const float p = e * inv;
                        d[v] = (c1 * wt * (p - hot) + c2 * (wtot * p - cwv(v))) * scale;
                    } else {
                        d[v] = (e * inv - hot) * scale;
                    }
                });
            }
        }
    }
    if (!sums) return;                           // the gradient-only launch: no partials, no ticket

    if ((t & 63) == 0) { s_red[0][t >> 6] = accA; s_red[1][t >> 6] = accB; s_hits[t >> 6] = hits; }
    __syncthreads();
    if (st_lds) {
        ull* st = reinterpret_cast<ull*>(a.stats);
        for (int i = t; i < 3 * V; i += 256) {
            const int c = s_stats[i];
            if (c) atomicAdd(st + i, (ull)c);
        }
    }
    if (!a.loss && !a.acc) return;               // statistics alone need no finishing pass
    CePartial* __restrict__ part = static_cast<CePartial*>(a.ws);
    ull* ticket = reinterpret_cast<ull*>(a.meta) + kCeMetaLossTicket;
    if (t == 0) {
        CePartial* mine = part + blockIdx.x;
        ce_put(&mine->a, (ull)__double_as_longlong(sum4(s_red[0])));
        ce_put(&mine->b, (ull)__double_as_longlong(sum4(s_red[1])));
        ce_put(&mine->hits, (ull)sum4(s_hits));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = ce_last_ticket(ticket, gridDim.x) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    // the finishing workgroup: thread g holds workgroup g's partial (the grid has at most kCeMaxGrid <= 256 workgroups)
    double A = 0.0, B = 0.0;
    long long H = 0;
    if (t < (int)gridDim.x) {
        A = __longlong_as_double((long long)ce_get(&part[t].a));
        B = __longlong_as_double((long long)ce_get(&part[t].b));
        H = (long long)ce_get(&part[t].hits);
    }
    A = wave_sum(A);
    B = wave_sum(B);
    H = wave_sum(H);
    __syncthreads();                             // (s_red and s_hits have been read by thread 0)
    if ((t & 63) == 0) { s_red[0][t >> 6] = A; s_red[1][t >> 6] = B; s_hits[t >> 6] = H; }
    __syncthreads();
    if (t == 0) {
        A = sum4(s_red[0]);
        B = sum4(s_red[1]);
        H = sum4(s_hits);
        if (a.loss) {
            double l = denom == 0.0 ? (double)NAN : ((1.0 - a.smooth) * A + (a.smooth / (double)V) * B) / denom;
            if (a.add_term) l += (double)a.add_scale * (double)*a.add_term;
            *a.loss = (float)l;
        }
        if (a.acc) *a.acc = (float)((double)H / (double)a.meta[kCeMetaValid]);      // no valid row: 0 / 0 = NaN
        ce_put(ticket, 0ull);                    // the next launch on this block starts at 0 again
    }
}

inline int ce_grid(long n, int cap) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, cap)); }

template <int NV>
void ce_w_dispatch(const CeWArgs& a, int grid, bool full, hipStream_t s) {
    if (full) hipLaunchKernelGGL((ce_w_kernel<NV, true>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ce_w_kernel<NV, false>), dim3(grid), dim3(256), 0, s, a);
}

}  // namespace

int pw_cross_entropy(const float* W, long ld_w, int rows, int V, const long long* tgt, float* dW, long ld_dw,
                     float scale, float out_scale, float* loss_sum, float* correct, hipStream_t s, const float* scale_dev,
                     const float* add_term, float add_scale, float* fwd_out, float fwd_scale) {
    // blocks: every block ends with one atomic pair on the same two words, and those serialise (~20 ns each): 2048 blocks (one row
    // per wave) measured 77 us for the loss glue of the B = 256 step, 512 blocks 54 us with the forward launch at 18.7 us against
    // 6.2 for the backward launch that has no sums (profiles/r06_p_timeline_full_step.txt).  With sums: 128 blocks (12 rows per
    // wave at 6144 rows); without (the backward launch): as many as there are rows to go round
    const int g = grid_for((long)rows * 64, 256, (loss_sum || correct) ? 128 : 512);
    hipLaunchKernelGGL(ce_kernel, dim3(g), dim3(256), 0, s, W, ld_w, rows, V, tgt, dW, ld_dw, scale, out_scale, loss_sum,
                       correct, scale_dev, add_term, add_scale, fwd_out, fwd_scale);
    return ok();
}

int ce_count_launch(const long long* tgt, long n, int V, const float* cw, int has_ignore, long long ignore, long long* out, long extra,
                    hipStream_t s) {
    if (!tgt || !out || n < 1 || n > (1l << 40) || V < 1 || extra < 0 || extra > (1l << 40)) return -1;
    if (hipMemsetAsync(out, 0, sizeof(long long) * (size_t)(kCeMetaWords + V + extra), s) != hipSuccess) return -2;
    ProfScope prof(PROF_HBM, 0.0, s, "class_counts", 8.0 * (double)n + 8.0 * V);
    hipLaunchKernelGGL(ce_count_kernel, dim3(ce_grid(n, 64)), dim3(256), 0, s, tgt, n, V, cw, has_ignore, ignore, out, token_host_status());
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

long ce_w_ws_bytes(int rows) { return rows < 1 ? -1 : (long)ce_grid((long)rows * 64, kCeMaxGrid) * (long)sizeof(CePartial); }

int ce_w_launch(const CeWArgs& a, hipStream_t s) {
    const bool sums = a.loss || a.acc || a.stats || a.conf;
    if (!a.W || !a.tgt || !a.meta || a.rows < 1 || a.V < 1 || a.V >= kAmEq || (!a.dW && !sums)) return -1;
    if (a.ld_w < a.V || (a.dW && a.ld_dw < a.V) || (a.fwd_out && !a.scale_dev) || (a.add_term && !a.loss)) return -1;
    if (!(a.smooth >= 0.0 && a.smooth <= 1.0) || ((a.loss || a.acc) && !a.ws)) return -1;
    // with sums every workgroup ends in a ticket and the finishing workgroup reads one partial per thread: few workgroups, several
    // rows a wave; the gradient-only launch has as many as there are rows to go round (pw_cross_entropy's two grids)
    const int grid = ce_grid((long)a.rows * 64, sums ? kCeMaxGrid : 512);
    const bool full = a.cw || a.smooth > 0.0;
    ProfScope prof(PROF_HBM, 0.0, s, sums ? "cross_entropy_w" : "cross_entropy_w_grad",
                   4.0 * (double)a.rows * a.V * (a.dW ? 2.0 : 1.0) + 8.0 * a.rows);
    if (a.V <= 64) ce_w_dispatch<1>(a, grid, full, s);
    else if (a.V <= 128) ce_w_dispatch<2>(a, grid, full, s);
    else if (a.V <= 256) ce_w_dispatch<4>(a, grid, full, s);
    else ce_w_dispatch<0>(a, grid, full, s);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
