// HBM-bound layout, gather and small helper kernels of the hot path: transposes and the fragment-major packing, column sums
// (bias gradients), one-hot expansion / token segment sums / table gradients (embedding gradients without contended atomics),
// the prologue launch, fills, copies and scales, argmax with the lowest-index tie rule, embedding, the measure split.  All are
// grid-stride and coalesced along the contiguous dimension; the 64-lane wave reductions are reduce.h's xor butterflies.
// The cross-entropy lives in ce.hip, KL / reparameterisation / free bits in latent.hip, the optimizer step in optim.hip, the
// sampling row kernels and the dropout mask in sample_rows.hip.
#include <algorithm>
#include "common.h"
#include "pointwise.h"
#include "chain.h"
#include "pw_launch.h"
#include "reduce.h"

namespace {

// out[c*ld_out + r] = in[r*ld_in + c]
__global__ void transpose_kernel(const float* __restrict__ in, long ld_in, float* __restrict__ out, long ld_out,
                                 int rows, int cols) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? in[(long)r * ld_in + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (r < rows && c < cols) out[(long)c * ld_out + r] = tile[tx][i];
    }
}

// Row-major -> fragment-major (ksplit.h): out[row/16][k/16][lane = ((k%16)/4)*16 + row%16][k%4] = Y(row, k) where
// Y(row,k) = in[row*ld + k] (transposed = 0) or in[k*ld + row] (transposed = 1).  Rows R..ceil16(R) are zero-filled.
// One thread per 16-byte lane slot; blockIdx.y = batch entry.
__global__ void pack_frag_kernel(const float* __restrict__ in, long ld, int R, int K, float* __restrict__ out,
                                 int transposed, long in_bstride, long out_bstride) {
    const int S = K >> 4;
    const long slots = (long)((R + 15) >> 4) * S * 64;
    in += blockIdx.y * in_bstride;
    out += blockIdx.y * out_bstride;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const long blk = i >> 6;
        const int sb = (int)(blk % S), rb = (int)(blk / S);
        const int row = 16 * rb + (lane & 15), k = 16 * sb + 4 * (lane >> 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < R) {
            if (!transposed) {
                const float* q = in + (long)row * ld + k;
                v = make_float4(q[0], q[1], q[2], q[3]);
            } else {
                const float* q = in + (long)k * ld + row;
                v = make_float4(q[0], q[ld], q[2 * ld], q[3 * ld]);
            }
        }
        *reinterpret_cast<float4*>(out + 4 * i) = v;
    }
}

// Up to 8 same-shaped matrices in one launch (the recurrent weights of a module): blockIdx.y = matrix.
struct PackList { const float* in[8]; float* out[8]; };
__global__ void pack_frag_multi_kernel(PackList pl, long ld, int R, int K, int transposed) {
    const int S = K >> 4;
    const long slots = (long)((R + 15) >> 4) * S * 64;
    const float* __restrict__ in = pl.in[blockIdx.y];
    float* __restrict__ out = pl.out[blockIdx.y];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const long blk = i >> 6;
        const int sb = (int)(blk % S), rb = (int)(blk / S);
        const int row = 16 * rb + (lane & 15), k = 16 * sb + 4 * (lane >> 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < R) {
            if (!transposed) {
                const float* q = in + (long)row * ld + k;
                v = make_float4(q[0], q[1], q[2], q[3]);
            } else {
                const float* q = in + (long)k * ld + row;
                v = make_float4(q[0], q[ld], q[2 * ld], q[3 * ld]);
            }
        }
        *reinterpret_cast<float4*>(out + 4 * i) = v;
    }
}

// out[n] (+)= sum_m X[m*ld + n].  Block = 64 columns x 4 row-lanes; grid.y splits rows; atomics combine.
__global__ void colsum_kernel(const float* __restrict__ X, long ld, int M, int N, float* __restrict__ out) {
    __shared__ float part[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const int rows_per = (M + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    float s = 0.f;
    if (c < N)
        for (int r = r0 + rl; r < r1; r += 4) s += X[(long)r * ld + c];
    part[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0 && c < N) {
        s = sum4(part, threadIdx.x);
        unsafeAtomicAdd(out + c, s);
    }
}

// several column sums in one launch: blockIdx.z picks the job (blocks outside its extent leave at once)
struct ColsumList { int n; PwColsumJob j[8]; };
__global__ void colsum_multi_kernel(ColsumList L) {
    __shared__ float part[4][64];
    const PwColsumJob& J = L.j[blockIdx.z];
    const int M = J.M, N = J.N;
    if ((int)blockIdx.x * 64 >= N) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const int rows_per = (M + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    if (r0 >= M) return;
    float s = 0.f;
    if (c < N)
        for (int r = r0 + rl; r < r1; r += 4) s += J.X[(long)r * J.ld + c];
    part[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0 && c < N) {
        s = sum4(part, threadIdx.x);
        unsafeAtomicAdd(J.out + c, s);
    }
}

// onehot[row, idx[(row/inner)*s_outer + (row%inner)*s_inner]] = 1 on a zeroed [rows, W] buffer
__global__ void onehot_kernel(const long long* __restrict__ idx, int inner, long s_outer, long s_inner, int rows, int W,
                              float* __restrict__ out) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const long long v = idx[(long)(r / inner) * s_outer + (long)(r % inner) * s_inner];
        if (v >= 0 && v < W) out[(long)r * W + v] = 1.f;
    }
}

// Gradient of a gather table: out[v][c] += sum over rows r with tok(r) == v of X[r][c]   (out [W][ncols], zeroed by the
// caller).  Row r = (r / inner, r % inner) has token idx[(r/inner)*s_outer + (r%inner)*s_inner].  The one-hot product this
// replaces read X through the MFMA path; this is one pass over X at HBM rate: a workgroup owns 256 columns x `rows_per`
// rows, a thread owns one column of the LDS table [W+1][256] (plain read-add-write: nobody else touches its slots; LDS
// float atomics measured 200 cycles per wave -- 116 us for the encoder's 75 MB; row W takes out-of-range tokens) and the
// table is flushed with one global atomic per non-zero slot.  Loads go 16 rows deep before the first add.
constexpr int kSegMaxW = 128, kSegDepth = 16;        // (W + 1) KB of LDS per workgroup: 129 KB of the CU's 160
// CW columns per workgroup, 256 / CW row groups with a table each (narrow inputs -- embedding gradients with E = 20..30
// columns -- keep all 256 lanes busy); optional per-row factor (the Dropout2d scale of an embedded sequence).
template <int CW>
__global__ __launch_bounds__(256) void token_segsum_kernel(
    const float* __restrict__ X, long ld, const long long* __restrict__ idx, int inner, long s_outer, long s_inner, int rows,
    int rows_per, int W, int ncols, float* __restrict__ out, const float* __restrict__ row_scale) {
    constexpr int RG = 256 / CW;
    extern __shared__ float tab[];                            // [RG][W + 1][CW]
    const int c = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int col = blockIdx.x * CW + c;
    float* const mine = tab + rg * (W + 1) * CW + c;
    for (int v = 0; v <= W; ++v) mine[v * CW] = 0.f;
    const int r0 = blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
    const int colc = min(col, ncols - 1);
    for (int rb = r0 + rg; rb < r1; rb += RG * kSegDepth) {
        int v[kSegDepth];
        float x[kSegDepth];
#pragma unroll
        for (int k = 0; k < kSegDepth; ++k) {
            const int r = min(rb + k * RG, rows - 1);
            const long long t = idx[(long)(r / inner) * s_outer + (long)(r % inner) * s_inner];
            v[k] = rb + k * RG < r1 && t >= 0 && t < W ? (int)t : W;
            x[k] = X[(long)r * ld + colc];
            if (row_scale) x[k] *= row_scale[r];
        }
#pragma unroll
        for (int k = 0; k < kSegDepth; ++k) mine[v[k] * CW] += x[k];
    }
    if (col < ncols)
        for (int v = 0; v < W; ++v) {
            const float x = mine[v * CW];
            if (x != 0.f) unsafeAtomicAdd(out + (long)v * ncols + col, x);
        }
}

// The two small products behind a gather table of input-side gate gradients dtab [W][ndir*N3] (ld = ndir*N3), E <= 16:
//   dW[d][j][e] (ld ldw) += sum_v dtab[v][d*N3 + j] * emb[v][e]          (blocks 0 .. nblk_a-1: a thread per (d, j, e))
//   demb[v][e]           += sum_d sum_j dtab[v][d*N3 + j] * Wih[d][j][e]  (then a block per (table row v, 512 columns))
struct TableGradArgs {
    const float* dtab; int W, N3, ndir, E;
    const float* emb; long ld_emb;                            // [W][E]
    const float* emb_last; float* demb_last;                  // optional: row W-1 of emb / demb lives elsewhere (the decoder's
                                                              // start symbol x_0 behind its V embedding rows)
    const float* Wih[2]; float* dW[2]; long ldw;              // [N3][E] (row stride ldw)
    float* demb; long ld_demb;                                // [W][E], accumulated (or null)
    int nblk_a, chunks;
};
__global__ __launch_bounds__(256) void table_grad_kernel(TableGradArgs a) {
    const int ncols = a.ndir * a.N3;
    __shared__ float sh[kSegMaxW * 16];
    if ((int)blockIdx.x < a.nblk_a) {
        for (int i = threadIdx.x; i < a.W * a.E; i += 256) {
            const int v = i / a.E, e = i % a.E;
            sh[i] = (v == a.W - 1 && a.emb_last) ? a.emb_last[e] : a.emb[(long)v * a.ld_emb + e];
        }
        __syncthreads();
        const int o = blockIdx.x * 256 + threadIdx.x;         // (col, e), e fastest
        if (o >= ncols * a.E) return;
        const int col = o / a.E, e = o - col * a.E;
        float acc = 0.f;
#pragma unroll 8
        for (int v = 0; v < a.W; ++v) acc += a.dtab[(long)v * ncols + col] * sh[v * a.E + e];
        const int d = col / a.N3, j = col - d * a.N3;
        a.dW[d][(long)j * a.ldw + e] += acc;
        return;
    }
    const int bb = blockIdx.x - a.nblk_a, v = bb / a.chunks, ch = bb - v * a.chunks;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int col = ch * 512 + threadIdx.x; col < min(ncols, (ch + 1) * 512); col += 256) {
        const int d = col / a.N3, j = col - d * a.N3;
        const float t = a.dtab[(long)v * ncols + col];
        const float* wr = a.Wih[d] + (long)j * a.ldw;
#pragma unroll
        for (int e = 0; e < 16; ++e) if (e < a.E) acc[e] += t * wr[e];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        float x = acc[e];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
        if (lane == 0) sh[wv * 16 + e] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.E) {
        float* dst = (v == a.W - 1 && a.demb_last) ? a.demb_last : a.demb + (long)v * a.ld_demb;
        unsafeAtomicAdd(dst + threadIdx.x, sh[threadIdx.x] + sh[16 + threadIdx.x] + sh[32 + threadIdx.x] + sh[48 + threadIdx.x]);
    }
}

// pw_prologue (pointwise.h): blockIdx.y picks the job, blockIdx.x strides over it
__global__ void prologue_kernel(PwPrologue a) {
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x, step = (long)gridDim.x * blockDim.x;
    const int job = blockIdx.y;
    if (job < 4) {
        if (job >= a.ntab) return;
        const PwTableJob& t = a.tab[job];
        const long n = (long)t.rows * t.N;
        for (long i = i0; i < n; i += step) {
            const int r = (int)(i / t.N), c = (int)(i - (long)r * t.N);
            const float* e = t.emb + r * t.ld_emb;
            const float* w = t.W + c * t.ldw;
            float acc = t.bias ? t.bias[c] : 0.f;
            for (int k = 0; k < t.E; ++k) acc = fmaf(e[k], w[k], acc);
            t.out[r * t.ld_out + c] = acc;
        }
    } else if (job == 4) {
        for (long i = i0; i < a.nzero; i += step) a.zero_words[i] = 0u;
        for (long i = i0; i < a.ncopy; i += step) a.copy_dst[i] = a.copy_src[i];
    } else if (job == 5) {
        if (a.axpb_n > 0) {
            const float av = *a.axpb_a;
            for (long i = i0; i < a.axpb_n; i += step) a.axpb_y[i] = av * a.axpb_x[i * a.axpb_incx] + a.axpb_b[i];
        }
        for (long i = i0; i < a.nfill; i += step) a.fill_ptr[i] = a.fill_val;
    } else {
        if (!a.tok_src) return;
        const long n = (long)a.tok_B * a.tok_T;
        bool bad = false;
        for (long i = i0; i < n; i += step) {
            const long long v = a.tok_src[i];
            bad |= a.tok_V > 0 && (v < 0 || v >= a.tok_V);
            if (a.tok_copy) a.tok_copy[i] = v;
            if (a.tok_shift) a.tok_shift[i] = (i % a.tok_T) == 0 ? a.tok_first : a.tok_src[i - 1];
        }
        if (bad && a.tok_bad) __hip_atomic_fetch_add(a.tok_bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}


__global__ void shift_tokens_kernel(const long long* __restrict__ target, int B, int T, long long first,
                                    long long* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * T; i += gridDim.x * blockDim.x)
        out[i] = i % T == 0 ? first : target[i - 1];
}

// x *= m      or      x *= selu'(a)  (a = SELU output)
__global__ void mul_kernel(float* __restrict__ x, const float* __restrict__ m, long n, int selu_grad) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        x[i] *= selu_grad ? selu_grad_from_out(m[i]) : m[i];
}

// in [A][B][K] -> out [B][A][K]
__global__ void swap01_kernel(const float* __restrict__ in, int A, int B, int K, float* __restrict__ out) {
    const long n = (long)A * B * K;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const long ab = i / K;
        const int b = (int)(ab % B), a = (int)(ab / B);
        out[((long)b * A + a) * K + k] = in[i];
    }
}

// samples[b*stride] = argmax_first(W[b,:]); one wavefront per row
__global__ void argmax_kernel(const float* __restrict__ W, long ld_w, int rows, int V, long long* __restrict__ out,
                              long stride) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int row = wave; row < rows; row += nwaves) {
        const float* w = W + (long)row * ld_w;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, w[v]);
        m = wave_max(m);
        int am = kAmNone;
        for (int v = lane; v < V; v += 64) am = min(am, am_key(w[v], m, v));
        am = am_index(wave_min(am));
        if (lane == 0) out[(long)row * stride] = am;
    }
}

// p[r*ld + c] = 0  (plain kernels instead of hipMemsetAsync / hipMemcpyAsync: the runtime's blit path showed 20-40 us
// bubbles around its fill/copy kernels in the step's timeline)
__global__ void zero2d_kernel(float* __restrict__ p, long ld, long rows, int cols) {
    const long n = rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        p[(i / cols) * ld + (i % cols)] = 0.f;
}
__global__ void copy_words_kernel(unsigned* __restrict__ dst, const unsigned* __restrict__ src, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = src[i];
}

__global__ void fill_i64_kernel(long long* p, long n, long long v) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

// dst[r*ld_d + c] = src[r*ld_s + c] * (mask ? (mask[r*ld_m + c] > 0) : 1)   (generic strided 2D copy)
__global__ void copy2d_kernel(float* __restrict__ dst, long ld_d, const float* __restrict__ src, long ld_s,
                              const float* __restrict__ pos, long ld_p, int rows, int cols) {
    const long n = (long)rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / cols), c = (int)(i % cols);
        float v = src[(long)r * ld_s + c];
        if (pos && !(pos[(long)r * ld_p + c] > 0.f)) v = 0.f;
        dst[(long)r * ld_d + c] = v;
    }
}

// [B,T,V] batch-first d(post-ReLU logits) -> [T,B,V] time-major d(pre-ReLU logits)
__global__ void dlogits_relayout_kernel(const float* __restrict__ dW, const float* __restrict__ Wt, int B, int T, int V,
                                        float* __restrict__ out) {
    const long n = (long)B * T * V;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int v = (int)(i % V);
        const long bt = i / V;
        const int tt = (int)(bt % T), b = (int)(bt / T);
        const float g = Wt[i] > 0.f ? dW[i] : 0.f;
        out[((long)tt * B + b) * V + v] = g;
    }
}

// out[g][b][c] = sum_{j<G} in[(g*G + j)][b][c]   (sum the ticks of each beat)
__global__ void group_sum_kernel(const float* __restrict__ in, int groups, int G, long inner, float* __restrict__ out) {
    const long n = (long)groups * inner;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long g = i / inner, r = i % inner;
        float s = 0.f;
        for (int j = 0; j < G; ++j) s += in[((long)g * G + j) * inner + r];
        out[i] = s;
    }
}

// y[i] = a * x[i*incx] + (b ? b[i] : 0)
__global__ void axpb_kernel(const float* a_ptr, const float* __restrict__ x, long incx, const float* __restrict__ b,
                            float* __restrict__ y, int n) {
    const float a = *a_ptr;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        y[i] = a * x[(long)i * incx] + (b ? b[i] : 0.f);
}

// Beat-RNN layer-0 input gradients: gi = b0 * w + b_ih  =>  dw[i*incw] += b0 * s[i]  (s = column sums of dgi);
// db0 = sum_rows sum_i dgi[row][i] * w[i*incw] is a ~1.5 M-term sum of both signs that nearly cancels: per-wave atomics in
// launch order moved it by up to 2e-4 of itself between runs (round 3's parity tests gave this one scalar its own bound).
// Now a fixed-order two-stage sum: kB0Parts blocks each reduce their rows in a fixed order into partial[block]
// (rowdot_partials_kernel), and one thread adds the partials in index order (here): bit-identical from run to run.
constexpr int kB0Parts = 64;
__global__ __launch_bounds__(256) void rowdot_partials_kernel(const float* __restrict__ X, long ld, int M, int N,
                                                              const float* __restrict__ w, long incw, float* __restrict__ partial) {
    __shared__ float red[256];
    const int per = (M + kB0Parts - 1) / kB0Parts, r0 = blockIdx.x * per, r1 = min(M, r0 + per);
    float acc = 0.f;
    for (int c = threadIdx.x; c < N; c += 256) {
        const float wc = w[(long)c * incw];
        float col = 0.f;
        for (int r = r0; r < r1; ++r) col += X[(long)r * ld + c];
        acc = fmaf(col, wc, acc);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void beat_input_grad_kernel(const float* __restrict__ s, const float* __restrict__ w, long incw,
                                       const float* b0, float* __restrict__ dw, float* __restrict__ db0, int n,
                                       const float* __restrict__ partial) {
    const float bb = *b0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        dw[(long)i * incw] += bb * s[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < kB0Parts; ++k) t += partial[k];
        *db0 += t;                                  // the only writer of this element in a backward call
    }
}

__global__ void scale_kernel(float* __restrict__ x, long n, float a) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] *= a;
}

// out[r, :] = table[idx[r], :]
__global__ void embedding_fwd_kernel(const float* __restrict__ table, const long long* __restrict__ idx, long rows, int E,
                                     float* __restrict__ out, const float* __restrict__ row_scale) {
    const long n = rows * E;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / E; const int e = (int)(i % E);
        out[i] = table[idx[r] * E + e] * (row_scale ? row_scale[r] : 1.f);
    }
}
// dtable[idx[r], :] += dout[r, :]
__global__ void embedding_bwd_kernel(const float* __restrict__ dout, const long long* __restrict__ idx, long rows, int E,
                                     float* __restrict__ dtable, const float* __restrict__ row_scale) {
    const long n = rows * E;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / E; const int e = (int)(i % E);
        const float sc = row_scale ? row_scale[r] : 1.f;
        if (sc != 0.f) unsafeAtomicAdd(dtable + idx[r] * E + e, dout[i] * sc);
    }
}

// Input feed: the dataset tensors are int32 (folk_dataset.py:852-861); the model wants int64 (utils/helpers.py:17-26).
// The H2D copy moves the 4-byte form, the widening happens here.
__global__ void tokens_i32_to_i64_kernel(const int* __restrict__ src, long long* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = src[i];
}
// score [B, M*L] int32 -> past [B, np, L], target [B, nt, L], future [B, M-np-nt, L] int64, each contiguous
// (LatentRNNTrainer.split_score, latent_rnn_trainer.py:134-160): one pass, every token read once and written once.
__global__ void split_measures_kernel(const int* __restrict__ score, int B, int M, int L, int n_past, int n_target,
                                      long long* __restrict__ past, long long* __restrict__ target,
                                      long long* __restrict__ future) {
    const long n = (long)B * M * L;
    const int n_future = M - n_past - n_target;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int l = (int)(i % L);
        const int m = (int)((i / L) % M);
        const long b = i / ((long)L * M);
        const long long v = score[i];
        if (m < n_past) past[(b * n_past + m) * L + l] = v;
        else if (m < n_past + n_target) target[(b * n_target + (m - n_past)) * L + l] = v;
        else future[(b * n_future + (m - n_past - n_target)) * L + l] = v;
    }
}

}  // namespace

int pw_transpose(const float* in, long ld_in, float* out, long ld_out, int rows, int cols, hipStream_t s) {
    dim3 grid((cols + 31) / 32, (rows + 31) / 32);
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, s, in, ld_in, out, ld_out, rows, cols);
    return ok();
}
int pw_pack_frag(const float* in, long ld, int R, int K, float* out, int transposed, int nbatch, long in_bstride,
                 long out_bstride, hipStream_t s) {
    if (K % 16 != 0 || R <= 0 || nbatch <= 0) return -1;
    const long slots = (long)((R + 15) / 16) * (K / 16) * 64;
    dim3 grid(grid_for(slots, 256, 1024), nbatch);
    hipLaunchKernelGGL(pack_frag_kernel, grid, dim3(256), 0, s, in, ld, R, K, out, transposed, in_bstride, out_bstride);
    return ok();
}
int pw_pack_frag_multi(const float* const* ins, float* const* outs, int n, long ld, int R, int K, int transposed,
                       hipStream_t s) {
    if (K % 16 != 0 || R <= 0 || n <= 0 || n > 8) return -1;
    PackList pl{};
    for (int i = 0; i < n; ++i) { pl.in[i] = ins[i]; pl.out[i] = outs[i]; }
    const long slots = (long)((R + 15) / 16) * (K / 16) * 64;
    dim3 grid(grid_for(slots, 256, 1024), n);
    hipLaunchKernelGGL(pack_frag_multi_kernel, grid, dim3(256), 0, s, pl, ld, R, K, transposed);
    return ok();
}
int pw_colsum(const float* X, long ld, int M, int N, float* out, hipStream_t s) {
    int gy = (M + 255) / 256;
    if (gy > 64) gy = 64;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64, gy), dim3(256), 0, s, X, ld, M, N, out);
    return ok();
}
int pw_colsum_multi(const PwColsumJob* jobs, int n, hipStream_t s) {
    if (n <= 0) return 0;
    if (n > 8) return -1;
    ColsumList L{};
    L.n = n;
    int maxN = 0, maxM = 0;
    for (int i = 0; i < n; ++i) {
        L.j[i] = jobs[i];
        if (jobs[i].N > maxN) maxN = jobs[i].N;
        if (jobs[i].M > maxM) maxM = jobs[i].M;
    }
    int gy = (maxM + 255) / 256;
    if (gy > 64) gy = 64;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(colsum_multi_kernel, dim3((maxN + 63) / 64, gy, n), dim3(256), 0, s, L);
    return ok();
}
int pw_onehot(const long long* idx, int inner, long s_outer, long s_inner, int rows, int W, float* out, int zero_first,
              hipStream_t s) {
    if (zero_first && pw_zero(out, (long)rows * W, s) != 0) return -2;
    hipLaunchKernelGGL(onehot_kernel, dim3(grid_for(rows)), dim3(256), 0, s, idx, inner, s_outer, s_inner, rows, W, out);
    return ok();
}
int pw_token_segsum(const float* X, long ld, const long long* idx, int inner, long s_outer, long s_inner, int rows, int W,
                    int ncols, float* out, hipStream_t s, const float* row_scale, int zero_first) {
    if (W > kSegMaxW) return -1;
    if (zero_first && pw_zero(out, (long)W * ncols, s) != 0) return -2;
    const int cw = ncols <= 32 ? 32 : (ncols <= 64 ? 64 : 256), rg = 256 / cw;
    const int col_blocks = (ncols + cw - 1) / cw;
    int row_blocks = 1;                                       // >= 384 workgroups (1.5 per CU, 3 fit), at least 64 rows per row group
    while (col_blocks * row_blocks < 384 && rows / (row_blocks * 2) >= 64 * rg) row_blocks *= 2;
    const int rows_per = (rows + row_blocks - 1) / row_blocks;
    const dim3 grid(col_blocks, row_blocks);
    const size_t lds = (size_t)(W + 1) * 256 * sizeof(float);
#define DISPATCH_SEG(C)                                                                                                        \
    do {                                                                                                                   \
        static bool attr = false;                              /* more than 64 KB of dynamic LDS needs the opt-in */        \
        if (!attr) {                                                                                                       \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&token_segsum_kernel<C>),                               \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                             \
            attr = true;                                                                                                   \
        }                                                                                                                  \
        hipLaunchKernelGGL(token_segsum_kernel<C>, grid, dim3(256), lds, s, X, ld, idx, inner, s_outer, s_inner, rows,     \
                           rows_per, W, ncols, out, row_scale);                                                            \
    } while (0)
    if (cw == 32) DISPATCH_SEG(32); else if (cw == 64) DISPATCH_SEG(64); else DISPATCH_SEG(256);
#undef DISPATCH_SEG
    return ok();
}
int pw_table_grad(const float* dtab, int W, int N3, int ndir, int E, const float* emb, long ld_emb, const float* const* Wih,
                  float* const* dW, long ldw, float* demb, long ld_demb, hipStream_t s, const float* emb_last,
                  float* demb_last) {
    if (E > 16 || W > kSegMaxW || ndir < 1 || ndir > 2) return -1;
    TableGradArgs a{};
    a.emb_last = emb_last; a.demb_last = demb_last;
    a.dtab = dtab; a.W = W; a.N3 = N3; a.ndir = ndir; a.E = E; a.emb = emb; a.ld_emb = ld_emb; a.ldw = ldw;
    for (int d = 0; d < ndir; ++d) { a.Wih[d] = Wih[d]; a.dW[d] = dW[d]; }
    a.demb = demb; a.ld_demb = ld_demb;
    a.nblk_a = (ndir * N3 * E + 255) / 256; a.chunks = (ndir * N3 + 511) / 512;
    hipLaunchKernelGGL(table_grad_kernel, dim3(a.nblk_a + (demb ? W * a.chunks : 0)), dim3(256), 0, s, a);
    return ok();
}
int pw_shift_tokens(const long long* target, int B, int T, long long first, long long* out, hipStream_t s) {
    hipLaunchKernelGGL(shift_tokens_kernel, dim3(grid_for((long)B * T)), dim3(256), 0, s, target, B, T, first, out);
    return ok();
}
int pw_mul(float* x, const float* m, long n, int selu_grad, hipStream_t s) {
    hipLaunchKernelGGL(mul_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, m, n, selu_grad);
    return ok();
}
int pw_swap01(const float* in, int A, int B, int K, float* out, hipStream_t s) {
    hipLaunchKernelGGL(swap01_kernel, dim3(grid_for((long)A * B * K)), dim3(256), 0, s, in, A, B, K, out);
    return ok();
}
int pw_argmax(const float* W, long ld_w, int rows, int V, long long* out, long stride, hipStream_t s) {
    hipLaunchKernelGGL(argmax_kernel, dim3(grid_for((long)rows * 64, 256, 1024)), dim3(256), 0, s, W, ld_w, rows, V, out, stride);
    return ok();
}
int pw_zero2d(float* p, long ld, long rows, int cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(zero2d_kernel, dim3(grid_for(rows * cols)), dim3(256), 0, s, p, ld, rows, cols);
    return ok();
}
int pw_zero(float* p, long n, hipStream_t s) { return pw_zero2d(p, n, 1, (int)n, s); }
int pw_copy_bytes(void* dst, const void* src, long nbytes, hipStream_t s) {
    if (nbytes <= 0) return 0;
    if (nbytes % 4 != 0) return -1;
    hipLaunchKernelGGL(copy_words_kernel, dim3(grid_for(nbytes / 4)), dim3(256), 0, s, (unsigned*)dst, (const unsigned*)src,
                       nbytes / 4);
    return ok();
}
int pw_fill_i64(long long* p, long n, long long v, hipStream_t s) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, n, v);
    return ok();
}
int pw_copy2d(float* dst, long ld_d, const float* src, long ld_s, const float* pos, long ld_p, int rows, int cols,
              hipStream_t s) {
    hipLaunchKernelGGL(copy2d_kernel, dim3(grid_for((long)rows * cols)), dim3(256), 0, s, dst, ld_d, src, ld_s, pos, ld_p, rows, cols);
    return ok();
}
int pw_dlogits_relayout(const float* dW, const float* Wt, int B, int T, int V, float* out, hipStream_t s) {
    hipLaunchKernelGGL(dlogits_relayout_kernel, dim3(grid_for((long)B * T * V)), dim3(256), 0, s, dW, Wt, B, T, V, out);
    return ok();
}
int pw_group_sum(const float* in, int groups, int G, long inner, float* out, hipStream_t s) {
    hipLaunchKernelGGL(group_sum_kernel, dim3(grid_for((long)groups * inner)), dim3(256), 0, s, in, groups, G, inner, out);
    return ok();
}
int pw_axpb(const float* a, const float* x, long incx, const float* b, float* y, int n, hipStream_t s) {
    hipLaunchKernelGGL(axpb_kernel, dim3(grid_for(n)), dim3(256), 0, s, a, x, incx, b, y, n);
    return ok();
}
int pw_beat_input_grad(const float* sv, const float* w, long incw, const float* b0, float* dw, float* db0, int n,
                       const float* X, long ld, int M, float* partial, hipStream_t s) {
    hipLaunchKernelGGL(rowdot_partials_kernel, dim3(kB0Parts), dim3(256), 0, s, X, ld, M, n, w, incw, partial);
    hipLaunchKernelGGL(beat_input_grad_kernel, dim3(grid_for(n)), dim3(256), 0, s, sv, w, incw, b0, dw, db0, n,
                       (const float*)partial);
    return ok();
}
int pw_scale(float* x, long n, float a, hipStream_t s) {
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, n, a);
    return ok();
}

int pw_embedding_fwd(const float* table, const long long* idx, long rows, int E, float* out, const float* row_scale,
                     hipStream_t s) {
    hipLaunchKernelGGL(embedding_fwd_kernel, dim3(grid_for(rows * E)), dim3(256), 0, s, table, idx, rows, E, out, row_scale);
    return ok();
}
int pw_embedding_bwd(const float* dout, const long long* idx, long rows, int E, float* dtable, const float* row_scale,
                     hipStream_t s, int num_embeddings) {
    // a small table: thousands of rows land on a handful of table rows and the per-element atomics serialise (100-160 us for
    // the metadata embeddings of AnticipationRNN); the segment-sum kernel adds them up in LDS first
    if (num_embeddings > 0 && num_embeddings <= kSegMaxW && rows >= 1024 && rows < (1L << 31))
        return pw_token_segsum(dout, E, idx, (int)rows, 0, 1, (int)rows, num_embeddings, E, dtable, s, row_scale, 0);
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3(grid_for(rows * E)), dim3(256), 0, s, dout, idx, rows, E, dtable, row_scale);
    return ok();
}
int pw_tokens_i32_to_i64(const int* src, long long* dst, long n, hipStream_t s) {
    hipLaunchKernelGGL(tokens_i32_to_i64_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, n);
    return ok();
}
int pw_split_measures(const int* score, int B, int M, int L, int n_past, int n_target, long long* past,
                      long long* target, long long* future, hipStream_t s) {
    hipLaunchKernelGGL(split_measures_kernel, dim3(grid_for((long)B * M * L)), dim3(256), 0, s, score, B, M, L, n_past,
                       n_target, past, target, future);
    return ok();
}
int pw_prologue(const PwPrologue& p, hipStream_t s) {
    PwPrologue q = p;
    q.tok_bad = q.tok_V > 0 ? token_host_status() : nullptr;
    // grid.x: one pass over the largest job -- the tick GRU's gather table, (V + 1) x 3H outputs of E dependent multiply-adds each, every
    // thread walking its own row of W_ih -- instead of six (48 workgroups per job until round 6: the launch took 11.8 us, a tenth of a
    // one-measure decode call); every job strides over the grid, so any width is correct
    long widest = 0;
    for (int j = 0; j < q.ntab && j < 4; ++j) widest = widest > (long)q.tab[j].rows * q.tab[j].N ? widest : (long)q.tab[j].rows * q.tab[j].N;
    widest = widest > q.nzero / 4 ? widest : q.nzero / 4;
    const int gx = (int)((widest + 255) / 256 < 48 ? 48 : ((widest + 255) / 256 > 512 ? 512 : (widest + 255) / 256));
    hipLaunchKernelGGL(prologue_kernel, dim3(gx, 7), dim3(256), 0, s, q);
    return ok();
}
