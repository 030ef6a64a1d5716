// Class-weighted, label-smoothed cross-entropy with an ignore index, and the per-class statistics of a batch (ce.hip, DESIGN.md
// section 28): torch.nn.functional.cross_entropy(x, t, weight=w, label_smoothing=e, ignore_index=i, reduction='mean').
//   valid_r = t_r != i and 0 <= t_r < V;  p = softmax(x_r);  W = sum_c w_c;  denom = sum_valid w[t_r]
//   loss = [(1 - e) sum_valid w[t_r] (lse_r - x_r[t_r]) + (e / V) sum_valid sum_c w_c (lse_r - x_r[c])] / denom
//   dloss / dx_r[c] = valid_r [(1 - e) w[t_r] (p_c - 1{c = t_r}) + (e / V) (W p_c - w_c)] / denom
// denom == 0 (every row ignored, or every present target has weight 0): the loss is NaN as torch's is, dW is ALL ZEROS (torch: zeros
// in the first case, NaN in the second).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// The plain cross-entropy (ce_kernel): loss_sum += out_scale * sum (lse - w[target]), correct += out_scale * hits, both through one
// float atomic pair per workgroup; dW = (softmax - onehot) * scale.  ce_w below is defined against its bits.
int pw_cross_entropy(const float* W, long ld_w, int rows, int V, const long long* tgt, float* dW, long ld_dw,
                     float scale, float out_scale, float* loss_sum, float* correct, hipStream_t s,
                     const float* scale_dev = nullptr, const float* add_term = nullptr, float add_scale = 0.f,
                     float* fwd_out = nullptr, float fwd_scale = 0.f);

// The block ce_count_launch leaves behind and ce_w_launch reads: kCeMetaWords int64 words, then counts[V].
constexpr int kCeMetaWords = 8;
constexpr int kCeMetaDenom = 0;                  // double: sum_c w_c counts_c, added in class order
constexpr int kCeMetaValid = 1;                  // int64: targets inside [0, V) that are not ignore_index
constexpr int kCeMetaBad = 2;                    // int64: targets outside [0, V) that are not ignore_index (treated as ignored)
constexpr int kCeMetaCountTicket = 3;            // workgroups of the counting launch that have finished
constexpr int kCeMetaLossTicket = 4;             // ... of a loss launch with sums; 0 between launches
constexpr int kCeMetaWsum = 5;                   // double: sum_c w_c in class order (V without weights)
constexpr int kCeLdsV = 1024;                    // up to this V the class weights and the per-class histograms of a workgroup live in LDS
constexpr int kCeMaxGrid = 128;                  // workgroups of a loss launch with sums = partials the finishing workgroup adds

struct CeWArgs {
    const float* W; long ld_w; int rows; int V;
    const long long* tgt;
    const float* cw;                             // class weights [V], or null = all ones
    double smooth;                               // e
    int has_ignore; long long ignore;
    long long* meta;                             // the counting launch's block: denom, n_valid, W and the ticket
    float* dW; long ld_dw;                       // nullable
    const float* scale_dev;                      // nullable device scalar multiplied into dW
    float* loss; float* acc;                     // nullable; WRITTEN (not accumulated)
    const float* add_term; float add_scale;      // loss += add_scale * add_term[0]
    float* fwd_out; float fwd_scale;             // fwd_out[0] = fwd_scale * scale_dev[0]
    long long* stats;                            // nullable [V, 3] += {target count, hits, predicted}
    long long* conf;                             // nullable [V, V] += 1 at [target, argmax]
    void* ws;                                    // ce_w_ws_bytes(rows) bytes when anything but dW is asked for
};

// out: kCeMetaWords + V + extra int64 on the device, all zeroed here (extra: words the caller wants zeroed along, e.g. the statistics
// of the loss launch that follows).  n_bad > 0 bumps the token status word (chain.h).
int ce_count_launch(const long long* tgt, long n, int V, const float* cw, int has_ignore, long long ignore, long long* out, long extra,
                    hipStream_t s);
long ce_w_ws_bytes(int rows);
int ce_w_launch(const CeWArgs& a, hipStream_t s);
