// The batched LSTM (lstm.hip): whole-sequence drivers and the two-layer pipeline.
#pragma once
#include <hip/hip_runtime.h>
size_t lstm_ws_bytes(int B, int T, int H, int save);
int lstm_seq_fwd(int B, int T, int H, const float* gi, const float* W_hh, const float* b_hh, const float* h0,
                 const float* c0, int reverse, float* out, float* hT, float* cT, void* ws, int save, hipStream_t s);
int lstm_seq_bwd(int B, int T, int H, const float* W_hh, const float* h0, const float* out, const float* dout,
                 const float* dhT, const float* dcT, int reverse, float* dgi, float* dW_hh, float* db_ih, float* db_hh,
                 float* dh0, float* dc0, void* ws, hipStream_t s);
// What an LSTM layer of (B rows, T steps, hidden size H) launches under the options set now, decided without a GPU call: every launch
// site of lstm.hip takes its numbers from here.  side_by_side = 1: the layer on its own (lstm_seq_fwd / _bwd: one chain launch over
// all T steps); 2: the two-layer pipeline (lstm2_seq_fwd / _bwd: two chain launches at a time on two streams, chunks of time steps).
struct LstmChainPlan {
    int ok;                                // the chain kernels take it (else: one launch per step; the pipeline: layer by layer)
    int ms, groups, members;               // row tile = 16 * ms rows per group; groups of `members` = H / 16 workgroups
    int workgroups, blocks;                // workgroups of one launch that stay for its T steps; blocks launched (chain::blocks_for)
    int tagged;                            // forward launches use the data-driven hand-off (pipeline only)
    int chunk, chunks, areas;              // steps per launch, launches per layer, one pre-zeroed backward counter area per chunk
    int capacity;                          // chain_capacity()
    int side_by_side, max_groups, counter_stride, counter_words;   // group counters: stride and words of one counter area
};
LstmChainPlan lstm_chain_plan(int B, int T, int H, int side_by_side);
bool lstm2_ok(int B, int T, int H);
// two stacked layers, pipelined over chunks of time steps on two streams (lstm.hip); return 1 = shape does not qualify
int lstm2_seq_fwd(int B, int T, int H, const float* gi0, const float* W_hh0, const float* b_hh0, const float* W_ih1,
                  const float* b_ih1, const float* W_hh1, const float* b_hh1, int reverse, float* out0, float* gi1,
                  float* out1, void* ws0, void* ws1, int save, hipStream_t s);
int lstm2_seq_bwd(int B, int T, int H, const float* W_hh0, const float* W_ih1, const float* W_hh1, const float* out0,
                  const float* out1, const float* dout1, int reverse, float* dgi0, float* dgi1, float* dout0, float* dW_hh0,
                  float* db_ih0, float* db_hh0, float* dW_ih1, float* dW_hh1, float* db_ih1, float* db_hh1, void* ws0,
                  void* ws1, hipStream_t s);
