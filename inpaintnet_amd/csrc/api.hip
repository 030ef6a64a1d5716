// extern "C" surface declared in include/inpaintnet_hip.h.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "seq.h"
#include "layout.h"
#include "vae.h"
#include "lstm.h"
#include "arnn_gen.h"
#include "chain.h"
#include "decode_chain.h"
#include "gemm_bf3.h"
#include "gru_step_bf3.h"
#include "side.h"
#include "mmd.h"
#include "iw.h"
#include "attr.h"
#include "ce.h"
#include "latent.h"
#include "optim.h"
#include "sample_rows.h"

namespace {

bool cfg_ok(const inet_vae_config* c) {
    return c && c->num_notes > 0 && c->emb_dim > 0 && c->enc_hidden > 0 && c->enc_hidden % 16 == 0 &&
           c->dec_hidden > 0 && c->dec_hidden % 16 == 0 && c->z_dim > 0 && c->beats > 0 && c->beats <= 4 &&
           c->ticks_per_beat > 0;
}

int entry_info(const ArenaBuilder& ab, int index, char* name, int cap, int64_t* off, int64_t* dims, int* ndim) {
    if (index < 0 || index >= (int)ab.entries.size()) return -1;
    const ParamEntry& e = ab.entries[index];
    if (name && cap > 0) { std::strncpy(name, e.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (off) *off = e.offset;
    if (dims) for (int i = 0; i < 4; ++i) dims[i] = e.dims[i];
    if (ndim) *ndim = e.ndim;
    return 0;
}

// pointers to the 16 tensors of a 2-layer bidirectional nn.GRU laid out by ArenaBuilder::add_gru
void bigru_ptrs(const float* w, float* g, int K, int H, GruDirPtr* P) {
    ArenaBuilder ab;
    GruDirOff off[4];
    ab.add_gru("g", K, H, 2, true, off);
    for (int i = 0; i < 4; ++i) {
        P[i].w_ih = w + off[i].w_ih; P[i].w_hh = w + off[i].w_hh; P[i].b_ih = w + off[i].b_ih; P[i].b_hh = w + off[i].b_hh;
        P[i].dw_ih = g ? g + off[i].w_ih : nullptr; P[i].dw_hh = g ? g + off[i].w_hh : nullptr;
        P[i].db_ih = g ? g + off[i].b_ih : nullptr; P[i].db_hh = g ? g + off[i].b_hh : nullptr;
        P[i].K = off[i].K;
    }
}

struct BiWs {
    BiGru2Ws g;
    float *x_tm, *gi0, *gvec, *out_tm, *dout_tm, *dx_tm, *tmp3h;
};
size_t bi_carve(int B, int T, int K, int H, int save, void* base, BiWs& w) {
    Carver cv(base);
    const size_t TB = (size_t)T * B;
    w.x_tm = cv.take<float>(TB * K);
    w.gi0 = cv.take<float>(TB * 6 * H);
    w.gvec = cv.take<float>(6 * H);
    w.out_tm = nullptr;
    bigru2_carve(cv, B, T, H, save, w.g);
    if (save) {
        w.dout_tm = cv.take<float>(TB * 2 * H);
        w.dx_tm = cv.take<float>(TB * K);
        w.tmp3h = cv.take<float>(3 * H + 64);                   // + 64 partial sums of the scalar input's gradient (pw_beat_input_grad)
    } else {
        w.dout_tm = w.dx_tm = w.tmp3h = nullptr;
    }
    return cv.bytes();
}

}  // namespace

extern "C" {

int inet_abi_version(void) { return INET_ABI_VERSION; }

int inet_vae_param_count(const inet_vae_config* cfg) {
    if (!cfg_ok(cfg)) return -1;
    return (int)VaeLayout(*cfg).ab.entries.size();
}
int64_t inet_vae_param_floats(const inet_vae_config* cfg) {
    if (!cfg_ok(cfg)) return -1;
    return VaeLayout(*cfg).ab.total;
}
int inet_vae_param_info(const inet_vae_config* cfg, int index, char* name, int name_cap, int64_t* offset_floats,
                        int64_t* dims, int* ndim) {
    if (!cfg_ok(cfg)) return -1;
    return entry_info(VaeLayout(*cfg).ab, index, name, name_cap, offset_floats, dims, ndim);
}
int inet_latent_param_count(const inet_latent_config* cfg) {
    if (!cfg || cfg->rnn_hidden % 16) return -1;
    return (int)LatentLayout(*cfg).ab.entries.size();
}
int64_t inet_latent_param_floats(const inet_latent_config* cfg) {
    if (!cfg || cfg->rnn_hidden % 16) return -1;
    return LatentLayout(*cfg).ab.total;
}
int inet_latent_param_info(const inet_latent_config* cfg, int index, char* name, int name_cap, int64_t* offset_floats,
                           int64_t* dims, int* ndim) {
    if (!cfg || cfg->rnn_hidden % 16) return -1;
    return entry_info(LatentLayout(*cfg).ab, index, name, name_cap, offset_floats, dims, ndim);
}

int64_t inet_vae_encoder_ws_bytes(const inet_vae_config* cfg, int batch, int save) {
    if (!cfg_ok(cfg) || batch <= 0) return -1;
    return (int64_t)vae_encoder_ws_bytes(*cfg, batch, save);
}
int inet_vae_encoder_fwd(const inet_vae_config* cfg, int batch, const int64_t* tokens, const float* params,
                         const float* mask, float* mu, float* logsigma, void* ws, int64_t ws_bytes, int save,
                         void* stream) {
    if (!cfg_ok(cfg) || batch <= 0 || !tokens || !params || !mu || !logsigma || !ws) return -1;
    if (ws_bytes < (int64_t)vae_encoder_ws_bytes(*cfg, batch, save)) return -1;
    return vae_encoder_fwd(*cfg, batch, (const long long*)tokens, params, mask, mu, logsigma, ws, save, (hipStream_t)stream);
}
int inet_vae_encoder_bwd(const inet_vae_config* cfg, int batch, const int64_t* tokens, const float* params,
                         float* grads, const float* mask, const float* dmu, const float* dlogsigma, void* ws,
                         int64_t ws_bytes, int stage, void* stream) {
    if (!cfg_ok(cfg) || batch <= 0 || !tokens || !params || !grads || !dmu || !dlogsigma || !ws) return -1;
    if (stage < 0 || stage > 2 || ws_bytes < (int64_t)vae_encoder_ws_bytes(*cfg, batch, 1)) return -1;
    return vae_encoder_bwd(*cfg, batch, (const long long*)tokens, params, grads, mask, dmu, dlogsigma, ws,
                           (hipStream_t)stream, stage);
}
int64_t inet_vae_decoder_ws_bytes(const inet_vae_config* cfg, int batch, int save) {
    if (!cfg_ok(cfg) || batch <= 0) return -1;
    return (int64_t)vae_decoder_ws_bytes(*cfg, batch, save);
}
int inet_vae_decoder_fwd(const inet_vae_config* cfg, int batch, const float* z, const int64_t* target,
                         int teacher_forced, const float* params, const float* mask_beat, const float* mask_tick,
                         float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                         uint64_t multinomial_seed, void* stream) {
    if (!cfg_ok(cfg) || batch <= 0 || !z || !params || !weights || !samples || !ws) return -1;
    if (ws_bytes < (int64_t)vae_decoder_ws_bytes(*cfg, batch, save)) return -1;
    return vae_decoder_fwd(*cfg, batch, z, (const long long*)target, teacher_forced, params, mask_beat, mask_tick,
                           weights, (long long*)samples, ws, save, (hipStream_t)stream, multinomial_seed, sample::Request{});
}
int inet_vae_decoder_sample_fx(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                               const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                               float temperature, const double* uniforms, int top_k, double top_p, float* logp,
                               const uint64_t* allow, const int32_t* forced, void* stream) {
    if (!cfg_ok(cfg) || batch <= 0 || !z || !params || !weights || !samples || !ws || !uniforms) return -1;
    if (allow && (int64_t)cfg->beats * cfg->ticks_per_beat > 64) return -1;    // (a constrained call: at most 64 ticks)
    sample::Request rq{uniforms, temperature, top_k, top_p, logp, nullptr, (const unsigned long long*)allow, (const int*)forced};
    rq.dense(cfg->beats * cfg->ticks_per_beat, cfg->num_notes);
    if (!rq.ok(cfg->num_notes)) return -1;
    if (ws_bytes < (int64_t)vae_decoder_ws_bytes(*cfg, batch, save)) return -1;
    return vae_decoder_fwd(*cfg, batch, z, nullptr, 0, params, mask_beat, mask_tick, weights, (long long*)samples, ws, save,
                           (hipStream_t)stream, 0, rq);
}
int inet_vae_decoder_sample_cx(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                               const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                               float temperature, const double* uniforms, int top_k, double top_p, float* logp,
                               const uint64_t* allow, void* stream) {
    return inet_vae_decoder_sample_fx(cfg, batch, z, params, mask_beat, mask_tick, weights, samples, ws, ws_bytes, save, temperature,
                                      uniforms, top_k, top_p, logp, allow, nullptr, stream);
}
int inet_vae_decoder_sample_ex(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                               const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                               float temperature, const double* uniforms, int top_k, double top_p, float* logp, void* stream) {
    return inet_vae_decoder_sample_cx(cfg, batch, z, params, mask_beat, mask_tick, weights, samples, ws, ws_bytes, save, temperature,
                                      uniforms, top_k, top_p, logp, nullptr, stream);
}
int inet_vae_decoder_sample(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                            const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                            float temperature, const double* uniforms, void* stream) {
    return inet_vae_decoder_sample_ex(cfg, batch, z, params, mask_beat, mask_tick, weights, samples, ws, ws_bytes, save, temperature,
                                      uniforms, 0, 1.0, nullptr, stream);
}
int inet_vae_decoder_bwd(const inet_vae_config* cfg, int batch, const float* dweights, const float* weights,
                         const int64_t* tokens_in, const float* params, float* grads, const float* mask_beat,
                         const float* mask_tick, float* dz, void* ws, int64_t ws_bytes, void* stream) {
    if (!cfg_ok(cfg) || batch <= 0 || !dweights || !weights || !tokens_in || !params || !ws) return -1;
    if (ws_bytes < (int64_t)vae_decoder_ws_bytes(*cfg, batch, 1)) return -1;
    return vae_decoder_bwd(*cfg, batch, dweights, weights, (const long long*)tokens_in, params, grads, mask_beat,
                           mask_tick, dz, ws, (hipStream_t)stream);
}

int inet_vae_ws_field(const inet_vae_config* cfg, int batch, int which, const char* name, int64_t* offset_floats,
                      int64_t* count) {
    if (!cfg_ok(cfg) || batch <= 0 || !name) return -1;
    long long off = 0, n = 0;
    const int rc = vae_ws_field(*cfg, batch, which, name, &off, &n);
    if (rc == 0) { if (offset_floats) *offset_floats = off; if (count) *count = n; }
    return rc;
}

int inet_cross_entropy(const float* weights, int64_t ld_w, int rows, int V, const int64_t* targets, float* dW,
                       int64_t ld_dw, float scale, float out_scale, float* loss_sum, float* correct, void* stream) {
    if (!weights || !targets || !loss_sum || !correct || rows <= 0 || V <= 0) return -1;
    return pw_cross_entropy(weights, ld_w, rows, V, (const long long*)targets, dW, ld_dw, scale, out_scale, loss_sum,
                            correct, (hipStream_t)stream);
}
int inet_cross_entropy_ex(const float* weights, int64_t ld_w, int rows, int V, const int64_t* targets, float* dW,
                          int64_t ld_dw, float scale, const float* scale_dev, float out_scale, float* loss_sum,
                          float* correct, const float* add_term, float add_scale, float* fwd_out, float fwd_scale,
                          void* stream) {
    if (!weights || !targets || rows <= 0 || V <= 0 || (!dW && !loss_sum && !correct) || (fwd_out && !scale_dev)) return -1;
    return pw_cross_entropy(weights, ld_w, rows, V, (const long long*)targets, dW, ld_dw, scale, out_scale, loss_sum,
                            correct, (hipStream_t)stream, scale_dev, add_term, add_scale, fwd_out, fwd_scale);
}
int inet_sample_multinomial(const float* weights, int64_t ld_w, int rows, int V, int64_t* out, int64_t stride,
                            uint64_t seed, uint64_t offset, void* stream) {
    if (!weights || !out || rows <= 0 || V <= 0) return -1;
    return pw_sample_multinomial(weights, ld_w, rows, V, (long long*)out, stride, seed, offset, (hipStream_t)stream);
}
int inet_sample_temperature(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                            int64_t u_stride, int64_t* out, int64_t stride, void* stream) {
    if (!weights || !uniforms || !out || rows <= 0 || V <= 0) return -1;
    sample::Request rq{uniforms, temperature};
    rq.ld_u = u_stride;
    return pw_sample(weights, ld_w, rows, V, (long long*)out, stride, rq, 1, (hipStream_t)stream);
}
int inet_sample_forced(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                       int64_t u_stride, int top_k, double top_p, int64_t* out, int64_t stride, float* logp, int64_t logp_stride,
                       const uint64_t* allow, int64_t allow_stride, const int32_t* forced, int64_t forced_stride, void* stream) {
    if (!weights || !uniforms || !out || rows <= 0 || V <= 0) return -1;
    sample::Request rq{uniforms, temperature, top_k, top_p, logp, nullptr, (const unsigned long long*)allow, (const int*)forced};
    rq.ld_u = u_stride; rq.ld_logp = logp_stride; rq.ld_allow = allow_stride; rq.ld_forced = forced_stride;
    // (the truncating kernel at the least, whatever the values: the three entries of this family promise it; pw_sample asks rq.ok())
    return pw_sample(weights, ld_w, rows, V, (long long*)out, stride, rq, 2, (hipStream_t)stream);
}
int inet_sample_constrained(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                            int64_t u_stride, int top_k, double top_p, int64_t* out, int64_t stride, float* logp, int64_t logp_stride,
                            const uint64_t* allow, int64_t allow_stride, void* stream) {
    return inet_sample_forced(weights, ld_w, rows, V, temperature, uniforms, u_stride, top_k, top_p, out, stride, logp, logp_stride,
                              allow, allow_stride, nullptr, 0, stream);
}
int inet_sample_truncated(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                          int64_t u_stride, int top_k, double top_p, int64_t* out, int64_t stride, float* logp, int64_t logp_stride,
                          void* stream) {
    return inet_sample_constrained(weights, ld_w, rows, V, temperature, uniforms, u_stride, top_k, top_p, out, stride, logp, logp_stride,
                                   nullptr, 0, stream);
}
int inet_reparam_kl(const float* mu, const float* logsigma, const float* eps, float* z, float* sigma, int64_t n,
                    float* kl_sum, void* stream) {
    if (!mu || !logsigma || n <= 0) return -1;
    return pw_reparam_kl(mu, logsigma, eps, z, sigma, n, kl_sum, (hipStream_t)stream);
}
int inet_latent_bwd(const float* dz, const float* mu, const float* logsigma, const float* eps, float kscale,
                    const float* kscale_dev, float* dmu, float* dlogsigma, int64_t n, void* stream) {
    if (!mu || !logsigma || !dmu || !dlogsigma || n <= 0) return -1;
    return pw_latent_bwd(dz, mu, logsigma, eps, kscale, kscale_dev, dmu, dlogsigma, n, (hipStream_t)stream);
}
int64_t inet_reparam_kl_fb_ws_bytes(int64_t rows, int Z, int per) { return pw_reparam_kl_fb_ws_bytes(rows, Z, per); }
int inet_reparam_kl_fb(const float* mu, const float* logsigma, const float* eps, float* z, int64_t rows, int Z, float free_nats,
                       int per, float* parts, float* keep, float* kl_sum, float* kl_raw, void* ws, int64_t ws_bytes, void* stream) {
    if (!mu || !logsigma || !parts || !keep || !kl_sum || !kl_raw || rows <= 0 || Z <= 0) return -1;
    if (!(free_nats >= 0.f) || !(free_nats <= 3.402823466e38f) || (per != 0 && per != 1)) return -1;       // negative, NaN, inf
    return pw_reparam_kl_fb(mu, logsigma, eps, z, rows, Z, free_nats, per, parts, keep, kl_sum, kl_raw, ws, ws_bytes, (hipStream_t)stream);
}
int inet_latent_bwd_fb(const float* dz, const float* mu, const float* logsigma, const float* eps, float kscale,
                       const float* kscale_dev, const float* keep, int per, float* dmu, float* dlogsigma, int64_t rows, int Z,
                       void* stream) {
    if (!mu || !logsigma || !keep || !dmu || !dlogsigma || rows <= 0 || Z <= 0 || (per != 0 && per != 1)) return -1;
    return pw_latent_bwd_fb(dz, mu, logsigma, eps, kscale, kscale_dev, keep, per, dmu, dlogsigma, rows, Z, (hipStream_t)stream);
}
int64_t inet_mmd_ws_bytes(int64_t B, int Z) { return B > (1 << 24) ? -1 : mmd_ws_bytes(B, Z); }
int inet_mmd(const float* x, const float* y, int64_t B, int Z, int kind, float var, double a, double c, double diag, double coeff,
             float* out4, float* grad, void* ws, int64_t ws_bytes, void* stream) {
    if (!x || !y || !out4 || B < 1 || B > (1 << 24) || Z < 1 || (kind != MMD_GAUSSIAN && kind != MMD_IMQ)) return -1;
    if (!(var > 0.f) || !std::isfinite(var) || !std::isfinite(a) || !std::isfinite(c) || !std::isfinite(diag) || !std::isfinite(coeff)) return -1;
    return mmd_launch(x, y, B, Z, kind, var, a, c, diag, coeff, out4, grad, ws, ws_bytes, (hipStream_t)stream);
}
// attribute-regularised latent dimensions (attr.hip)
int inet_measure_attrs(const int64_t* tokens, int64_t B, int T, int V, int slur_index, int rest_index, int none_index, const int32_t* midi,
                       int midi_lo, int midi_hi, float* out, void* stream) {
    return attr_measure_launch((const long long*)tokens, B, T, V, slur_index, rest_index, none_index, midi, midi_lo, midi_hi, out,
                               (hipStream_t)stream);
}
int64_t inet_attr_reg_ws_bytes(int64_t B, int A) { return B > (1 << 24) ? -1 : attr_reg_ws_bytes(B, A); }
int inet_attr_reg(const float* z, int64_t B, int Z, const int32_t* dims, int A, const float* attrs, float delta, double coeff, float* out,
                  int64_t* counts, float* grad, void* ws, int64_t ws_bytes, void* stream) {
    if (!z || !dims || !attrs || !out || !counts || B < 1 || B > (1 << 24) || Z < 1 || A < 1 || A > kAttrMaxA) return -1;
    if (!std::isfinite(delta) || !std::isfinite(coeff)) return -1;
    AttrDims d{};
    for (int a = 0; a < A; ++a) {
        if (dims[a] < 0 || dims[a] >= Z) return -1;
        for (int b = 0; b < a; ++b)
            if (dims[b] == dims[a]) return -1;
        d.d[a] = dims[a];
    }
    return attr_reg_launch(z, B, Z, d, A, attrs, delta, coeff, out, (long long*)counts, grad, ws, ws_bytes, (hipStream_t)stream);
}
// class-weighted, label-smoothed cross-entropy and the per-class statistics (ce.hip); ignore_index: a HOST pointer, null = none
int inet_class_counts(const int64_t* targets, int64_t n, int V, const float* class_weight, const int64_t* ignore_index, int64_t* out,
                      int64_t extra_words, void* stream) {
    return ce_count_launch((const long long*)targets, n, V, class_weight, ignore_index != nullptr, ignore_index ? *ignore_index : 0,
                           (long long*)out, extra_words, (hipStream_t)stream);
}
int64_t inet_cross_entropy_w_ws_bytes(int rows) { return ce_w_ws_bytes(rows); }
int inet_cross_entropy_w(const float* weights, int64_t ld_w, int rows, int V, const int64_t* targets, const float* class_weight,
                         double label_smoothing, const int64_t* ignore_index, int64_t* meta, float* dW, int64_t ld_dw,
                         const float* scale_dev, float* loss, float* accuracy, const float* add_term, float add_scale, float* fwd_out,
                         float fwd_scale, int64_t* class_stats, int64_t* confusion, void* ws, int64_t ws_bytes, void* stream) {
    if (rows < 1 || ((loss || accuracy) && (!ws || ws_bytes < ce_w_ws_bytes(rows)))) return -1;
    CeWArgs a{weights, ld_w, rows, V, (const long long*)targets, class_weight, label_smoothing, ignore_index != nullptr,
              ignore_index ? *ignore_index : 0, (long long*)meta, dW, ld_dw, scale_dev, loss, accuracy, add_term, add_scale, fwd_out,
              fwd_scale, (long long*)class_stats, (long long*)confusion, ws};
    return ce_w_launch(a, (hipStream_t)stream);
}
// the importance-weighted log-likelihood (iw.hip): the launchers refuse a bad argument themselves, before anything is launched
int inet_iw_draw(const float* mu, const float* logsigma, const float* eps, int64_t eps_stride_b, float* z, float* logr, int64_t B, int Kc,
                 int Z, void* stream) {
    return iw_draw_launch(mu, logsigma, eps, eps_stride_b, z, logr, B, Kc, Z, (hipStream_t)stream);
}
int inet_nll_rows(const float* weights, int64_t ld_w, const int64_t* targets, const float* logr, float* nll, float* logw, int64_t ld_out,
                  int64_t R, int group, int T, int V, void* stream) {
    return nll_rows_launch(weights, ld_w, (const long long*)targets, logr, nll, logw, ld_out, R, group, T, V, (hipStream_t)stream);
}
int inet_iw_finish(const float* logw, const float* nll, int64_t ld, int64_t B, int K, double* out, void* stream) {
    return iw_finish_launch(logw, nll, ld, B, K, out, (hipStream_t)stream);
}
// the four entry points of the optimizer step: one check, one launcher (pw_adam_step)
static int adam_step_checked(const PwAdamStep& a, void* stream) {
    if (!a.p || !a.g || !a.m || !a.v || a.n <= 0 || a.step < 1) return -1;
    if (!(a.weight_decay >= 0.f) || !(a.weight_decay <= 3.402823466e38f)) return -1;            // negative, NaN, inf
    if (!(a.ema_decay >= 0.f) || !(a.ema_decay < 1.f)) return -1;                               // outside [0, 1), NaN
    if (a.partials && !(a.max_norm > 0.f)) return -1;                                           // NaN fails the comparison; without partials max_norm is ignored
    return pw_adam_step(a, (hipStream_t)stream);
}
int inet_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, int step, float gscale, void* stream) {
    return adam_step_checked({p, g, m, v, n, lr, beta1, beta2, eps, step, gscale, 0.f, nullptr, 0.f, nullptr, nullptr, 0.f, nullptr, nullptr},
                             stream);
}
int inet_adam_step_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, int step, float gscale, const float* step_flag, uint32_t* report, void* stream) {
    return adam_step_checked({p, g, m, v, n, lr, beta1, beta2, eps, step, gscale, 0.f, nullptr, 0.f, nullptr, nullptr, 0.f, step_flag, report},
                             stream);
}
int inet_sqnorm_parts(void) { return pw_sqnorm_parts(); }
int inet_grad_sqnorm(const float* g, int64_t n, double* partials, void* stream) {
    if (!g || !partials || n <= 0 || ((uintptr_t)g & 15)) return -1;
    return pw_grad_sqnorm(g, n, partials, (hipStream_t)stream);
}
int inet_adam_step_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, int step, float gscale, float max_norm, const double* partials, const float* step_flag,
                        uint32_t* report, void* stream) {
    if (!partials) return -1;
    return adam_step_checked({p, g, m, v, n, lr, beta1, beta2, eps, step, gscale, max_norm, partials, 0.f, nullptr, nullptr, 0.f, step_flag,
                              report}, stream);
}
int inet_adam_step_w(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                     int step, float gscale, float max_norm, const double* partials, float weight_decay,
                     const uint32_t* decay_mask, float* ema, float ema_decay, const float* step_flag, uint32_t* report,
                     void* stream) {
    return adam_step_checked({p, g, m, v, n, lr, beta1, beta2, eps, step, gscale, max_norm, partials, weight_decay, decay_mask, ema,
                              ema_decay, step_flag, report}, stream);
}
int inet_step_flag_export(float* dst, void* stream) {
    if (!dst) return -1;
    return pw_step_flag_export(dst, (hipStream_t)stream);
}
int inet_token_status(int reset) {
    unsigned* p = token_host_status();
    if (!p) return -2;
    const int v = (int)__atomic_load_n(p, __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(p, 0u, __ATOMIC_RELAXED);
    return v;
}
int inet_epoch_stats_add(float* sums, const float* loss, const float* accuracy, void* stream) {
    if (!sums || !loss) return -1;
    return pw_epoch_stats_add(sums, loss, accuracy, (hipStream_t)stream);
}
int inet_epoch_stats_add_ex(float* sums, const float* loss, const float* accuracy, const float* step_flag, void* stream) {
    if (!sums || !loss) return -1;
    return pw_epoch_stats_add(sums, loss, accuracy, (hipStream_t)stream, step_flag);
}
int inet_dropout_mask(float* out, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream) {
    if (!out || n <= 0 || p < 0.f || p >= 1.f) return -1;
    return pw_dropout_mask(out, n, p, seed, offset, (hipStream_t)stream);
}

int64_t inet_bigru2_ws_bytes(int batch, int T, int K, int H, int save) {
    if (batch <= 0 || T <= 0 || K <= 0 || H <= 0 || H % 16) return -1;
    BiWs w;
    return (int64_t)bi_carve(batch, T, K, H, save, nullptr, w);
}

int inet_bigru2_fwd(int B, int T, int K, int H, const float* x, const float* x_scalar, const float* weights,
                    const float* h0, const float* mask, float* out, float* h_n, void* ws, int64_t ws_bytes, int save,
                    void* stream) {
    if (B <= 0 || T <= 0 || K <= 0 || H <= 0 || H % 16 || !weights || !ws) return -1;
    if (ws_bytes < inet_bigru2_ws_bytes(B, T, K, H, save)) return -1;
    if (!x && !(x_scalar && K == 1)) return -1;
    hipStream_t s = (hipStream_t)stream;
    BiWs w;
    bi_carve(B, T, K, H, save, ws, w);
    GruDirPtr P[4];
    bigru_ptrs(weights, nullptr, K, H, P);
    BiGru2In in{};
    if (x) {
        INET_TRY(pw_swap01(x, B, T, K, w.x_tm, s));                  // [B,T,K] -> [T,B,K]
        for (int dir = 0; dir < 2; ++dir)
            INET_TRY(linear_fwd(w.x_tm, K, P[dir].w_ih, K, P[dir].b_ih, w.gi0 + dir * 3L * H, 6L * H, T * B, 3 * H, K, EPI_NONE, s));
        in.gi0[0] = w.gi0; in.gi0[1] = w.gi0 + 3L * H; in.gi0_ld = 6L * H; in.gi0_ts = (long)B * 6 * H;
    } else {
        for (int dir = 0; dir < 2; ++dir) {
            INET_TRY(pw_axpb(x_scalar, P[dir].w_ih, 1, P[dir].b_ih, w.gvec + dir * 3L * H, 3 * H, s));
            in.gvec[dir] = w.gvec + dir * 3L * H;
        }
    }
    const long BH = (long)B * H;
    float* hn[4] = {nullptr, nullptr, nullptr, nullptr};
    if (h_n) for (int i = 0; i < 4; ++i) hn[i] = h_n + i * BH;
    SyncLedger areas(w.g.sync);                                      // (nothing zeroed yet: the core does where it pays)
    INET_TRY(bigru2_core_fwd(B, T, H, P, in, h0, mask, h_n ? hn : nullptr, H, w.g, save, s, areas));
    if (out) INET_TRY(pw_swap01(w.g.h1, T, B, 2 * H, out, s));       // [T,B,2H] -> [B,T,2H]
    return 0;
}

int inet_bigru2_bwd(int B, int T, int K, int H, const float* x, const float* x_scalar, const float* weights,
                    float* grads, const float* mask, const float* dout, const float* dh_n, float* dx,
                    float* dx_scalar, float* dh0, void* ws, int64_t ws_bytes, void* stream) {
    if (B <= 0 || T <= 0 || K <= 0 || H <= 0 || H % 16 || !weights || !ws) return -1;
    if (ws_bytes < inet_bigru2_ws_bytes(B, T, K, H, 1)) return -1;
    if (!x && !(x_scalar && K == 1)) return -1;
    hipStream_t s = (hipStream_t)stream;
    BiWs w;
    bi_carve(B, T, K, H, 1, ws, w);
    GruDirPtr P[4];
    bigru_ptrs(weights, grads, K, H, P);
    const long BH = (long)B * H;
    if (bigru2_ws_opts_peek(w.g) != 0) return -3;                    // (before the first write: the carve may differ)
    if (dout) INET_TRY(pw_swap01(dout, B, T, 2 * H, w.dout_tm, s));
    const float* dhn[4] = {nullptr, nullptr, nullptr, nullptr};
    if (dh_n) for (int i = 0; i < 4; ++i) dhn[i] = dh_n + i * BH;
    INET_TRY(bigru2_core_bwd(B, T, H, P, mask, dout ? w.dout_tm : nullptr, dh_n ? dhn : nullptr, H, dh0, w.g, s));
    for (int dir = 0; dir < 2; ++dir) {
        const float* dgi = w.g.dgi0 + dir * 3L * H;
        if (x) {
            if (grads) INET_TRY(linear_wgrad(dgi, 6L * H, w.x_tm, K, P[dir].dw_ih, K, T * B, 3 * H, K, side_fork(s)));
            if (dx) INET_TRY(linear_dgrad(dgi, 6L * H, P[dir].w_ih, K, w.dx_tm, K, T * B, 3 * H, K, EPI_NONE, nullptr, 0,
                                          dir == 0 ? ACC_STORE : ACC_ADD, s));
        } else if (grads) {
            INET_TRY(pw_zero(w.tmp3h, 3L * H, s));
            INET_TRY(pw_colsum(dgi, 6L * H, T * B, 3 * H, w.tmp3h, s));
            if (!dx_scalar) return -1;
            INET_TRY(pw_beat_input_grad(w.tmp3h, P[dir].w_ih, 1, x_scalar, P[dir].dw_ih, dx_scalar, 3 * H, dgi, 6L * H, T * B,
                                        w.tmp3h + 3 * H, s));
        }
    }
    if (x && dx) INET_TRY(pw_swap01(w.dx_tm, T, B, K, dx, s));
    return side_join(s);
}

int inet_gemm(const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb, int b_kmajor, float* C,
              int64_t ldc, int M, int N, int K, const float* bias, const float* aux, int64_t ldaux, int epi, int acc,
              void* stream) {
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || epi < 0 || epi > 5 || acc < 0 || acc > 1) return -1;
    return launch_gemm(gemm_args(A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N, K, bias, epi, aux, ldaux, acc),
                       (hipStream_t)stream);
}

int inet_gemm_bf3(const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb, int b_kmajor, float* C,
                  int64_t ldc, int M, int N, int K, const float* bias, int acc, int ksplit, void* stream) {
    if (!A || !B || !C || acc < 0 || acc > 1 || ksplit < 0 || !gemm_bf3_ok(M, N, K)) return -1;
    if ((a_kmajor && M % 64) || (b_kmajor && N % 64)) return -1;
    hipStream_t s = (hipStream_t)stream;
    unsigned char* scratch = nullptr;
    const size_t ab = bf3_bytes(M, K), bb = bf3_bytes(N, K);
    if (hipMalloc(&scratch, ab + bb) != hipSuccess) return -2;
    int rc = bf3_split(A, lda, a_kmajor, M, K, scratch, (long)bf3_piece_bytes(M, K), K / 32, 0, 0, s);
    if (rc == 0) rc = bf3_split(B, ldb, b_kmajor, N, K, scratch + ab, (long)bf3_piece_bytes(N, K), K / 32, 0, 0, s);
    if (rc == 0) {
        Bf3Gemm g{};
        g.A = scratch; g.a_piece = (long)bf3_piece_bytes(M, K); g.a_kb = K / 32;
        g.B = scratch + ab; g.b_piece = (long)bf3_piece_bytes(N, K); g.b_kb = K / 32;
        g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.bias = bias; g.epi = EPI_NONE; g.acc = acc; g.ksplit = ksplit;
        rc = launch_gemm_bf3(g, s);
    }
    if (hipStreamSynchronize(s) != hipSuccess) rc = -2;
    (void)hipFree(scratch);
    return rc;
}

int inet_gemm_batched(const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb, int b_kmajor, float* C,
                      int64_t ldc, int M, int N, int K, int nbatch, int64_t batchA, int64_t batchB, int64_t batchC,
                      void* stream) {
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || nbatch < 1 || nbatch > 8) return -1;
    GemmArgs g = gemm_args(A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N, K, nullptr, EPI_NONE, nullptr, 0, ACC_ADD);
    g.nbatch = nbatch; g.batchA = batchA; g.batchB = batchB; g.batchC = batchC;
    return launch_gemm(g, (hipStream_t)stream);
}

int inet_gemm_group(int n, const inet_gemm_desc* list, void* stream) {
    GemmArgs g[kGemmGroupMax];
    if (n < 1 || n > kGemmGroupMax || !list) return -1;
    for (int i = 0; i < n; ++i) {
        const inet_gemm_desc& d = list[i];
        if (!d.A || !d.B || !d.C || d.M <= 0 || d.N <= 0 || d.K <= 0 || d.epi < 0 || d.epi > 5 || d.acc < 0 || d.acc > 1) return -1;
        g[i] = gemm_args(d.A, d.lda, d.a_kmajor, d.B, d.ldb, d.b_kmajor, d.C, d.ldc, d.M, d.N, d.K, d.bias, d.epi, d.aux, d.ldaux, d.acc);
    }
    return launch_gemm_group(g, n, (hipStream_t)stream);
}

int inet_linear_fwd(const float* x, const float* W, const float* b, float* y, int M, int N, int K, int epi,
                    void* stream) {
    if (!x || !W || !y || M <= 0 || N <= 0 || K <= 0 || epi < 0 || epi > 2) return -1;
    return linear_fwd(x, K, W, K, b, y, N, M, N, K, epi, (hipStream_t)stream);
}
int inet_linear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db, int M, int N,
                    int K, void* stream) {
    if (!dy || M <= 0 || N <= 0 || K <= 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        if (!W) return -1;
        // an input width that is not a multiple of 64 (AnticipationRNN: 20 embedding + 256 constraint columns) would send the
        // whole product to the LDS-tiled fallback: the leading K % 64 columns go there alone, the rest to the direct kernels
        const int r = K % 64;
        if (r && K - r >= 128 && M >= 1024) {
            INET_TRY(launch_gemm(gemm_args(dy, N, 0, W, K, 1, dx, K, M, r, N), s));
            INET_TRY(launch_gemm(gemm_args(dy, N, 0, W + r, K, 1, dx + r, K, M, K - r, N), s));
        } else INET_TRY(linear_dgrad(dy, N, W, K, dx, K, M, N, K, EPI_NONE, nullptr, 0, ACC_STORE, s));
    }
    if (dW || db) {
        hipStream_t ss = side_fork(s);                       // leaf work
        if (dW) { if (!x) return -1; INET_TRY(linear_wgrad(dy, N, x, K, dW, K, M, N, K, ss)); }
        if (db) INET_TRY(pw_colsum(dy, N, M, N, db, ss));
        return side_join(s);
    }
    return 0;
}

int64_t inet_lstm_ws_bytes(int batch, int T, int H, int save) {
    if (batch <= 0 || T <= 0 || H <= 0 || H % 16) return -1;
    return (int64_t)lstm_ws_bytes(batch, T, H, save);
}
int inet_lstm_fwd(int B, int T, int H, const float* gi, const float* W_hh, const float* b_hh, const float* h0,
                  const float* c0, int reverse, float* out, float* hT, float* cT, void* ws, int64_t ws_bytes, int save,
                  void* stream) {
    if (B <= 0 || T <= 0 || H <= 0 || H % 16 || !gi || !W_hh || !b_hh || !out || !ws) return -1;
    if (ws_bytes < (int64_t)lstm_ws_bytes(B, T, H, save)) return -1;
    return lstm_seq_fwd(B, T, H, gi, W_hh, b_hh, h0, c0, reverse, out, hT, cT, ws, save, (hipStream_t)stream);
}
int inet_lstm_bwd(int B, int T, int H, const float* W_hh, const float* h0, const float* out, const float* dout,
                  const float* dhT, const float* dcT, int reverse, float* dgi, float* dW_hh, float* db_ih, float* db_hh,
                  float* dh0, float* dc0, void* ws, int64_t ws_bytes, void* stream) {
    if (B <= 0 || T <= 0 || H <= 0 || H % 16 || !W_hh || !out || !dgi || !ws) return -1;
    if ((dW_hh != nullptr) != (db_hh != nullptr) || (dW_hh != nullptr) != (db_ih != nullptr)) return -1;
    if (ws_bytes < (int64_t)lstm_ws_bytes(B, T, H, 1)) return -1;
    return lstm_seq_bwd(B, T, H, W_hh, h0, out, dout, dhT, dcT, reverse, dgi, dW_hh, db_ih, db_hh, dh0, dc0, ws,
                        (hipStream_t)stream);
}
int inet_lstm2_ok(int B, int T, int H) { return B > 0 && T > 0 && H > 0 && H % 16 == 0 && lstm2_ok(B, T, H) ? 1 : 0; }
int inet_lstm2_fwd(int B, int T, int H, const float* gi0, const float* W_hh0, const float* b_hh0, const float* W_ih1,
                   const float* b_ih1, const float* W_hh1, const float* b_hh1, int reverse, float* out0, float* gi1,
                   float* out1, void* ws0, void* ws1, int64_t ws_bytes, int save, void* stream) {
    if (B <= 0 || T <= 0 || H <= 0 || H % 16 || !gi0 || !W_hh0 || !b_hh0 || !W_ih1 || !b_ih1 || !W_hh1 || !b_hh1 || !out0 ||
        !gi1 || !out1 || !ws0 || !ws1 || ws0 == ws1)
        return -1;
    if (ws_bytes < (int64_t)lstm_ws_bytes(B, T, H, save)) return -1;
    return lstm2_seq_fwd(B, T, H, gi0, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, reverse, out0, gi1, out1, ws0, ws1, save,
                         (hipStream_t)stream);
}
int64_t inet_arnn_generate_ws_floats(int L, int E, int Hc, int H, int U, int V) {
    if (L <= 0 || E <= 0 || Hc < 0 || H <= 0 || H % 16 || U <= 0 || V <= 0) return -1;
    return (int64_t)arnn_generate_ws_floats(ArnnGenNet{E, Hc, H, U, V}, L);
}
int inet_arnn_generate(int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_stride,
                       const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0, const float* W_ih1,
                       const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                       const float* W2, const float* b2, const float* hc_init, const int64_t* first_tok, int64_t* tokens, float* ws,
                       int64_t ws_floats, void* stream) {
    if (L <= 0 || E <= 0 || Hc < 0 || H <= 0 || H % 16 || U <= 0 || V <= 0 || !emb || (Hc && !oc0) || !W_ih0 || !b_ih0 || !W_hh0 ||
        !b_hh0 || !W_ih1 || !b_ih1 || !W_hh1 || !b_hh1 || !W1 || !b1 || !W2 || !b2 || !tokens || !ws)
        return -1;
    const ArnnGenNet net{E, Hc, H, U, V, emb, W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, W1, b1, W2, b2};
    if (ws_floats < (int64_t)arnn_generate_ws_floats(net, L)) return -1;
    return arnn_generate(net, L, oc0, (long)oc_stride, hc_init, (const long long*)first_tok, (long long*)tokens, ws, (hipStream_t)stream);
}
int64_t inet_arnn_sample_ws_floats(int R, int L, int E, int Hc, int H, int U, int V) {
    if (R < 1 || L < 1 || E <= 0 || Hc < 0 || H <= 0 || H % 16 || U <= 0 || V <= 0) return -1;
    return (int64_t)arnn_sample_ws_floats(ArnnGenNet{E, Hc, H, U, V}, R, L);
}
int inet_arnn_sample_fx(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                        int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                        const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                        const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                        int64_t* tokens, float* ws, int64_t ws_floats, int top_k, double top_p, float* logp, float* logits,
                        const uint64_t* allow, const int32_t* forced, void* stream) {
    if (R < 1 || L < 1 || E <= 0 || Hc < 0 || H <= 0 || H % 16 || U <= 0 || V <= 0 || !emb || (Hc && !oc0) || !W_ih0 || !b_ih0 ||
        !W_hh0 || !b_hh0 || !W_ih1 || !b_ih1 || !W_hh1 || !b_hh1 || !W1 || !b1 || !W2 || !b2 || !uniforms || !tokens || !ws)
        return -1;
    if (oc_row_stride < 0 || oc_batch_stride < 0) return -1;
    sample::Request rq{uniforms, temperature, top_k, top_p, logp, logits, (const unsigned long long*)allow, (const int*)forced};
    rq.dense(L, V);
    if (!rq.ok(V)) return -1;
    const ArnnGenNet net{E, Hc, H, U, V, emb, W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, W1, b1, W2, b2};
    if (ws_floats < (int64_t)arnn_sample_ws_floats(net, R, L)) return -1;
    return arnn_sample(net, R, L, oc0, (long)oc_row_stride, (long)oc_batch_stride, hc_init, (long long*)tokens, ws, (hipStream_t)stream, rq);
}
int inet_arnn_sample_cx(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                        int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                        const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                        const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                        int64_t* tokens, float* ws, int64_t ws_floats, int top_k, double top_p, float* logp, float* logits,
                        const uint64_t* allow, void* stream) {
    return inet_arnn_sample_fx(R, L, E, Hc, H, U, V, emb, oc0, oc_row_stride, oc_batch_stride, W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1,
                               W_hh1, b_hh1, W1, b1, W2, b2, temperature, uniforms, hc_init, tokens, ws, ws_floats, top_k, top_p, logp,
                               logits, allow, nullptr, stream);
}
int inet_arnn_sample_ex(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                        int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                        const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                        const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                        int64_t* tokens, float* ws, int64_t ws_floats, int top_k, double top_p, float* logp, float* logits,
                        void* stream) {
    return inet_arnn_sample_cx(R, L, E, Hc, H, U, V, emb, oc0, oc_row_stride, oc_batch_stride, W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1,
                               W_hh1, b_hh1, W1, b1, W2, b2, temperature, uniforms, hc_init, tokens, ws, ws_floats, top_k, top_p, logp,
                               logits, nullptr, stream);
}
int inet_arnn_sample(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                     int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                     const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                     const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                     int64_t* tokens, float* ws, int64_t ws_floats, void* stream) {
    return inet_arnn_sample_ex(R, L, E, Hc, H, U, V, emb, oc0, oc_row_stride, oc_batch_stride, W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1,
                               W_hh1, b_hh1, W1, b1, W2, b2, temperature, uniforms, hc_init, tokens, ws, ws_floats, 0, 1.0, nullptr,
                               nullptr, stream);
}
int inet_lstm2_bwd(int B, int T, int H, const float* W_hh0, const float* W_ih1, const float* W_hh1, const float* out0,
                   const float* out1, const float* dout1, int reverse, float* dgi0, float* dgi1, float* dout0,
                   float* dW_hh0, float* db_ih0, float* db_hh0, float* dW_ih1, float* dW_hh1, float* db_ih1, float* db_hh1,
                   void* ws0, void* ws1, int64_t ws_bytes, void* stream) {
    if (B <= 0 || T <= 0 || H <= 0 || H % 16 || !W_hh0 || !W_ih1 || !W_hh1 || !out0 || !out1 || !dout1 || !dgi0 || !dgi1 ||
        !dout0 || !ws0 || !ws1 || ws0 == ws1)
        return -1;
    const int given = (dW_hh0 != nullptr) + (db_ih0 != nullptr) + (db_hh0 != nullptr) + (dW_ih1 != nullptr) +
                      (dW_hh1 != nullptr) + (db_ih1 != nullptr) + (db_hh1 != nullptr);
    if (given != 0 && given != 7) return -1;
    if (ws_bytes < (int64_t)lstm_ws_bytes(B, T, H, 1)) return -1;
    return lstm2_seq_bwd(B, T, H, W_hh0, W_ih1, W_hh1, out0, out1, dout1, reverse, dgi0, dgi1, dout0, dW_hh0, db_ih0, db_hh0,
                         dW_ih1, dW_hh1, db_ih1, db_hh1, ws0, ws1, (hipStream_t)stream);
}
int inet_embedding_fwd(const float* table, const int64_t* idx, int64_t rows, int E, float* out, const float* row_scale,
                       void* stream) {
    if (!table || !idx || !out || rows <= 0 || E <= 0) return -1;
    return pw_embedding_fwd(table, (const long long*)idx, rows, E, out, row_scale, (hipStream_t)stream);
}
int inet_embedding_bwd(const float* dout, const int64_t* idx, int64_t rows, int E, float* dtable, const float* row_scale,
                       int num_embeddings, void* stream) {
    if (!dout || !idx || !dtable || rows <= 0 || E <= 0 || num_embeddings < 0) return -1;
    hipStream_t ss = side_fork((hipStream_t)stream);        // leaf work: nothing downstream reads an embedding's gradient
    INET_TRY(pw_embedding_bwd(dout, (const long long*)idx, rows, E, dtable, row_scale, ss, num_embeddings));
    return side_join((hipStream_t)stream);
}
int inet_relu_bwd(const float* dy, const float* y, float* dpre, int64_t n, void* stream) {
    if (!dy || !y || !dpre || n <= 0) return -1;
    return pw_copy2d(dpre, n, dy, n, y, n, 1, (int)n, (hipStream_t)stream);
}
int inet_argmax(const float* w, int64_t ld, int rows, int V, int64_t* out, int64_t stride, void* stream) {
    if (!w || !out || rows <= 0 || V <= 0) return -1;
    return pw_argmax(w, ld, rows, V, (long long*)out, stride, (hipStream_t)stream);
}

int inet_tokens_to_i64(const int32_t* src, int64_t* dst, int64_t n, void* stream) {
    if (!src || !dst || n <= 0) return -1;
    return pw_tokens_i32_to_i64(src, (long long*)dst, n, (hipStream_t)stream);
}
int inet_split_score(const int32_t* score, int batch, int n_measures, int measure_len, int n_past, int n_target,
                     int64_t* past, int64_t* target, int64_t* future, void* stream) {
    if (!score || batch <= 0 || n_measures <= 0 || measure_len <= 0 || n_past < 0 || n_target < 0 ||
        n_past + n_target > n_measures)
        return -1;
    if ((n_past > 0 && !past) || (n_target > 0 && !target) || (n_measures - n_past - n_target > 0 && !future)) return -1;
    return pw_split_measures(score, batch, n_measures, measure_len, n_past, n_target, (long long*)past,
                             (long long*)target, (long long*)future, (hipStream_t)stream);
}

int inet_set_option(int key, int value) {
    if (key == 0) { side_set_enabled(value); return 0; }
    if (key == 1) { side_set_defer(value); return 0; }
    if (key == 4) { chain_set_enabled(value); return 0; }
    if (key == 2) { if (value < -1 || value > 4) return -1; gemm_set_force_cfg(value); return 0; }
    if (key == 3) { if (value < 0) return -1; gemm_set_force_split(value); return 0; }
    if (key == 5) { if (value < 0 || value > 4) return -1; gemm_set_direct(value); return 0; }
    if (key == 6) { chain_arm_fault(value); return 0; }
    if (key == 7) { if (value != 0 && value != 9) return -1; chain2_set_mode(value); return 0; }
    if (key == 8) { if (value != 0 && value != 9) return -1; bf3_set_mode(value); return 0; }
    if (key == 9) { if (value < 0 || value > 7) return -1; bf3_set_emit_mask(value); return 0; }
    // (keys 10, 11 -- which layers' weight gradients run on the bf16 pipe; the second-generation BPTT kernel -- were removed in round 4)
    if (key == 12) { gru_step_bf3_set_min_tiles(value); return 0; }
    if (key == 13) { if (value < 0 || value > 3) return -1; side_set_active(value); return 0; }
    if (key == 14) { if (value < 0 || value > 4) return -1; arnn_gen_set_mode(value); return 0; }
    if (key == 15) { if (value < 0 || value > 5) return -1; decode_b1_set_mode(value); return 0; }
    if (key == 16) {                                           // entry threshold of the slow-wait recorder, in polls (chain.h)
        unsigned* d = chain_dev_status();
        const unsigned polls = (unsigned)value;
        if (value < (int)chain::kSlowSpins || !d) return -1;
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(d + chain::kRecWord + 1, &polls, 4, hipMemcpyHostToDevice) != hipSuccess) return -2;
        return 0;
    }
    return -1;
}

int inet_chain_status(int reset) {
    unsigned* p = chain_host_status();
    if (!p) return -2;
    const int v = (int)__atomic_load_n(p, __ATOMIC_RELAXED);
    if (reset && v != 0 && chain_status_reset() != 0) return -2;   // (device-side twin too: needs the device idle)
    return v;
}

int inet_debug_read(void* dst, int64_t nbytes) {
    unsigned* d = chain_dev_status();
    if (!dst || nbytes <= 0 || nbytes > kChainDiagBytes || !d) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    return hipMemcpy(dst, d + kChainDiagWord, (size_t)nbytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}

int inet_slow_waits(unsigned* dst, int max_entries, int reset, int64_t* noted) {
    unsigned* d = chain_dev_status();
    if (!d || max_entries < 0 || (max_entries > 0 && !dst)) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    unsigned head[3] = {0, 0, 0};                             // waits noted, entry threshold, slow waits
    if (hipMemcpy(head, d + chain::kRecWord, sizeof head, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    if (noted) *noted = (int64_t)head[0];
    const unsigned slow = head[2];
    const int have = (int)(slow < (unsigned)chain::kRecEntries ? slow : (unsigned)chain::kRecEntries);
    const int n = have < max_entries ? have : max_entries;
    if (n > 0 && hipMemcpy(dst, d + chain::kRecWord + 8, (size_t)n * 32, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    if (reset && head[0] != 0) {                              // (the threshold, word 1, stays)
        if (hipMemset(d + chain::kRecWord, 0, 4) != hipSuccess ||
            hipMemset(d + chain::kRecWord + 2, 0, 4 * (size_t)(chain::kRecWords - 2)) != hipSuccess) return -2;
    }
    return (int)(slow > 0x7fffffffu ? 0x7fffffffu : slow);
}

int inet_decode_b1_plan(int B, int V, int Z, int* out8) { return decode_b1_plan_check(B, V, Z, out8); }
int inet_decode_b1_plan_sample(int B, int V, int Z, int* out8) { return decode_b1_plan_check(B, V, Z, out8, 1); }
int inet_decode_b1_plan_trunc(int B, int V, int Z, int* out8) { return decode_b1_plan_check(B, V, Z, out8, 2); }
int inet_vae_decoder_route(const inet_vae_config* cfg, int batch, int save, int teacher_forced, int flags, int level, int32_t* out, int n_out) {
    if (!cfg_ok(cfg) || batch <= 0 || flags < 0 || flags > 7) return -1;
    return vae_decoder_route(*cfg, batch, save, teacher_forced, flags, level, out, n_out);
}

namespace {
// the arguments of a product as the planners read them (shape, layout, leading dimensions, modes; no operand is touched)
bool plan_args(int64_t akm, int64_t bkm, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t has_bias, int64_t epi,
               int64_t acc, GemmArgs* g) {
    static const float some_bias = 0.f;
    if (M <= 0 || N <= 0 || K <= 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX || epi < 0 || epi > 5 || acc < 0 || acc > 1) return false;
    *g = gemm_args(nullptr, lda, akm != 0, nullptr, ldb, bkm != 0, nullptr, N, (int)M, (int)N, (int)K, has_bias ? &some_bias : nullptr,
                   (int)epi, nullptr, 0, (int)acc);
    return true;
}
void plan_out(const GemmPlan& p, int repeat, int products, int32_t* out, double* work, char* label, int cap) {
    const int32_t v[16] = {p.family, p.cfg, p.tile_m, p.tile_n, p.splits, p.k_per_split, p.tiles_n, p.tiles, (int32_t)p.grid.x,
                           (int32_t)p.grid.y, (int32_t)p.grid.z, p.zero_fill, p.two_pass, repeat * (1 + p.zero_fill + p.two_pass),
                           products, 0};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
    work[0] = p.flops; work[1] = p.bytes;
    std::snprintf(label, (size_t)cap, "%s", p.label);
}
}  // namespace

int inet_gemm_plan(int a_kmajor, int b_kmajor, int M, int N, int K, int64_t lda, int64_t ldb, int has_bias, int epi, int acc,
                   int nbatch, int32_t* out16, double* work2, char* label, int cap) {
    GemmArgs g;
    if (!out16 || !work2 || !label || cap <= 0 || nbatch < 1 || nbatch > 8) return -1;
    if (!plan_args(a_kmajor, b_kmajor, M, N, K, lda, ldb, has_bias, epi, acc, &g)) return -1;
    if (nbatch > 1 && (has_bias || epi != EPI_NONE || acc != ACC_ADD)) return -1;       // (what inet_gemm_batched computes)
    g.nbatch = nbatch;
    GemmPlan p = gemm_plan(g);
    const bool each = p.family == GEMM_EACH;
    if (each) { g.nbatch = 0; p = gemm_plan(g); }
    plan_out(p, each ? nbatch : 1, each ? nbatch : 1, out16, work2, label, cap);
    return 0;
}

int inet_gemm_group_plan(int n, const int64_t* desc, int32_t* out, double* work, char* label, int cap) {
    GemmArgs list[kGemmGroupMax];
    if (n < 1 || n > kGemmGroupMax || !desc || !out || !work || !label || cap <= 0) return -1;
    for (int i = 0; i < n; ++i) {
        const int64_t* d = desc + 10 * i;
        if (!plan_args(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], &list[i])) return -1;
    }
    const GemmPlan p = gemm_group_plan(list, n);
    if (p.family != GEMM_EACH) { plan_out(p, 1, 1, out, work, label, cap); return 0; }
    for (int i = 0; i < n; ++i) plan_out(gemm_plan(list[i]), 1, n, out + 16 * i, work + 2 * i, label + (size_t)cap * i, cap);
    return 0;
}

int inet_gru_chain_plan(int H, int B, int T, int nprob, int save, int64_t* out32) {
    if (H <= 0 || B <= 0 || T <= 0 || nprob < 1 || nprob > 4 || !out32) return -1;
    const auto put = [&](int64_t* o, const GruLayerPlan& p, int K) {
        const int64_t v[16] = {p.route, p.rows, p.launches, p.b.gen, p.b.MS, p.b.SQ, p.b.OCC, p.b.EMR, p.two_at_a_time, p.ring, p.groups,
                               p.members, p.ring_floats, (int64_t)chain_ring_floats(B, K), chain_capacity(), kChainMaxGroups};
        for (int i = 0; i < 16; ++i) o[i] = v[i];
    };
    put(out32, gru_layer_fwd_plan(H, B, T, nprob, save != 0, true, true, true), H);
    if (save) put(out32 + 16, gru_layer_bwd_plan(H, B, T, nprob, true, true, true), 3 * H);
    else for (int i = 16; i < 32; ++i) out32[i] = -1;
    return 0;
}

int inet_lstm_chain_plan(int B, int T, int H, int pipeline, int64_t* out) {
    if (B < 1 || T < 1 || H < 1 || !out) return -1;
    const LstmChainPlan p = lstm_chain_plan(B, T, H, pipeline ? 2 : 1);
    const int64_t v[16] = {p.ok, p.ms, p.groups, p.members, p.workgroups, p.blocks, p.tagged, p.chunk, p.chunks, p.areas, p.capacity,
                           p.side_by_side, p.max_groups, p.counter_stride, p.counter_words, 0};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
    return 0;
}

int inet_preload(void) { return preload_kernels(); }
int inet_kernel_count(void) { return preload_kernel_count(); }

int inet_side_join(void* stream) { return side_join_now((hipStream_t)stream); }
int inet_side_wait(void* stream) { return side_wait_on((hipStream_t)stream); }
int inet_twin_stream(void** stream) {
    if (!stream) return -1;
    *stream = (void*)twin_stream();
    return *stream ? 0 : -2;
}

int inet_gru_step(int B, int H, const float* gi, const float* h_prev, const float* W_hh, const float* b_hh,
                  float* h_new, float* sv5, void* stream) {
    if (B <= 0 || H <= 0 || H % 16 || !gi || !h_prev || !W_hh || !b_hh || !h_new) return -1;
    GruFwdBatch bt{};
    bt.H = H; bt.nprob = 1;
    GruFwdProb& P = bt.p[0];
    P.B = B; P.h_prev = h_prev; P.ld_hprev = H; P.W_hh = W_hh; P.b_hh = b_hh;
    P.gi_dense = gi; P.ld_gi = 3L * H; P.h_new = h_new; P.ld_hnew = H;
    if (sv5) {
        const long as = (long)B * H;
        P.sv_r = sv5; P.sv_z = sv5 + as; P.sv_n = sv5 + 2 * as; P.sv_ghn = sv5 + 3 * as; P.sv_hprev = sv5 + 4 * as;
    }
    return launch_gru_fwd(bt, (hipStream_t)stream);
}

}  // extern "C"
