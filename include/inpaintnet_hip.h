/* inpaintnet_hip.h -- C ABI of the MI355X (gfx950) InpaintNet hot path.
 *
 * Drop-in boundary.  The reference has no FFI: its callers see Python classes
 * (SURVEY.md section 8b).  This header is the C-ABI the repo introduces
 * UNDERNEATH those classes; each entry point cites the reference method whose
 * arithmetic it replaces.  The modules of inpaintnet_amd/ bind it with ctypes and expose
 * the reference's own signatures (MeasureVAE.forward, LatentRNN.forward,
 * Trainer.step ...); INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    stated; the caller owns all memory (parameters, gradients, optimizer
 *    state, workspaces, outputs).  The library never allocates device memory.
 *  - all floating point is fp32; token tensors are int64 (as produced by
 *    utils/helpers.py:17-26 to_cuda_variable_long).
 *  - calls are asynchronous on `stream` (a hipStream_t passed as void*).
 *  - return value: 0 = ok, -1 = invalid argument, -2 = launch/runtime failure, -3 = a *_bwd call on a workspace whose forward
 *    call ran under other library options (inet_set_option keys 4, 7, 8, 9, 12: they decide which kernels run and which piece
 *    buffers exist).
 *  - parameters live in ONE flat fp32 arena per model, laid out in the
 *    reference's state_dict() order; gradients / Adam
 *    moments use arenas of identical layout.  inet_*_param_info() is the
 *    single description of that layout.
 *  - a workspace written by a *_fwd call with save=1 must be handed unchanged to
 *    the matching *_bwd call; every call checks ws_bytes against *_ws_bytes() and
 *    returns -1 rather than touching an undersized workspace.
 */
#ifndef INPAINTNET_HIP_H
#define INPAINTNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INET_ABI_VERSION 1

typedef struct inet_vae_config {
    int32_t num_notes;      /* V  = len(dataset.note2index_dicts[0])   measure_vae.py:56   */
    int32_t emb_dim;        /* E  note_embedding_dim (10)              measure_vae.py:13   */
    int32_t enc_hidden;     /* encoder_hidden_size (512); 2 layers, bidirectional          */
    int32_t z_dim;          /* latent_space_dim (256)                                      */
    int32_t dec_hidden;     /* decoder_hidden_size (512); 2 layers                         */
    int32_t beats;          /* 4, hard-coded at decoder.py:446                             */
    int32_t ticks_per_beat; /* 6, hard-coded at decoder.py:450                             */
} inet_vae_config;

typedef struct inet_latent_config {
    int32_t z_dim;          /* vae_model.latent_space_dim                latent_rnn.py:48  */
    int32_t rnn_hidden;     /* rnn_hidden_size (512): context GRUs; generator uses 2x      */
    int32_t auto_reg;       /* generator input = z (1) or the scalar x_0 (0)  :70-74       */
} inet_latent_config;

int inet_abi_version(void);

/* ---- parameter arena layout -------------------------------------------------------- */
/* MeasureVAE state_dict (encoder.* then decoder.*), MeasureVAE/encoder.py:28-52, decoder.py:335-372 */
int     inet_vae_param_count(const inet_vae_config* cfg);
int64_t inet_vae_param_floats(const inet_vae_config* cfg);
/* name: caller buffer; dims: int64[4]; returns 0 or -1 */
int     inet_vae_param_info(const inet_vae_config* cfg, int index, char* name, int name_cap,
                            int64_t* offset_floats, int64_t* dims, int* ndim);
/* trainable LatentRNN parameters (context_rnn_past/future, generation_rnn, generation_linear, x_0),
 * LatentRNN/latent_rnn.py:53-83 */
int     inet_latent_param_count(const inet_latent_config* cfg);
int64_t inet_latent_param_floats(const inet_latent_config* cfg);
int     inet_latent_param_info(const inet_latent_config* cfg, int index, char* name, int name_cap,
                               int64_t* offset_floats, int64_t* dims, int* ndim);

/* ---- MeasureVAE encoder: Encoder.forward, MeasureVAE/encoder.py:104-134 -------------- */
int64_t inet_vae_encoder_ws_bytes(const inet_vae_config* cfg, int batch, int save);
/* tokens [B,T] int64 row-major (T = beats*ticks_per_beat); params: VAE arena;
 * mask: null, or [T,B,2H] fp32 pre-scaled {0,1/(1-p)} inter-layer dropout mask (time-major);
 * outputs mu, logsigma [B,Z] */
int inet_vae_encoder_fwd(const inet_vae_config* cfg, int batch, const int64_t* tokens, const float* params,
                         const float* mask, float* mu, float* logsigma, void* ws, int64_t ws_bytes, int save,
                         void* stream);
/* autograd of the above (utils/trainer.py:150 loss.backward): accumulates into `grads` (VAE arena layout).
 * stage 0 = the whole pass.  A data-parallel caller may split it: stage 1 = Linear heads + GRU layer 1 (afterwards the
 * arena ranges [weight_ih_l1, note_embedding) and [linear_mean.0.weight, end of the encoder) are final and their
 * all-reduce can start), then stage 2 = GRU layer 0 + embedding on the same `ws`. */
int inet_vae_encoder_bwd(const inet_vae_config* cfg, int batch, const int64_t* tokens, const float* params,
                         float* grads, const float* mask, const float* dmu, const float* dlogsigma, void* ws,
                         int64_t ws_bytes, int stage, void* stream);

/* ---- MeasureVAE decoder: HierarchicalDecoder.forward, MeasureVAE/decoder.py:412-529 -- */
int64_t inet_vae_decoder_ws_bytes(const inet_vae_config* cfg, int batch, int save);
/* z [B,Z]; target [B,T] int64 (read iff teacher_forced); mask_beat [beats,B,H], mask_tick [T,B,H] or null;
 * weights [B,T,V] post-ReLU logits; samples [B,1,T] int64 (= target if teacher forced; else argmax, lowest index on
 * ties, or -- multinomial_seed != 0, decoder.py:506-509 sampling = 'multinomial' -- one draw per tick and row from
 * softmax(weights) with a counter-based generator keyed (multinomial_seed, tick * B + row)) */
int inet_vae_decoder_fwd(const inet_vae_config* cfg, int batch, const float* z, const int64_t* target,
                         int teacher_forced, const float* params, const float* mask_beat, const float* mask_tick,
                         float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                         uint64_t multinomial_seed, void* stream);
/* The free-running decode with TEMPERATURE SAMPLING: inet_vae_decoder_fwd's arguments without target, teacher_forced and
 * multinomial_seed, plus the temperature and one uniform per (row, tick), uniforms [B,T] doubles on the device (row-major).  For
 * tick t of row b, with x = weights[b,t,:] (the post-ReLU logits, unchanged): s = temperature * x in f32, e_v = expf(s_v - max s),
 * inclusive prefix in f64; samples[b,0,t] = the first v with prefix_v > uniforms[b,t] * total (np.random.choice's order, the rule of
 * inet_arnn_sample) -- the token that is fed back into tick t + 1.  Where the rule does not apply (max s or the total not finite, a
 * NaN among s, a uniform outside [0, 1) or NaN) the tick takes the argmax, lowest index among equals.  Tokens always lie in [0, V).
 * One to sixteen rows with H = 512, V <= 128, no tick mask and save = 0 run as ONE register-resident launch (csrc/decode_b1.hip, its
 * sampling build; inet_decode_b1_plan_sample); every other shape runs tick by tick with inet_sample_temperature's kernel behind each
 * output projection.  A sampled call never runs a kernel that ignores its uniforms: the launch labels of the profile start with
 * "sample_" (sample_decode_b1..., sample_temperature ...).  -1: a null pointer, a non-finite temperature, V > 512, a workspace
 * smaller than inet_vae_decoder_ws_bytes(cfg, batch, save). */
int inet_vae_decoder_sample(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                            const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                            float temperature, const double* uniforms, void* stream);
/* The same behind TOP-K / NUCLEUS TRUNCATION, with the drawn tokens' log-probabilities.  For one (row, tick), with s, m = max s and
 * e_v = expf(s_v - m) as above:  order the tokens by (s_v descending, v ascending) -- over s, not x: the temperature may be negative;
 * every zero logit ties with every other, and the lowest index ranks first --;  K = top_k if 1 <= top_k < V, else V (top_k <= 0 or
 * >= V: off);  A_i = the f64 sum of e over the first i tokens of the order;  n = the smallest i <= K with A_i >= top_p * A_K (the
 * nucleus is taken of what top-k kept; top_p = 1: n = K, nothing evaluated; n >= 1 always).  The first n tokens of the order are
 * kept, and samples[b,0,t] = the first v in INDEX order among the kept whose inclusive f64 prefix of kept e exceeds uniforms[b,t] * S,
 * S = the kept total: inet_vae_decoder_sample's rule on the truncated distribution, and with truncation off that rule bit for bit.
 * logp (nullable; [B,T] floats on the device) receives (s_tok - m) - log(S) as f32, the drawn token's log-probability under the
 * truncated distribution.  Where the sampling rule does not apply the tick takes the argmax as above and its logp is NaN.
 * top_k = 1 with temperature > 0 is the argmax decode for any uniforms in [0, 1).  inet_vae_decoder_sample is this call with
 * (top_k, top_p, logp) = (0, 1.0, null) and runs the kernels it always ran; a call with truncation on or a logp runs the truncating
 * build of the register-resident launch (inet_decode_b1_plan_trunc) or, for every other shape, inet_sample_truncated's kernel tick
 * by tick, and never a kernel that ignores top_k / top_p: its launch labels start with "trunc_" (trunc_decode_b1..., trunc_sample ...).
 * -1 where inet_vae_decoder_sample returns it, and for a top_p that is NaN, <= 0 or > 1. */
int inet_vae_decoder_sample_ex(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                               const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                               float temperature, const double* uniforms, int top_k, double top_p, float* logp, void* stream);
/* The same behind PER-TICK TOKEN CONSTRAINTS: a mask of allowed tokens per (row, tick), applied in front of the truncated rule inside the
 * launch (the token of tick t is fed back into tick t + 1 there; csrc/sample.h).
 * Mask layout.  `allow` is an array of 64-bit words [rows][T][NW], with NW = ceil(V / 64).  Token v is allowed iff bit v % 64 of word
 * v / 64 is set.  Bits at or above V are ignored.  A null `allow` means no constraint.
 * For one (row, tick), with logits x[0..V), temperature T, uniform u, top_k and top_p:
 *  0. Empty mask.  A mask with no bit set in [0, V) counts as all ones for that tick.  The Python surfaces refuse such a tick with
 *     ValueError before any launch.
 *  1. Scores.  s_v = T x_v in f32.  The NaN test of section 10 runs over all V values of s, as today.  The mask therefore does not
 *     change which ticks fall back.  Then s_v = -inf for every banned v, and m = the maximum over the allowed tokens.
 *  2. Truncation and draw.  Steps 2-7 of section 11 run unchanged on these s, with V and K = top_k unchanged.  Banned tokens tie at
 *     -inf and rank last.  Their e = expf(-inf - m) is 0, so they add no mass and cannot be the first prefix above u S.  A top_k above
 *     the number of allowed tokens keeps all of them.  logp is taken under the masked and truncated distribution.
 *  3. Fallback.  Where the rule does not apply (a NaN among s, m or S not finite, u outside [0, 1) or NaN), the tick takes today's
 *     argmax rule on the logits with every banned entry replaced by -inf.  The decode kernel may use its padding value -1 instead,
 *     which lies below every post-ReLU logit.  logp is NaN there.  The token is still an allowed one.
 * (Sections 10 and 11 of DESIGN.md: the sampling rule of inet_vae_decoder_sample and the truncated rule of inet_vae_decoder_sample_ex.)
 * Consequences: a null mask or a mask of all ones gives inet_vae_decoder_sample_ex bit for bit (tokens, logits, logp); a one-bit mask
 * returns that token for every u and every finite T, with logp exactly 0 (NaN on a fallback tick); no banned token is ever returned;
 * for T > 0 the masked draw on x equals the unmasked draw on x with -inf written at the banned places.
 * allow: [B][T][NW] words on the device, or null -- then this IS inet_vae_decoder_sample_ex.  A constrained call runs the masked build
 * of the register-resident launch (the truncated call's plan: inet_decode_b1_plan_trunc) or, for every other shape,
 * inet_sample_constrained's kernel tick by tick: its launch labels start with "cons_" (cons_decode_b1..., cons_sample ...).
 * -1 where inet_vae_decoder_sample_ex returns it, and for a mask with more than 64 ticks. */
int inet_vae_decoder_sample_cx(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                               const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                               float temperature, const double* uniforms, int top_k, double top_p, float* logp,
                               const uint64_t* allow, void* stream);
/* The same with FORCED TOKENS: a per-(row, tick) token that is fed back like a drawn one and whose log-probability is taken under the same
 * masked and truncated distribution a draw would have used (csrc/sample.h).  Every tick forced: the call scores a given
 * filling (a teacher-forced evaluation pass inside the one launch); the first ticks forced: it continues a prefix.
 * Layout.
 *  - `forced` is an array of `int32` `[rows][T]`.
 *  - A value `f` with `0 <= f < V` forces that tick.
 *  - Every other value makes the tick free.  The Python surfaces write -1 for a free tick.
 *  - A null `forced` means no tick is forced.
 * At a free tick nothing changes.  Section 13's rule runs as it does today.
 * At a forced tick with token `f`:
 *  1. Scores and truncation.
 *     - Steps 0-2 of section 13 run unchanged on the tick's logits: s = T x in f32, the NaN test, the mask, m, and the top-k / nucleus
 *       truncation.
 *     - S is the kept total.
 *     - The tick's uniform is not used.  The rule is evaluated as with u = 0, so a uniform outside [0, 1) or NaN at a forced tick
 *       causes no fallback.
 *  2. Token.
 *     - The token is `f`.  It is reported in `samples` and fed back into tick t + 1.
 *     - This holds whether or not `f` is allowed or kept, and it holds on a fallback tick too.
 *  3. Log-probability.  logp = (s_f - m) - log S as f32.
 *     - It is exactly -inf when `f` is banned or truncated away (s_f = -inf).
 *     - It is NaN where the rule does not apply: a NaN among s, or m or S not finite.
 * Consequences.  The tests hold each of these exactly.
 *  (a) No forced tick.  A null `forced`, or one with no value in [0, V), gives inet_vae_decoder_sample_cx bit for bit in tokens, logits
 *      and logp.
 *  (b) Replay.  Force, at every tick, the tokens that a sampled, truncated or constrained call returned.  The replay uses the same
 *      temperature, top_k, top_p and mask, and any uniforms at all.  It returns that call's logits and logp bit for bit, with NaN where
 *      that call had NaN.
 *  (c) A banned forced token is still returned and fed back.  Its logp is -inf.
 *  (d) One-bit mask.  A forced tick whose mask has the single bit `f` set has logp exactly 0.0f.
 *  (e) Free ticks of a partly forced call follow section 13's rule on the trajectory behind the forced tokens.
 * forced: [B][T] int32 on the device, or null -- then this IS inet_vae_decoder_sample_cx.  allow may be null beside it (a mask of all
 * ones).  A forced call runs the forced build of the register-resident launch (the constrained call's plan: inet_decode_b1_plan_trunc) or,
 * for every other shape, inet_sample_forced's kernel tick by tick: its launch labels start with "force_" (force_decode_b1...,
 * force_sample ...).  -1 where inet_vae_decoder_sample_cx returns it. */
int inet_vae_decoder_sample_fx(const inet_vae_config* cfg, int batch, const float* z, const float* params, const float* mask_beat,
                               const float* mask_tick, float* weights, int64_t* samples, void* ws, int64_t ws_bytes, int save,
                               float temperature, const double* uniforms, int top_k, double top_p, float* logp,
                               const uint64_t* allow, const int32_t* forced, void* stream);
/* dweights [B,T,V] = dLoss/dweights; weights = the forward output; grads may be null (frozen decoder:
 * LatentRNN/latent_rnn.py:42-43) in which case only dz [B,Z] is produced.  `tokens_in` are the tokens that
 * were fed back (= samples of the forward call). */
int inet_vae_decoder_bwd(const inet_vae_config* cfg, int batch, const float* dweights, const float* weights,
                         const int64_t* tokens_in, const float* params, float* grads, const float* mask_beat,
                         const float* mask_tick, float* dz, void* ws, int64_t ws_bytes, void* stream);

/* Test hook: float offset and element count of a named intermediate inside a workspace written with save=1.
 * which 0 = encoder workspace: "a_mu", "a_ls" [B,2H] (SELU outputs of linear_mean.0 / linear_log_std.0, encoder.py:36-52);
 * which 1 = decoder workspace: "hb0" [B,2H] (z_to_beat_rnn_input), "ht0" [beats,B,2H] (beat_emb_to_tick_rnn_hidden),
 * "c_all" [beats,B,H] (beat_emb_to_tick_rnn_input), decoder.py:335-372.  Parity tests read the sign of these SELU outputs
 * to align the derivative branch of near-zero pre-activations with the oracle's. */
int inet_vae_ws_field(const inet_vae_config* cfg, int batch, int which, const char* name, int64_t* offset_floats,
                      int64_t* count);

/* ---- losses: VAETrainer.loss_and_acc_for_batch, vae_trainer.py:16-40,128-139; utils/trainer.py:271-306 */
/* rows of V logits (row stride ld_w); *loss_sum += out_scale * sum_rows (lse - w[target]); *correct += out_scale *
 * #correct (argmax_first: the rule of inet_argmax, NaN included) -- out_scale = 1/rows gives the reference's means without a
 * follow-up kernel; dW (nullable, row stride ld_dw) = (softmax - onehot) * scale.  Targets must lie in [0, V). */
int inet_cross_entropy(const float* weights, int64_t ld_w, int rows, int V, const int64_t* targets, float* dW,
                       int64_t ld_dw, float scale, float out_scale, float* loss_sum, float* correct, void* stream);
/* The same with the glue of VAETrainer.loss_and_acc_for_batch (vae_trainer.py:29-40) folded in: loss_sum / correct may be
 * null (gradient-only call); dW is additionally multiplied by the device scalar scale_dev[0] when given (the upstream
 * gradient of the loss, so that autograd's backward needs no elementwise pass over dW); *loss_sum also receives
 * add_scale * add_term[0] once when add_term is given (the KL term: loss = CE + beta/B * KL complete in one launch);
 * fwd_out[0] = fwd_scale * scale_dev[0] when given (the gradient to hand on to the producer of add_term). */
int inet_cross_entropy_ex(const float* weights, int64_t ld_w, int rows, int V, const int64_t* targets, float* dW,
                          int64_t ld_dw, float scale, const float* scale_dev, float out_scale, float* loss_sum,
                          float* correct, const float* add_term, float add_scale, float* fwd_out, float fwd_scale,
                          void* stream);
/* z = mu + eps*exp(logsigma) (measure_vae.py:119); sigma out (nullable); kl_sum += sum(0.5(s^2+mu^2-1) - ls) */
int inet_reparam_kl(const float* mu, const float* logsigma, const float* eps, float* z, float* sigma, int64_t n,
                    float* kl_sum, void* stream);
/* dmu = dz + k*mu; dlogsigma = dz*eps*sigma + k*(sigma^2-1), k = kscale * (kscale_dev ? *kscale_dev : 1): the gradient of
 * z (dz, nullable) and of the KL sum (a device scalar from autograd, nullable) in one pass */
int inet_latent_bwd(const float* dz, const float* mu, const float* logsigma, const float* eps, float kscale,
                    const float* kscale_dev, float* dmu, float* dlogsigma, int64_t n, void* stream);

/* The KL term with a floor ("free bits").  mu, logsigma [rows, Z] contiguous; KL[b,d] = 0.5(s^2 + mu^2 - 1) - ls.
 * per = 0 ('measure'): part[b] = sum_d KL[b,d], rows parts, thr = free_nats.  per = 1 ('dim'): part[d] = sum_b KL[b,d], Z parts,
 * thr = (float)(rows * free_nats).  kept = !(part <= thr): a tie is floored, a NaN part is kept.  Writes z = mu + eps*exp(logsigma)
 * (z nullable; eps nullable, read as 0), parts[] and keep[] (1.0f / 0.0f); *kl_sum += sum(kept ? part : thr); *kl_raw += sum(part).
 * Every sum -- the parts and the two scalars -- is added in a fixed order, without float atomics: the same inputs give the same parts,
 * keep bits and scalars in every run, and with every part kept the amounts added onto kl_sum and kl_raw are the same bits.  Two
 * launches: the elementwise pass, then one finishing workgroup (the floor and the scalars; for per = 1 also the column sums, from the
 * first launch's per-workgroup partials in `ws`: inet_reparam_kl_fb_ws_bytes(rows, Z, per) bytes of device memory, nothing to zero;
 * 0 for per = 0, when ws may be null).  16-byte loads when Z % 4 == 0 and mu, logsigma, eps and z are 16-byte aligned.  -1: a null required pointer, rows <= 0, Z <= 0, free_nats negative, NaN or inf, per outside {0, 1},
 * ws_bytes too small -- before any launch. */
int64_t inet_reparam_kl_fb_ws_bytes(int64_t rows, int Z, int per);
int inet_reparam_kl_fb(const float* mu, const float* logsigma, const float* eps, float* z, int64_t rows, int Z, float free_nats,
                       int per, float* parts, float* keep, float* kl_sum, float* kl_raw, void* ws, int64_t ws_bytes, void* stream);
/* inet_latent_bwd with the keep vector inet_reparam_kl_fb left: the KL gradient reaches an element only where its part (row for
 * per = 0, column for per = 1) is kept -- k or 0 is SELECTED per element: dmu = dz + kk*mu; dlogsigma = dz*eps*sigma + kk*(sigma^2-1).
 * With every part kept the results are inet_latent_bwd's bit for bit; a floored part hands dz on bit for bit. */
int inet_latent_bwd_fb(const float* dz, const float* mu, const float* logsigma, const float* eps, float kscale,
                       const float* kscale_dev, const float* keep, int per, float* dmu, float* dlogsigma, int64_t rows, int Z,
                       void* stream);

/* The MMD (InfoVAE / WAE-MMD) latent loss between two samples.  x (z_tilde), y (z_prior) [B, Z] contiguous;
 * d(u,v) = sum_z (u_z - v_z)^2; kind 0 'gaussian': k = exp(-d / var), 1 'imq': k = var / (var + d); S_xx, S_yy, S_xy = the sums of k
 * over all B^2 pairs, diagonals included.  out4 = {coeff (a (S_xx - diag B) + a (S_yy - diag B) - c S_xy), S_xx, S_yy, S_xy};
 * grad (nullable: the value only) [B, Z] = d out4[0] / d x.  The estimator is the caller's (a, c, diag): unbiased (1/(B(B-1)), 2/B^2,
 * 1), biased (1/B^2, 2/B^2, 0), the reference's (1/(B(B-1))/2, 2/B^2, 0).  A distance is a sum of squared differences in a fixed
 * order, so a diagonal kernel value is exactly 1; no float atomics: the same inputs give the same bits in out4 and grad.  Two
 * launches (pair, finish) through `ws`: inet_mmd_ws_bytes(B, Z) bytes of device memory, nothing to zero.  x and y may be the same
 * memory; 4-byte alignment suffices.  -1: a null x, y or out4, B < 1, B > 2^24, Z < 1, var not finite or <= 0, a, c, diag or coeff not
 * finite, kind outside {0, 1}, ws null or ws_bytes too small -- before any launch. */
int64_t inet_mmd_ws_bytes(int64_t B, int Z);
int inet_mmd(const float* x, const float* y, int64_t B, int Z, int kind, float var, double a, double c, double diag, double coeff,
             float* out4, float* grad, void* ws, int64_t ws_bytes, void* stream);

/* Attribute-regularised latent dimensions (AR-VAE, Pati & Lerch 2020).
 *
 * inet_measure_attrs: tokens [B, T] int64 -> out [B, 4] float32, the columns (num_notes, note_range, rhy_entropy, beat_strength) of the
 * reference's dataset (folk_dataset.py:607-708), each ONE float operation on ONE exact integer, so that equal attributes are equal bits:
 *   num_notes     = (T - #slur - #rest) / T
 *   note_range    = (max midi - min midi) / (midi_hi - midi_lo) over the row's pitched tokens (not slur, rest or None, midi[token] >= 0);
 *                   0 for a row with none -- per ROW (the reference never resets its has_note flag between rows)
 *   rhy_entropy   = logf(n), n = the number of non-slur ticks; 0 for n = 0 (the reference: NaN)
 *   beat_strength = (1000 n0 + 150 n3 + 8 nrest) / 1000, the non-slur ticks at t % 6 == 0, at t % 6 == 3 and elsewhere
 * V: the vocabulary; slur_index, rest_index, none_index: the three symbols, -1 = the vocabulary has none; midi: V device int32, -1 for
 * a token without a pitch.  A token outside [0, V) makes its row's four values NaN and never indexes the table.  One coalesced read of
 * the tokens, no atomics.  -1: a null pointer, B < 1, B > 2^24, V < 1, T not a positive multiple of 6 or > 96, an index outside
 * [-1, V), midi_hi <= midi_lo -- before any launch.
 *
 * inet_attr_reg: z [B, Z] float32; dims: A distinct latent dimensions (HOST ints), 1 <= A <= 8; attrs [B, A] float32, any attributes.
 * With x = z[:, dims[a]], t_ij = tanhf(delta (x_i - x_j)), s_ij = sgn(attrs[i, a] - attrs[j, a]), sgn(0) = 0:
 *   L_a = (1 / B^2) sum_ij |t_ij - s_ij|;   out[1 + A] = {coeff sum_a L_a, L_0, .., L_{A-1}}
 *   counts [A][3] int64 over ordered pairs i != j: concordant (s != 0 and sgn(x_i - x_j) == s), discordant (== -s), attribute-tied (s == 0)
 *   grad (nullable: the value only) [B, A] = d out[0] / d z[:, dims[a]] = (2 coeff delta / B^2) sum_j sgn(t_ij - s_ij) (1 - t_ij^2)
 * A NaN in z or attrs reaches the value.  No atomics, every float sum in an order that depends on (B, A) alone: the same inputs give
 * the same bits, and the value's bits do not depend on grad.  Two launches (pair, finish) through `ws`: inet_attr_reg_ws_bytes(B, A)
 * bytes of device memory, nothing to zero.  -1: a null z, dims, attrs, out or counts, B < 1, B > 2^24, Z < 1, A outside [1, 8], a
 * dimension outside [0, Z) or named twice, delta or coeff not finite, ws null or ws_bytes too small -- before any launch. */
int inet_measure_attrs(const int64_t* tokens, int64_t B, int T, int V, int slur_index, int rest_index, int none_index, const int32_t* midi,
                       int midi_lo, int midi_hi, float* out, void* stream);
int64_t inet_attr_reg_ws_bytes(int64_t B, int A);
int inet_attr_reg(const float* z, int64_t B, int Z, const int32_t* dims, int A, const float* attrs, float delta, double coeff, float* out,
                  int64_t* counts, float* grad, void* ws, int64_t ws_bytes, void* stream);

/* Class-weighted, label-smoothed cross-entropy with an ignore index, and per-class statistics.  The definition
 * is torch.nn.functional.cross_entropy(x, t, weight=w, label_smoothing=e, ignore_index=i, reduction='mean'):
 *   valid_r = t_r != i and 0 <= t_r < V;  p = softmax(x_r);  W = sum_c w_c;  denom = sum_valid w[t_r]
 *   loss = [(1 - e) sum_valid w[t_r] (lse_r - x_r[t_r]) + (e / V) sum_valid sum_c w_c (lse_r - x_r[c])] / denom
 *   dloss / dx_r[c] = valid_r [(1 - e) w[t_r] (p_c - 1{c = t_r}) + (e / V) (W p_c - w_c)] / denom
 * class_weight: V device floats (finite, >= 0; 0 is legal), null = all ones.  ignore_index: a HOST pointer, null = nothing is ignored.
 * ONE divergence from torch: with denom == 0 (every row ignored, or every present target has weight 0) the loss is NaN as torch's is,
 * but dW is ALL ZEROS (torch: zeros in the first case, NaN in the second).
 *
 * inet_class_counts: targets, n int64 on the device -> out, 8 + V + extra_words int64 words on the device, ALL zeroed
 * by the call (extra_words >= 0: room the caller wants zeroed along, such as the class_stats of the loss launch that follows):
 *   out[0] the bits of the double denom = sum_c w_c counts_c, added in class order: a pure function of the counts; out[1] n_valid;
 *   out[2] n_bad; out[5] the bits of the double W; out[3], out[4] tickets of the launches, 0 between calls; out[8 + c] counts[c].
 * Integer atomics only: the same bits on every call.  A target outside [0, V) that is not ignore_index is never used as an index: it
 * is treated as ignored, counted in n_bad, and the launch sets the token status word (inet_token_status), as a bad embedding index does.
 * -1: a null targets or out, n < 1, n > 2^40, V < 1, extra_words < 0.
 *
 * inet_cross_entropy_w: one wavefront per row of `weights` (row stride ld_w >= V; the padding is never read), the row read once.
 * meta: the block inet_class_counts left for the SAME targets, weights and ignore_index (denom, n_valid and W are read from it; the
 * backward reuses the forward's).  Outputs, each nullable, at least one given:
 *   dW [rows, ld_dw >= V] = dloss / dx [* scale_dev[0]], the padding never written; an ignored row is exactly 0
 *   loss[0] = the loss [+ add_scale * add_term[0]];  accuracy[0] = hits / n_valid over the valid rows, unweighted, argmax_first
 *     (inet_argmax's rule); both WRITTEN, not accumulated
 *   fwd_out[0] = fwd_scale * scale_dev[0] (needs scale_dev)
 *   class_stats [V, 3] int64 += {rows with this target, of those the hits, rows with this argmax}; confusion [V, V] int64 += 1 at
 *     [target, argmax]: the caller zeroes them, a loop over batches accumulates
 * With dW alone (the backward) there is no sum and no finishing pass.  Float sums go through one double partial per workgroup and the
 * workgroup that finishes last, which adds them in a fixed order that depends on rows alone: no float atomics, loss, accuracy and dW
 * have the same bits from call to call, the loss the same bits with or without dW.  Without class_weight, smoothing and ignored rows,
 * dW and the hit count are inet_cross_entropy_ex's bits (scale = 1 / rows).  ws: inet_cross_entropy_w_ws_bytes(rows) bytes, needed
 * for loss or accuracy, nothing to zero.  -1: a null weights, targets or meta, rows < 1, V < 1, no output, ld_w < V, ld_dw < V,
 * label_smoothing outside [0, 1], fwd_out without scale_dev, add_term without loss, ws missing or too small -- before any launch. */
int inet_class_counts(const int64_t* targets, int64_t n, int V, const float* class_weight, const int64_t* ignore_index, int64_t* out,
                      int64_t extra_words, void* stream);
int64_t inet_cross_entropy_w_ws_bytes(int rows);
int inet_cross_entropy_w(const float* weights, int64_t ld_w, int rows, int V, const int64_t* targets, const float* class_weight,
                         double label_smoothing, const int64_t* ignore_index, int64_t* meta, float* dW, int64_t ld_dw,
                         const float* scale_dev, float* loss, float* accuracy, const float* add_term, float add_scale, float* fwd_out,
                         float fwd_scale, int64_t* class_stats, int64_t* confusion, void* ws, int64_t ws_bytes, void* stream);

/* The importance-weighted log-likelihood of a measure: the IWAE bound of Burda et al. 2016.  For a measure x_b
 * (T = 24 tokens) the encoder gives mu_b, ls_b (log sigma), both [Z].  For k = 0..K-1 and eps[b,k,:] standard normal:
 *   z[b,k,d]   = mu[b,d] + eps[b,k,d] * exp(ls[b,d])
 *   logr[b,k]  = log p(z) - log q(z|x) = sum_d ( 0.5 eps^2 - 0.5 z^2 + ls[b,d] )     (the 2*pi terms cancel)
 *   nll[b,k]   = - sum_t log softmax(weights[b,k,t,:])[ x[b,t] ]
 *                (weights come from the decoder run on z[b,k] with x_b's own tokens fed back: teacher-forced, eval mode, no dropout)
 *   logw[b,k]  = logr[b,k] - nll[b,k]
 *   m = max_k logw;  s1 = sum_k exp(logw - m);  s2 = sum_k exp(2 (logw - m))
 *   iwae[b] = m + log(s1 / K)         lower bound on log p(x_b), tight as K grows
 *   elbo[b] = (sum_k logw) / K        the single-sample bound, averaged
 *   ess[b]  = s1^2 / s2               effective sample size, in [1, K]
 *   rec[b]  = (sum_k nll) / K
 *   kl[b]   = -(sum_k logr) / K, the Monte-Carlo KL, formed as -(sum_k logw + sum_k nll) / K: rec + kl = -elbo
 * A NaN anywhere in a measure's logw row: iwae, elbo and ess are all NaN.  m == -inf (every sample has zero weight): iwae = elbo =
 * -inf and ess = 0.  A +inf in the row: whatever IEEE gives (NaN).  No float atomics, every sum in a fixed order: two calls on the
 * same inputs give the same bits.  Every entry returns -1 for a bad argument before any launch, -2 for a failed launch.
 *
 * inet_iw_draw: one wavefront per row r = b * Kc + j of a chunk of Kc samples: reads mu + b Z, logsigma + b Z and eps + b *
 * eps_stride_b + j * Z (a chunk of a larger (B, K, Z) tensor needs no copy), writes z[r,:] ([B*Kc, Z] contiguous) and logr[r].  The
 * element is inet_reparam_kl's: expf, mu + eps * s.  16-byte loads and stores where Z % 4 == 0, eps_stride_b % 4 == 0 and mu,
 * logsigma, eps, z are 16-byte aligned (a lane adds the terms of d = 4 lane .. 4 lane + 3, then 256 further on), else a scalar path
 * (d = lane, lane + 64, ...); in both a lane adds in ascending d and a xor tree adds the lanes.  -1: a null pointer, B, Kc or Z < 1,
 * B * Kc > 2^24, eps_stride_b < Kc * Z. */
int inet_iw_draw(const float* mu, const float* logsigma, const float* eps, int64_t eps_stride_b, float* z, float* logr, int64_t B, int Kc,
                 int Z, void* stream);
/* One workgroup of four waves per measure row r < R: weights [R*T, V] with row stride ld_w >= V, targets int64 [R, T], logr (nullable:
 * reads as 0) [R].  Wave w takes ticks w, w + 4, ...; per tick inet_cross_entropy's arithmetic (the maximum, expf(x - m) added per lane
 * in ascending v, the xor tree, lse = m + logf(se), the term lse - x[target]); lane 0 adds its ticks in ascending order, the four
 * partial sums meet as (p0 + p1) + (p2 + p3).  nll and logw = logr - nll (each nullable, not both) are written at [(r / group) * ld_out
 * + r % group]: a chunk of `group` samples per measure lands in its columns of a (B, K) array with ld_out = K.  A target outside [0, V)
 * writes NaN for that row and reads nothing through it; a -inf logit at the target gives nll = +inf, logw = -inf.  -1: weights or
 * targets null, nll and logw both null, R, group, T or V < 1, R > 2^24, ld_w < V, R % group != 0, ld_out < group. */
int inet_nll_rows(const float* weights, int64_t ld_w, const int64_t* targets, const float* logr, float* nll, float* logw, int64_t ld_out,
                  int64_t R, int group, int T, int V, void* stream);
/* One wavefront per measure b < B over logw, nll [B, K] (float32, row stride ld >= K); all arithmetic in double on the widened values:
 * the maximum, then s1, s2, sum logw, sum nll per lane in ascending k and a xor tree.  out [B, 5] float64 = {iwae, elbo, ess, rec, kl};
 * iwae is formed as m + log(s1 / K), in this order (K = 1 and K equal weights are exact).  -1: a null pointer, B or K < 1, B > 2^24,
 * ld < K. */
int inet_iw_finish(const float* logw, const float* nll, int64_t ld, int64_t B, int K, double* out, void* stream);

/* rows of V (post-ReLU) logits -> out[row*stride] ~ Multinomial(softmax(row))  (decoder.py:506-509): inverse-CDF draw with
 * one counter-based uniform per row keyed (seed, offset + row): row r of a call at `offset` is row 0 of a call at offset + r.
 * The token drawn always has mass (exp(w - max) > 0 in float32): where rounding leaves every prefix sum at or below
 * u * total (u close to 1), it is the last token with mass, never a trailing token without any. */
int inet_sample_multinomial(const float* weights, int64_t ld_w, int rows, int V, int64_t* out, int64_t stride,
                            uint64_t seed, uint64_t offset, void* stream);

/* The sampling rule of inet_vae_decoder_sample on rows of V logits (row stride ld_w), one wavefront per row: out[row*stride] = the
 * first v whose prefix of expf(temperature * w_v - max) (f64 prefix) exceeds uniforms[row*u_stride] * total; inet_argmax's rule for a
 * row where that does not apply (a NaN among temperature * w, a maximum or total that is not finite, a uniform outside [0, 1) or
 * NaN).  The result always lies in [0, V).  -1: a null pointer, rows <= 0, V <= 0, V > 512, a non-finite temperature. */
int inet_sample_temperature(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                            int64_t u_stride, int64_t* out, int64_t stride, void* stream);
/* The truncated rule of inet_vae_decoder_sample_ex on rows of V logits, one wavefront per row: out[row*stride] = the token,
 * logp[row*logp_stride] (logp nullable) = its log-probability under the truncated distribution; inet_argmax's rule and a NaN logp
 * for a row where the sampling rule does not apply.  -1 where inet_sample_temperature returns it, and for a top_p that is NaN, <= 0
 * or > 1. */
int inet_sample_truncated(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                          int64_t u_stride, int top_k, double top_p, int64_t* out, int64_t stride, float* logp, int64_t logp_stride,
                          void* stream);
/* The constrained rule of inet_vae_decoder_sample_cx on rows of V logits, one wavefront per row: allow + row*allow_stride (the stride
 * counted in words) = the row's ceil(V / 64) words of allowed tokens, up to 8; a null allow: inet_sample_truncated.  A row where the
 * sampling rule does not apply takes inet_argmax's rule over its allowed tokens (a banned entry counts as -inf and is never returned)
 * and a NaN logp.  -1 where inet_sample_truncated returns it. */
int inet_sample_constrained(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                            int64_t u_stride, int top_k, double top_p, int64_t* out, int64_t stride, float* logp, int64_t logp_stride,
                            const uint64_t* allow, int64_t allow_stride, void* stream);
/* The forced rule of inet_vae_decoder_sample_fx on rows of V logits, one wavefront per row: forced[row*forced_stride] = the row's forced
 * token, a value outside [0, V) = a free row, which is inet_sample_constrained's row; a null forced: inet_sample_constrained.  A forced row
 * returns its token whatever the mask, the truncation and the logits hold, ignores its uniform, and reports logp = (s_f - m) - log S: -inf
 * where the token is banned or truncated away, NaN where the rule does not apply.  allow may be null beside forced (all ones).  -1 where
 * inet_sample_constrained returns it. */
int inet_sample_forced(const float* weights, int64_t ld_w, int rows, int V, float temperature, const double* uniforms,
                       int64_t u_stride, int top_k, double top_p, int64_t* out, int64_t stride, float* logp, int64_t logp_stride,
                       const uint64_t* allow, int64_t allow_stride, const int32_t* forced, int64_t forced_stride, void* stream);

/* ---- optimizer: torch.optim.Adam as built at utils/trainer.py:32-35, stepped at :172-177 -------- */
/* p,g,m,v: arenas of n floats; step is 1-based; grads are multiplied by gscale first (1/world_size for DP).
 * The four entry points below are ONE kernel: inet_adam_step_w with everything it adds switched off IS
 * inet_adam_step_clip, and that without partials IS inet_adam_step_ex -- the same launch, not a bit-identical twin. */
int inet_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, int step, float gscale, void* stream);
/* The same step for a caller that must know, without stalling the queue, what the kernel decided (round 4):
 *  - step_flag (nullable; TWO device floats): when given, word 0 ALONE decides whether the step is applied -- non-zero = skip.  A
 *    data-parallel caller writes its rank's status there with inet_step_flag_export() -- word 0 = a chain kernel of this rank
 *    timed out, word 1 = a prologue kernel of this rank met a token outside the vocabulary -- and sums the words over ranks
 *    together with the gradients (a 16-byte head in front of the gradient arena: no extra collective), so that every rank skips
 *    a step ANY rank's chain kernels failed in and the replicas stay bit-identical.  Null: this process's own status word decides,
 *    as in inet_adam_step.
 *  - report (nullable): FOUR 32-bit words of caller-owned, device-visible HOST memory (pinned / host-mapped), zeroed by the
 *    caller before the call; the kernel sets [0] = 1 when it has run, [1] = 1 if it skipped the step, [2] = 1 if a parameter
 *    became NaN / inf in this update -- the observable behaviour of MeasureVAE/encoder.py:111-116 and decoder.py:424-429
 *    (ValueError "... has become nan") without a host scan of the weights per forward --, [3] = 1 if step_flag[1] is non-zero
 *    (decoder.py:36-45 check_index: every rank raises its ValueError at the same step).  The caller reads the record behind an
 *    event of its own some steps later: inpaintnet_amd/trainer.py keeps a ring of 16 records per Trainer and reads the one of
 *    step k when it has queued step k + 12 (INET_REPORT_LAG).  The lag is how far the host may run ahead of the GPU and must be
 *    generous: a lag of 2 cost the B = 256 step 5 % (profiles/r04_b_report_lag.txt); Trainer.finish() reads what is outstanding. */
int inet_adam_step_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, int step, float gscale, const float* step_flag, uint32_t* report, void* stream);
/* Clip the gradient by its global norm and skip a step whose gradient is not finite, on the device.  The rule,
 * for the gradient arena g[0..n), gscale and 0 < max_norm <= +inf:
 *   1. S = sum (double)g_i * (double)g_i -- every square exact in f64, the sum in f64 in a FIXED order that depends on n only;
 *      norm = |gscale| * sqrt(S) in f64.
 *   2. nonfinite = !isfinite(norm): true iff some element is inf or NaN (a finite f32 arena cannot overflow the f64 sum).
 *   3. c = max_norm / (norm + 1e-6) in f64, torch's clip_grad_norm_ coefficient; scale = c < 1 ? (float)c : 1.0f; clipped = c < 1.
 *      max_norm = +inf never clips; it still measures the norm and still skips non-finite steps.
 *   4. The chain / step flag says skip (inet_adam_step_ex's rule, unchanged): the step is skipped, only report[1] is set, nonfinite
 *      and clipped are reported as 0.
 *   5. Otherwise, nonfinite: p, m, v are left bit for bit untouched, report[5] = 1, report[1] and report[2] stay 0 -- not a chain
 *      failure.
 *   6. Otherwise Adam runs exactly as inet_adam_step_ex with gscale replaced by the single f32 product gscale * scale: with
 *      scale == 1.0f p, m, v are bit-identical to inet_adam_step_ex on the same inputs.
 * Two launches on `stream`: inet_grad_sqnorm writes ALL inet_sqnorm_parts() doubles of `partials` (device memory the caller allocates
 * once and reuses; nothing to zero), inet_adam_step_clip sums them in every workgroup in one fixed order and applies steps 2-6.
 * g must be 16-byte aligned.  report (nullable): EIGHT 32-bit words of host-mapped memory zeroed by the caller: [0..3] as in
 * inet_adam_step_ex, [4] = clipped, [5] = skipped for a non-finite gradient, [6] = the bits of (float)norm (written whenever the kernel
 * ran, also on a skip), [7] = 0.  step_flag: as in inet_adam_step_ex.  -1 for a max_norm that is NaN or <= 0, before any launch. */
int inet_sqnorm_parts(void);
int inet_grad_sqnorm(const float* g, int64_t n, double* partials, void* stream);
int inet_adam_step_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, int step, float gscale, float max_norm, const double* partials, const float* step_flag,
                        uint32_t* report, void* stream);
/* The optimizer step with decoupled weight decay (AdamW) and an exponential moving average of the weights, in one launch
 * (DESIGN.md section 19).  Inputs: everything inet_adam_step_clip takes, with `partials` now nullable; weight_decay >= 0, finite;
 * decay_mask, nullable device uint32 words, ceil(n / 32) of them -- bit i & 31 of word i >> 5 set means element i decays, null means
 * every element decays (torch.optim.AdamW's default); ema, a nullable device arena of n floats; ema_decay in [0, 1).  The rule:
 *   1. Skip and scale are exactly today's.  With partials: the rule of inet_adam_step_clip, steps 1-6, norm, clip coefficient,
 *      non-finite drop and flag precedence included.  Without partials: inet_adam_step_ex's rule -- only the chain / step flag skips,
 *      and max_norm is ignored.
 *   2. A skipped or dropped step leaves p, m, v AND ema bit for bit untouched.
 *   3. An applied step: the launcher computes decay = (float)(1.0 - (double)lr * (double)weight_decay) and
 *      omd = (float)(1.0 - (double)ema_decay), once, on the host.  Per element: m, v as today; p1 = decays(i) ? p * decay : p (the
 *      product rounded to f32 on its own); p_new = p1 - lr_over_bc1 * (m / denom) as today.  This is torch's _single_tensor_adamw
 *      order, param.mul_(1 - lr * wd) before the update.  report[2] ("a parameter left the finite range") tests p_new.
 *   4. After an applied step, if ema is given: e_new = fmaf(ema_decay, e, omd * p_new), the product rounded on its own.  ema_decay == 0
 *      therefore gives e_new == p_new bit for bit.
 *   5. With weight_decay == 0, decay is exactly 1.0f: with ema null as well, p, m, v and the report are bit-identical to
 *      inet_adam_step_clip (with partials) or inet_adam_step_ex (without) on the same inputs.
 * report (nullable): host-mapped words zeroed by the caller, [0..3] as inet_adam_step_ex.  With partials EIGHT words: [4..6] are
 * inet_adam_step_clip's (clipped, dropped, norm bits), [7] stays 0.  Without partials the kernel stores to [0..3] only: FOUR words
 * are enough, and a longer record keeps whatever its other words held.
 * p, g, m, v and ema must be 16-byte aligned.  Data parallel: decay and EMA are element-wise functions of values that are
 * bit-identical on every rank behind the all-reduce, so replicas and their EMA arenas stay bit-identical with nothing to coordinate.
 * -1, before any launch, for: null p, g, m or v; n <= 0; step < 1; weight_decay negative, NaN or inf; ema_decay outside [0, 1) or
 * NaN; partials given with !(max_norm > 0). */
int inet_adam_step_w(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                     int step, float gscale, float max_norm, const double* partials, float weight_decay,
                     const uint32_t* decay_mask, float* ema, float ema_decay, const float* step_flag, uint32_t* report,
                     void* stream);
/* dst: the TWO floats described above (chain status, token status of this process) */
int inet_step_flag_export(float* dst, void* stream);
/* Number of prologue launches that met a token index outside [0, num_notes) since the last reset (encoder input tokens,
 * teacher-forcing targets): decoder.py:36-45 check_index raises ValueError; here the host-mapped counter is read by the Python
 * layer at its status reads (Trainer.step, the inference wrappers).  reset != 0 clears it.  -2: could not be allocated. */
int inet_token_status(int reset);
/* Epoch statistics of the training loop (utils/trainer.py:124-163 accumulates mean_loss / mean_accuracy per batch):
 * sums[0] += *loss, sums[1] += *accuracy (nullable), sums[2] += 1 -- on the device, and only while no chain launch of this
 * process has timed out since the last inet_chain_status(reset): a step the optimizer kernel skipped (inet_adam_step reads the
 * same flag) does not enter the means either. */
int inet_epoch_stats_add(float* sums, const float* loss, const float* accuracy, void* stream);
/* step_flag as in inet_adam_step_ex: the batch enters the means iff its optimizer step was applied */
int inet_epoch_stats_add_ex(float* sums, const float* loss, const float* accuracy, const float* step_flag, void* stream);


/* ---- dropout masks (nn.GRU inter-layer dropout, encoder.py:32, decoder.py:346,365) --- */
int inet_dropout_mask(float* out, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream);

/* ---- generic 2-layer bidirectional GRU: nn.GRU(batch_first, bidirectional, num_layers=2) as used at
 *      LatentRNN/latent_rnn.py:53-82,186-193,228-233 ------------------------------------ */
/* weights: pointer to the 16 tensors of the GRU in state_dict order inside an arena
 * (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, *_l0_reverse, *_l1, *_l1_reverse), each 16-byte aligned
 * as produced by inet_latent_param_info.  x [B,T,K] batch-first (or x_scalar: device pointer to ONE float
 * broadcast as a [B,T,1] input when K == 1 and x == null); h0 [4,B,H] or null (zeros);
 * mask null or [T,B,2H]; out (nullable) [B,T,2H]; h_n (nullable) [4,B,H]. */
int64_t inet_bigru2_ws_bytes(int batch, int T, int K, int H, int save);
int inet_bigru2_fwd(int batch, int T, int K, int H, const float* x, const float* x_scalar, const float* weights,
                    const float* h0, const float* mask, float* out, float* h_n, void* ws, int64_t ws_bytes, int save,
                    void* stream);
/* dout (nullable) [B,T,2H], dh_n (nullable) [4,B,H]; grads: same 16-tensor block in the grad arena;
 * dx (nullable) [B,T,K]; dx_scalar (nullable, 1 float, accumulated); dh0 (nullable) [4,B,H] */
int inet_bigru2_bwd(int batch, int T, int K, int H, const float* x, const float* x_scalar, const float* weights,
                    float* grads, const float* mask, const float* dout, const float* dh_n, float* dx,
                    float* dx_scalar, float* dh0, void* ws, int64_t ws_bytes, void* stream);

/* ---- generic fp32 MFMA GEMM (nn.Linear and friends): C[M,N] (op)= epi(A . B^T + bias) -- */
/* a_kmajor/b_kmajor: 0 => operand(row,k) = P[row*ld + k]; 1 => P[k*ld + row].
 * epi: 0 none, 1 SELU, 2 ReLU, 3 *selu'(aux), 4 *aux, 5 *(aux>0).  acc: 0 store, 1 add. */
int inet_gemm(const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb, int b_kmajor, float* C,
              int64_t ldc, int M, int N, int K, const float* bias, const float* aux, int64_t ldaux, int epi,
              int acc, void* stream);
/* `nbatch` such products of one shape in one launch where a batched kernel applies (the two directions of a bi-GRU
 * layer's weight gradients: utils/trainer.py's loss.backward() over encoder.py:53-60), one after the other otherwise:
 * problem i reads A + i*batchA, B + i*batchB and accumulates (acc is always "add") into C + i*batchC (element strides). */
int inet_gemm_batched(const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb, int b_kmajor, float* C,
                      int64_t ldc, int M, int N, int K, int nbatch, int64_t batchA, int64_t batchB, int64_t batchC,
                      void* stream);
/* n = 1..4 INDEPENDENT products in one launch where a grouped kernel applies (csrc/gemm.hip launch_gemm_group: few-row products of
 * one M on the wave-per-column kernel, products of one operand layout and a common tile on the workgroup split-K kernel;
 * inet_gemm_group_plan tells which), one after the other otherwise.  Every product is described by the arguments inet_gemm takes
 * for it and keeps its own shape, K, leading dimensions, bias, epilogue and accumulation mode.  The destinations of one group must
 * not overlap element for element (the products run concurrently); interleaved strided destinations -- rows of one product between
 * the rows of another -- are allowed.  -1 and no launch for n outside 1..4, a null list and whatever inet_gemm rejects in any
 * product (null A, B or C; M, N or K <= 0; epi outside 0..5; acc outside 0..1). */
typedef struct inet_gemm_desc {
    const float* A; int64_t lda; int32_t a_kmajor;
    const float* B; int64_t ldb; int32_t b_kmajor;
    float* C; int64_t ldc;
    int32_t M, N, K;
    const float* bias;
    const float* aux; int64_t ldaux;
    int32_t epi, acc;
} inet_gemm_desc;
int inet_gemm_group(int n, const inet_gemm_desc* list, void* stream);

/* The same product on the bf16 matrix cores at fp32 accuracy (csrc/gemm_bf3.hip): both operands are split exactly into three
 * bf16 pieces in MFMA fragment order (a scratch allocated for the call: this entry exists for tests and benchmarks; inside the
 * library the pieces live in the callers' workspaces), then C (op)= A . B^T + bias with nine (six) piece products per
 * element product accumulated in f32.  M % 192 == 0, N % 128 == 0, K % 32 == 0 (k-major operands: rows % 64 == 0), else -1.
 * ksplit: 0 = chosen by the library, else the k range is split that many ways over the grid (f32 atomics).  acc: 0 store, 1 add. */
int inet_gemm_bf3(const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb, int b_kmajor, float* C,
                  int64_t ldc, int M, int N, int K, const float* bias, int acc, int ksplit, void* stream);

/* nn.Linear forward / backward (LatentRNN.generation_linear, latent_rnn.py:83,232,250):
 * y[M,N] = epi(x[M,K] W[N,K]^T + b), epi in {0 none, 1 SELU, 2 ReLU};
 * backward (no activation): dx[M,K] = dy W (nullable), dW += dy^T x (nullable), db += colsum(dy) (nullable); dW and db are
 * leaf work: they run on the library's side stream (joined before return unless joins are deferred, inet_set_option 1) */
int inet_linear_fwd(const float* x, const float* W, const float* b, float* y, int M, int N, int K, int epi,
                    void* stream);
int inet_linear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db, int M, int N,
                    int K, void* stream);

/* ---- single-layer LSTM over T steps: torch.nn.LSTM(num_layers=1, batch_first) as stacked by
 *      lstm_with_activations, AnticipationRNN/anticipation_rnn_gauss_reg_model.py:14-39,110-133.
 * gi [T,B,4H] time-major input-side pre-activations (x W_ih^T + b_ih, formed by inet_linear_fwd); gate order i,f,g,o;
 * h0/c0 [B,H] or null (zeros); reverse != 0 processes t = T-1..0 (the constraint LSTM, :467-474); out [T,B,H];
 * hT/cT nullable [B,H].  Backward: dout [T,B,H] (nullable), dhT/dcT (nullable) -> dgi [T,B,4H] (gate gradients: the
 * caller forms dx and dW_ih with inet_linear_bwd); dW_hh/db_ih/db_hh accumulated when all three are given. */
int64_t inet_lstm_ws_bytes(int batch, int T, int H, int save);
int inet_lstm_fwd(int batch, int T, int H, const float* gi, const float* W_hh, const float* b_hh, const float* h0,
                  const float* c0, int reverse, float* out, float* hT, float* cT, void* ws, int64_t ws_bytes, int save,
                  void* stream);
int inet_lstm_bwd(int batch, int T, int H, const float* W_hh, const float* h0, const float* out, const float* dout,
                  const float* dhT, const float* dcT, int reverse, float* dgi, float* dW_hh, float* db_ih, float* db_hh,
                  float* dh0, float* dc0, void* ws, int64_t ws_bytes, void* stream);
/* Two stacked LSTM layers with zero initial states (the loop of lstm_with_activations over lstm_list,
 * anticipation_rnn_gauss_reg_model.py:14-39) as a pipeline over chunks of time steps: layer 1 runs chunk c on a second
 * stream while layer 0 runs chunk c+1.  gi0 [T,B,4H] (x W_ih0^T + b_ih0); out0/out1 [T,B,H]; gi1 [T,B,4H] scratch;
 * ws0/ws1: one inet_lstm_ws_bytes workspace per layer.  Backward: dout1 [T,B,H] -> dgi0, dgi1 [T,B,4H] (the caller forms
 * dx and dW_ih0 from dgi0 with inet_linear_bwd); dout0 [T,B,H] scratch; the weight / bias gradients (all given or all
 * null) are accumulated.  Both return 1 (and do nothing) when the shape does not qualify for the pipeline: the caller
 * then runs inet_lstm_fwd / inet_lstm_bwd layer by layer. */
int inet_lstm2_ok(int batch, int T, int H);       /* 1 when inet_lstm2_fwd / _bwd will take the shape */
int inet_lstm2_fwd(int batch, int T, int H, const float* gi0, const float* W_hh0, const float* b_hh0, const float* W_ih1,
                   const float* b_ih1, const float* W_hh1, const float* b_hh1, int reverse, float* out0, float* gi1,
                   float* out1, void* ws0, void* ws1, int64_t ws_bytes, int save, void* stream);
int inet_lstm2_bwd(int batch, int T, int H, const float* W_hh0, const float* W_ih1, const float* W_hh1,
                   const float* out0, const float* out1, const float* dout1, int reverse, float* dgi0, float* dgi1,
                   float* dout0, float* dW_hh0, float* db_ih0, float* db_hh0, float* dW_ih1, float* dW_hh1,
                   float* db_ih1, float* db_hh1, void* ws0, void* ws1, int64_t ws_bytes, void* stream);

/* The sequential part of AnticipationRNN's free-running pass (AnticipationRNN/anticipation_rnn_gauss_reg_model.py:190-259): the
 * generation LSTMs feed the argmax of BATCH ELEMENT 0 back to the whole batch (:253-256), so the token sequence depends on that one
 * row.  L ticks of [embedding of the previous token (start: token 0) | oc0 + t * oc_stride (the tick's constraint output, Hc floats)]
 * -> LSTM 0 -> LSTM 1 -> ReLU(linear_1) -> note head -> argmax (numpy order: NaN is the maximum, lowest index among equals), without a
 * host round trip: ONE persistent launch of 13 workgroups with their weights in registers for the reference's configuration (H = U =
 * 256, V <= 128; csrc/arnn_gen.hip, round 5: two hand-offs per tick), four small launches per tick otherwise (inet_set_option key 14 /
 * INET_ARNN_GEN: 0 = always the launches, 1 = persistent kernel, 2 = its workgroups on one XCD, 3 = default: 2 + XCD-local granule stores); tokens [L] int64 on the device.  emb [.,E]; W_ih0 [4H, E+Hc]; W_ih1, W_hh* [4H,H]; W1 [U,H]; W2 [V,U].  hc_init
 * (nullable: zeros) = the state the ticks go on from, [layer][h | c][H]; first_tok (nullable: token 0) = device pointer to the token in
 * front of the first tick -- forward_inpaint (:261-346) generates a window behind a teacher-forced prefix.  The caller then runs the
 * whole batch over these tokens with the batched kernels (inpaintnet_amd.arnn._forward_no_tf / forward_inpaint). */
int64_t inet_arnn_generate_ws_floats(int L, int E, int Hc, int H, int U, int V);
int inet_arnn_generate(int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_stride,
                       const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0, const float* W_ih1,
                       const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                       const float* W2, const float* b2, const float* hc_init, const int64_t* first_tok, int64_t* tokens, float* ws,
                       int64_t ws_floats, void* stream);
/* AnticipationRNN's temperature-sampled generation (ConstraintModelGaussianReg.generate, AnticipationRNN/
 * anticipation_rnn_gauss_reg_model.py:570-679) for R independent rows.  Row r runs L ticks of [embedding of the previous token
 * (tick 0: token 0) | oc0 + r * oc_batch_stride + t * oc_row_stride (Hc floats)] -> LSTM 0 -> LSTM 1 -> ReLU(linear_1) -> note head,
 * from the state hc_init[r] ([R][layer][h | c][H], nullable: zeros), and DRAWS token t from softmax(temperature * logits) with the
 * uniform uniforms[r][t] in [0, 1) (host-side doubles) in np.random.choice's order: the first v with sum_{w <= v} p_w > u (prefix
 * in f64).  A NaN logit, a non-finite total or a uniform outside [0, 1) take the argmax rule of inet_arnn_generate for that tick;
 * tokens [R][L] int64 on the device are always inside [0, V).  H = U = 256, V <= 128 with inet_set_option key 14 != 0 and the chain
 * kernels on: the persistent token pass of inet_arnn_generate with the sampling head, up to 8 rows per launch (each an independent
 * team of 13 workgroups; more rows, or a chain capacity below 13 x rows: successive launches); otherwise four launches per tick,
 * row after row.  Returns -1 on invalid arguments (R < 1, L < 1, a workspace smaller than inet_arnn_sample_ws_floats, a non-finite
 * temperature, a null pointer where one is required), -2 on a launch failure; timeouts of the persistent launch are reported by
 * inet_chain_status. */
int64_t inet_arnn_sample_ws_floats(int R, int L, int E, int Hc, int H, int U, int V);
int inet_arnn_sample(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                     int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                     const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                     const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                     int64_t* tokens, float* ws, int64_t ws_floats, void* stream);
/* The same behind TOP-K / NUCLEUS TRUNCATION, with the drawn tokens' log-probabilities and the logits they were drawn from.  The rule
 * is the one stated for inet_vae_decoder_sample_ex, applied to s = temperature * logits of the note head (not ReLU'd: ties are rare
 * there, and still fall lowest index first).  logp (nullable; [R][L] floats on the device) receives (s_tok - m) - log(S) as f32; a
 * tick that takes the argmax rule (a NaN among s, a maximum or total that is not finite, a uniform outside [0, 1) or NaN) has a NaN
 * logp.  logits (nullable; [R][L][V] floats on the device) receives every tick's note-head output, the x of that rule.
 * inet_arnn_sample is this call with (top_k, top_p, logp, logits) = (0, 1.0, null, null) and runs the kernels it always ran; a call
 * with truncation on, a logp or a logits pointer runs the truncating build of the persistent token pass or, for the other shapes, the
 * truncating head of the per-tick launches, and never a kernel that ignores them: its launch labels start with "trunc_"
 * (trunc_arnn_token_sample R.. L.. V.., trunc_arnn_ticks L.. V..).  The persistent pass has a truncating build for V <= 64; with
 * H = U = 256 and 64 < V <= 128 a truncated call runs the per-tick launches.  With (0, 1.0) and a logp or logits pointer the tokens
 * equal inet_arnn_sample's bit for bit wherever both run the same kind of launch (every shape but that one, where the logits are
 * summed in another order and the tokens agree outside the rule's rounding margins).
 * The workspace is inet_arnn_sample_ws_floats'.  -1 where inet_arnn_sample returns it, and for a top_p that is NaN, <= 0 or > 1. */
int inet_arnn_sample_ex(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                        int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                        const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                        const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                        int64_t* tokens, float* ws, int64_t ws_floats, int top_k, double top_p, float* logp, float* logits,
                        void* stream);
/* The same behind PER-TICK TOKEN CONSTRAINTS: a mask of allowed tokens per (row, tick), applied in front of the truncated rule inside the
 * launch (the token of tick t is fed back into tick t + 1 there).  The rule is the one stated for inet_vae_decoder_sample_cx (DESIGN.md
 * section 13: steps 0 to 3, the mask layout [rows][L][NW] with NW = ceil(V / 64), and its consequences), applied to s = temperature *
 * logits of the note head.  The note head is not ReLU'd: a fallback tick replaces the banned logits by -inf (there is no padding value
 * below every logit), and takes its NaN ballots and its maximum over the ALLOWED entries alone -- a NaN at a banned place does not win
 * (inet_sample_constrained's reading of "still an allowed one").  logits receives the unmasked note-head output.
 * allow: [R][L][NW] words on the device, or null -- then this IS inet_arnn_sample_ex.  A constrained call is a truncating call: it runs
 * the masked build of the persistent token pass (V <= 64) or, for the other shapes, the masked head of the per-tick launches, and never a
 * kernel that ignores the mask: its launch labels start with "cons_" (cons_arnn_token_sample R.. L.. V.., cons_arnn_ticks L.. V..).
 * -1 where inet_arnn_sample_ex returns it. */
int inet_arnn_sample_cx(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                        int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                        const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                        const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                        int64_t* tokens, float* ws, int64_t ws_floats, int top_k, double top_p, float* logp, float* logits,
                        const uint64_t* allow, void* stream);
/* The same behind FORCED TOKENS: the log-probability the model gives to a filling it did not draw.  The rule is the one stated for
 * inet_vae_decoder_sample_fx (word for word: layout, free tick, forced tick and consequences (a) to (e)), applied
 * to s = temperature * logits of the note head, with the two model-specific points of inet_arnn_sample_cx.
 *
 * Layout.
 *  - `forced` is an array of `int32` `[rows][L]`.
 *  - A value `f` with `0 <= f < V` forces that tick.
 *  - Every other value makes the tick free.  The Python surfaces write -1 for a free tick.
 *  - A null `forced` means no tick is forced: then this IS inet_arnn_sample_cx.
 *
 * At a forced tick with token `f`:
 *  - Steps 0 to 2 of the rule run on the tick's logits: the NaN test, the mask, m, and the truncation.  The tick's uniform is not used.
 *    The rule is evaluated as with u = 0, so a uniform of 1.0, 2.0 or NaN at a forced tick causes no fallback.
 *  - The token is `f`.  It is stored in `tokens` and fed back into tick t + 1.  This holds whether or not `f` is allowed or kept, and on
 *    a fallback tick too.
 *  - logp = (s_f - m) - log S as f32.  It is exactly -inf when `f` is banned or truncated away.  It is NaN where the rule does not
 *    apply: a NaN among s, or m or S not finite.
 *  - The note head is not ReLU'd.  On a fallback tick a free tick takes inet_arnn_sample_cx's argmax over the allowed entries.  A forced
 *    tick takes `f`.
 *  - The returned logits stay the unmasked ones.
 *
 * A forced call is a truncating, masked call (allow nullable: no token banned).  It runs the forced build of the persistent token pass
 * (V <= 64) or, for the other shapes, the forced head of the per-tick launches, and never a kernel that ignores the forced words: its
 * launch labels start with "force_" (force_arnn_token_sample R.. L.. V.., force_arnn_ticks L.. V..).
 * -1 where inet_arnn_sample_cx returns it (so for `forced` without uniforms). */
int inet_arnn_sample_fx(int R, int L, int E, int Hc, int H, int U, int V, const float* emb, const float* oc0, int64_t oc_row_stride,
                        int64_t oc_batch_stride, const float* W_ih0, const float* b_ih0, const float* W_hh0, const float* b_hh0,
                        const float* W_ih1, const float* b_ih1, const float* W_hh1, const float* b_hh1, const float* W1, const float* b1,
                        const float* W2, const float* b2, float temperature, const double* uniforms, const float* hc_init,
                        int64_t* tokens, float* ws, int64_t ws_floats, int top_k, double top_p, float* logp, float* logits,
                        const uint64_t* allow, const int32_t* forced, void* stream);
/* nn.Embedding forward / backward (rows of E floats gathered by int64 index; backward accumulates with atomics).
 * row_scale (nullable, [rows]) multiplies each gathered row: the Dropout2d on the shifted note embeddings
 * (drop_input, anticipation_rnn_gauss_reg_model.py:437-442) and the all-zero first time step (:373-376). */
int inet_embedding_fwd(const float* table, const int64_t* idx, int64_t rows, int E, float* out, const float* row_scale,
                       void* stream);
/* num_embeddings: rows of the table (0 = not told): small tables take a segment-sum kernel instead of per-element atomics.
 * dtable is accumulated into (zero it first for a fresh gradient); rows whose row_scale is 0 add nothing.
 * Every index MUST lie in [0, num_embeddings) -- the table's row count where num_embeddings is 0.  Nothing checks it (the models'
 * tokens are range-checked where they enter: inet_token_status): the segment-sum path (num_embeddings <= 128 and rows >= 1024)
 * happens to drop a row whose index does not, the atomic path (and inet_embedding_fwd) addresses through it, outside the table. */
int inet_embedding_bwd(const float* dout, const int64_t* idx, int64_t rows, int E, float* dtable, const float* row_scale,
                       int num_embeddings, void* stream);
/* dpre = dy where y > 0 else 0   (backward of the ReLU fused into inet_linear_fwd epi=2) */
int inet_relu_bwd(const float* dy, const float* y, float* dpre, int64_t n, void* stream);
/* out[r*stride] = argmax_v w[r*ld + v] by np.argmax's rule (Tensor.max(1)): the lowest index among equal maxima (-0.0 == +0.0),
 * and a NaN counts as the maximum -- the lowest NaN of a row wins, before any +inf.  The result always lies in [0, V), whatever the
 * row holds (callers gather with it).  inet_arnn_generate and the `correct` count of inet_cross_entropy follow the same rule. */
int inet_argmax(const float* w, int64_t ld, int rows, int V, int64_t* out, int64_t stride, void* stream);

/* ---- input feed: the dataset tensors are int32 `score (N,1,384)` (DatasetManager/the_session/folk_dataset.py:852-861),
 *      the models take int64 (utils/helpers.py:17-26 to_cuda_variable_long).  The H2D copy moves the int32 form; these
 *      widen / split on the device. ------------------------------------------------------------------------------ */
/* dst[i] = src[i]: VAETrainer.process_batch_data (MeasureVAE/vae_trainer.py:42-55) -- (B,1,384) viewed as (B*16,24) */
int inet_tokens_to_i64(const int32_t* src, int64_t* dst, int64_t n, void* stream);
/* score [B, n_measures*measure_len] int32 -> past [B,n_past,L], target [B,n_target,L], future [B,rest,L] int64, each
 * contiguous: LatentRNNTrainer.split_score / split_to_measures (LatentRNN/latent_rnn_trainer.py:134-176) */
int inet_split_score(const int32_t* score, int batch, int n_measures, int measure_len, int n_past, int n_target,
                     int64_t* past, int64_t* target, int64_t* future, void* stream);

/* single GRU step (test hook for the fused step kernel; semantics of torch.nn.GRUCell with the input-side
 * gate pre-activations gi [B,3H] already formed) -- r,z,n,ghn,hprev saves are nullable [B,H] */
int inet_gru_step(int batch, int H, const float* gi, const float* h_prev, const float* W_hh, const float* b_hh,
                  float* h_new, float* sv5, void* stream);

/* ---- runtime options: key 0 = overlap the weight-gradient GEMMs of the backward pass with the BPTT chains on
 * a second, lower-priority HIP stream (default 1; also INET_SIDE_STREAM=0 in the environment) */
int inet_set_option(int key, int value);
/* key 2 = force the batched-GEMM tile configuration: value -1 = cost model (default), 0..4 = 64x64, 128x128, 192x64,
 * 192x128, 192x192 block tiles; key 3 = forced split-K factor (0 = cost model) of the
 * LDS-tiled kernel while key 2 is forced, and of the TN-direct and workgroup split-K kernels where they take the shape.  Test hooks: the
 * parity tests drive every tile configuration through the same shapes (keys 2 and 3). */
/* key 1 = deferred joins (default 0).  With 0 every *_bwd entry point makes `stream` wait for the side stream before
 * it returns.  With 1 it does not: the caller must keep every workspace passed to a *_bwd call alive and call
 * inet_side_join(stream) before anything reads the gradient arena (optimizer step, all-reduce) or frees those
 * workspaces.  Lets the leaf GEMMs of one module's backward overlap the next module's BPTT chain. */
/* key 4 = chain kernels (default 1; INET_CHAIN=0): one persistent launch per recurrent layer, weights resident in
 * registers, the hidden state exchanged between workgroups once per step (csrc/chain.h).  0 = one launch per step. */
/* key 5 = LDS-free GEMM kernels (csrc/gemm.hip): 0 = LDS-tiled kernels only, 1 = by shape
 * (default: shared-strip direct kernels for the big products, workgroup split-K for the medium / small ones), 2 = the
 * direct kernels whenever the shape qualifies (test hook), 3 = direct kernels only (no split-K), 4 = split-K first, also for
 * the long weight-gradient products. */
/* key 6 = test hook: value 1 arms ONE injected fault -- the next forward GRU chain launch loses a workgroup, its group runs
 * into the bounded spin (~0.4 s) and inet_chain_status() turns non-zero: lets the failure path (optimizer skip, fallback to
 * per-step kernels) be tested on a healthy GPU. */
/* key 7 = generation of the GRU FORWARD chain kernels: 9 (default; INET_CHAIN2) = second generation (csrc/gru_chain2.hip: one row
 * block per wave, W in LDS, the contraction on the bf16 matrix cores with every fp32 operand split exactly into three bf16 pieces
 * and all nine piece products accumulated in f32 = the products of fp32 arithmetic), 0 = first generation (f32-input MFMA, W in
 * registers).  The BPTT chains always run on the first generation. */
/* key 8 = the encoder's large products (csrc/gemm_bf3.hip; INET_GEMM_BF3): 9 (default) = on the bf16 matrix cores through the same
 * exact three-piece split, nine piece products; 0 = on the f32-input kernels of csrc/gemm.hip.
 * key 9 = which bf16 pieces the chain kernels write themselves (bit 0 the forward chains' rows, 1 their transposed pieces,
 * 2 the BPTT kernel's dgi rows; default 7) -- what they do not write, bf3_split launches make from the f32 arrays: same results.
 * (Round 3's keys 10 and 11 and the value 6 of keys 7 / 8 -- weight-gradient pipe per layer, second-generation BPTT kernel, six
 * piece products -- selected builds that lost their A/Bs or were not fp32 arithmetic; they were removed in round 4: -1.)
 * key 12 = big-batch GRU forward steps on the bf16 pipe (csrc/gru_step_bf3.hip): a layer whose single time
 * step has at least this many tiles of 128 rows x 64 units (default 256 = one per CU: B = 2048 at H = 512, two directions) runs one
 * product per step with the GRU cell as its epilogue instead of chunked chain launches; 0 = never.  The threshold decides per shape
 * whether a workspace holds the step kernels' W_hh pieces, so a *_bwd call compares the VALUE with the one its forward call ran under
 * (-3 on any difference, before it writes anything), not what the two values mean for some shape.
 * key 13 = how many of the side streams take leaf work in rotation from now on (0 = all that exist, default; 1: what a process with
 * a gradient exchange beside its steps wants -- inpaintnet_amd.dp sets it: the runtime deals FOUR hardware queues, and caller + two
 * side streams + the exchange's two streams measured 4.94 ms per B = 256 step against 3.87 with one side stream).
 * key 14 = AnticipationRNN's token pass (inet_arnn_generate; INET_ARNN_GEN): 3 (default) = one persistent launch where the shape
 * allows, its 13 workgroups on every 8th workgroup id (one XCD as dispatched today) and -- once they have FOUND themselves on one XCD
 * (they compare XCC ids at the start of the launch) -- granules as plain stores that stay in that XCD's L2; 2 = the same with
 * agent-scope stores; 1 = on 13 consecutive ids; 0 = four launches per tick; 4 = test hook: 3's request on consecutive ids (the
 * XCC-id check must refuse it).
 * key 15 = the free-running decode of ONE to SIXTEEN measures at H = 512 (inference; csrc/decode_b1.hip; INET_DECODE_B1): 4 (default) =
 * 3 with every team's critical workgroups (C + 16 TBi, or the 16 CB of the merged build) on workgroup ids of one residue mod 8 --
 * one XCD under today's round-robin dispatch -- and, once they have CHECKED that they share an XCD, XCD-local copies of h0 / h1
 * written with plain stores next to the agent-scope ones (correct under any placement: a failed check uses the agent-scope copies; 5 = test
 * hook: the same request on consecutive workgroup ids, where the check has to refuse); 3 =
 * one or two measures: ONE register-resident persistent launch for the whole call behind the prologue launch (129 workgroups: 49 for
 * the 24 ticks -- two hand-offs per tick; one where a single workgroup kind can hold layer 1, the head and the argmax: one row with
 * V <= 64 -- and 80 for the beat path); three to sixteen: teams of the 49 tick workgroups in one launch, two rows per team up to ten
 * measures, four beyond -- up to six measures still with the beat path's workgroups in the same launch, beyond behind the beat path's
 * own launches; 2 / 1 = the tick path only, behind the beat path's eight launches, on
 * every 4th workgroup id / on consecutive ids; 0 = decode_chain.hip's 32-member exchange kernel.
 * Keys 4, 7-12, 14 must not change between a forward call and its backward call, nor between sizing a workspace and using it. */
int inet_side_join(void* stream);
/* `stream` -- a THIRD stream, not the one the library calls were issued on -- waits for all side-stream work queued so far.
 * Unlike inet_side_join nothing is consumed: the issuing stream still joins the same work at its own next join (a
 * data-parallel bucket's all-reduce stream orders itself behind the leaf GEMMs this way without the backward pass waiting). */
int inet_side_wait(void* stream);
/* The library's second compute stream ("twin": hipStream_t through *stream; created on first use, before the side streams).  The
 * HIP runtime deals its hardware queues to streams in creation order and a process that keeps more than four of them busy is
 * time-sliced (a fifth stream that carried the optimizer launch made every LatentRNN step 1.7x slower: DESIGN.md section 8), so a
 * caller that wants work beside the library's own -- the trainer's late optimizer launch, a data-parallel bucket's pre-processing --
 * borrows this stream instead of creating one; it orders it against its own stream with events.  The two-layer LSTM pipelines use
 * the same stream inside their calls (never across calls).  -2 if the stream could not be created. */
int inet_twin_stream(void** stream);
/* Number of chain-kernel workgroups that gave up waiting for their group since the last reset (0 = healthy; every
 * in-kernel spin is bounded, so a broken hand-off shows up here instead of hanging the GPU).  Complete after the
 * stream has been synchronised; a non-zero value read earlier is already a definite failure (the counter lives in
 * host-mapped memory: reading it costs nothing and needs no synchronisation).  While it is non-zero inet_adam_step
 * leaves parameters and moments untouched (a device-side twin of the counter is read by the kernel), so a failed step
 * can never reach the weights.  reset != 0 clears both (synchronises the device).  -2: the counter could not be allocated. */
int inet_chain_status(int reset);
/* Diagnostics: copies the first nbytes (<= 16384) of the library's device-side scratch area to the host (synchronises the device).
 * Only instrumented builds write there -- csrc/gru_chain2.hip compiled with -DINET_CHAIN2_STAMPS=1 records the wall-clock stamps of
 * one wave's steps (tools/chain2_anatomy.py) --, a normal build leaves it zero. */
int inet_debug_read(void* dst, int64_t nbytes);
/* The slow-wait recorder.  Every bounded wait on a group / row-block counter inside a persistent kernel that needed at least 64 polls (a
 * steady-state hand-off takes 3-8; a counter poll is ~0.4 us; granule waits, polled by every thread, only from 4096 polls on) is NOTED (*noted, if not null: how many since the last reset); a
 * wait of at least the entry threshold (default 16384 polls ~ 6 ms, inet_set_option key 16: any value >= 16) or one that GAVE UP is SLOW and files one entry
 * when it ends: 8 words {kernel id (1 = gru_chain fwd, 2 = bwd, 3 = gru_chain2 fwd, 5 = lstm fwd, 6 = lstm bwd, 8 = decode_chain,
 * 9 = arnn token pass, 10 = decode_b1) | XCC id << 8 | gave up << 15 | site << 16 (0 = group counter, 1 = granule, 2 = row-block
 * counter, 3 = tagged fragments), workgroup id, expected tag / counter, polls, wall clock lo, hi (100 MHz), 0, 0}.  Copies up to
 * max_entries (<= 127 are kept: the FIRST ones since the last reset) into dst and returns how many waits were slow since the last
 * reset (may exceed what is kept); reset != 0 clears counts and entries (not the threshold).  Synchronises the device.  Noted
 * waits are normal wherever launches overlap -- the members of a chain group wait ~100 us at their first step while the launch
 * becomes resident beside a weight-gradient product --; slow ones are the trace an unexplained timeout or a stalled launch leaves
 * behind (csrc/chain.h record_slow).  -1 bad arguments, -2 runtime failure. */
int inet_slow_waits(unsigned* dst, int max_entries, int reset, int64_t* noted);
/* The launch plan of the register-resident decode (csrc/decode_b1.hip) for a call of B measures with V notes and latent size Z, and
 * a host-side self-check of it -- no GPU needed (tests/test_decode_plan.py).  out8 = {teams, rows per team, shared recurrent groups,
 * critical workgroups per team, placed (1: workgroup ids are mapped to roles so that a team's critical workgroups share a residue mod
 * 8), grid, live workgroups, ok}; Z != 256 gives the plan of a call whose beat path runs as launches of its own (as a beat dropout
 * mask does).  ok = the plan names an instantiation of the kernel, every row is in one team, the rows that the teams, the shared groups
 * and the folded beat path address are inside the call's granule areas, the build is merged exactly where no C role is placed, shared
 * groups only in a placed launch, every (team, role) the kernel expects appears exactly once among the ids of the grid, every team's
 * critical roles sit on ONE residue, no residue carries more than 32 live workgroups, grid and live workgroups fit the chip.  0, or -1
 * for a call the register-resident launch does not take (B > 16, V > 128, no plan fits the chip's INET_CHAIN_CUS / CU count, ...). */
int inet_decode_b1_plan(int B, int V, int Z, int* out8);
/* The same for a temperature-sampled call (inet_vae_decoder_sample): the same planner with its `sample` input set, the same
 * self-check.  -1 also under inet_set_option key 15 != 4: the sampling build exists for the default mode's plans. */
int inet_decode_b1_plan_sample(int B, int V, int Z, int* out8);
/* ... and for a truncated call (inet_vae_decoder_sample_ex with truncation on or a logp): the truncating build has a merged build
 * for one row with V <= 32 alone (the others would spill registers), so more of its plans place workgroup C. */
/* (A constrained call -- inet_vae_decoder_sample_cx with a mask -- has the truncated call's plan: every masked build fits.  A forced call
 *  -- inet_vae_decoder_sample_fx with forced tokens -- has it too: every forced build fits.) */
int inet_decode_b1_plan_trunc(int B, int V, int Z, int* out8);
/* What a decoder forward call launches, under the options set now (inet_set_option keys 4, 15) and on this chip (CUs, or
 * INET_CHAIN_CUS), without a GPU or a workspace: the route function that inet_vae_decoder_fwd and the inet_vae_decoder_sample entries
 * ask themselves (csrc/vae.hip dec_route).  flags: bit 0 = a multinomial seed, bit 1 = mask_beat given, bit 2 = mask_tick given; level:
 * 0 = argmax, 1 = temperature, 2 = truncated or logp, 3 = a mask of allowed tokens, 4 = forced tokens.  out (n_out >= 13; 13 values are
 * written, 16 where n_out >= 16) = {beat path
 * (0 = one launch per step, 1 = chain launches, 2 = folded into the register-resident launch), tick path (0 = teacher-forced chains,
 * 1 = teacher-forced steps, 2 = one fused launch, 3 = fused launches over row chunks, 4 = tick by tick), beats per teacher-forced chain
 * launch, rows per chunk (512 / 256), the fused launch is the register-resident one, ... with the beat path inside it, words the
 * prologue zeroes (0 = none, 1 = the sync areas, 2 = the register-resident launch's granules and the sync areas), fragment-major twins
 * packed: the beat layers' W_hh, the tick layers' three, the output projection's, the initial tick hiddens (0 = no, 1 = once for all
 * rows, 2 = per chunk), the workspace carries twins at all, the first fused launch finds its counters zeroed by the prologue (0 where
 * row-chunked beat chains counted on them: it zeroes them itself); [13] bit a = the beat path's launches count on sync area a of the
 * workspace, [14] the same for the tick path's, [15] how many chain or fused launches of the call zero their own counters (their area
 * was counted on since the prologue zeroed it)}: [12] .. [15] are what a dry run of the call's ledger of sync areas (csrc/sync_areas.h)
 * over the route's launches gives, the ledger the call itself takes its areas from.  0, or -1 for a call the entries refuse (more than 4 beats, a level above
 * 0 with teacher forcing or a seed), a level outside 0..4, flags outside 0..7, a null or short output -- nothing is written then. */
int inet_vae_decoder_route(const inet_vae_config* cfg, int batch, int save, int teacher_forced, int flags, int level, int32_t* out,
                           int n_out);
/* What inet_gemm (nbatch = 1) / inet_gemm_batched (nbatch 2..8: no bias, epi 0, acc 1) launch for a call, under the options set now
 * (inet_set_option keys 2, 3, 5), without a GPU: the dispatcher's planner (csrc/gemm.hip gemm_plan) behind the C-ABI.  out16 = {family
 * (0 = few-row gemv, 1 = TN-direct, 2 = kc-direct, 3 = workgroup split-K, 4 = LDS-tiled), tile configuration, tile rows, tile columns,
 * splits, K per split, tiles along N, tiles, grid x, y, z, zero fill in front (split-K of a storing call), epilogue pass behind (split-K
 * with a non-linear epilogue), kernel launches in all, products run one after the other (1: one launch takes the call; nbatch: a batched
 * call no batched kernel takes -- the plan is then that of one product), 0}; work2 = algorithmic {FLOPs, bytes} of the launch; label (cap
 * bytes) = its name in the profile (inet_prof_dump).  0, or -1 for what the two entries reject (sizes <= 0, epi outside 0..5, acc
 * outside 0..1, nbatch outside 1..8) and for a null output -- nothing is written then. */
int inet_gemm_plan(int a_kmajor, int b_kmajor, int M, int N, int K, int64_t lda, int64_t ldb, int has_bias, int epi, int acc,
                   int nbatch, int32_t* out16, double* work2, char* label, int cap);
/* The same for n = 1..4 independent products handed to the library's grouped launch (the two heads of the encoder, a module's leaf
 * weight gradients): desc = n x {a_kmajor, b_kmajor, M, N, K, lda, ldb, has_bias, epi, acc}.  One launch takes the group (few-row gemv
 * group, workgroup split-K group): row 0 of out [n][16], work [n][2], label [n][cap] describes it and out[14] = 1; else every product
 * runs on its own plan, row i describes product i and out[14] = n. */
int inet_gemm_group_plan(int n, const int64_t* desc, int32_t* out, double* work, char* label, int cap);
/* What one GRU layer of nprob independent problems (directions) over B rows, T steps and hidden size H launches, forward and -- with
 * save != 0 -- backward, under the options set now (inet_set_option keys 4, 7, 8, 12) and for a workspace that carries every optional
 * buffer (as inet_bigru2_ws_bytes carves them), without a GPU: the plan functions that gru_layer_fwd / gru_layer_bwd (csrc/seq.hip)
 * branch on, behind the C-ABI.  out32 = the forward plan [0..15], the backward plan [16..31] (all -1 without save), each {route (0 =
 * f32 kernels, one launch per step; 1 = first-generation chain; 2 = second-generation chain; 3 = bf16-pipe step kernels), rows per
 * launch, launches (row chunks of a chain route; T on a step route), kernel generation, MS, SQ, OCC, EMR of the chain launch's build
 * (csrc/gru_chain.h ChainBuild; EMR: the build that writes piece outputs is the one that runs when the caller gives their buffers; 0
 * on a step route), chunk launches run two at a time on two streams, ring layout (0 = the layer's whole ring buffer, slots adjacent;
 * 1 = a ring of its own per chunk; 2 = each chunk on its rows of the two slots of the full-batch ring), workgroup groups and members
 * per group of one launch, floats of the ring buffer the launches address, floats the workspace carves for it, the chip's chain
 * capacity in workgroups (CUs, or INET_CHAIN_CUS), group counters of a sync area}.  0, or -1 for H, B, T <= 0, nprob outside 1..4 or a
 * null output -- nothing is written then. */
int inet_gru_chain_plan(int H, int B, int T, int nprob, int save, int64_t* out32);
/* What an LSTM layer of B rows, T steps and hidden size H launches under the options set now (inet_set_option key 4), without a GPU:
 * the planner every launch site of csrc/lstm.hip reads.  pipeline = 0: inet_lstm_fwd / _bwd (one chain launch over all T steps);
 * pipeline != 0: inet_lstm2_fwd / _bwd, which run two chain launches side by side -- both must be resident together, so the row
 * tile is the smallest MS in {1, 2, 4} with 2 * groups * (H / 16) <= chain capacity, and no tile means the pipeline refuses the
 * shape (inet_lstm2_ok = 0).  out16 = {ok (0: one launch per step; the pipeline: inet_lstm2_fwd returns 1), MS (16 * MS rows per
 * group), groups, members per group (H / 16), workgroups of one launch that stay for all its steps (groups * members), blocks
 * launched, forward launches on the tagged hand-off (label suffix " tag"), time steps per launch (pipeline: the chunk), launches per
 * layer, one backward counter area per chunk (pipeline with at most 16 chunks), chain capacity in workgroups (CUs, or
 * INET_CHAIN_CUS), launches side by side (1 or 2), group counters of a counter area, words between two group counters, words of a
 * counter area, 0}; everything in front of the chain capacity is 0 when ok is.  0, or -1 for B, T, H < 1 or a null output -- nothing is
 * written then. */
int inet_lstm_chain_plan(int B, int T, int H, int pipeline, int64_t* out16);
/* Loads every kernel of the library on the CURRENT device (code objects and function objects, which the HIP runtime otherwise
 * builds lazily on the launch path of each kernel's first launch: csrc/preload.hip) without launching anything.  Idempotent per
 * device; returns the number of kernels touched (0 when the device was done already), -2 without a device or on a runtime
 * failure.  The trainers call it at construction, so that no training step pays a first launch. */
int inet_preload(void);
/* Number of __global__ kernels the library registered with the HIP runtime (no GPU needed). */
int inet_kernel_count(void);

/* ---- measurement hooks (bench.py roofline line; not part of the reference surface) --------------- */
/* class 0 = batched MFMA GEMM, 1 = fused GRU/LSTM step forward, 2 = fused GRU/LSTM step backward, 3 = HBM-bound
 * pointwise kernels (the fused Adam update).  While enabled every
 * launch of those kernels is bracketed by hipEventRecord on its stream; read() synchronises and returns the
 * number of launches, the summed event time (ms) and the summed algorithmic FLOPs (2*M*N*K) of the class. */
int inet_prof_enable(int on);
int inet_prof_read(int cls, int64_t* launches, double* total_ms, double* total_flops);
/* per-launch CSV (class,label,us,gflop,mbytes) of everything recorded since inet_prof_enable(1); the label names the
 * kernel instantiation and shape, mbytes = algorithmic HBM bytes of the launch (operands once, results once) */
int inet_prof_dump(const char* path);

#ifdef __cplusplus
}
#endif
#endif /* INPAINTNET_HIP_H */
