"""Thin functional layer over the C-ABI: torch tensors in, torch tensors out.

torch is used here only for device memory and the current stream; every number
is produced by the HIP kernels behind include/inpaintnet_hip.h.  All functions
are asynchronous on torch's current stream.
"""
import contextlib
import ctypes as C
import math

import torch

from . import _lib
from ._lib import VaeConfig, LatentConfig, check, ptr, stream_ptr


# Whether autograd is recording OUTSIDE the custom Function whose forward is running (inside Function.forward grad mode is
# always off, and ctx.needs_input_grad only reflects requires_grad flags -- a trainable model evaluated under
# torch.no_grad() would otherwise save its backward activations and miss the save-free inference kernels).
_OUTER_GRAD = [True]


class TrackedFunction(torch.autograd.Function):
    """autograd.Function whose call() records the caller's grad mode first (read it with ops.outer_grad())."""

    @classmethod
    def call(cls, *args):
        _OUTER_GRAD[0] = torch.is_grad_enabled()
        return cls.apply(*args)


def outer_grad():
    return _OUTER_GRAD[0]


def _f32c(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return t


def _i64c(t):
    assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return t


def vae_config(num_notes, emb_dim=10, enc_hidden=512, z_dim=256, dec_hidden=512, beats=4, ticks_per_beat=6):
    return VaeConfig(num_notes, emb_dim, enc_hidden, z_dim, dec_hidden, beats, ticks_per_beat)


def _entries(cfg, count_fn, info_fn):
    n = count_fn(C.byref(cfg))
    if n < 0:
        raise ValueError("invalid model configuration (hidden sizes must be multiples of 16)")
    out = []
    for i in range(n):
        name = C.create_string_buffer(160)
        off = C.c_int64()
        dims = (C.c_int64 * 4)()
        nd = C.c_int()
        check(info_fn(C.byref(cfg), i, name, 160, C.byref(off), dims, C.byref(nd)), "param_info")
        out.append((name.value.decode(), off.value, tuple(dims[j] for j in range(nd.value))))
    return out


def vae_param_table(cfg):
    """[(state_dict key, offset in floats, shape)], total floats -- from the C library."""
    L = _lib.lib()
    return _entries(cfg, L.inet_vae_param_count, L.inet_vae_param_info), L.inet_vae_param_floats(C.byref(cfg))


def latent_param_table(cfg):
    L = _lib.lib()
    return _entries(cfg, L.inet_latent_param_count, L.inet_latent_param_info), L.inet_latent_param_floats(C.byref(cfg))


def _ws(nbytes, device):
    return torch.empty((int(nbytes) + 3) // 4, dtype=torch.float32, device=device)


# ----------------------------------------------------------------------------- encoder
def encoder_ws(cfg, B, save, device):
    n = _lib.lib().inet_vae_encoder_ws_bytes(C.byref(cfg), B, int(save))
    if n < 0:
        raise ValueError("encoder_ws: invalid arguments")
    return _ws(n, device)


def encoder_fwd(cfg, tokens, params, mask=None, save=False, ws=None):
    """tokens [B,T] int64 -> mu, logsigma [B,Z], ws"""
    _i64c(tokens); _f32c(params)
    B = tokens.shape[0]
    if ws is None:
        ws = encoder_ws(cfg, B, save, tokens.device)
    mu = torch.empty(B, cfg.z_dim, dtype=torch.float32, device=tokens.device)
    ls = torch.empty_like(mu)
    check(_lib.lib().inet_vae_encoder_fwd(C.byref(cfg), B, ptr(tokens), ptr(params), ptr(mask), ptr(mu), ptr(ls),
                                          ptr(ws), ws.numel() * 4, int(save), stream_ptr()), "inet_vae_encoder_fwd")
    return mu, ls, ws


# ----------------------------------------------------------------------------- deferred side-stream joins
_DEFER = False
_HELD = []


def side_defer(on, release=True):
    """Deferred joins (include/inpaintnet_hip.h, inet_set_option key 1): the *_bwd calls stop making the current stream
    wait for the side stream; every tensor they were given is kept alive here until side_join().  release=False when
    leaving deferred mode: the current stream joins, the held tensors stay until release_held() (Trainer.step keeps
    them across the gradient exchange)."""
    global _DEFER
    if not on and _DEFER:
        side_join(release=release)
    _DEFER = bool(on)
    check(_lib.lib().inet_set_option(1, int(_DEFER)), "inet_set_option")


def side_join(release=True):
    """Make the current stream wait for all side-stream work, then release the tensors held for it."""
    check(_lib.lib().inet_side_join(stream_ptr()), "inet_side_join")
    if release:
        _HELD.clear()


def release_held():
    _HELD.clear()


def side_join_on(stream):
    """Make `stream` (a torch.cuda.Stream that is NOT the one the library calls were issued on) wait for all side-stream
    work queued so far.  Nothing is consumed or released (inet_side_wait): the issuing stream has not been ordered after
    that work and still joins it at its own next join (dp.start_bucket uses this to start an all-reduce behind the leaf
    GEMMs without stalling the backward pass)."""
    check(_lib.lib().inet_side_wait(C.c_void_p(stream.cuda_stream)), "inet_side_wait")


def arnn_generate_ok(E, Hc, H, U, V):
    """The shapes the one-row kernels of inet_arnn_generate are built for (csrc/arnn_gen.hip: arnn_ticks_ok, the template bounds;
    keep the two equal); callers keep their per-tick loop for anything else."""
    return E + Hc <= 320 and H <= 256 and H % 16 == 0 and U <= 256 and V <= 256


def arnn_generate(emb, oc0, W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, W1, b1, W2, b2, hc_init=None, first_tok=None):
    """inet_arnn_generate: the L argmax tokens of batch element 0 of AnticipationRNN's free-running pass.  oc0 [L,Hc] (rows may be
    strided); hc_init [2,2,H] (layer, h|c) or None (zeros); first_tok: 1-element int64 device tensor or None (token 0);
    -> tokens [L] int64 on the device, no host round trip."""
    L, Hc = oc0.shape
    assert oc0.stride(1) == 1
    E, H, U, V = emb.shape[1], W_hh0.shape[1], W1.shape[0], W2.shape[0]
    net = [ptr(_f32c(t)) for t in (W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, W1, b1, W2, b2)]
    nws = int(_lib.lib().inet_arnn_generate_ws_floats(L, E, Hc, H, U, V))
    ws = torch.empty(nws, dtype=torch.float32, device=emb.device)
    tokens = torch.empty(L, dtype=torch.int64, device=emb.device)
    check(_lib.lib().inet_arnn_generate(L, E, Hc, H, U, V, ptr(_f32c(emb)), ptr(oc0), oc0.stride(0), *net,
                                        ptr(_f32c(hc_init) if hc_init is not None else None),
                                        ptr(_i64c(first_tok) if first_tok is not None else None), ptr(tokens), ptr(ws), nws,
                                        stream_ptr()), "inet_arnn_generate")
    _hold(ws, oc0, hc_init, first_tok)
    if _ARNN_KEEP_WS:                                # diagnostics (tools/arnn_token_pass.py reads the kernel's phase stamps out of it)
        _ARNN_KEEP_WS[:] = [ws]
    return tokens


_ARNN_KEEP_WS = []


def arnn_sample(emb, oc, W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, W1, b1, W2, b2, temperature, uniforms, hc_init=None,
                top_k=None, top_p=None, want_logp=False, want_logits=False, allowed=None, forced=None):
    """inet_arnn_sample: AnticipationRNN's temperature-sampled generation for R independent rows.  oc [R,L,Hc] (the rows' constraint
    outputs; strided rows and ticks allowed); uniforms [R,L] float64 (one np.random.random_sample() double per tick; a host array is
    copied to the device); hc_init [R,2,2,H] (layer, h|c) or None (zeros).  Token t of row r is the first v whose
    softmax(temperature * logits) prefix exceeds uniforms[r, t] (np.random.choice's rule) -> tokens [R,L] int64 on the device, no
    host round trip.
    Every call goes through inet_arnn_sample_fx, the widest entry, with nulls for what it does not ask (the library picks the
    kernels by what it is handed: a plain call runs the kernels of inet_arnn_sample).  With one of top_k / top_p / want_logp /
    want_logits: the draw behind csrc/sample.h's top-k / nucleus truncation (top_k None, <= 0 or >= V: off; top_p None or 1: off,
    else in (0, 1)) -> (tokens, logp [R,L] float32 or None: the drawn tokens' log-probabilities under the truncated distribution,
    NaN where a tick took the argmax rule; logits [R,L,V] float32 or None: the note head's output every tick drew from).
    allowed: pack_allowed()'s words [R,L,ceil(V/64)], int64, contiguous, on the device: the tokens each (row, tick) may return,
    applied inside the launch in front of the truncation (csrc/sample.h).  A constrained call is a truncating
    one: allowed alone runs with (top_k, top_p) = (0, 1.0), and the return is the triple above.
    forced: int32 [R,L], contiguous, on the device, -1 for a free tick: a value in [0, V) is that tick's token, returned and fed
    back whatever the mask, the truncation and the uniform hold, with its log-probability under the masked and truncated
    distribution (-inf for a banned or truncated token; csrc/sample.h).  forced alone runs with (top_k, top_p)
    = (0, 1.0) and returns logp."""
    ex = top_k is not None or top_p is not None or want_logp or want_logits or allowed is not None or forced is not None
    k = _top_k(top_k)
    if top_p is not None and not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"arnn_sample: top_p {top_p!r} outside (0, 1]")
    R, L, Hc = oc.shape
    if allowed is not None:
        nw = (W2.shape[0] + 63) // 64
        if not (isinstance(allowed, torch.Tensor) and allowed.is_cuda and allowed.dtype == torch.int64 and allowed.is_contiguous()
                and tuple(allowed.shape) == (R, L, nw)):
            raise ValueError(f"arnn_sample: allowed must be pack_allowed()'s contiguous int64 device tensor of shape {(R, L, nw)}")
    if forced is not None:
        if not (isinstance(forced, torch.Tensor) and forced.is_cuda and forced.dtype == torch.int32 and forced.is_contiguous()
                and tuple(forced.shape) == (R, L)):
            raise ValueError(f"arnn_sample: forced must be a contiguous int32 device tensor of shape {(R, L)}")
        want_logp = True
    assert oc.is_cuda and oc.dtype == torch.float32 and oc.stride(2) == 1
    E, H, U, V = emb.shape[1], W_hh0.shape[1], W1.shape[0], W2.shape[0]
    net = [ptr(_f32c(t)) for t in (W_ih0, b_ih0, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, W1, b1, W2, b2)]
    u = torch.as_tensor(uniforms, dtype=torch.float64).to(emb.device).contiguous()
    if tuple(u.shape) != (R, L):
        raise ValueError(f"arnn_sample: uniforms of shape {tuple(u.shape)}, expected {(R, L)}")
    if hc_init is not None and tuple(hc_init.shape) != (R, 2, 2, H):
        raise ValueError(f"arnn_sample: hc_init of shape {tuple(hc_init.shape)}, expected {(R, 2, 2, H)}")
    nws = int(_lib.lib().inet_arnn_sample_ws_floats(R, L, E, Hc, H, U, V))
    if nws < 0:
        raise ValueError("inet_arnn_sample_ws_floats: invalid arguments")
    ws = torch.empty(nws, dtype=torch.float32, device=emb.device)
    tokens = torch.empty(R, L, dtype=torch.int64, device=emb.device)
    logp = torch.empty(R, L, dtype=torch.float32, device=emb.device) if want_logp else None
    logits = torch.empty(R, L, V, dtype=torch.float32, device=emb.device) if want_logits else None
    # one entry, the widest, with nulls for what the call does not ask: the library picks the kernels by what it is handed
    check(_lib.lib().inet_arnn_sample_fx(R, L, E, Hc, H, U, V, ptr(_f32c(emb)), ptr(oc), oc.stride(1), oc.stride(0), *net,
                                         float(temperature), ptr(u), ptr(_f32c(hc_init) if hc_init is not None else None), ptr(tokens),
                                         ptr(ws), nws, k, 1.0 if top_p is None else float(top_p), ptr(logp), ptr(logits), ptr(allowed),
                                         ptr(forced), stream_ptr()), "inet_arnn_sample_fx")
    _hold(ws, oc, u, hc_init, allowed, forced)
    return (tokens, logp, logits) if ex else tokens


_twin = {}


def twin_stream(device=None):
    """The library's second compute stream as a torch stream (inet_twin_stream).  Work that should run beside the caller's stream
    goes HERE, not on a new torch.cuda.Stream(): a fifth busy stream in the process gets every stream time-sliced."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _twin:
        h = C.c_void_p()
        check(_lib.lib().inet_twin_stream(C.byref(h)), "inet_twin_stream")
        _twin[key] = torch.cuda.ExternalStream(h.value, device=dev)
    return _twin[key]


def _hold(*tensors):
    if _DEFER:
        _HELD.append(tensors)


def encoder_bwd(cfg, tokens, params, grads, mask, dmu, dls, ws, stage=0):
    """stage 0: the whole pass; 1 then 2: heads + layer 1, then layer 0 + embedding (include/inpaintnet_hip.h)."""
    B = tokens.shape[0]
    _f32c(dmu); _f32c(dls); _f32c(grads)
    _hold(tokens, params, grads, mask, dmu, dls, ws)
    check(_lib.lib().inet_vae_encoder_bwd(C.byref(cfg), B, ptr(tokens), ptr(params), ptr(grads), ptr(mask), ptr(dmu),
                                          ptr(dls), ptr(ws), ws.numel() * 4, int(stage), stream_ptr()),
          "inet_vae_encoder_bwd")


# ----------------------------------------------------------------------------- decoder
def decoder_ws(cfg, B, save, device):
    n = _lib.lib().inet_vae_decoder_ws_bytes(C.byref(cfg), B, int(save))
    if n < 0:
        raise ValueError("decoder_ws: invalid arguments")
    return _ws(n, device)


def decoder_fwd(cfg, z, target, teacher_forced, params, mask_beat=None, mask_tick=None, save=False, ws=None,
                multinomial_seed=0, temperature=None, uniforms=None, top_k=None, top_p=None, logp=None, allowed=None,
                forced=None):
    """z [B,Z] -> weights [B,T,V], samples [B,1,T] int64, ws.  multinomial_seed != 0: the fed-back tokens are drawn from
    softmax(weights) (decoder.py:506-509) instead of the argmax.  temperature + uniforms ([B,T] float64 on the device, one uniform
    per row and tick): inet_vae_decoder_sample_fx, the widest entry, with nulls for what the call does not ask -- a free-running
    call whose tokens are drawn from softmax(temperature * weights) by csrc/sample.h's rule.  top_k / top_p / logp (with a
    temperature only): the draw behind sample.h's top-k / nucleus truncation (top_k None, <= 0 or >= V: off; top_p None or 1: off,
    else in (0, 1)), and logp, a contiguous float32 [B,T] device tensor, receives the drawn tokens' log-probabilities under the
    truncated distribution (NaN where a tick took the argmax).
    allowed (with a temperature only): pack_allowed()'s words [B,T,ceil(V/64)], int64, contiguous, on the device: the tokens every
    (row, tick) may return, applied in front of the truncation inside the launch (csrc/sample.h's rule).
    forced (with a temperature only): int32 [B,T], contiguous, on the device: the token every (row, tick) returns and feeds back, -1
    (any value outside [0, V)) for a free tick; its logp is taken under the masked and truncated distribution (-inf for a banned or
    truncated token), with or without `allowed`."""
    if (temperature is None) != (uniforms is None):
        raise ValueError("decoder_fwd: temperature and uniforms go together")
    if temperature is None and (top_k is not None or top_p is not None or logp is not None or allowed is not None or forced is not None):
        raise ValueError("decoder_fwd: top_k / top_p / logp / allowed / forced without a temperature")
    if top_p is not None and not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"decoder_fwd: top_p {top_p!r} outside (0, 1]")
    _f32c(z); _f32c(params)
    B = z.shape[0]
    T = cfg.beats * cfg.ticks_per_beat
    if temperature is not None:
        if teacher_forced or multinomial_seed:
            raise ValueError("decoder_fwd: temperature sampling is a free-running call without a multinomial seed")
        if not math.isfinite(float(temperature)):
            raise ValueError(f"decoder_fwd: temperature {temperature!r} is not finite")
        if not (uniforms.is_cuda and uniforms.dtype == torch.float64 and uniforms.is_contiguous() and tuple(uniforms.shape) == (B, T)):
            raise ValueError(f"decoder_fwd: uniforms must be a contiguous float64 device tensor of shape {(B, T)}")
        if logp is not None and not (logp.is_cuda and logp.dtype == torch.float32 and logp.is_contiguous() and tuple(logp.shape) == (B, T)):
            raise ValueError(f"decoder_fwd: logp must be a contiguous float32 device tensor of shape {(B, T)}")
        if allowed is not None:
            nw = (cfg.num_notes + 63) // 64
            if not (allowed.is_cuda and allowed.dtype == torch.int64 and allowed.is_contiguous() and tuple(allowed.shape) == (B, T, nw)):
                raise ValueError(f"decoder_fwd: allowed must be pack_allowed()'s contiguous int64 device tensor of shape {(B, T, nw)}")
        if forced is not None and not (forced.is_cuda and forced.dtype == torch.int32 and forced.is_contiguous() and tuple(forced.shape) == (B, T)):
            raise ValueError(f"decoder_fwd: forced must be a contiguous int32 device tensor of shape {(B, T)}")
    if target is not None:
        _i64c(target)
    if ws is None:
        ws = decoder_ws(cfg, B, save, z.device)
    weights = torch.empty(B, T, cfg.num_notes, dtype=torch.float32, device=z.device)
    samples = torch.empty(B, 1, T, dtype=torch.int64, device=z.device)
    if temperature is not None:                      # one entry, the widest, with nulls for what the call does not ask
        check(_lib.lib().inet_vae_decoder_sample_fx(C.byref(cfg), B, ptr(z), ptr(params), ptr(mask_beat), ptr(mask_tick), ptr(weights),
                                                    ptr(samples), ptr(ws), ws.numel() * 4, int(save), float(temperature), ptr(uniforms),
                                                    _top_k(top_k), 1.0 if top_p is None else float(top_p), ptr(logp), ptr(allowed),
                                                    ptr(forced), stream_ptr()),
              "inet_vae_decoder_sample_fx")
        _hold(uniforms, logp, allowed, forced)
        return weights, samples, ws
    check(_lib.lib().inet_vae_decoder_fwd(C.byref(cfg), B, ptr(z), ptr(target), int(bool(teacher_forced)), ptr(params),
                                          ptr(mask_beat), ptr(mask_tick), ptr(weights), ptr(samples), ptr(ws),
                                          ws.numel() * 4, int(save), int(multinomial_seed) & (2 ** 64 - 1), stream_ptr()),
          "inet_vae_decoder_fwd")
    return weights, samples, ws


DECODER_ROUTE_KEYS = ("beats", "ticks", "npl", "chunk_rows", "b1", "b1_fused", "zero", "pack_beat_twins", "pack_tick_twins", "pack_out_w",
                      "pack_ht0", "pk", "fused_prezeroed", "beat_areas", "tick_areas", "self_zeroed")
DECODER_BEATS = ("steps", "chained", "folded")
DECODER_TICKS = ("TfChained", "TfSteps", "Fused", "FusedChunked", "PerTick")
DECODER_ZERO = ("none", "sync", "b1ex+sync")
DECODER_HT0 = ("no", "once", "per_chunk")


def decoder_route(cfg, B, save=False, teacher_forced=False, multinomial_seed=False, mask_beat=False, mask_tick=False, level=0):
    """What decoder_fwd launches for such a call under the options set now, without a GPU (inet_vae_decoder_route, the function the
    launch itself asks): a dict of DECODER_ROUTE_KEYS with "beats", "ticks", "zero" and "pack_ht0" as names (DECODER_BEATS,
    DECODER_TICKS, DECODER_ZERO, DECODER_HT0) and the flags as bools; "beat_areas" / "tick_areas": bit a = the path's launches count on sync
    area a; "self_zeroed": how many launches zero their own counters.  level: 0 argmax, 1 temperature, 2 truncated, 3 masked, 4 forced."""
    out = (C.c_int32 * 16)()
    flags = int(bool(multinomial_seed)) | 2 * int(mask_beat is not None and mask_beat is not False) | \
        4 * int(mask_tick is not None and mask_tick is not False)
    check(_lib.lib().inet_vae_decoder_route(C.byref(cfg), int(B), int(bool(save)), int(bool(teacher_forced)), flags, int(level), out, 16),
          "inet_vae_decoder_route")
    r = dict(zip(DECODER_ROUTE_KEYS, out))
    r["beats"], r["ticks"] = DECODER_BEATS[r["beats"]], DECODER_TICKS[r["ticks"]]
    r["zero"], r["pack_ht0"] = DECODER_ZERO[r["zero"]], DECODER_HT0[r["pack_ht0"]]
    for k in ("b1", "b1_fused", "pack_beat_twins", "pack_tick_twins", "pack_out_w", "pk", "fused_prezeroed"):
        r[k] = bool(r[k])
    return r


def decoder_bwd(cfg, dweights, weights, samples, params, grads, mask_beat, mask_tick, ws, need_dz=True):
    B = weights.shape[0]
    _f32c(dweights); _f32c(weights); _i64c(samples)
    dz = torch.empty(B, cfg.z_dim, dtype=torch.float32, device=weights.device) if need_dz else None
    _hold(dweights, weights, samples, params, grads, mask_beat, mask_tick, ws)
    check(_lib.lib().inet_vae_decoder_bwd(C.byref(cfg), B, ptr(dweights), ptr(weights), ptr(samples), ptr(params),
                                          ptr(grads), ptr(mask_beat), ptr(mask_tick), ptr(dz), ptr(ws), ws.numel() * 4,
                                          stream_ptr()), "inet_vae_decoder_bwd")
    return dz


# ----------------------------------------------------------------------------- losses
def cross_entropy(weights2d, targets1d, out2, dW=None, scale=1.0, out_scale=1.0):
    """weights2d [rows,V] (row stride = stride(0)); out2: 2-float accumulator (loss_sum, correct), both times out_scale."""
    rows, V = weights2d.shape
    assert weights2d.stride(1) == 1
    _i64c(targets1d)
    check(_lib.lib().inet_cross_entropy(ptr(weights2d), weights2d.stride(0), rows, V, ptr(targets1d), ptr(dW),
                                        dW.stride(0) if dW is not None else 0, float(scale), float(out_scale),
                                        ptr(out2[0:1]), ptr(out2[1:2]), stream_ptr()), "inet_cross_entropy")


def cross_entropy_ex(weights2d, targets1d, loss_sum=None, correct=None, dW=None, scale=1.0, scale_dev=None, out_scale=1.0,
                     add_term=None, add_scale=0.0, fwd_out=None, fwd_scale=0.0):
    """inet_cross_entropy_ex: cross_entropy() with nullable outputs, a device-scalar factor on dW and an extra term added to
    the loss (loss_sum / correct / add_term / scale_dev: 1-element float tensors or None)."""
    rows, V = weights2d.shape
    assert weights2d.stride(1) == 1
    _i64c(targets1d)
    check(_lib.lib().inet_cross_entropy_ex(ptr(weights2d), weights2d.stride(0), rows, V, ptr(targets1d), ptr(dW),
                                           dW.stride(0) if dW is not None else 0, float(scale), ptr(scale_dev),
                                           float(out_scale), ptr(loss_sum), ptr(correct), ptr(add_term), float(add_scale),
                                           ptr(fwd_out), float(fwd_scale), stream_ptr()), "inet_cross_entropy_ex")


CE_META_WORDS = 8                    # the words in front of the counts (include/inpaintnet_hip.h): denom, n_valid, n_bad, two tickets, W, two spare


class ClassCounts:
    """What inet_class_counts left on the device: `block` (CE_META_WORDS + V int64) and views of it -- counts (V,) int64, n_valid and
    n_bad () int64, denom () float64 = sum_c w_c counts_c.  Reading any of them is the caller's synchronisation."""
    __slots__ = ("block", "V", "counts", "extra", "n_valid", "n_bad", "denom")

    def __init__(self, block, V):
        self.block, self.V = block, V
        self.counts = block[CE_META_WORDS:CE_META_WORDS + V]
        self.extra = block[CE_META_WORDS + V:]                                  # the words the caller asked to have zeroed along
        self.n_valid, self.n_bad = block[1], block[2]
        self.denom = block[0:1].view(torch.float64)[0]


def _ce_common(name, V, weight, label_smoothing, ignore_index, device):
    """(class weights or None, smoothing as a float, ignore_index as a ctypes reference or None), checked."""
    if weight is not None:
        if not (isinstance(weight, torch.Tensor) and weight.dtype == torch.float32 and weight.dim() == 1 and weight.numel() == V
                and weight.is_contiguous() and weight.device == device):
            raise ValueError(f"{name}: weight must be None or a contiguous float32 tensor of {V} class weights on the logits' device")
    e = float(label_smoothing)
    if not 0.0 <= e <= 1.0:                                                     # (NaN fails both comparisons)
        raise ValueError(f"{name}: label_smoothing must lie in [0, 1], got {label_smoothing!r}")
    if ignore_index is not None:
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not -2 ** 63 <= ignore_index < 2 ** 63:
            raise ValueError(f"{name}: ignore_index must be None or an int, got {ignore_index!r}")
        ignore_index = C.byref(C.c_int64(ignore_index))
    return weight, e, ignore_index


def class_counts(targets, V, weight=None, ignore_index=None, extra=0):
    """targets: any shape, int64, contiguous, on the device -> ClassCounts (inet_class_counts): the histogram
    of the targets over [0, V), how many are valid, how many lie outside [0, V) without being ignore_index (never used as an index;
    the launch sets the token status word: check_tokens() raises) and denom = sum_c weight_c counts_c in double, in class order.
    Integer atomics only: the same bits on every call.  extra: int64 words behind the counts that the call zeroes along (`.extra`)."""
    if not (isinstance(targets, torch.Tensor) and targets.is_cuda and targets.dtype == torch.int64 and targets.is_contiguous()
            and targets.numel() >= 1):
        raise ValueError("class_counts: targets must be a non-empty contiguous int64 device tensor")
    if isinstance(V, bool) or not isinstance(V, int) or V < 1:
        raise ValueError(f"class_counts: V must be an int >= 1, got {V!r}")
    weight, _, ign = _ce_common("class_counts", V, weight, 0.0, ignore_index, targets.device)
    block = torch.empty(CE_META_WORDS + V + int(extra), dtype=torch.int64, device=targets.device)
    check(_lib.lib().inet_class_counts(ptr(targets), targets.numel(), V, ptr(weight), ign, ptr(block), int(extra), stream_ptr()),
          "inet_class_counts")
    return ClassCounts(block, V)


def cross_entropy_w(weights2d, targets1d, counted, weight=None, label_smoothing=0.0, ignore_index=None, loss=None, accuracy=None,
                    dW=None, scale_dev=None, add_term=None, add_scale=0.0, fwd_out=None, fwd_scale=0.0, class_stats=None,
                    confusion=None):
    """inet_cross_entropy_w: torch's F.cross_entropy(weights2d, targets1d, weight, label_smoothing=,
    ignore_index=, reduction='mean') and its gradient, one wavefront per row, the row read once.  counted: the ClassCounts of the SAME
    targets, weight and ignore_index (the backward passes the forward's).  Outputs, each optional: loss / accuracy (1-element float
    tensors, written), dW [rows, >= V] (times scale_dev[0] when given; an ignored row is exactly 0), fwd_out = fwd_scale * scale_dev,
    class_stats (V, 3) int64 += {target count, hits, predicted}, confusion (V, V) int64 += 1 at [target, argmax] (the caller zeroes
    them).  add_term / add_scale: loss += add_scale * add_term[0].  With denom == 0 the loss is NaN and dW all zeros."""
    rows, V = weights2d.shape
    assert weights2d.is_cuda and weights2d.dtype == torch.float32 and weights2d.stride(1) == 1
    _i64c(targets1d)
    if targets1d.numel() != rows:
        raise ValueError(f"cross_entropy_w: {rows} rows of logits but {targets1d.numel()} targets")
    if not isinstance(counted, ClassCounts) or counted.V != V:
        raise ValueError("cross_entropy_w: counted must be the ClassCounts of these targets at this V")
    weight, e, ign = _ce_common("cross_entropy_w", V, weight, label_smoothing, ignore_index, weights2d.device)
    for name, t, shape in (("class_stats", class_stats, (V, 3)), ("confusion", confusion, (V, V))):
        if t is not None and not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"cross_entropy_w: {name} must be a contiguous int64 device tensor of shape {shape}")
    if dW is not None:
        assert dW.is_cuda and dW.dtype == torch.float32 and dW.stride(1) == 1 and dW.shape[0] == rows and dW.shape[1] == V
    L = _lib.lib()
    ws = _ws(L.inet_cross_entropy_w_ws_bytes(rows), weights2d.device) if loss is not None or accuracy is not None else None
    check(L.inet_cross_entropy_w(ptr(weights2d), weights2d.stride(0), rows, V, ptr(targets1d), ptr(weight), e, ign, ptr(counted.block),
                                 ptr(dW), dW.stride(0) if dW is not None else 0, ptr(scale_dev), ptr(loss), ptr(accuracy),
                                 ptr(add_term), float(add_scale), ptr(fwd_out), float(fwd_scale), ptr(class_stats), ptr(confusion),
                                 ptr(ws), ws.numel() * 4 if ws is not None else 0, stream_ptr()), "inet_cross_entropy_w")


def sample_multinomial(weights2d, seed, offset=0):
    """One draw per row from softmax(weights2d[row]) (decoder.py:506-509), counter-based generator (seed, offset + row)."""
    rows, V = weights2d.shape
    assert weights2d.stride(1) == 1 and weights2d.dtype == torch.float32
    out = torch.empty(rows, dtype=torch.int64, device=weights2d.device)
    check(_lib.lib().inet_sample_multinomial(ptr(weights2d), weights2d.stride(0), rows, V, ptr(out), 1,
                                             int(seed) & (2 ** 64 - 1), int(offset), stream_ptr()), "inet_sample_multinomial")
    return out


def sample_temperature(weights2d, temperature, uniforms):
    """inet_sample_temperature: one token per row of weights2d [rows,V] (row stride = stride(0)) from softmax(temperature * row) with
    the row's uniform (uniforms [rows] float64 on the device, any stride), by csrc/sample.h's rule."""
    rows, V = weights2d.shape
    assert weights2d.stride(1) == 1 and weights2d.dtype == torch.float32
    assert uniforms.is_cuda and uniforms.dtype == torch.float64 and tuple(uniforms.shape) == (rows,)
    out = torch.empty(rows, dtype=torch.int64, device=weights2d.device)
    check(_lib.lib().inet_sample_temperature(ptr(weights2d), weights2d.stride(0), rows, V, float(temperature), ptr(uniforms),
                                             uniforms.stride(0), ptr(out), 1, stream_ptr()), "inet_sample_temperature")
    return out


def _top_k(top_k):
    """top_k as the C int the library takes: None = 0 (off), anything beyond an int's range is off as well; ValueError for a value
    that is no integer (2.5, NaN)"""
    if top_k is None:
        return 0
    if isinstance(top_k, bool) or top_k != top_k or top_k in (float("inf"), float("-inf")) or int(top_k) != top_k:
        raise ValueError(f"top_k {top_k!r} is not an integer")
    return max(0, min(int(top_k), 2 ** 31 - 1))


def pack_allowed(allowed):
    """bool [..., V] (a tensor or an array: token v may be returned) -> int64 [..., ceil(V / 64)] with the bit patterns of csrc/sample.h's
    mask words: token v is bit v % 64 of word v // 64, the bits at or above V are zero.  Packed on the host; the result lies on the
    input's device (the CPU for an array).  ValueError for a (row, tick) with nothing allowed, or for what is no boolean mask."""
    import numpy as np
    dev = allowed.device if isinstance(allowed, torch.Tensor) else torch.device("cpu")
    a = allowed.detach().cpu().numpy() if isinstance(allowed, torch.Tensor) else np.asarray(allowed)
    if a.dtype != np.bool_ or a.ndim < 1 or a.shape[-1] < 1:
        raise ValueError("pack_allowed: a boolean mask [..., V] with V >= 1")
    if not a.any(-1).all():
        where = np.argwhere(~a.any(-1))[0].tolist()
        raise ValueError(f"pack_allowed: nothing is allowed at {where}")
    V = a.shape[-1]
    nw = (V + 63) // 64
    bits = np.zeros(a.shape[:-1] + (nw * 64,), dtype=np.uint8)
    bits[..., :V] = a
    words = np.packbits(bits.reshape(a.shape[:-1] + (nw, 64)), axis=-1, bitorder="little")     # 8 bytes per word, the lowest first
    words = np.ascontiguousarray(words).view("<u8").reshape(a.shape[:-1] + (nw,)).astype(np.int64)
    return torch.from_numpy(words).to(dev)


def sample_truncated(weights2d, temperature, uniforms, top_k=None, top_p=None, want_logp=True, allowed=None, forced=None):
    """inet_sample_forced with nulls for what is not given (inet_sample_truncated's kernel at the least): sample_temperature() behind
    csrc/sample.h's top-k / nucleus truncation (top_k None, <= 0 or >= V: off; top_p None or 1: off, else in (0, 1)) -> (tokens
    [rows] int64, logp [rows] float32: the drawn tokens' log-probabilities under the truncated distribution, NaN where a row took
    the argmax rule; None with want_logp=False).  allowed: pack_allowed()'s words [rows, ceil(V / 64)] (int64 on the device, any row
    stride): the tokens each row may return.  forced: int32 [rows] on the device: the token each row returns whatever its mask and
    logits hold, -1 for a free row; its logp is taken under the masked and truncated distribution."""
    rows, V = weights2d.shape
    assert weights2d.stride(1) == 1 and weights2d.dtype == torch.float32
    assert uniforms.is_cuda and uniforms.dtype == torch.float64 and tuple(uniforms.shape) == (rows,)
    out = torch.empty(rows, dtype=torch.int64, device=weights2d.device)
    logp = torch.empty(rows, dtype=torch.float32, device=weights2d.device) if want_logp else None
    if allowed is not None:
        if not (allowed.is_cuda and allowed.dtype == torch.int64 and tuple(allowed.shape) == (rows, (V + 63) // 64) and allowed.stride(1) == 1):
            raise ValueError(f"sample_truncated: allowed must be pack_allowed()'s int64 device tensor of shape {(rows, (V + 63) // 64)}")
    if forced is not None and not (forced.is_cuda and forced.dtype == torch.int32 and tuple(forced.shape) == (rows,)):
        raise ValueError(f"sample_truncated: forced must be an int32 device tensor of shape {(rows,)}")
    check(_lib.lib().inet_sample_forced(ptr(weights2d), weights2d.stride(0), rows, V, float(temperature), ptr(uniforms),
                                        uniforms.stride(0), _top_k(top_k), 1.0 if top_p is None else float(top_p), ptr(out), 1,
                                        ptr(logp), 1, ptr(allowed), allowed.stride(0) if allowed is not None else 0, ptr(forced),
                                        forced.stride(0) if forced is not None else 0, stream_ptr()), "inet_sample_forced")
    return out, logp


def reparam_kl(mu, ls, eps, kl_sum=None, want_sigma=False):
    _f32c(mu); _f32c(ls)
    z = torch.empty_like(mu)
    sigma = torch.empty_like(mu) if want_sigma else None
    check(_lib.lib().inet_reparam_kl(ptr(mu), ptr(ls), ptr(eps), ptr(z), ptr(sigma), mu.numel(), ptr(kl_sum),
                                     stream_ptr()), "inet_reparam_kl")
    return z, sigma


def latent_bwd(dz, mu, ls, eps, kscale, kscale_dev=None):
    """Gradients of (mu, logsigma) from dz (nullable) and from the KL sum, whose upstream gradient is
    kscale * kscale_dev[0] (kscale_dev: optional device scalar)."""
    dmu = torch.empty_like(mu)
    dls = torch.empty_like(mu)
    _hold(kscale_dev)
    check(_lib.lib().inet_latent_bwd(ptr(dz), ptr(mu), ptr(ls), ptr(eps), float(kscale), ptr(kscale_dev), ptr(dmu),
                                     ptr(dls), mu.numel(), stream_ptr()), "inet_latent_bwd")
    return dmu, dls


FB_PER = {"measure": 0, "dim": 1}


def _fb_per(per):
    if per not in FB_PER:
        raise ValueError(f"free_nats_per must be 'measure' or 'dim', got {per!r}")
    return FB_PER[per]


def reparam_kl_fb(mu, ls, eps, free_nats, per, kl_sum=None, kl_raw=None, want_z=True):
    """The reparameterisation with the KL term summed into parts and floored at free_nats (include/inpaintnet_hip.h
    inet_reparam_kl_fb).  mu, ls [rows, Z]; eps the same shape or None (reads as 0); per 'measure' (a part per
    row, threshold free_nats) or 'dim' (a part per column, threshold rows * free_nats).  kl_sum / kl_raw: one-element device tensors
    the floored / the plain sum is ADDED onto (None: new zeroed ones).  -> (z or None, parts, keep, kl_sum, kl_raw); keep holds 1.0
    where a part is kept, !(part <= threshold), else 0.0."""
    _f32c(mu); _f32c(ls)
    if mu.dim() != 2 or ls.shape != mu.shape or (eps is not None and _f32c(eps).shape != mu.shape):
        raise ValueError("reparam_kl_fb: mu, logsigma (and eps) must be [rows, Z] tensors of one shape")
    rows, Z = mu.shape
    p = _fb_per(per)
    dev = mu.device
    z = torch.empty_like(mu) if want_z else None
    parts = torch.empty(Z if p else rows, dtype=torch.float32, device=dev)
    keep = torch.empty_like(parts)
    if kl_sum is None:
        kl_sum = torch.zeros(1, dtype=torch.float32, device=dev)
    if kl_raw is None:
        kl_raw = torch.zeros(1, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = L.inet_reparam_kl_fb_ws_bytes(rows, Z, p)
    ws = _ws(nbytes, dev) if nbytes > 0 else None
    check(L.inet_reparam_kl_fb(ptr(mu), ptr(ls), ptr(eps), ptr(z), rows, Z, float(free_nats), p, ptr(parts), ptr(keep),
                               ptr(_f32c(kl_sum)), ptr(_f32c(kl_raw)), ptr(ws), 0 if ws is None else ws.numel() * 4, stream_ptr()),
          "inet_reparam_kl_fb")
    return z, parts, keep, kl_sum, kl_raw


def latent_bwd_fb(dz, mu, ls, eps, kscale, keep, per, kscale_dev=None):
    """latent_bwd with reparam_kl_fb's keep vector: the KL gradient, kscale * kscale_dev[0], reaches the elements of kept parts only."""
    _f32c(mu); _f32c(ls); _f32c(keep)
    rows, Z = mu.shape
    p = _fb_per(per)
    if keep.numel() != (Z if p else rows):
        raise ValueError(f"latent_bwd_fb: keep must hold {Z if p else rows} elements for per={per!r}")
    dmu = torch.empty_like(mu)
    dls = torch.empty_like(mu)
    _hold(kscale_dev)
    check(_lib.lib().inet_latent_bwd_fb(ptr(dz), ptr(mu), ptr(ls), ptr(eps), float(kscale), ptr(kscale_dev), ptr(keep), p, ptr(dmu),
                                        ptr(dls), rows, Z, stream_ptr()), "inet_latent_bwd_fb")
    return dmu, dls


MMD_KERNEL = {"gaussian": 0, "imq": 1}
MMD_ESTIMATORS = ("unbiased", "biased", "reference")


def mmd_weights(B, estimator):
    """(a, c, diag) of value = coeff (a (S_xx - diag B) + a (S_yy - diag B) - c S_xy) for B samples a side:
    'unbiased' (B >= 2) drops the self terms' diagonals and divides by B (B - 1); 'biased' is the V-statistic; 'reference' is
    VAETrainer.compute_mmd_loss of the reference as written, diagonals in, 1 / (B (B - 1)) / 2 on the self terms (1 at B = 1)."""
    if estimator not in MMD_ESTIMATORS:
        raise ValueError(f"mmd estimator must be one of {MMD_ESTIMATORS}, got {estimator!r}")
    B = int(B)
    if B < 1:
        raise ValueError("mmd: B must be >= 1")
    c = 2.0 / (B * B)
    if estimator == "unbiased":
        if B < 2:
            raise ValueError("the 'unbiased' MMD estimator needs B >= 2")
        return 1.0 / (B * (B - 1)), c, 1.0
    if estimator == "biased":
        return 1.0 / (B * B), c, 0.0
    return (1.0 / (B * (B - 1)) / 2 if B > 1 else 1.0), c, 0.0


def mmd(z, z_prior, kernel="gaussian", bandwidth=None, estimator="unbiased", coeff=1.0, want_grad=False):
    """The MMD between the samples z and z_prior, both [B, Z] (include/inpaintnet_hip.h inet_mmd).  kernel
    'gaussian' exp(-d / bandwidth) or 'imq' bandwidth / (bandwidth + d) on the squared distance d; bandwidth None: 2 Z, the expected
    squared distance of two prior draws.  -> (out4, grad): out4 = {value, S_xx, S_yy, S_xy} on the device; grad = d value / d z
    [B, Z] with want_grad, else None (the value launches only).  Two calls on the same inputs give the same bits."""
    _f32c(z); _f32c(z_prior)
    if z.dim() != 2 or z_prior.shape != z.shape:
        raise ValueError(f"mmd: z and z_prior must be [B, Z] tensors of one shape, got {tuple(z.shape)} and {tuple(z_prior.shape)}")
    if kernel not in MMD_KERNEL:
        raise ValueError(f"mmd kernel must be 'gaussian' or 'imq', got {kernel!r}")
    B, Z = z.shape
    a, c, diag = mmd_weights(B, estimator)
    var = 2.0 * Z if bandwidth is None else float(bandwidth)
    if not (var > 0.0 and math.isfinite(var)):
        raise ValueError(f"mmd bandwidth must be finite and > 0, got {var}")
    coeff = float(coeff)
    if not math.isfinite(coeff):
        raise ValueError(f"mmd coeff must be finite, got {coeff}")
    dev = z.device
    out4 = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(z) if want_grad else None
    L = _lib.lib()
    ws = _ws(L.inet_mmd_ws_bytes(B, Z), dev)
    _hold(z, z_prior, ws)
    check(L.inet_mmd(ptr(z), ptr(z_prior), B, Z, MMD_KERNEL[kernel], var, a, c, diag, coeff, ptr(out4), ptr(grad), ptr(ws),
                     ws.numel() * 4, stream_ptr()), "inet_mmd")
    return out4, grad


ATTR_MAX_DIMS = 8


def measure_attributes(tokens, spec):
    """tokens [B, T] int64 on the device, T a multiple of 6 (at most 96) -> [B, 4] float32, the columns attributes.ATTRIBUTES of every
    measure (include/inpaintnet_hip.h inet_measure_attrs).  spec: an attributes.AttributeSpec.  A token outside
    [0, spec.num_tokens) makes its row NaN."""
    from .attributes import ATTRIBUTES, AttributeSpec
    if not isinstance(spec, AttributeSpec):
        raise ValueError(f"measure_attributes: spec must be an AttributeSpec, got {type(spec).__name__}")
    if not (isinstance(tokens, torch.Tensor) and tokens.is_cuda and tokens.dtype == torch.int64 and tokens.dim() == 2
            and tokens.is_contiguous()):
        raise ValueError("measure_attributes: tokens must be a contiguous [B, T] int64 device tensor")
    B, T = tokens.shape
    if B < 1 or T < 6 or T % 6 != 0 or T > 96:
        raise ValueError(f"measure_attributes: tokens must be [B >= 1, T] with T a positive multiple of 6, at most 96; got {(B, T)}")
    out = torch.empty(B, len(ATTRIBUTES), dtype=torch.float32, device=tokens.device)
    midi = spec.midi_table(tokens.device)
    _hold(tokens, midi)
    check(_lib.lib().inet_measure_attrs(ptr(tokens), B, T, spec.num_tokens, spec.slur_index, spec.rest_index, spec.none_index, ptr(midi),
                                        spec.pitch_range[0], spec.pitch_range[1], ptr(out), stream_ptr()), "inet_measure_attrs")
    return out


def attr_dims(dims, Z):
    """dims as a list of 1 .. 8 distinct ints inside [0, Z), or a ValueError."""
    try:
        dims = list(dims)
    except TypeError:
        raise ValueError(f"attr_reg: dims must be a sequence of latent dimensions, got {dims!r}")
    if not 1 <= len(dims) <= ATTR_MAX_DIMS:
        raise ValueError(f"attr_reg: between 1 and {ATTR_MAX_DIMS} dimensions a call, got {len(dims)}")
    for d in dims:
        if isinstance(d, bool) or not isinstance(d, int) or not 0 <= d < Z:
            raise ValueError(f"attr_reg: every dimension must be an int in [0, {Z}), got {d!r}")
    if len(set(dims)) != len(dims):
        raise ValueError(f"attr_reg: the dimensions must be distinct, got {dims}")
    return dims


def attr_reg(z, dims, attrs, delta=10.0, coeff=1.0, want_grad=False):
    """The attribute regularisation of AR-VAE (include/inpaintnet_hip.h inet_attr_reg): z [B, Z], dims: A distinct
    latent dimensions (1 <= A <= 8, host ints), attrs [B, A] float32 -- any attributes.  -> (out, counts, G): out [1 + A] = {coeff sum_a
    L_a, L_0, ..}, L_a = mean_ij |tanh(delta (z_i - z_j)) - sgn(a_i - a_j)| on dimension dims[a]; counts [A, 3] int64 = {concordant,
    discordant, attribute-tied} ordered pairs i != j; G = d out[0] / d z[:, dims] [B, A] with want_grad, else None (the value launches
    only).  Two calls on the same inputs give the same bits, and the value's bits do not depend on want_grad."""
    for name, t in (("z", z), ("attrs", attrs)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
            raise ValueError(f"attr_reg: {name} must be a contiguous 2-d float32 device tensor")
    B, Z = z.shape
    if B < 1 or Z < 1:
        raise ValueError(f"attr_reg: z must be [B >= 1, Z >= 1], got {tuple(z.shape)}")
    dims = attr_dims(dims, Z)
    A = len(dims)
    if tuple(attrs.shape) != (B, A):
        raise ValueError(f"attr_reg: attrs must be [{B}, {A}] (one column per dimension), got {tuple(attrs.shape)}")
    delta, coeff = float(delta), float(coeff)
    if not (abs(delta) <= 3.4028234663852886e38):                               # NaN, inf, or past the largest float32
        raise ValueError(f"attr_reg delta must be finite, got {delta}")
    if not math.isfinite(coeff):
        raise ValueError(f"attr_reg coeff must be finite, got {coeff}")
    dev = z.device
    out = torch.empty(1 + A, dtype=torch.float32, device=dev)
    counts = torch.empty(A, 3, dtype=torch.int64, device=dev)
    grad = torch.empty(B, A, dtype=torch.float32, device=dev) if want_grad else None
    L = _lib.lib()
    ws = _ws(L.inet_attr_reg_ws_bytes(B, A), dev)
    _hold(z, attrs, ws)
    check(L.inet_attr_reg(ptr(z), B, Z, (C.c_int32 * A)(*dims), A, ptr(attrs), delta, coeff, ptr(out), ptr(counts), ptr(grad), ptr(ws),
                          ws.numel() * 4, stream_ptr()), "inet_attr_reg")
    return out, counts, grad


def _iw_f32(name, t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise ValueError(f"{name}: {what} must be a float32 device tensor")
    return t


def iw_draw(mu, ls, eps):
    """K-sample reparameterisation with each draw's density ratio (include/inpaintnet_hip.h inet_iw_draw).
    mu, ls [B, Z] contiguous; eps [B, Kc, Z] standard normal draws, rows contiguous -- a chunk eps_all[:, k0:k1] of a larger (B, K, Z)
    tensor is taken as it is, without a copy.  -> (z [B * Kc, Z], logr [B * Kc]), row b * Kc + j: z = mu[b] + eps[b, j] * exp(ls[b]),
    logr = log p(z) - log q(z | x) = sum_d (0.5 eps^2 - 0.5 z^2 + ls).  Two calls on the same inputs give the same bits."""
    for name, t in (("mu", mu), ("ls", ls), ("eps", eps)):
        _iw_f32("iw_draw", t, name)
    if mu.dim() != 2 or ls.shape != mu.shape or not (mu.is_contiguous() and ls.is_contiguous()):
        raise ValueError(f"iw_draw: mu and ls must be contiguous [B, Z] tensors of one shape, got {tuple(mu.shape)} and {tuple(ls.shape)}")
    B, Z = mu.shape
    if eps.dim() != 3 or eps.shape[0] != B or eps.shape[2] != Z or B < 1 or Z < 1 or eps.shape[1] < 1:
        raise ValueError(f"iw_draw: eps must be [B, Kc, Z] = [{B}, Kc >= 1, {Z}], got {tuple(eps.shape)}")
    Kc = eps.shape[1]
    if eps.stride(2) != 1 or eps.stride(1) != Z or (B > 1 and eps.stride(0) < Kc * Z):
        raise ValueError(f"iw_draw: the rows eps[b, j, :] must be contiguous and a measure's Kc rows adjacent, got strides {eps.stride()}")
    if ls.device != mu.device or eps.device != mu.device:
        raise ValueError("iw_draw: mu, ls and eps must lie on one device")
    if B * Kc > 1 << 24:
        raise ValueError(f"iw_draw: B * Kc = {B * Kc} rows exceed 2^24; draw in chunks")
    z = torch.empty(B * Kc, Z, dtype=torch.float32, device=mu.device)
    logr = torch.empty(B * Kc, dtype=torch.float32, device=mu.device)
    _hold(mu, ls, eps, z, logr)
    check(_lib.lib().inet_iw_draw(ptr(mu), ptr(ls), ptr(eps), max(eps.stride(0), Kc * Z), ptr(z), ptr(logr), B, Kc, Z, stream_ptr()),
          "inet_iw_draw")
    return z, logr


def nll_rows(weights, targets, logr=None, group=None, out_nll=None, out_logw=None, ld_out=None):
    """The negative log-likelihood of every measure row under its own logits (include/inpaintnet_hip.h inet_nll_rows, DESIGN.md
    section 26).  weights [R, T, V] float32 (the decoder's output; the last dimension contiguous, the rows [R * T] evenly strided),
    targets [R, T] int64 contiguous, logr [R] float32 contiguous or None (reads as 0).  nll[r] = -sum_t log softmax(weights[r, t])[
    targets[r, t]] and logw[r] = logr[r] - nll[r] are written at [r // group, r % group] of their outputs (group None: 1).  out_nll /
    out_logw: float32 [R / group, group] views with contiguous rows of one row stride -- the columns of a chunk in a (B, K) array; when
    only one is given the other is not computed (None comes back); when neither is given both are allocated with row stride ld_out
    (None: group).  ld_out with outputs given must be their row stride.  A target outside [0, V) leaves NaN in that row.
    -> (nll, logw)."""
    _iw_f32("nll_rows", weights, "weights")
    if weights.dim() != 3 or min(weights.shape) < 1:
        raise ValueError(f"nll_rows: weights must be [R, T, V], got {tuple(weights.shape)}")
    R, T, V = weights.shape
    ld_w = weights.stride(1)
    if weights.stride(2) != 1 or ld_w < V or (R > 1 and weights.stride(0) != T * ld_w):
        raise ValueError(f"nll_rows: weights must have a contiguous last dimension and evenly strided rows, got strides {weights.stride()}")
    if not (isinstance(targets, torch.Tensor) and targets.dtype == torch.int64 and tuple(targets.shape) == (R, T)
            and targets.is_contiguous() and targets.device == weights.device):
        raise ValueError(f"nll_rows: targets must be a contiguous int64 [{R}, {T}] tensor on the weights' device")
    if logr is not None:
        _iw_f32("nll_rows", logr, "logr")
        if tuple(logr.shape) != (R,) or not logr.is_contiguous() or logr.device != weights.device:
            raise ValueError(f"nll_rows: logr must be a contiguous [{R}] tensor on the weights' device")
    group = 1 if group is None else int(group)
    if group < 1 or R % group != 0:
        raise ValueError(f"nll_rows: group must be >= 1 and divide R = {R}, got {group}")
    if R > 1 << 24:
        raise ValueError(f"nll_rows: R = {R} rows exceed 2^24; score in chunks")
    rows_out = R // group
    given = [o for o in (out_nll, out_logw) if o is not None]
    if given:
        for o in given:
            _iw_f32("nll_rows", o, "an output")
            if tuple(o.shape) != (rows_out, group) or o.stride(1) != 1 or o.device != weights.device \
                    or (rows_out > 1 and o.stride(0) < group):
                raise ValueError(f"nll_rows: an output must be a [{rows_out}, {group}] view with contiguous rows on the weights' device")
        ld = given[0].stride(0) if rows_out > 1 else (group if ld_out is None else int(ld_out))
        if any(rows_out > 1 and o.stride(0) != ld for o in given) or (ld_out is not None and int(ld_out) != ld):
            raise ValueError("nll_rows: the outputs and ld_out must agree on one row stride")
    else:
        ld = group if ld_out is None else int(ld_out)
        if ld < group:
            raise ValueError(f"nll_rows: ld_out must be >= group = {group}, got {ld}")
        out_nll = torch.empty(rows_out, ld, dtype=torch.float32, device=weights.device)[:, :group]
        out_logw = torch.empty(rows_out, ld, dtype=torch.float32, device=weights.device)[:, :group]
    _hold(weights, targets, logr, out_nll, out_logw)
    check(_lib.lib().inet_nll_rows(ptr(weights), ld_w, ptr(targets), ptr(logr), ptr(out_nll), ptr(out_logw), ld, R, group, T, V,
                                   stream_ptr()), "inet_nll_rows")
    return out_nll, out_logw


IW_COLUMNS = ("iwae", "elbo", "ess", "rec", "kl")


def iw_finish(logw, nll):
    """The log-mean-exp over the samples and what comes out of the same pass (include/inpaintnet_hip.h inet_iw_finish, DESIGN.md
    section 26).  logw, nll [B, K] float32 of one shape and row stride, rows contiguous -> float64 [B, 5], the columns IW_COLUMNS =
    (iwae, elbo, ess, rec, kl): iwae = m + log(s1 / K), elbo = mean logw, ess = s1^2 / s2, rec = mean nll, kl = -mean (logw + nll),
    all in double.  A NaN in a row of logw: iwae, elbo, ess NaN; every weight -inf: (-inf, -inf, 0)."""
    _iw_f32("iw_finish", logw, "logw"); _iw_f32("iw_finish", nll, "nll")
    if logw.dim() != 2 or nll.shape != logw.shape or min(logw.shape) < 1:
        raise ValueError(f"iw_finish: logw and nll must be [B, K] tensors of one shape, got {tuple(logw.shape)} and {tuple(nll.shape)}")
    B, K = logw.shape
    if nll.device != logw.device or logw.stride(1) != 1 or nll.stride(1) != 1 or (B > 1 and (logw.stride(0) < K or nll.stride(0) != logw.stride(0))):
        raise ValueError("iw_finish: logw and nll must lie on one device with contiguous rows of one row stride")
    if B > 1 << 24:
        raise ValueError(f"iw_finish: B = {B} exceeds 2^24")
    out = torch.empty(B, 5, dtype=torch.float64, device=logw.device)
    _hold(logw, nll, out)
    check(_lib.lib().inet_iw_finish(ptr(logw), ptr(nll), logw.stride(0) if B > 1 else K, B, K, ptr(out), stream_ptr()), "inet_iw_finish")
    return out


def _adam_arenas(p, g, m, v, partials, report):
    """What every optimizer entry point asks of its tensors: four float32 arenas of one size; `partials` (where given) what
    grad_sqnorm left; `report` (where given) pinned int32 words, four of them, eight with partials.  Returns the size."""
    n = p.numel()
    for t in (p, g, m, v):
        assert _f32c(t).numel() == n
    if partials is not None:
        assert partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= sqnorm_parts()
    if report is not None:
        assert report.dtype == torch.int32 and report.numel() >= (4 if partials is None else 8) and report.is_pinned() \
            and report.is_contiguous()
    return n


def adam_step(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, step_flag=None, report=None):
    """report: 4 int32 words of PINNED host memory, zeroed by the caller; the kernel sets [0] executed, [1] skipped, [2] a
    parameter became non-finite.  step_flag: 1-element device tensor that alone decides whether the step is applied (the ranks'
    summed chain status, include/inpaintnet_hip.h inet_adam_step_ex)."""
    n = _adam_arenas(p, g, m, v, None, report)
    if report is None and step_flag is None:
        check(_lib.lib().inet_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, float(lr), float(b1), float(b2),
                                        float(eps), int(step), float(gscale), stream_ptr()), "inet_adam_step")
    else:
        check(_lib.lib().inet_adam_step_ex(ptr(p), ptr(g), ptr(m), ptr(v), n, float(lr), float(b1), float(b2),
                                           float(eps), int(step), float(gscale), ptr(step_flag), ptr(report), stream_ptr()),
              "inet_adam_step_ex")


def sqnorm_parts():
    """How many float64 partial sums grad_sqnorm writes (a constant of the library)."""
    return int(_lib.lib().inet_sqnorm_parts())


def grad_sqnorm(g, partials=None):
    """partials[b] = the float64 sum of squares of workgroup b's share of g; sum(partials) = |g|^2 in a fixed order that depends on
    g.numel() only.  Every entry is written.  `partials`: a device float64 tensor of sqnorm_parts() elements the caller allocates once
    and reuses (None: a new one).  Returns it."""
    _f32c(g)
    if partials is None:
        partials = torch.empty(sqnorm_parts(), dtype=torch.float64, device=g.device)
    assert partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= sqnorm_parts()
    check(_lib.lib().inet_grad_sqnorm(ptr(g), g.numel(), ptr(partials), stream_ptr()), "inet_grad_sqnorm")
    return partials


def adam_step_clip(p, g, m, v, lr, step, max_norm, partials, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, step_flag=None, report=None):
    """adam_step behind global-norm clipping and the non-finite skip (include/inpaintnet_hip.h inet_adam_step_clip states the rule):
    `partials` is what grad_sqnorm(g) left, max_norm in (0, inf].  report: EIGHT int32 words of PINNED host memory, zeroed by the
    caller: [0..3] as adam_step's, [4] clipped, [5] skipped for an inf / NaN gradient, [6] the bits of float32(norm), [7] 0."""
    assert partials is not None
    n = _adam_arenas(p, g, m, v, partials, report)
    check(_lib.lib().inet_adam_step_clip(ptr(p), ptr(g), ptr(m), ptr(v), n, float(lr), float(b1), float(b2), float(eps),
                                         int(step), float(gscale), float(max_norm), ptr(partials), ptr(step_flag), ptr(report),
                                         stream_ptr()), "inet_adam_step_clip")


def pack_decay_mask(n, ranges, device="cuda"):
    """The decay mask of inet_adam_step_w for an arena of n elements: ceil(n / 32) 32-bit words (an int32 tensor: the bits are what
    counts), bit i & 31 of word i >> 5 set for every element i of one of `ranges`, a list of [start, stop) element ranges.  Built on
    the host, copied to `device` once."""
    import numpy as np
    bits = np.zeros(((int(n) + 31) // 32) * 32, dtype=np.uint8)
    for start, stop in ranges:
        if not 0 <= start <= stop <= n:
            raise ValueError(f"decay range [{start}, {stop}) outside the arena of {n} elements")
        bits[start:stop] = 1
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return torch.from_numpy(words.view(np.int32).copy()).to(device)


def adamw_step(p, g, m, v, lr, step, weight_decay=0.0, decay_mask=None, ema=None, ema_decay=0.0, max_norm=None, partials=None,
               b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, step_flag=None, report=None):
    """adam_step (partials None) or adam_step_clip (partials = what grad_sqnorm(g) left, max_norm in (0, inf]) with decoupled weight
    decay and an exponential moving average of the weights in the same launch (include/inpaintnet_hip.h inet_adam_step_w states the
    rule): p is scaled by float32(1 - lr * weight_decay) in front of the update where decay_mask (pack_decay_mask; None: everywhere)
    says so, and ema (None: none) becomes ema_decay * ema + float32(1 - ema_decay) * p behind it.  A skipped or dropped step leaves
    ema alone as well.  report: int32 words of PINNED host memory, zeroed by the caller: [0..3] as adam_step's; with partials EIGHT
    words, [4..6] as adam_step_clip's and [7] 0; without partials four are enough and words beyond them are left alone."""
    n = _adam_arenas(p, g, m, v, partials, report)
    if ema is not None:
        assert _f32c(ema).numel() == n
    if decay_mask is not None:
        assert decay_mask.is_cuda and decay_mask.dtype == torch.int32 and decay_mask.is_contiguous() \
            and decay_mask.numel() >= (n + 31) // 32
    assert partials is None or max_norm is not None, "partials without max_norm"
    check(_lib.lib().inet_adam_step_w(ptr(p), ptr(g), ptr(m), ptr(v), n, float(lr), float(b1), float(b2), float(eps), int(step),
                                      float(gscale), 0.0 if max_norm is None else float(max_norm), ptr(partials),
                                      float(weight_decay), ptr(decay_mask), ptr(ema), float(ema_decay), ptr(step_flag),
                                      ptr(report), stream_ptr()), "inet_adam_step_w")


def step_flag_export(dst):
    """dst[0] = 1.0 if a chain launch of this process has timed out since the last reset else 0.0 (on the current stream)."""
    check(_lib.lib().inet_step_flag_export(ptr(_f32c(dst)), stream_ptr()), "inet_step_flag_export")


def token_status(reset=False):
    """Prologue launches that saw a token index outside [0, num_notes) since the last reset (host-mapped counter)."""
    return int(_lib.lib().inet_token_status(int(bool(reset))))


class TokenRangeError(ValueError):
    """decoder.py:36-45 check_index: a token index outside the vocabulary reached the model."""


def check_tokens(what=""):
    if token_status() > 0:
        n = token_status(reset=True)
        raise TokenRangeError(f"Invalid Value of index: {n} launch(es) met a token outside [0, num_notes) "
                              f"({what or 'inet_token_status'}); the results computed from it are not valid")


def dropout_mask(shape, p, seed, offset, device):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(_lib.lib().inet_dropout_mask(ptr(out), out.numel(), float(p), int(seed) & (2 ** 64 - 1),
                                       int(offset) & (2 ** 64 - 1), stream_ptr()), "inet_dropout_mask")
    return out


# ----------------------------------------------------------------------------- measurement hooks
PROF_CLASSES = ("gemm_f32_mfma", "gru_step_fwd", "gru_step_bwd", "hbm_pointwise")


def prof_enable(on):
    check(_lib.lib().inet_prof_enable(int(bool(on))), "inet_prof_enable")


def set_option(key, value):
    """inet_set_option (include/inpaintnet_hip.h): 0 side stream, 1 deferred joins, 2 GEMM tile force, 3 GEMM split force, 4 chain kernels,
    5 LDS-free GEMM kernels (0 never / 1 by shape / 2 whenever the shape qualifies / 3 direct kernels only, no workgroup split-K / 4
    workgroup split-K first)."""
    check(_lib.lib().inet_set_option(int(key), int(value)), "inet_set_option")


@contextlib.contextmanager
def one_k_range():
    """Inside the block every f32 product the planner would hand to a split-K kernel runs the LDS-tiled kernel in tile configuration 0
    with ONE k range per output tile (inet_set_option keys 2 and 3, the settings tests/test_gpu_bench_sizes.py forces): no zero fill
    and no f32 atomics, whose order of accumulation changes from launch to launch -- two identical calls of the encoder or the decoder
    then return the same bits.  Leaving the block hands the choice back to the planner (-1, 0): the options are
    process-wide and have no getter, so a caller that had forced them itself finds them reset."""
    set_option(2, 0)
    set_option(3, 1)
    try:
        yield
    finally:
        set_option(2, -1)
        set_option(3, 0)


def prof_dump(path):
    """Per-launch CSV (class,label,us,gflop) of the launches since prof_enable(True)."""
    check(_lib.lib().inet_prof_dump(str(path).encode()), "inet_prof_dump")


def prof_read():
    """{class: (launches, total_ms, total_flops)} for the launches since prof_enable(True)."""
    out = {}
    for i, name in enumerate(PROF_CLASSES):
        n = C.c_int64()
        ms = C.c_double()
        fl = C.c_double()
        check(_lib.lib().inet_prof_read(i, C.byref(n), C.byref(ms), C.byref(fl)), "inet_prof_read")
        out[name] = (n.value, ms.value, fl.value)
    return out


# ----------------------------------------------------------------------------- generic ops
def gemm(A, B, M, N, K, a_kmajor=False, b_kmajor=False, bias=None, epi=0, aux=None, out=None, accumulate=False):
    """C[M,N] (op)= epi(sum_k A(m,k) B(n,k) + bias).  A, B are 2-D (possibly row-strided) fp32 tensors."""
    assert A.stride(1) == 1 and B.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    check(_lib.lib().inet_gemm(ptr(A), A.stride(0), int(a_kmajor), ptr(B), B.stride(0), int(b_kmajor), ptr(out),
                               out.stride(0), M, N, K, ptr(bias), ptr(aux), aux.stride(0) if aux is not None else 0,
                               int(epi), int(accumulate), stream_ptr()), "inet_gemm")
    return out


GEMM_PLAN_KEYS = ("family", "cfg", "tile_m", "tile_n", "splits", "k_per_split", "tiles_n", "tiles", "grid_x", "grid_y", "grid_z",
                  "zero_fill", "two_pass", "launches", "products")
GEMM_FAMILIES = ("gemv", "tn_direct", "kc_direct", "ks", "tiled")


def gemm_plan(M, N, K, a_kmajor=False, b_kmajor=False, lda=None, ldb=None, bias=False, epi=0, accumulate=False, nbatch=1):
    """What gemm() (nbatch = 1) or gemm_batched() launches for a call under the options set now, without a GPU (inet_gemm_plan): a dict
    of GEMM_PLAN_KEYS plus "flops", "bytes" and "label" -- the launch's name in a prof_dump()."""
    out, work, label = (C.c_int32 * 16)(), (C.c_double * 2)(), C.create_string_buffer(96)
    lda = (M if a_kmajor else K) if lda is None else lda
    ldb = (N if b_kmajor else K) if ldb is None else ldb
    check(_lib.lib().inet_gemm_plan(int(a_kmajor), int(b_kmajor), M, N, K, lda, ldb, int(bool(bias)), int(epi), int(accumulate), int(nbatch),
                                    out, work, label, 96), "inet_gemm_plan")
    return dict(zip(GEMM_PLAN_KEYS, list(out)), flops=work[0], bytes=work[1], label=label.value.decode())


GRU_PLAN_KEYS = ("route", "rows", "launches", "gen", "MS", "SQ", "OCC", "EMR", "two_at_a_time", "ring", "groups", "members", "ring_floats",
                 "ring_capacity", "chain_capacity", "max_groups")
GRU_ROUTES = ("step", "chain1", "chain2", "step_bf3")
GRU_RINGS = ("full", "own", "rows")


def gru_chain_plan(H, B, T, nprob=2, save=True):
    """What one GRU layer of nprob directions launches for (H, B, T) under the options set now, without a GPU (inet_gru_chain_plan):
    (forward, backward), each a dict of GRU_PLAN_KEYS with "route" and "ring" as names (GRU_ROUTES, GRU_RINGS); backward is None
    without save."""
    out = (C.c_int64 * 32)()
    check(_lib.lib().inet_gru_chain_plan(H, B, T, nprob, int(bool(save)), out), "inet_gru_chain_plan")
    plans = []
    for o in (out[:16], out[16:]):
        p = dict(zip(GRU_PLAN_KEYS, o))
        if p["route"] < 0:
            plans.append(None)
            continue
        p["route"], p["ring"] = GRU_ROUTES[p["route"]], GRU_RINGS[p["ring"]]
        plans.append(p)
    return tuple(plans)


def gemm_group(products):
    """Up to four INDEPENDENT products in one launch where a grouped kernel applies (inet_gemm_group; gemm_group_plan tells), one after
    the other otherwise.  products: dicts of gemm()'s arguments -- A, B, M, N, K, out (required here), and optionally a_kmajor,
    b_kmajor, bias, epi, aux, accumulate.  The destinations must not overlap element for element.  Returns the destinations."""
    descs = (_lib.GemmDesc * max(len(products), 1))()
    for d, p in zip(descs, products):
        A, B, out, aux = p["A"], p["B"], p["out"], p.get("aux")
        assert A.stride(1) == 1 and B.stride(1) == 1 and out.stride(1) == 1 and (aux is None or aux.stride(1) == 1)
        d.A, d.lda, d.a_kmajor = A.data_ptr(), A.stride(0), int(p.get("a_kmajor", False))
        d.B, d.ldb, d.b_kmajor = B.data_ptr(), B.stride(0), int(p.get("b_kmajor", False))
        d.C, d.ldc = out.data_ptr(), out.stride(0)
        d.M, d.N, d.K = p["M"], p["N"], p["K"]
        d.bias = None if p.get("bias") is None else p["bias"].data_ptr()
        d.aux, d.ldaux = (None, 0) if aux is None else (aux.data_ptr(), aux.stride(0))
        d.epi, d.acc = int(p.get("epi", 0)), int(p.get("accumulate", False))
    check(_lib.lib().inet_gemm_group(len(products), descs, stream_ptr()), "inet_gemm_group")
    return [p["out"] for p in products]


def gemm_group_plan(products):
    """What gemm_group() launches for these products under the options set now, without a GPU (inet_gemm_group_plan).  products: dicts
    of gemm_plan()'s arguments (M, N, K, and optionally a_kmajor, b_kmajor, lda, ldb, bias, epi, accumulate) or the dicts given to
    gemm_group() (the leading dimensions are then those of A and B).  One dict like gemm_plan()'s per product: when one launch takes
    the group, row 0 describes it ("products" == 1) and the other rows are empty; else row i is the plan of product i on its own and
    "products" == len(products)."""
    n = len(products)
    desc = (C.c_int64 * (10 * max(n, 1)))()
    for i, p in enumerate(products):
        akm, bkm = bool(p.get("a_kmajor", False)), bool(p.get("b_kmajor", False))
        lda = p["A"].stride(0) if "A" in p else p.get("lda")
        ldb = p["B"].stride(0) if "B" in p else p.get("ldb")
        lda = (p["M"] if akm else p["K"]) if lda is None else lda
        ldb = (p["N"] if bkm else p["K"]) if ldb is None else ldb
        bias = p.get("bias")
        desc[10 * i:10 * i + 10] = [int(akm), int(bkm), p["M"], p["N"], p["K"], lda, ldb, int(bias is not None and bias is not False),
                                    int(p.get("epi", 0)), int(p.get("accumulate", False))]
    out, work, label = (C.c_int32 * (16 * max(n, 1)))(), (C.c_double * (2 * max(n, 1)))(), C.create_string_buffer(96 * max(n, 1))
    check(_lib.lib().inet_gemm_group_plan(n, desc, out, work, label, 96), "inet_gemm_group_plan")
    return [dict(zip(GEMM_PLAN_KEYS, out[16 * i:16 * i + 16]), flops=work[2 * i], bytes=work[2 * i + 1],
                 label=label.raw[96 * i:96 * (i + 1)].split(b"\0")[0].decode()) for i in range(n)]


def epoch_stats_add(sums, loss, accuracy=None, step_flag=None):
    """sums[:3] += (loss, accuracy, 1) on the device unless the step was skipped (step_flag: the ranks' summed chain status as
    given to adam_step; None: this process's own status word) -- inet_epoch_stats_add_ex."""
    check(_lib.lib().inet_epoch_stats_add_ex(ptr(sums), ptr(loss), ptr(accuracy), ptr(step_flag), stream_ptr()),
          "inet_epoch_stats_add_ex")


def gemm_bf3(A, B, M, N, K, a_kmajor=False, b_kmajor=False, bias=None, out=None, accumulate=False, ksplit=0):
    """The same product through exact three-piece bf16 splits on the bf16 matrix cores (csrc/gemm_bf3.hip); test / bench
    entry: the pieces are made in a scratch allocated for the call."""
    assert A.stride(1) == 1 and B.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    check(_lib.lib().inet_gemm_bf3(ptr(A), A.stride(0), int(a_kmajor), ptr(B), B.stride(0), int(b_kmajor), ptr(out),
                                   out.stride(0), M, N, K, ptr(bias), int(accumulate), int(ksplit), stream_ptr()),
          "inet_gemm_bf3")
    return out


def gemm_batched(A, B, out, M, N, K, nbatch, batchA, batchB, batchC, a_kmajor=True, b_kmajor=True):
    """out_i[M,N] += A_i . B_i^T for nbatch problems of one shape (element strides between problems), one launch where
    a batched kernel applies.  A, B, out: the 2-D views of problem 0."""
    assert A.stride(1) == 1 and B.stride(1) == 1 and out.stride(1) == 1
    check(_lib.lib().inet_gemm_batched(ptr(A), A.stride(0), int(a_kmajor), ptr(B), B.stride(0), int(b_kmajor), ptr(out),
                                       out.stride(0), M, N, K, int(nbatch), int(batchA), int(batchB), int(batchC),
                                       stream_ptr()), "inet_gemm_batched")
    return out


def linear_fwd(x, W, b, epi=0):
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    check(_lib.lib().inet_linear_fwd(ptr(_f32c(x)), ptr(_f32c(W)), ptr(b), ptr(y), M, N, K, int(epi), stream_ptr()),
          "inet_linear_fwd")
    return y


def linear_bwd(dy, x, W, dW=None, db=None, need_dx=True):
    M, N = dy.shape
    K = W.shape[1]
    dx = torch.empty(M, K, dtype=torch.float32, device=dy.device) if need_dx else None
    _hold(dy, x, W, dW, db)                                  # dW / db run on the side stream
    check(_lib.lib().inet_linear_bwd(ptr(_f32c(dy)), ptr(x), ptr(W), ptr(dx), ptr(dW), ptr(db), M, N, K,
                                     stream_ptr()), "inet_linear_bwd")
    return dx


def lstm_ws(B, T, H, save, device):
    n = _lib.lib().inet_lstm_ws_bytes(B, T, H, int(save))
    if n < 0:
        raise ValueError("lstm_ws: invalid arguments")
    return _ws(n, device)


def lstm_fwd(gi_tm, W_hh, b_hh, H, reverse=False, h0=None, c0=None, save=False, want_state=False):
    """gi_tm [T,B,4H] -> out [T,B,H] (+ hT, cT), ws"""
    T, B, _ = gi_tm.shape
    dev = gi_tm.device
    ws = lstm_ws(B, T, H, save, dev)
    out = torch.empty(T, B, H, dtype=torch.float32, device=dev)
    hT = torch.empty(B, H, dtype=torch.float32, device=dev) if want_state else None
    cT = torch.empty(B, H, dtype=torch.float32, device=dev) if want_state else None
    check(_lib.lib().inet_lstm_fwd(B, T, H, ptr(_f32c(gi_tm)), ptr(W_hh), ptr(b_hh), ptr(h0), ptr(c0), int(reverse),
                                   ptr(out), ptr(hT), ptr(cT), ptr(ws), ws.numel() * 4, int(save), stream_ptr()),
          "inet_lstm_fwd")
    return out, hT, cT, ws


def lstm_bwd(W_hh, out, dout, H, reverse, ws, dW_hh=None, db_ih=None, db_hh=None, h0=None, dhT=None, dcT=None,
             want_dstate=False):
    T, B, _ = out.shape
    dev = out.device
    dgi = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
    dh0 = torch.empty(B, H, dtype=torch.float32, device=dev) if want_dstate else None
    dc0 = torch.empty(B, H, dtype=torch.float32, device=dev) if want_dstate else None
    _hold(W_hh, h0, out, dout, dhT, dcT, dgi, dW_hh, db_ih, db_hh, ws)
    check(_lib.lib().inet_lstm_bwd(B, T, H, ptr(W_hh), ptr(h0), ptr(out), ptr(dout), ptr(dhT), ptr(dcT), int(reverse),
                                   ptr(dgi), ptr(dW_hh), ptr(db_ih), ptr(db_hh), ptr(dh0), ptr(dc0), ptr(ws),
                                   ws.numel() * 4, stream_ptr()), "inet_lstm_bwd")
    return dgi, dh0, dc0


LSTM_PLAN_KEYS = ("ok", "MS", "groups", "members", "workgroups", "blocks", "tagged", "chunk_steps", "chunks", "areas", "chain_capacity",
                  "side_by_side", "max_groups", "counter_stride", "counter_words")


def lstm_chain_plan(B, T, H, pipeline=False):
    """What one LSTM layer launches for (B, T, H) under the options set now, without a GPU (inet_lstm_chain_plan): a dict of
    LSTM_PLAN_KEYS.  pipeline: the plan of lstm2_fwd / lstm2_bwd (two chain launches side by side) instead of lstm_fwd / lstm_bwd."""
    out = (C.c_int64 * 16)()
    check(_lib.lib().inet_lstm_chain_plan(int(B), int(T), int(H), int(bool(pipeline)), out), "inet_lstm_chain_plan")
    return dict(zip(LSTM_PLAN_KEYS, out[:15]))


def lstm2_ok(B, T, H):
    return bool(_lib.lib().inet_lstm2_ok(int(B), int(T), int(H)))


def lstm2_fwd(gi0_tm, W_hh0, b_hh0, W_ih1, b_ih1, W_hh1, b_hh1, H, reverse=False, save=False):
    """Two stacked layers, zero initial states, pipelined over chunks of time steps (csrc/lstm.hip lstm2_seq_fwd).
    gi0_tm [T,B,4H] -> (out0, out1 [T,B,H], ws0, ws1), or None when the shape does not qualify."""
    T, B, _ = gi0_tm.shape
    dev = gi0_tm.device
    ws0, ws1 = lstm_ws(B, T, H, save, dev), lstm_ws(B, T, H, save, dev)
    out0 = torch.empty(T, B, H, dtype=torch.float32, device=dev)
    out1 = torch.empty(T, B, H, dtype=torch.float32, device=dev)
    gi1 = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
    _hold(gi0_tm, gi1, out0, out1, ws0, ws1)                 # the second stream's work is not ordered by the allocator
    rc = _lib.lib().inet_lstm2_fwd(B, T, H, ptr(_f32c(gi0_tm)), ptr(W_hh0), ptr(b_hh0), ptr(W_ih1), ptr(b_ih1), ptr(W_hh1),
                                   ptr(b_hh1), int(reverse), ptr(out0), ptr(gi1), ptr(out1), ptr(ws0), ptr(ws1),
                                   ws0.numel() * 4, int(save), stream_ptr())
    if rc == 1:
        return None
    check(rc, "inet_lstm2_fwd")
    return out0, out1, ws0, ws1


def lstm2_bwd(W_hh0, W_ih1, W_hh1, out0, out1, dout1, H, reverse, ws0, ws1, grads=None):
    """-> dgi0 [T,B,4H] (dgi1 is consumed inside).  grads: (dW_hh0, db_ih0, db_hh0, dW_ih1, dW_hh1, db_ih1, db_hh1) or None."""
    T, B, _ = out1.shape
    dev = out1.device
    dgi0 = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
    dgi1 = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
    dout0 = torch.empty(T, B, H, dtype=torch.float32, device=dev)
    g = tuple(grads) if grads is not None else (None,) * 7
    _hold(W_hh0, W_ih1, W_hh1, out0, out1, dout1, dgi0, dgi1, dout0, ws0, ws1, *g)
    check(_lib.lib().inet_lstm2_bwd(B, T, H, ptr(W_hh0), ptr(W_ih1), ptr(W_hh1), ptr(out0), ptr(out1), ptr(_f32c(dout1)),
                                    int(reverse), ptr(dgi0), ptr(dgi1), ptr(dout0), *[ptr(x) for x in g], ptr(ws0), ptr(ws1),
                                    ws0.numel() * 4, stream_ptr()), "inet_lstm2_bwd")
    return dgi0


def embedding_fwd(table, idx, row_scale=None):
    rows = idx.numel()
    E = table.shape[1]
    out = torch.empty(rows, E, dtype=torch.float32, device=table.device)
    check(_lib.lib().inet_embedding_fwd(ptr(table), ptr(_i64c(idx)), rows, E, ptr(out), ptr(row_scale), stream_ptr()),
          "inet_embedding_fwd")
    return out


def embedding_bwd(dout, idx, dtable, row_scale=None):
    rows = idx.numel()
    _hold(dout, idx, dtable, row_scale)                      # runs on the side stream
    check(_lib.lib().inet_embedding_bwd(ptr(_f32c(dout)), ptr(_i64c(idx)), rows, dtable.shape[1], ptr(dtable),
                                        ptr(row_scale), int(dtable.shape[0]), stream_ptr()), "inet_embedding_bwd")


def relu_bwd(dy, y):
    out = torch.empty_like(dy)
    check(_lib.lib().inet_relu_bwd(ptr(_f32c(dy)), ptr(_f32c(y)), ptr(out), dy.numel(), stream_ptr()), "inet_relu_bwd")
    return out


def argmax_rows(w2d, out=None):
    rows, V = w2d.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=w2d.device)
    check(_lib.lib().inet_argmax(ptr(w2d), w2d.stride(0), rows, V, ptr(out), 1, stream_ptr()), "inet_argmax")
    return out


def gru_step(gi, h_prev, W_hh, b_hh, save=False):
    B, H = h_prev.shape
    h_new = torch.empty_like(h_prev)
    sv = torch.empty(5, B, H, dtype=torch.float32, device=gi.device) if save else None
    check(_lib.lib().inet_gru_step(B, H, ptr(_f32c(gi)), ptr(_f32c(h_prev)), ptr(_f32c(W_hh)), ptr(_f32c(b_hh)),
                                   ptr(h_new), ptr(sv), stream_ptr()), "inet_gru_step")
    return h_new, sv


def bigru2_ws(B, T, K, H, save, device):
    n = _lib.lib().inet_bigru2_ws_bytes(B, T, K, H, int(save))
    if n < 0:
        raise ValueError("bigru2_ws: invalid arguments")
    return _ws(n, device)


def bigru2_fwd(x, x_scalar, weights, H, B, T, K, h0=None, mask=None, want_out=True, want_hn=True, save=False,
               ws=None):
    """x [B,T,K] or None (then x_scalar: 1-element tensor, K == 1).  weights: view of the arena starting at
    the GRU's weight_ih_l0.  Returns out [B,T,2H] | None, h_n [4,B,H] | None, ws."""
    dev = weights.device
    if ws is None:
        ws = bigru2_ws(B, T, K, H, save, dev)
    out = torch.empty(B, T, 2 * H, dtype=torch.float32, device=dev) if want_out else None
    hn = torch.empty(4, B, H, dtype=torch.float32, device=dev) if want_hn else None
    check(_lib.lib().inet_bigru2_fwd(B, T, K, H, ptr(x), ptr(x_scalar), ptr(weights), ptr(h0), ptr(mask), ptr(out),
                                     ptr(hn), ptr(ws), ws.numel() * 4, int(save), stream_ptr()), "inet_bigru2_fwd")
    return out, hn, ws


def bigru2_bwd(x, x_scalar, weights, grads, H, B, T, K, mask, dout, dhn, ws, want_dx=False, dx_scalar=None,
               want_dh0=False):
    dev = weights.device
    dx = torch.empty(B, T, K, dtype=torch.float32, device=dev) if (want_dx and x is not None) else None
    dh0 = torch.empty(4, B, H, dtype=torch.float32, device=dev) if want_dh0 else None
    _hold(x, x_scalar, weights, grads, mask, dout, dhn, ws)
    check(_lib.lib().inet_bigru2_bwd(B, T, K, H, ptr(x), ptr(x_scalar), ptr(weights), ptr(grads), ptr(mask),
                                     ptr(dout), ptr(dhn), ptr(dx), ptr(dx_scalar), ptr(dh0), ptr(ws), ws.numel() * 4,
                                     stream_ptr()), "inet_bigru2_bwd")
    return dx, dh0


# ----------------------------------------------------------------------------- input feed
def tokens_to_long(t):
    """int32 device tensor -> int64 of the same shape (utils/helpers.py:17-26 on the device)."""
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    out = torch.empty(t.shape, dtype=torch.int64, device=t.device)
    check(_lib.lib().inet_tokens_to_i64(ptr(t), ptr(out), t.numel(), stream_ptr()), "inet_tokens_to_i64")
    return out


def split_score(score, n_past, n_target, measure_len):
    """score (B,1,L) or (B,L) int32 on the device -> past, future, target int64 (B,n,measure_len), one kernel."""
    assert score.is_cuda and score.dtype == torch.int32 and score.is_contiguous()
    B = score.shape[0]
    L = score.numel() // B
    M = L // measure_len
    n_future = M - n_past - n_target
    mk = lambda n: torch.empty(B, n, measure_len, dtype=torch.int64, device=score.device)
    past, target, future = mk(n_past), mk(n_target), mk(n_future)
    check(_lib.lib().inet_split_score(ptr(score), B, M, measure_len, n_past, n_target, ptr(past), ptr(target),
                                      ptr(future), stream_ptr()), "inet_split_score")
    return past, future, target


def ws_field(cfg, ws, B, which, name):
    """Test hook: view of a named intermediate (flat) inside an encoder (which=0) / decoder (which=1) workspace."""
    off, n = C.c_int64(), C.c_int64()
    check(_lib.lib().inet_vae_ws_field(C.byref(cfg), B, int(which), name.encode(), C.byref(off), C.byref(n)),
          "inet_vae_ws_field")
    return ws[off.value:off.value + n.value]


def chain_status(reset=False):
    """Workgroups of chain kernels that timed out waiting for their group since the last reset (0 = healthy).
    Complete after a synchronisation; a non-zero value read earlier is already a failure (host-mapped counter)."""
    return int(_lib.lib().inet_chain_status(int(bool(reset))))


class ChainTimeoutError(RuntimeError):
    """A persistent (chain) kernel gave up waiting for its group: results computed since are not valid."""


_KERNEL_NAMES = {1: "gru_chain_fwd", 2: "gru_chain_bwd", 3: "gru_chain2_fwd", 4: "gru_chain2_bwd", 5: "lstm_chain_fwd", 6: "lstm_chain_bwd",
                 7: "lstm_pipeline", 8: "decode_chain", 9: "arnn_token_pass", 10: "decode_b1"}
_SITE_NAMES = {0: "group counter", 1: "granule", 2: "row-block counter", 3: "tagged fragments"}


def slow_waits(reset=False, max_entries=127):
    """The library's slow-wait recorder (include/inpaintnet_hip.h inet_slow_waits).  Returns {"count": waits of at least the entry
    threshold (default 16384 polls, set_option(16, polls)) or that gave up, since the last reset; "noted": waits of at least 64 polls
    (normal wherever launches overlap); "entries": the first 127 slow ones, decoded}.  Synchronises the device.  A slow wait is what
    an unexplained timeout or a stalled launch leaves behind: which kernel, which workgroup on which XCD, what it waited for and
    for how many polls (a counter poll is ~0.4 us, a granule poll ~1 us)."""
    import numpy as np
    buf = np.zeros((max(int(max_entries), 1), 8), dtype=np.uint32)
    noted = C.c_int64(0)
    n = int(_lib.lib().inet_slow_waits(C.c_void_p(buf.ctypes.data), int(max_entries), int(bool(reset)), C.byref(noted)))
    if n < 0:
        return {"count": n, "noted": 0, "entries": []}
    out = []
    for e in buf[:min(n, int(max_entries), 127)]:
        w0 = int(e[0])
        out.append({"kernel": _KERNEL_NAMES.get(w0 & 0xff, str(w0 & 0xff)), "xcc": (w0 >> 8) & 0xf, "gave_up": bool(w0 & 0x8000),
                    "site": _SITE_NAMES.get(w0 >> 16, str(w0 >> 16)), "workgroup": int(e[1]), "expected": int(e[2]), "polls": int(e[3]),
                    "clock_10ns": int(e[4]) | (int(e[5]) << 32)})
    return {"count": n, "noted": int(noted.value), "entries": out}


def slow_waits_summary(reset=False, top=6):
    """One line for error messages and logs: the count and the longest few waits of the recorder."""
    r = slow_waits(reset=reset)
    if r["count"] <= 0:
        return f"no slow waits recorded ({r['count']}; {r['noted']} waits of 64+ polls noted)"
    es = sorted(r["entries"], key=lambda e: -e["polls"])[:top]
    return f"{r['count']} slow waits ({r['noted']} of 64+ polls noted); longest: " + "; ".join(
        f"{e['kernel']} wg {e['workgroup']} xcc {e['xcc']} {e['site']} expected {e['expected']} after {e['polls']} polls"
        + (" GAVE UP" if e["gave_up"] else "") for e in es)


def preload():
    """First-touch of every kernel of the library on the current device (csrc/preload.hip): code objects and function objects the HIP
    runtime would otherwise build on the launch path of each kernel's first launch.  Idempotent per device; the trainers and the
    models call it at construction so that no step pays a first launch.  Returns the number of kernels touched (0: done before)."""
    n = int(_lib.lib().inet_preload())
    if n < 0:
        raise _lib.InetError("inet_preload: no HIP device, or a kernel of the library could not be loaded on it")
    return n


def check_chains(what=""):
    """Raise if any chain-kernel workgroup has timed out (reads the host-mapped counter: no synchronisation, ~1 us).
    The inference wrappers call it after their device->host reads (Trainer.step() reads step reports instead: check_steps).
    Also raises TokenRangeError (a ValueError) if a prologue met a token outside the vocabulary (decoder.py:36-45)."""
    n = chain_status()
    if n > 0:
        raise ChainTimeoutError(f"{n} chain-kernel workgroups gave up waiting for their group ({what or 'inet_chain_status'}): "
                                "the results are not valid.  All workgroups of such a launch must be resident at once -- "
                                "is the GPU shared, partitioned or CU-masked?  INET_CHAIN=0 (or ops.set_option(4, 0)) "
                                f"selects the per-step kernels.  Recorder: {slow_waits_summary()}")
    check_tokens(what)
