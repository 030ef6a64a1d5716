"""The narrower C entries of the three sampling families, which `ops` no longer calls: each of inet_vae_decoder_sample / _ex / _cx,
inet_arnn_sample / _ex / _cx and inet_sample_truncated / _constrained, called directly, returns the tokens and log-probabilities of its
family's widest entry (_fx / inet_sample_forced) called with nulls for what the narrower one does not take, bit for bit.  The cases are
the smallest of tests/draw_launches.py: the decoder at B = 1, AnticipationRNN at R = 2 / V = 48, the row kernels at 5 x 65."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import draw_launches as DL

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops, synthetic
    from inpaintnet_amd._lib import ptr, stream_ptr

K, P = DL.TOP_K, DL.TOP_P


def same(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(a, b))


def decoder_call(entry, tail):
    """entry(cfg, B, z, params, ..., temperature, uniforms, *tail(logp), stream) at B = 1, V = 20 -> (tokens, logp)"""
    from tests.test_gpu_decode_plans import decoder
    B, V = DL.DECODER[0]
    cfg, _, params = decoder(V, 256)
    z = torch.from_numpy(synthetic.det_normal(f"draw_launches/z/{V}/{B}", (B, 256))).cuda()
    u = torch.from_numpy(synthetic.det_uniform(f"draw_launches/u/{V}/{B}", (B, 24), 0.0, 1.0).astype(np.float64)).cuda()
    ws = ops.decoder_ws(cfg, B, False, z.device)
    w = torch.empty(B, 24, V, dtype=torch.float32, device="cuda")
    s = torch.zeros(B, 1, 24, dtype=torch.int64, device="cuda")
    lp = torch.full((B, 24), 7.0, dtype=torch.float32, device="cuda")
    rc = getattr(_lib.lib(), entry)(C.byref(cfg), B, ptr(z), ptr(params), None, None, ptr(w), ptr(s), ptr(ws), ws.numel() * 4, 0,
                                    DL.DEC_TEMP, ptr(u), *tail(lp), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and ops.chain_status() == 0, (entry, rc)
    return s, lp


def test_decoder_entries():
    B, V = DL.DECODER[0]
    allow = ops.pack_allowed(torch.from_numpy(DL.allow_mask(B, 24, V))).cuda().contiguous()
    fx = "inet_vae_decoder_sample_fx"
    assert same(decoder_call("inet_vae_decoder_sample", lambda lp: ()), decoder_call(fx, lambda lp: (0, 1.0, None, None, None)))
    assert same(decoder_call("inet_vae_decoder_sample_ex", lambda lp: (K, P, ptr(lp))),
                decoder_call(fx, lambda lp: (K, P, ptr(lp), None, None)))
    assert same(decoder_call("inet_vae_decoder_sample_cx", lambda lp: (K, P, ptr(lp), ptr(allow))),
                decoder_call(fx, lambda lp: (K, P, ptr(lp), ptr(allow), None)))


def arnn_call(entry, tail):
    """entry(R, L, ..., temperature, uniforms, hc_init, tokens, ws, ws_floats, *tail(logp), stream) at R = 2, V = 48 -> (tokens, logp)"""
    from tests import arnn_trunc_ref as AR
    R, V = DL.ARNN[0]
    E, Hc, H, U = (AR.FULL[k] for k in ("E", "Hc", "H", "U"))
    W = [torch.from_numpy(w).cuda() for w in AR.net(V, **AR.FULL)]
    oc, hc, u = AR.case(V, R, 0, **AR.FULL)
    oc, hc, u = torch.from_numpy(oc).cuda(), torch.from_numpy(hc).cuda(), torch.from_numpy(u).cuda()
    L = oc.shape[1]
    nws = int(_lib.lib().inet_arnn_sample_ws_floats(R, L, E, Hc, H, U, V))
    ws = torch.empty(nws, dtype=torch.float32, device="cuda")
    tok = torch.zeros(R, L, dtype=torch.int64, device="cuda")
    lp = torch.full((R, L), 7.0, dtype=torch.float32, device="cuda")
    rc = getattr(_lib.lib(), entry)(R, L, E, Hc, H, U, V, ptr(W[0]), ptr(oc), oc.stride(1), oc.stride(0), *[ptr(w) for w in W[1:]],
                                    DL.ARNN_TEMP, ptr(u), ptr(hc), ptr(tok), ptr(ws), nws, *tail(lp), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and ops.chain_status() == 0, (entry, rc)
    return tok, lp


def test_arnn_entries():
    from tests import arnn_trunc_ref as AR
    R, V = DL.ARNN[0]
    allow = ops.pack_allowed(torch.from_numpy(DL.allow_mask(R, AR.L, V))).cuda().contiguous()
    fx = "inet_arnn_sample_fx"
    assert same(arnn_call("inet_arnn_sample", lambda lp: ()), arnn_call(fx, lambda lp: (0, 1.0, None, None, None, None)))
    assert same(arnn_call("inet_arnn_sample_ex", lambda lp: (K, P, ptr(lp), None)),
                arnn_call(fx, lambda lp: (K, P, ptr(lp), None, None, None)))
    assert same(arnn_call("inet_arnn_sample_cx", lambda lp: (K, P, ptr(lp), None, ptr(allow))),
                arnn_call(fx, lambda lp: (K, P, ptr(lp), None, ptr(allow), None)))


def rows_call(entry, tail):
    """entry(w, ld, rows, V, temperature, u, 1, top_k, top_p, out, 1, logp, 1, *tail, stream) at 5 x 65 -> (tokens, logp)"""
    w = torch.from_numpy(synthetic.det_normal("draw_launches/rows/w", (DL.ROWS, DL.ROWS_V))).cuda()
    u = torch.from_numpy(synthetic.det_uniform("draw_launches/rows/u", (DL.ROWS,), 0.0, 1.0).astype(np.float64)).cuda()
    out = torch.zeros(DL.ROWS, dtype=torch.int64, device="cuda")
    lp = torch.full((DL.ROWS,), 7.0, dtype=torch.float32, device="cuda")
    rc = getattr(_lib.lib(), entry)(ptr(w), w.stride(0), DL.ROWS, DL.ROWS_V, DL.ROWS_TEMP, ptr(u), 1, K, P, ptr(out), 1, ptr(lp), 1, *tail,
                                    stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (entry, rc)
    return out, lp


def test_row_entries():
    allow = ops.pack_allowed(torch.from_numpy(DL.allow_mask(DL.ROWS, 1, DL.ROWS_V)[:, 0])).cuda().contiguous()
    assert same(rows_call("inet_sample_truncated", ()), rows_call("inet_sample_forced", (None, 0, None, 0)))
    assert same(rows_call("inet_sample_constrained", (ptr(allow), allow.stride(0))),
                rows_call("inet_sample_forced", (ptr(allow), allow.stride(0), None, 0)))
