"""Every plan of the register-resident decode (csrc/decode_b1.hip) that a free-running inference call can get, on the GPU: the beat path
folded into the launch (latent size 256), behind its own launches (another latent size, or a beat dropout mask), and on partitions of
the chip (INET_CHAIN_CUS) -- against decode_chain.hip's exchange kernel (inet_set_option key 15 = 0) and the float64 oracle.  A plan
whose roles do not match the kernel it launches does not return a slightly wrong number: it stores granules past its area or waits
for a workgroup nobody placed, and such a wait ends in the bounded-spin timeout that chain_status() reports."""
import csv
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import layout, ops, synthetic
    from oracle import torch_ref as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("folded", "z128", "beat_mask")        # Z = 256 (beat path in the launch up to six measures), Z = 128, Z = 256 + beat mask


def decoder(V, Z):
    from tests.test_gpu_kernels import pack
    c = G.CFGS["full"]
    cfg = ops.vae_config(V, c["E"], c["H"], Z, c["H"])
    table, total = ops.vae_param_table(cfg)
    P = {k: torch.from_numpy(synthetic.det_param(k, s)) for k, s in layout.vae_param_shapes(V, c["E"], c["H"], Z, c["H"]).items()}
    return cfg, P, pack(table, total, P)


def labels_of(fn):
    """Runs fn() with the launch profile on: (its result, the labels of its launches)."""
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        with tempfile.TemporaryDirectory() as td:
            ops.prof_dump(os.path.join(td, "l.csv"))
            labels = [r["label"] for r in csv.DictReader(open(os.path.join(td, "l.csv")))]
    finally:
        ops.prof_enable(False)
    return out, labels


def decode(cfg, z, params, mask_beat, mode):
    """One free-running inference call under decode mode `mode`; a bounded-spin timeout fails here, with the slow-wait record."""
    ops.set_option(15, mode)
    (w, s_, _), labels = labels_of(lambda: ops.decoder_fwd(cfg, z, None, False, params, mask_beat=mask_beat))
    status = ops.chain_status()
    assert status == 0, (mode, tuple(z.shape), status, ops.slow_waits_summary())
    return w.clone(), s_.clone(), labels


def inputs(variant, V, B, tag):
    Z = 128 if variant == "z128" else 256
    z = torch.from_numpy(synthetic.det_normal(f"plans/{tag}/{variant}/{V}/{B}", (B, Z))).cuda()
    mb = ops.dropout_mask((4, B, 512), 0.5, 1000 * V + B, 0, "cuda") if variant == "beat_mask" else None
    return z, mb


def oracle(P, z, mb, feed):
    """float64 reference with the kernel's fed-back tokens (a near-tie cannot de-synchronise the trajectories)."""
    P64 = {k: v.double() for k, v in P.items()}
    masks = {"beat": mb.permute(1, 0, 2).double().cpu()} if mb is not None else None
    with torch.no_grad():
        return O.decoder_forward(P64, z.double().cpu(), None, False, masks=masks, feed_tokens=feed.cpu()[:, 0])


def check_against_oracle(w, s_, wr, sr, V, what):
    top2 = torch.topk(wr, 2, dim=-1).values
    ok = ((top2[..., 0] - top2[..., 1]) > 1e-4).numpy()
    assert int(s_.min()) >= 0 and int(s_.max()) < V, what
    assert G.rel_err(w.cpu(), wr) < 2e-5, (what, G.rel_err(w.cpu(), wr))
    assert np.array_equal(s_.cpu().numpy()[:, 0][ok], sr.numpy()[:, 0][ok]), what


def run_sizes(variant, V, sizes):
    Z = 128 if variant == "z128" else 256
    cfg, P, params = decoder(V, Z)
    same_rows = total_rows = 0
    try:
        for B in sizes:
            z, mb = inputs(variant, V, B, "gpu")
            w4, s4, labels = decode(cfg, z, params, mb, 4)
            # the register-resident launch ran (never a quiet fall-back): with the beat path folded in where it fits
            folded = variant == "folded" and B <= 6
            want = f"decode_b1_beats T24 B{B} " if folded else f"decode_b1 T24 B{B} "
            assert any(l.startswith(want) for l in labels), (variant, V, B, sorted(set(labels)))
            wr, sr = oracle(P, z, mb, s4)
            check_against_oracle(w4, s4, wr, sr, V, (variant, V, B))
            w0, s0, _ = decode(cfg, z, params, mb, 0)
            scale = float(w0.abs().max())
            assert float((w4[:, 0] - w0[:, 0]).abs().max()) < 2e-5 * scale, (variant, V, B)     # tick 0 depends on no token
            same = (s4 == s0).all(dim=-1).reshape(-1)
            same_rows += int(same.sum()); total_rows += B
            if bool(same.any()):
                assert float((w4[same] - w0[same]).abs().max()) < 2e-5 * scale, (variant, V, B)
    finally:
        ops.set_option(15, 4)
    assert same_rows >= 0.9 * total_rows, (variant, V, same_rows, total_rows)


@pytest.mark.parametrize("V", [20, 48, 100])
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_call_size_against_the_exchange_kernel_and_the_oracle(variant, V):
    """B = 1 .. 16 under mode 4 (the default): logits to fp32 round-off of the float64 oracle, tokens exact on ticks with a margin and
    inside [0, V); against the exchange kernel tick 0 on every row and whole rows wherever both sampled the same tokens."""
    run_sizes(variant, V, range(1, 17))


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_widest_head_at_a_few_call_sizes(variant):
    run_sizes(variant, 128, (1, 4, 6, 9, 16))


def test_four_measures_through_the_public_decoder_with_another_latent_size():
    """The LatentRNN inpainting call's size (four measures) through MeasureVAE.decoder with latent_space_dim = 128, as
    tools/decode_latency.py calls it: the beat path runs as launches of its own, the ticks on decode_b1.hip's plan for it."""
    from inpaintnet_amd.measure_vae import MeasureVAE
    V, B = 48, 4
    ds = synthetic.SyntheticFolkDataset(num_notes=V)
    vae = MeasureVAE(ds, latent_space_dim=128, encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    P = {k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape))) for k, v in vae.state_dict().items()}
    vae.load_state_dict(P)
    vae.eval()
    z = torch.from_numpy(synthetic.det_normal("plans/public/z128", (B, 128))).cuda()
    score = torch.zeros(B, 24, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        (w, s_), labels = labels_of(lambda: vae.decoder(z, score, train=False))
    assert ops.chain_status() == 0, ops.slow_waits_summary()
    assert any(l.startswith(f"decode_b1 T24 B{B} ") for l in labels), sorted(set(labels))
    assert w.shape == (B, 24, V) and s_.shape == (B, 1, 24)
    wr, sr = oracle(P, z, None, s_)
    check_against_oracle(w, s_, wr, sr, V, "public")


def capacity_run():
    """(In a child process with INET_CHAIN_CUS set.)  B in {1, 3, 4, 6, 9, 12, 16} x V in {48, 100} x latent size {256, 128} under
    mode 4 against the exchange kernel of the same process.  Every call the planner takes must run decode_b1.hip; the first failure
    ends the run (nothing more is launched behind a timeout)."""
    import ctypes as C
    from inpaintnet_amd import _lib
    L = _lib.lib()
    done = []
    try:
        for V in (48, 100):
            for Z in (256, 128):
                cfg, P, params = decoder(V, Z)
                for B in (1, 3, 4, 6, 9, 12, 16):
                    out = (C.c_int * 8)()
                    ops.set_option(15, 4)
                    taken = L.inet_decode_b1_plan(B, V, Z, out) == 0
                    z = torch.from_numpy(synthetic.det_normal(f"plans/cus/{V}/{Z}/{B}", (B, Z))).cuda()
                    w4, s4, labels = decode(cfg, z, params, None, 4)
                    ran = any(l.startswith("decode_b1") for l in labels)
                    assert ran == taken, (V, Z, B, list(out), sorted(set(labels)))
                    w0, s0, _ = decode(cfg, z, params, None, 0)
                    scale = float(w0.abs().max())
                    assert int(s4.min()) >= 0 and int(s4.max()) < V, (V, Z, B)
                    assert float((w4[:, 0] - w0[:, 0]).abs().max()) < 2e-5 * scale, (V, Z, B)
                    same = (s4 == s0).all(dim=-1).reshape(-1)
                    if bool(same.any()):
                        assert float((w4[same] - w0[same]).abs().max()) < 2e-5 * scale, (V, Z, B)
                    done.append([V, Z, B, int(taken), int(same.sum())])
    finally:
        ops.set_option(15, 4)
    return done


CHILD = ("import json, sys\n"
         "sys.path.insert(0, sys.argv[1])\n"
         "import torch\n"
         "from tests.test_gpu_decode_plans import capacity_run\n"
         "print('RESULT ' + json.dumps(capacity_run()))\n")


def test_partitions_of_the_chip_against_the_exchange_kernel():
    """INET_CHAIN_CUS is read once per process: one child process per capacity, one after the other, each with a time limit; a
    child that fails ends the test before the next one starts."""
    for cap in (240, 200, 129):
        env = dict(os.environ, INET_CHAIN_CUS=str(cap))
        env.pop("INET_DECODE_B1", None)
        r = subprocess.run([sys.executable, "-c", CHILD, REPO], env=env, cwd=REPO, capture_output=True, text=True, timeout=480)
        assert r.returncode == 0, (cap, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        done = json.loads(r.stdout.split("RESULT ", 1)[1])
        assert len(done) == 28, (cap, done)
        rows = sum(d[2] for d in done)
        assert sum(d[4] for d in done) >= 0.9 * rows, (cap, done)
