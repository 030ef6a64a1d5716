#!/usr/bin/env python3
"""The token pass of AnticipationRNN's free-running step alone (ops.arnn_generate, L = 384): python tools/arnn_token_pass.py
With INET_ARNN_GEN_STAMPS=1 the persistent kernel (csrc/arnn_gen.hip) also leaves wall-clock stamps of the phases of a tick in its
workspace: the anatomy of a tick as workgroup C (layer-0 cell, linear_1, head, argmax) and workgroup Bi_0 (layer-1 product + cell)
see it is printed below the timings.
    python tools/arnn_token_pass.py [V] --sample [--rows 1,8] [--temperature 6.0] [--top-k 8] [--top-p 0.9] [--mask] [--forced] [--rounds 5] [--iters 20]
times the SAMPLING build (ops.arnn_sample, L = 384, R independent rows) and the TRUNCATING build on the same inputs instead: the plain
call, the call that only asks for logp (truncation off), and one call per truncation given -- top-k alone, top-p alone, both when both
are given -- with device events, per round the median of --iters calls, over the rounds the median (range), and each truncating call's
cost per tick over the sampling build.  --mask adds, behind every truncating call, the CONSTRAINED call of the same arguments
(ops.arnn_sample's allowed=: the masked build) under tests/decoder_constraint_ref.plan_mask(V, R, T=L) -- every fourth tick fixed, a fifth
of the tokens banned elsewhere, the words packed once -- with its cost per tick over that truncating call.  --forced (with --mask) adds,
behind every constrained call, two calls of the FORCED build (ops.arnn_sample's forced=) under the same mask: the constrained call through
it (no tick forced: every word -1) and the ALL-FORCED call (tick t of row r forced to (5 r + 11 t + 2) % V), with the all-forced call's
cost per tick over the constrained call of the same build."""
import os, sys, time, types
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, bench
from inpaintnet_amd import ops, synthetic
from inpaintnet_amd.arnn import ConstraintModelGaussianReg
sys.stdout = sys.stderr
NOTES = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else bench.NUM_NOTES    # (V > 64: the two-register-set build of the token pass)


def _flag(name, default, conv):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
ds = synthetic.SyntheticFolkDataset(num_notes=NOTES)
ds.metadatas = [types.SimpleNamespace(num_values=6), types.SimpleNamespace(num_values=6)]
m = ConstraintModelGaussianReg(ds, note_embedding_dim=10, metadata_embedding_dim=2, num_lstm_constraints_units=256,
                               num_lstm_generation_units=256, linear_hidden_size=256, num_layers=2, dropout_input_prob=0.2,
                               dropout_prob=0.2, unary_constraint=True, teacher_forcing=True)
pr = m.param
oc0 = torch.randn(384, 256, device="cuda") * 0.1
args = (pr("note_embeddings.0.weight"), oc0, pr("lstm_generation.0.weight_ih_l0"), pr("lstm_generation.0.bias_ih_l0"),
        pr("lstm_generation.0.weight_hh_l0"), pr("lstm_generation.0.bias_hh_l0"), pr("lstm_generation.1.weight_ih_l0"),
        pr("lstm_generation.1.bias_ih_l0"), pr("lstm_generation.1.weight_hh_l0"), pr("lstm_generation.1.bias_hh_l0"),
        pr("linear_1.weight"), pr("linear_1.bias"), pr("linear_ouput_notes.0.weight"), pr("linear_ouput_notes.0.bias"))


def sample_builds():
    import numpy as np
    L, H = 384, 256
    rows = _flag("--rows", (1, 8), lambda v: tuple(int(x) for x in v.split(",")))
    temp, rounds, iters = _flag("--temperature", 6.0, float), _flag("--rounds", 5, int), _flag("--iters", 20, int)
    top_k, top_p = _flag("--top-k", None, int), _flag("--top-p", None, float)
    calls = [("sampling build", {}), ("truncating build, logp only", dict(want_logp=True))]
    if top_k is not None:
        calls.append((f"top_k={top_k}", dict(top_k=top_k, want_logp=True)))
    if top_p is not None:
        calls.append((f"top_p={top_p}", dict(top_p=top_p, want_logp=True)))
    if top_k is not None and top_p is not None:
        calls.append((f"top_k={top_k}, top_p={top_p}", dict(top_k=top_k, top_p=top_p, want_logp=True)))
    if "--mask" in sys.argv:
        from tests.decoder_constraint_ref import plan_mask
        forced = "--forced" in sys.argv
        calls = [c for name, kw in calls for c in ([(name, kw)] + ([(name + ", mask", dict(kw, mask=name))] if kw else []) +
                                                   ([(name + ", mask, forced build, no tick forced", dict(kw, mask=name, forced=-1)),
                                                     (name + ", mask, all forced", dict(kw, mask=name + ", mask, forced build, no tick forced",
                                                                                        forced=1))] if kw and forced else []))]
    for R in rows:
        if "--mask" in sys.argv:
            words = ops.pack_allowed(torch.from_numpy(plan_mask(NOTES, R, L))).cuda().contiguous()
            rr, tt = np.meshgrid(np.arange(R), np.arange(L), indexing="ij")
            fwords = {-1: torch.full((R, L), -1, dtype=torch.int32, device="cuda"),
                      1: torch.from_numpy(((5 * rr + 11 * tt + 2) % NOTES).astype(np.int32)).cuda().contiguous()}
        oc = torch.randn(R, L, H, device="cuda") * 0.5
        u = torch.from_numpy(np.random.RandomState(1).random_sample((R, L))).cuda()
        hc = torch.zeros(R, 2, 2, H, device="cuda")
        med = {}
        for name, kw in calls:
            kw = dict(kw)
            base = kw.pop("mask", None)                         # (the truncating call this constrained call is compared with)
            if base is not None:
                kw["allowed"] = words
            if "forced" in kw:
                kw["forced"] = fwords[kw["forced"]]
            fn = lambda: ops.arnn_sample(args[0], oc, *args[2:], temp, u, hc_init=hc, **kw)
            for _ in range(3): fn()
            torch.cuda.synchronize()
            per_round = []
            for _ in range(rounds):
                ts = []
                for _ in range(iters):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); fn(); b.record(); b.synchronize()
                    ts.append(a.elapsed_time(b))
                per_round.append(sorted(ts)[len(ts) // 2])
            med[name] = sorted(per_round)[len(per_round) // 2]
            over = "" if not kw else f"  {1e3 * (med[name] - med['sampling build']) / L:+.2f} us per tick over the sampling build"
            if base is not None:
                over = f"  {1e3 * (med[name] - med[base]) / L:+.2f} us per tick over " + \
                    ("the constrained call of the same build" if name.endswith("all forced") else "the truncating call")
            print(f"V = {NOTES}, R = {R}, T = {temp}: {name}: {med[name]:.4f} ms ({min(per_round):.4f} .. {max(per_round):.4f}), "
                  f"{1e3 * med[name] / L:.2f} us per tick{over}  chain status {ops.chain_status()}")


if "--sample" in sys.argv:
    sample_builds()
    sys.exit(0)

# option key 14: 0 = four launches per tick (round 4), 1 = one persistent launch (csrc/arnn_gen.hip), 2 = ... on one XCD
for mode in (0, 1, 2, 3):
    ops.set_option(14, mode)
    for _ in range(3): t = ops.arnn_generate(*args)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10): t = ops.arnn_generate(*args)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 10
    print(f"V = {NOTES}, mode {mode}: token pass, 384 ticks: {1e3 * dt:.2f} ms  ({1e6 * dt / 384:.2f} us per tick)  tokens {t[:8].tolist()} "
          f"chain status {ops.chain_status()}")
ops.set_option(14, 2)

if os.environ.get("INET_ARNN_GEN_STAMPS") == "1":
    L, V = 384, NOTES
    ops._ARNN_KEEP_WS.append(None)
    t = ops.arnn_generate(*args)
    torch.cuda.synchronize()
    ws = ops._ARNN_KEEP_WS[0]
    off = L * 1024 + V * 1024 + (2 * (4 * 256 + 2 * 1024 + 16) + 64) + 64      # csrc/arnn_gen.hip arnn_token_pass_stamps_offset
    st = ws[off:off + 32 * L].cpu().view(torch.int64).view(2, L, 8).double() * 0.01        # us (100 MHz wall clock)
    c, b = st[0, 8:L - 1], st[1, 8:L - 1]
    names_c = ["tok known -> gates, cell, publish h0", "wait for h1 (Bi's product + cell + two hand-offs)", "barrier", "linear_1 product + barrier",
               "head product + barrier", "argmax + barrier", "look at next tick's hh0 (requested under the head)"]
    print("C, mean us per phase over ticks 8..L-2:")
    for i, n in enumerate(names_c):
        print(f"  {float((c[:, i + 1] - c[:, i]).mean()):6.2f}  {n}")
    print(f"  {float((st[0, 9:L, 0] - st[0, 8:L - 1, 0]).mean()):6.2f}  tick period")
    names_b = ["wait for hh1 (requested early)", "wait for h0", "barrier", "W_ih1 product + barrier", "cell + publish h1"]
    print("Bi_0:")
    for i, n in enumerate(names_b):
        print(f"  {float((b[:, i + 1] - b[:, i]).mean()):6.2f}  {n}")
    # one-way hand-off estimates from the two clocks (the wall clock is chip-wide): C publishes h0 (stamp 1) -> Bi_0 has it (stamp 2)
    print(f"  h0: C published -> Bi_0 holds it {float((b[:, 2] - c[:, 1]).mean()):6.2f} us;  h1: Bi_0 published -> C holds it "
          f"{float((c[:, 2] - b[:, 5]).mean()):6.2f} us")
