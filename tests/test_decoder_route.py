"""The route of a decoder forward call (csrc/vae.hip dec_route behind inet_vae_decoder_route / ops.decoder_route), checked on the host:
which beat path and tick path a call shape takes, and that what follows from the two -- the words the prologue zeroes, the twins that
are packed -- fits them for every call shape, option and chip size.  The launch asks the same function, and
tests/test_gpu_decoder_launches.py holds its launches to the ones recorded in front of the refactor; a route whose parts disagree
shows up on a GPU as a chain launch on counters nobody zeroed or a step kernel reading twins nobody packed."""
import itertools

import pytest

from inpaintnet_amd import _lib, ops

BS = tuple(range(1, 18)) + (32, 256, 512, 600, 768, 1024)
CALLS = (("inference", False, False), ("TF + save", True, True), ("free + save", True, False))      # name, save, teacher_forced
CAPACITIES = (256, 252, 250, 248, 245, 240, 230, 212, 200, 180, 160, 140, 129, 128, 100)           # tests/test_decode_plan.py's


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


def cfg_of(V=48, Z=256, H=512):
    return ops.vae_config(V, 10, H, Z, H)


def route(B, V=48, Z=256, H=512, **kw):
    return ops.decoder_route(cfg_of(V, Z, H), B, **kw)


TRAIN = dict(save=True, mask_beat=True, mask_tick=True)
# the cases of tests/decoder_launches.py on 256 CUs: call -> the parts of the route the case is there for
TABLE = (
    (dict(B=1), dict(beats="folded", ticks="Fused", b1=True, b1_fused=True, zero="b1ex+sync", pack_ht0="no")),
    (dict(B=4, Z=128), dict(beats="chained", ticks="Fused", b1=True, b1_fused=False, zero="b1ex+sync", pack_beat_twins=False)),
    (dict(B=2, mask_beat=True), dict(beats="chained", ticks="Fused", b1=True, b1_fused=False, zero="b1ex+sync", pack_beat_twins=False)),
    (dict(B=17), dict(ticks="Fused", b1=False, zero="sync", pack_ht0="once", pack_tick_twins=False, fused_prezeroed=True)),
    (dict(B=768), dict(beats="chained", ticks="FusedChunked", chunk_rows=256, pack_ht0="per_chunk", zero="sync", fused_prezeroed=False)),
    (dict(B=17, chains=0), dict(beats="steps", ticks="PerTick", zero="none", pack_tick_twins=True, pack_out_w=True, pack_ht0="once")),
    (dict(B=17, V=50, chains=0), dict(beats="steps", ticks="PerTick", zero="none", pack_tick_twins=True, pack_out_w=False)),
    (dict(B=17, multinomial_seed=True), dict(ticks="PerTick", pack_tick_twins=True, pack_ht0="once")),
    (dict(B=17, level=2), dict(ticks="PerTick", pack_tick_twins=True, pack_ht0="once")),
    (dict(B=3, H=64), dict(beats="steps", ticks="PerTick", pk=False, zero="none", pack_beat_twins=False, pack_tick_twins=False,
                           pack_out_w=False, pack_ht0="no")),
    (dict(B=3, H=64, teacher_forced=True), dict(beats="steps", ticks="TfSteps", pk=False, zero="none", pack_beat_twins=False,
                                               pack_tick_twins=False, pack_out_w=False, pack_ht0="no")),
    (dict(B=32, teacher_forced=True, **TRAIN), dict(beats="chained", ticks="TfChained", npl=4, zero="sync", pack_tick_twins=False)),
    (dict(B=256, teacher_forced=True, **TRAIN), dict(beats="chained", ticks="TfChained", npl=2, zero="sync", pack_tick_twins=False)),
    (dict(B=32, **TRAIN), dict(beats="chained", ticks="Fused", b1=False, zero="sync", pack_ht0="once")),
    (dict(B=1024, teacher_forced=True, save=True), dict(beats="chained", ticks="TfChained", zero="sync", pack_ht0="no")),
    (dict(B=32, teacher_forced=True, save=True, chains=0), dict(beats="steps", ticks="TfSteps", zero="none", pack_beat_twins=True,
                                                                 pack_tick_twins=True, pack_out_w=False, pack_ht0="once")),
)


@pytest.mark.parametrize("call,want", TABLE, ids=[" ".join(f"{k}={v}" for k, v in c.items()) for c, _ in TABLE])
def test_the_route_of_every_recorded_case(L, call, want):
    call = dict(call)
    chains = call.pop("chains", 1)
    try:
        assert L.inet_set_option(4, chains) == 0 and L.inet_set_option(15, 4) == 0
        got = route(**call)
    finally:
        L.inet_set_option(4, 1)
    assert {k: got[k] for k in want} == want, got


def violations(r, B, Z, H, save, tf, seed, mb, mt, level, chains):
    """The invariants that hold for every route, as a list of the ones this route breaks."""
    bad = []
    chain_beats, folded = r["beats"] == "chained", r["beats"] == "folded"
    fused, steps = r["ticks"] in ("Fused", "FusedChunked"), r["ticks"] in ("TfSteps", "PerTick")
    if (r["zero"] != "none") != (chain_beats or fused or r["ticks"] == "TfChained"):
        bad.append("sync words zeroed exactly for a chain, fused or b = 1 launch")
    if (r["zero"] == "b1ex+sync") != r["b1"]:
        bad.append("b1ex zeroed exactly for the b = 1 launch")
    if r["pack_beat_twins"] != (r["pk"] and r["beats"] == "steps") or r["pack_tick_twins"] != (r["pk"] and steps):
        bad.append("twins packed exactly for a per-step consumer")
    if r["pack_out_w"] and not (r["pk"] and r["ticks"] == "PerTick"):
        bad.append("out_w packed for the per-tick projection alone")
    # (decode_chain.hip's whole launch reads the packed initial hiddens as the step kernels do; the b = 1 launch and the chains do not)
    once = r["pk"] and (steps or (r["ticks"] == "Fused" and not r["b1"]))
    if r["pack_ht0"] != ("per_chunk" if r["ticks"] == "FusedChunked" else "once" if once else "no"):
        bad.append("ht0 packed once for step kernels and decode_chain's whole launch, per chunk for chunks")
    if level > 0 and (r["ticks"] == "FusedChunked" or (r["ticks"] == "Fused" and not r["b1"])):
        bad.append("a sampled call is fused only in the b = 1 launch")
    if r["b1_fused"] != folded or (r["b1_fused"] and not (r["b1"] and Z == 256 and not mb)):
        bad.append("b1_fused: Z = 256, no beat mask, no beat-path launches")
    if r["b1"] and not (r["ticks"] == "Fused" and B <= 16 and not save and not mt and not tf and not seed):
        bad.append("b1: inference of at most 16 rows without a tick mask")
    if (r["ticks"] in ("TfChained", "TfSteps")) != tf or (r["npl"] > 0) != (r["ticks"] == "TfChained") or r["npl"] not in (0, 1, 2, 4):
        bad.append("teacher-forced paths and npl")
    if (r["chunk_rows"] != 0) != (r["ticks"] == "FusedChunked") or (r["chunk_rows"] and (r["chunk_rows"] not in (256, 512) or
                                                                                      B % r["chunk_rows"] or B <= r["chunk_rows"])):
        bad.append("chunk rows")
    if seed and not tf and r["ticks"] != "PerTick":
        bad.append("a free-running multinomial draw runs tick by tick")
    if not r["pk"] and (r["beats"] != "steps" or not steps):
        bad.append("no twins: step kernels only")
    if not chains and (r["beats"] != "steps" or not steps):
        bad.append("chains off: step kernels only")
    # Row-chunked beat chains count on the area behind their layer's (csrc/seq.hip gru_layer_fwd), layer 1's on the fused launches'
    # counters: the first fused launch may call them zeroed only where the beat layers ran as one launch each (or not as chains).
    # (Found with case 05 of tests/decoder_launches.py: stale counters let a workgroup read tokens nobody had written yet.)
    beat_plan = ops.gru_chain_plan(H, B, 4, nprob=1, save=save)[0]
    chunked = chain_beats and beat_plan["launches"] > 1
    if r["fused_prezeroed"] != (fused and not chunked):
        bad.append("the first fused launch zeroes its counters behind row-chunked beat chains")
    return bad


def sweep_violations(L):
    """Every call shape under chains on / off on this process's chip.  Restores the options."""
    bad, seen = [], set()
    try:
        for chains in (1, 0):
            assert L.inet_set_option(4, chains) == 0 and L.inet_set_option(15, 4) == 0
            for (V, Z, H), B, (_, save, tf), level, seed, mb, mt in itertools.product(
                    ((48, 256, 512), (48, 128, 512), (50, 256, 512), (48, 256, 64)), BS, CALLS, range(5), (False, True), (False, True),
                    (False, True)):
                kw = dict(save=save, teacher_forced=tf, multinomial_seed=seed, mask_beat=mb, mask_tick=mt, level=level)
                if level > 0 and (tf or seed):                       # the entries refuse it, and so does the query
                    try:
                        route(B, V, Z, H, **kw)
                        bad.append(("accepted", V, Z, H, B, kw))
                    except ValueError:
                        pass
                    continue
                r = route(B, V, Z, H, **kw)
                seen.add((r["beats"], r["ticks"]))
                for what in violations(r, B, Z, H, save, tf, seed, mb, mt, level, chains):
                    bad.append((what, chains, V, Z, H, B, kw, r))
    finally:
        L.inet_set_option(4, 1)
        L.inet_set_option(15, 4)
    return bad, sorted(seen)


def test_every_route_is_consistent_on_the_full_chip(L):
    bad, seen = sweep_violations(L)
    assert not bad, (len(bad), bad[:6])
    # every tick path and every beat path is taken somewhere in the sweep
    assert {t for _, t in seen} == set(ops.DECODER_TICKS) and {b for b, _ in seen} == set(ops.DECODER_BEATS), seen


def test_every_route_is_consistent_below_the_full_chip():
    """The same sweep on partitions of the chip: INET_CHAIN_CUS is read once per process, so one child process per capacity, one after
    the other, each with a time limit."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, %r)\n"
            "from inpaintnet_amd import _lib\n"
            "from tests.test_decoder_route import sweep_violations\n"
            "print('VIOLATIONS ' + json.dumps(sweep_violations(_lib.lib())[0][:4]))\n") % repo
    failed = {}
    for cap in CAPACITIES[1:]:
        env = dict(os.environ, INET_CHAIN_CUS=str(cap))
        env.pop("INET_DECODE_B1", None)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=repo, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (cap, r.returncode, r.stderr[-2000:])
        bad = json.loads(r.stdout.split("VIOLATIONS ", 1)[1])
        if bad:
            failed[cap] = bad
    assert not failed, failed


def test_calls_the_query_refuses(L):
    import ctypes as C
    cfg, out = cfg_of(), (C.c_int32 * 13)()
    ok = lambda *a: L.inet_vae_decoder_route(*a)                                      # noqa: E731
    assert ok(C.byref(cfg), 1, 0, 0, 0, 0, out, 13) == 0
    for args in ((0, 0, 0, 0, 0), (1, 0, 0, 8, 0), (1, 0, 0, -1, 0), (1, 0, 0, 0, 5), (1, 0, 0, 0, -1), (1, 0, 1, 0, 1), (1, 0, 0, 1, 2)):
        assert ok(C.byref(cfg), *args, out, 13) == -1, args
    assert ok(C.byref(cfg), 1, 0, 0, 0, 0, out, 12) == -1 and ok(C.byref(cfg), 1, 0, 0, 0, 0, None, 13) == -1
    assert ok(None, 1, 0, 0, 0, 0, out, 13) == -1
    five = ops.vae_config(48, 10, 512, 256, 512, beats=5)
    assert ok(C.byref(five), 1, 0, 0, 0, 0, out, 13) == -1
