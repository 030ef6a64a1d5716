"""The route of a decoder forward call (csrc/vae.hip dec_route behind inet_vae_decoder_route / ops.decoder_route), checked on the host:
which beat path and tick path a call shape takes, and that what follows from the two -- the words the prologue zeroes, the twins that
are packed -- fits them for every call shape, option and chip size.  The launch asks the same function, and
tests/test_gpu_decoder_launches.py holds its launches to the ones recorded in front of the refactor; a route whose parts disagree
shows up on a GPU as a chain launch on counters nobody zeroed or a step kernel reading twins nobody packed.
tests/golden/decoder_routes.json (tools/record_decoder_routes.py) pins the routes of the whole sweep to the revision in front of the
sync-area ledger."""
import ctypes
import functools
import hashlib
import itertools
import json
import os
import subprocess
import sys

import pytest

from inpaintnet_amd import _lib, ops

# (320 / 576 / 768: the smallest batches whose beat chains run in row chunks on 128 / 256 chips and in front of fused chunks; on 64 and 40 CUs
# -- INET_CHAIN_CUS is at least 100 here -- that would be 192 and 128)
BS = tuple(range(1, 18)) + (32, 256, 320, 512, 576, 600, 768, 1024)
CALLS = (("inference", False, False), ("TF + save", True, True), ("free + save", True, False))      # name, save, teacher_forced
CAPACITIES = (256, 252, 250, 248, 245, 240, 230, 212, 200, 180, 160, 140, 129, 128, 100)           # tests/test_decode_plan.py's
CONFIGS = ((48, 256, 512), (48, 128, 512), (50, 256, 512), (48, 256, 64))                          # V, Z, H
SYNC_AREAS = 8                                                                                      # csrc/gru_chain.h kSyncAreas
ROUTES_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_routes.json")


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


@functools.lru_cache(maxsize=None)
def row_chunks(H, B, T, nprob, save, chains):
    """launches of a forward chain layer that runs in row chunks under option 4 = `chains` (which the caller has set), else 0"""
    p = ops.gru_chain_plan(H, B, T, nprob=nprob, save=save)[0]
    return p["launches"] if p["route"] in ("chain1", "chain2") and p["launches"] > 1 else 0


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
    # The sync areas, as the dry run of the call's ledger reports them (csrc/sync_areas.h, csrc/vae.hip dec_route_areas).  The fused launches
    # count on area 2, and so does a row-chunked beat layer 1 (the area behind its own): the first fused launch may call the area zeroed
    # exactly where the beat path left it alone.  (Found with case 05 of tests/decoder_launches.py: stale counters let a workgroup read
    # tokens nobody had written yet.)
    if (r["beat_areas"] | r["tick_areas"]) >> SYNC_AREAS:
        bad.append("every area is inside the block")
    if r["fused_prezeroed"] != (fused and not r["beat_areas"] >> 2 & 1):
        bad.append("the first fused launch zeroes its counters exactly where the beat path counted on them")
    # launches that zero their own counters: never more than the rule in front of the ledger gave -- every launch of a row-chunked forward
    # layer, the first fused launch behind row-chunked beat chains, fused chunks after the first -- and none where every layer is one launch
    beat_chunks = row_chunks(H, B, 4, 1, save, chains) if chain_beats else 0
    tick_chunks = row_chunks(H, B, 6, r["npl"], save, chains) if r["ticks"] == "TfChained" else 0
    fused_launches = B // r["chunk_rows"] if r["chunk_rows"] else int(fused)
    before = 2 * beat_chunks + 2 * (4 // r["npl"]) * tick_chunks if r["npl"] else 2 * beat_chunks
    before += (fused_launches - 1) + int(bool(beat_chunks)) if fused else 0
    if r["self_zeroed"] > before or r["self_zeroed"] < 0:
        bad.append("no launch zeroes its counters that did not before the ledger")
    if not beat_chunks and not tick_chunks and fused_launches <= 1 and r["self_zeroed"] != 0:
        bad.append("one launch per layer: nobody zeroes its own counters")
    return bad


def sweep(L, check=True):
    """Every call shape under chains on / off on this process's chip -> (the violations, the (beat path, tick path) pairs seen, per
    "V Z H chains" the SHA-256 over the 13 integers of every route in sweep order and their count).  check=False: the digests alone (the
    recorder's, on a library in front of the ledger).  Restores the options."""
    bad, seen, digests = [], set(), {}
    out = (ctypes.c_int32 * 13)()
    try:
        for chains in (1, 0):
            assert L.inet_set_option(4, chains) == 0 and L.inet_set_option(15, 4) == 0
            for V, Z, H in CONFIGS:
                h, n, cfg = hashlib.sha256(), 0, cfg_of(V, Z, H)
                for B, (_, save, tf), level, seed, mb, mt in itertools.product(BS, CALLS, range(5), (False, True), (False, True), (False, True)):
                    kw = dict(save=save, teacher_forced=tf, multinomial_seed=seed, mask_beat=mb, mask_tick=mt, level=level)
                    rc = L.inet_vae_decoder_route(ctypes.byref(cfg), B, int(save), int(tf), int(seed) | 2 * int(mb) | 4 * int(mt), level, out, 13)
                    if level > 0 and (tf or seed):                   # the entries refuse it, and so does the query
                        if rc != -1:
                            bad.append(("accepted", V, Z, H, B, kw))
                        continue
                    assert rc == 0, (rc, V, Z, H, B, kw)
                    h.update(b"".join(int(v).to_bytes(4, "little", signed=True) for v in out))
                    n += 1
                    if not check:
                        continue
                    r = route(B, V, Z, H, **kw)
                    seen.add((r["beats"], r["ticks"]))
                    for what in violations(r, B, Z, H, save, tf, seed, mb, mt, level, chains):
                        bad.append((what, chains, V, Z, H, B, kw, r))
                digests[f"V{V} Z{Z} H{H} chains{chains}"] = [h.hexdigest(), n]
    finally:
        L.inet_set_option(4, 1)
        L.inet_set_option(15, 4)
    return bad, sorted(seen), digests


def sweep_in_child(cap, tree=None, check=True):
    """sweep() on a chip of `cap` CUs: INET_CHAIN_CUS is read once per process, so a child process, with a time limit.  tree: a built
    checkout whose library to ask (this one's by default).  -> (the first violations, the digests)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, %r)\n"
            "from inpaintnet_amd import _lib, ops\n"
            "sys.path.insert(0, %r)\n"
            "from tests.test_decoder_route import sweep\n"
            "bad, _, digests = sweep(_lib.lib(), %r)\n"
            "print('SWEEP ' + json.dumps([bad[:4], digests]))\n") % (os.path.abspath(tree or repo), repo, check)
    env = dict(os.environ, INET_CHAIN_CUS=str(cap))
    env.pop("INET_DECODE_B1", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=repo, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (cap, r.returncode, r.stderr[-2000:])
    return tuple(json.loads(r.stdout.split("SWEEP ", 1)[1]))


child = functools.lru_cache(maxsize=None)(sweep_in_child)        # one child per capacity for the tests below


def test_every_route_is_consistent_on_the_full_chip(L):
    bad, seen, _ = sweep(L)
    assert not bad, (len(bad), bad[:6])
    # every tick path and every beat path is taken somewhere in the sweep
    assert {t for _, t in seen} == set(ops.DECODER_TICKS) and {b for b, _ in seen} == set(ops.DECODER_BEATS), seen


def test_every_route_is_consistent_below_the_full_chip():
    """The same sweep on partitions of the chip, one child process per capacity, one after the other."""
    failed = {cap: child(cap)[0] for cap in CAPACITIES[1:] if child(cap)[0]}
    assert not failed, failed


def test_every_route_is_the_one_recorded_in_front_of_the_ledger():
    """Per capacity, configuration and chains on / off: the digest over the 13 integers of every route of the sweep, and their count, as
    tools/record_decoder_routes.py took them from the revision the fixture names."""
    with open(ROUTES_FIXTURE) as f:
        fx = json.load(f)
    assert fx["BS"] == list(BS) and [int(c) for c in fx["capacities"]] == list(CAPACITIES)
    differ = {(cap, k): (v, fx["capacities"][str(cap)].get(k)) for cap in CAPACITIES for k, v in child(cap)[1].items()
              if v != fx["capacities"][str(cap)].get(k)}
    assert not differ, differ
    assert all(len(fx["capacities"][str(cap)]) == 2 * len(CONFIGS) for cap in CAPACITIES)


def test_the_rows_the_ledger_checks_are_there(L):
    """The routes the new assertions of violations() are for: row-chunked beat chains in front of fused chunks (256 CUs: 3 x 256 at B = 768)
    and in front of chunked teacher-forced chains (9 x 64 at B = 576); on 128 CUs 5 x 64 at B = 320."""
    r = route(768, **TRAIN)
    assert (r["ticks"], r["chunk_rows"], r["fused_prezeroed"], r["beat_areas"], r["tick_areas"]) == ("FusedChunked", 256, False, 0b111, 0b100)
    assert r["self_zeroed"] == 3 + 3          # of each beat layer's three launches the first two / the second find a clean area; no fused launch
    r = route(576, teacher_forced=True, **TRAIN)
    tick_chunks = ops.gru_chain_plan(512, 576, 6, nprob=r["npl"])[0]["launches"]
    assert (r["ticks"], ops.gru_chain_plan(512, 576, 4, nprob=1)[0]["launches"], r["beat_areas"]) == ("TfChained", 9, 0b111) and tick_chunks > 1
    assert r["fused_prezeroed"] is False and 0 < r["self_zeroed"] < 2 * 9 + 2 * (4 // r["npl"]) * tick_chunks
    r = route(256, teacher_forced=True, **TRAIN)
    assert (r["npl"], r["beat_areas"], r["tick_areas"], r["self_zeroed"]) == (2, 0b11, 0b111100, 0)


def test_calls_the_query_refuses(L):
    C = ctypes
    cfg, out = cfg_of(), (C.c_int32 * 13)()
    ok = lambda *a: L.inet_vae_decoder_route(*a)                                      # noqa: E731
    assert ok(C.byref(cfg), 1, 0, 0, 0, 0, out, 13) == 0
    for args in ((0, 0, 0, 0, 0), (1, 0, 0, 8, 0), (1, 0, 0, -1, 0), (1, 0, 0, 0, 5), (1, 0, 0, 0, -1), (1, 0, 1, 0, 1), (1, 0, 0, 1, 2)):
        assert ok(C.byref(cfg), *args, out, 13) == -1, args
    assert ok(C.byref(cfg), 1, 0, 0, 0, 0, out, 12) == -1 and ok(C.byref(cfg), 1, 0, 0, 0, 0, None, 13) == -1
    assert ok(None, 1, 0, 0, 0, 0, out, 13) == -1
    five = ops.vae_config(48, 10, 512, 256, 512, beats=5)
    assert ok(C.byref(five), 1, 0, 0, 0, 0, out, 13) == -1
    # n_out 13 .. 15 writes the 13 values of old, 16 the areas behind them
    wide = (C.c_int32 * 16)(*([77] * 16))
    assert ok(C.byref(cfg), 768, 0, 0, 0, 0, wide, 15) == 0 and list(wide[13:]) == [77] * 3
    assert ok(C.byref(cfg), 768, 0, 0, 0, 0, wide, 16) == 0 and list(wide[12:]) == [0, 0b111, 0b100, 6]
