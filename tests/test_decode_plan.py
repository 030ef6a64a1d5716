"""The launch planner of the register-resident decode (csrc/decode_b1.hip make_plan / place_role), checked on the host for every call
size and vocabulary class: which workgroup id plays which role is pure arithmetic, and a mistake in it shows up on a GPU as a hang
until the bounded spins run out -- here it shows up as ok == 0.  (Plans per size: the table in front of make_plan.)"""
import ctypes as C

import pytest

from inpaintnet_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


def plan(L, B, V, Z=256):
    out = (C.c_int * 8)()
    rc = L.inet_decode_b1_plan(B, V, Z, out)
    keys = ("teams", "team_rows", "rgroups", "crit", "placed", "grid", "live", "ok")
    return rc, dict(zip(keys, list(out)))


@pytest.mark.parametrize("V", [20, 32, 48, 64, 80, 100, 128])
@pytest.mark.parametrize("B", list(range(1, 17)))
def test_every_role_once_critical_roles_on_one_residue(L, B, V):
    rc, p = plan(L, B, V)
    assert rc == 0, (B, V)
    assert p["ok"] == 1, (B, V, p)
    assert p["placed"] == 1 and p["grid"] <= 256 and p["live"] <= 256, (B, V, p)
    assert p["teams"] * p["team_rows"] >= B


def test_the_plans_per_call_size(L):
    """The table in csrc/decode_b1.hip, at V = 48 (merged build for one-row teams) and V = 100 (not merged)."""
    for V, merged in ((48, True), (100, False)):
        got = {B: plan(L, B, V)[1] for B in range(1, 17)}
        assert got[1]["teams"] == 1 and got[1]["live"] == (128 if merged else 129)          # 16 CB + 16 TA + 16 TBh + 80 | + C
        assert got[1]["crit"] == (32 if merged else 17)
        for B in (2, 3):                                    # whole one-row teams + the beat path
            assert (got[B]["teams"], got[B]["team_rows"], got[B]["rgroups"]) == (B, 1, 0), (V, B, got[B])
            assert got[B]["live"] == B * (48 if merged else 49) + 80
        assert got[4]["team_rows"] == 1 and got[4]["rgroups"] == 2                              # four measures: shared groups
        assert got[4]["crit"] == (32 if merged else 17)                                         # merged: CB + TA per team, TBh pairs
        assert got[4]["live"] == (4 * 32 + 2 * 16 + 80 if merged else 4 * 17 + 2 * 32 + 80)
        for B in (5, 6):                                    # one-row critical teams + groups of three rows + the beat path
            assert (got[B]["team_rows"], got[B]["rgroups"], got[B]["crit"]) == (1, 2, 16 if merged else 17), (V, B, got[B])
        for B in (7, 8, 9, 10):                             # whole two-row teams
            assert (got[B]["team_rows"], got[B]["rgroups"]) == (2, 0) and got[B]["live"] == got[B]["teams"] * 49
        for B in range(11, 17):                             # two-row critical teams + groups of six rows
            assert got[B]["team_rows"] == 2 and got[B]["rgroups"] == (2 * ((B + 1) // 2) + 5) // 6 and got[B]["crit"] == 17
            assert got[B]["live"] == got[B]["teams"] * 17 + got[B]["rgroups"] * 32


def test_calls_the_launch_does_not_take(L):
    assert plan(L, 17, 48)[0] == -1 and plan(L, 0, 48)[0] == -1 and plan(L, 4, 129)[0] == -1


# ---- every plan the decoder accepts (round-6 review: non-fused calls of four to six measures launched a template built for other
# rows; below the full chip the acceptance and the launch sized different grids) ----
VS = (1, 20, 32, 33, 48, 64, 65, 100, 128, 129)
ZS = (256, 128, 24)                                   # 256: the beat path folded in; any other latent size: behind its own launches
CAPACITIES = (256, 252, 250, 248, 245, 240, 230, 212, 200, 180, 160, 140, 129, 128, 100)


def sweep_violations(L, cap):
    """Every call size (B = 1 .. 17) x vocabulary x latent size under decode modes 1 to 5 on a chip of `cap` CUs.  The invariant: a
    call the planner accepts (rc == 0) passes its self-check (ok == 1) and fits the chip, a call outside the limits (B > 16, V > 128) is
    refused (rc == -1), and on the full chip every call inside them is accepted.  Restores the default mode."""
    bad = []
    try:
        for m in (1, 2, 3, 4, 5):
            assert L.inet_set_option(15, m) == 0
            for Z in ZS:
                for B in range(1, 18):
                    for V in VS:
                        rc, p = plan(L, B, V, Z)
                        inside = B <= 16 and V <= 128
                        if not inside and rc != -1:
                            bad.append(("accepted outside the limits", m, Z, B, V, rc, p))
                        elif inside and cap == 256 and rc != 0:
                            bad.append(("refused on the full chip", m, Z, B, V, rc, p))
                        elif rc == 0 and not (p["ok"] == 1 and p["grid"] <= cap and p["live"] <= cap and p["teams"] * p["team_rows"] >= B
                                              and (p["rgroups"] == 0 or p["placed"] == 1)):
                            bad.append(("inconsistent plan", m, Z, B, V, rc, p))
    finally:
        L.inet_set_option(15, 4)
    return bad


def test_every_plan_the_decoder_accepts_passes_its_check(L):
    """All five decode modes x B = 1 .. 17 x ten vocabularies x three latent sizes on this process's chip (the full one)."""
    bad = sweep_violations(L, 256)
    assert not bad, (len(bad), bad[:12])


def test_every_plan_the_decoder_accepts_below_the_full_chip():
    """The same sweep on partitions of the chip: INET_CHAIN_CUS is read once per process, so one child process per capacity, one after
    the other, each with a time limit."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, %r)\n"
            "from inpaintnet_amd import _lib\n"
            "from tests.test_decode_plan import sweep_violations\n"
            "print('VIOLATIONS ' + json.dumps(sweep_violations(_lib.lib(), int(sys.argv[1]))))\n") % repo
    failed = {}
    for cap in CAPACITIES:
        env = dict(os.environ, INET_CHAIN_CUS=str(cap))
        env.pop("INET_DECODE_B1", None)
        r = subprocess.run([sys.executable, "-c", code, str(cap)], env=env, cwd=repo, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (cap, r.returncode, r.stderr[-2000:])
        bad = json.loads(r.stdout.split("VIOLATIONS ", 1)[1])
        if bad:
            failed[cap] = (len(bad), bad[:4])
    assert not failed, failed


def test_the_plans_per_call_size_behind_the_beat_paths_launches(L):
    """The table in csrc/decode_b1.hip for calls whose beat path runs as launches of its own (a latent size other than 256, or a beat
    mask): four to six measures are whole two-row teams -- the one-row teams and groups of three rows of the folded plan would launch
    a template built for other rows."""
    for V in (20, 48, 100):
        got = {B: plan(L, B, V, Z=128) for B in range(1, 17)}
        assert all(rc == 0 and p["ok"] == 1 and p["placed"] == 1 for rc, p in got.values()), (V, got)
        got = {B: p for B, (rc, p) in got.items()}
        merged1, merged2 = V <= 64, V <= 32            # (one-row teams / two-row teams of the merged build)
        assert (got[1]["teams"], got[1]["team_rows"], got[1]["rgroups"]) == (1, 1, 0)
        for B in (1, 2, 3):                            # whole one-row teams, no beat path: 16 CB + 16 TA + 16 TBh, or C + 48
            assert (got[B]["teams"], got[B]["team_rows"], got[B]["rgroups"]) == (B, 1, 0), (V, B, got[B])
            assert got[B]["crit"] == (32 if merged1 else 17) and got[B]["live"] == B * (48 if merged1 else 49), (V, B, got[B])
        for B in range(4, 11):                         # whole two-row teams
            assert (got[B]["teams"], got[B]["team_rows"], got[B]["rgroups"]) == ((B + 1) // 2, 2, 0), (V, B, got[B])
            assert got[B]["crit"] == (32 if merged2 else 17) and got[B]["live"] == got[B]["teams"] * (48 if merged2 else 49), (V, B, got[B])
        for B in range(11, 17):                        # two-row critical teams + groups of six rows
            assert (got[B]["team_rows"], got[B]["rgroups"]) == (2, (2 * ((B + 1) // 2) + 5) // 6), (V, B, got[B])
            assert got[B]["crit"] == (16 if merged2 else 17) and got[B]["live"] == got[B]["teams"] * got[B]["crit"] + got[B]["rgroups"] * 32
        assert got[4]["live"] <= 98 and got[6]["live"] <= 147


FUSED_TABLE = {   # B: (V = 20, 48, 65, 100) -> (teams, team_rows, rgroups, crit, placed, grid, live), mode 4, Z = 256, 256 CUs
    1: ((1, 1, 0, 32, 1, 249, 128), (1, 1, 0, 32, 1, 249, 128), (1, 1, 0, 17, 1, 129, 129), (1, 1, 0, 17, 1, 129, 129)),
    2: ((2, 1, 0, 32, 1, 250, 176), (2, 1, 0, 32, 1, 250, 176), (2, 1, 0, 17, 1, 178, 178), (2, 1, 0, 17, 1, 178, 178)),
    3: ((3, 1, 0, 32, 1, 251, 224), (3, 1, 0, 32, 1, 251, 224), (3, 1, 0, 17, 1, 227, 227), (3, 1, 0, 17, 1, 227, 227)),
    4: ((4, 1, 2, 32, 1, 252, 240), (4, 1, 2, 32, 1, 252, 240), (4, 1, 2, 17, 1, 212, 212), (4, 1, 2, 17, 1, 212, 212)),
    5: ((5, 1, 2, 16, 1, 224, 224), (5, 1, 2, 16, 1, 224, 224), (5, 1, 2, 17, 1, 229, 229), (5, 1, 2, 17, 1, 229, 229)),
    6: ((6, 1, 2, 16, 1, 240, 240), (6, 1, 2, 16, 1, 240, 240), (6, 1, 2, 17, 1, 246, 246), (6, 1, 2, 17, 1, 246, 246)),
    7: ((4, 2, 0, 32, 1, 252, 192), (4, 2, 0, 17, 1, 196, 196), (4, 2, 0, 17, 1, 196, 196), (4, 2, 0, 17, 1, 196, 196)),
    8: ((4, 2, 0, 32, 1, 252, 192), (4, 2, 0, 17, 1, 196, 196), (4, 2, 0, 17, 1, 196, 196), (4, 2, 0, 17, 1, 196, 196)),
    9: ((5, 2, 0, 32, 1, 253, 240), (5, 2, 0, 17, 1, 245, 245), (5, 2, 0, 17, 1, 245, 245), (5, 2, 0, 17, 1, 245, 245)),
    10: ((5, 2, 0, 32, 1, 253, 240), (5, 2, 0, 17, 1, 245, 245), (5, 2, 0, 17, 1, 245, 245), (5, 2, 0, 17, 1, 245, 245)),
    11: ((6, 2, 2, 16, 1, 160, 160), (6, 2, 2, 17, 1, 166, 166), (6, 2, 2, 17, 1, 166, 166), (6, 2, 2, 17, 1, 166, 166)),
    12: ((6, 2, 2, 16, 1, 160, 160), (6, 2, 2, 17, 1, 166, 166), (6, 2, 2, 17, 1, 166, 166), (6, 2, 2, 17, 1, 166, 166)),
    13: ((7, 2, 3, 16, 1, 208, 208), (7, 2, 3, 17, 1, 215, 215), (7, 2, 3, 17, 1, 215, 215), (7, 2, 3, 17, 1, 215, 215)),
    14: ((7, 2, 3, 16, 1, 208, 208), (7, 2, 3, 17, 1, 215, 215), (7, 2, 3, 17, 1, 215, 215), (7, 2, 3, 17, 1, 215, 215)),
    15: ((8, 2, 3, 16, 1, 224, 224), (8, 2, 3, 17, 1, 232, 232), (8, 2, 3, 17, 1, 232, 232), (8, 2, 3, 17, 1, 232, 232)),
    16: ((8, 2, 3, 16, 1, 224, 224), (8, 2, 3, 17, 1, 232, 232), (8, 2, 3, 17, 1, 232, 232), (8, 2, 3, 17, 1, 232, 232)),
}


def test_the_folded_plans_on_the_full_chip_are_the_measured_ones(L):
    """The plans behind the measured decode latencies (beat path folded in up to six measures), pinned: teams, rows, groups, critical
    workgroups, grid and live workgroups of every call size and vocabulary class."""
    keys = ("teams", "team_rows", "rgroups", "crit", "placed", "grid", "live")
    for B, per_v in FUSED_TABLE.items():
        for V, want in zip((20, 48, 65, 100), per_v):
            rc, p = plan(L, B, V)
            assert rc == 0 and p["ok"] == 1 and tuple(p[k] for k in keys) == want, (B, V, p, want)
