"""The launches of the decoder calls, pinned to the ones recorded from the revision in front of the dec_route refactor
(tests/decoder_launches.py, tests/golden/decoder_launches.json): per case the same launch labels in the same
order, forward and backward, and, where the recording reproduced itself, the same weights and samples bit for bit.  ROUTE says which
launches make a case the route it stands for: the fixture itself is held to that, so a re-recording that misses a route fails here."""
import pytest
import torch

from tests import decoder_launches as DL

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic

CASES = DL.cases()


def count(labels, head):
    return sum(l.startswith(head) for l in labels)


# case -> what its forward labels must show
ROUTE = {
    "01 B1 inference": lambda l: l == ["decode_b1_beats T24 B1 H512 V48"],
    "02 B4 Z128 inference": lambda l: count(l, "decode_b1 T24 B4 ") == 1 and count(l, "decode_b1_beats") == 0 and len(l) == 8,
    "03 B2 beat mask inference": lambda l: count(l, "decode_b1 T24 B2 ") == 1 and count(l, "decode_b1_beats") == 0 and len(l) == 7,
    "04 B17 inference": lambda l: count(l, "decode_chain ") == 1 and count(l, "gru_fwd") == 0,
    "05 B768 inference": lambda l: [x for x in l if x.startswith("decode_")] == ["decode_chain ms2 T24 B256 H512 V48"] * 3,
    "06 B17 chains off": lambda l: count(l, "decode_") + count(l, "gru_chain") == 0 and count(l, "gru_fwd") == 2 * 24 + 2 * 4 and
    count(l, "logits_argmax") == 24,
    "07 B17 V50 chains off": lambda l: count(l, "decode_") + count(l, "logits_argmax") == 0 and count(l, "gru_fwd") == 2 * 24 + 2 * 4 and
    count(l, "M17 N50 K512 ") == 24,
    "08 B17 multinomial": lambda l: count(l, "decode_") + count(l, "logits_argmax") == 0 and count(l, "gru_fwd") == 2 * 24 and
    count(l, "M17 N48 K512 ") == 24,
    # (the four beat-path products of 4 x 17 rows keep one k range: " s1 ", where the argmax call of case 08 splits them)
    "09 B17 temperature top_p": lambda l: count(l, "decode_") == 0 and count(l, "trunc_sample B17 V48") == 24 and
    [" s1 " in x for x in l if x.startswith("M68 ")] == [True] * 4,
    "10 H64 B3 free and teacher-forced": lambda l: count(l, "decode_") + count(l, "gru_chain") == 0 and not any(" pk1 " in x for x in l) and
    sum(" pk0 " in x for x in l) == 2 * (4 + 24) + 2 * 4 + 2 * 6,
    "11 B32 teacher-forced train": lambda l: count(l, "gru_chain_fwd") == 4 and sum(" np4 T6 B32 " in x for x in l) == 2,
    "12 B256 teacher-forced train": lambda l: count(l, "gru_chain_fwd") == 6 and sum(" np2 T6 B256 " in x for x in l) == 4,
    "13 B32 free-running train": lambda l: count(l, "decode_chain_train ") == 1 and count(l, "gru_fwd") == 0,
    "14 B1024 teacher-forced train": lambda l: sum(" np1 T4 B512 " in x for x in l) == 4 and sum(" np4 T6 B128 " in x for x in l) == 16 and
    count(l, "gru_fwd") == 0,
    "15 B32 teacher-forced train chains off": lambda l: count(l, "gru_chain") == 0 and sum(" pk1 np4 B32 " in x for x in l) == 2 * 6,
    "16 B768 free-running train": lambda l: [x.split(" ms")[0] for x in l if x.startswith("decode_")] == ["decode_chain_train"] * 3 and
    sum(x.startswith("decode_chain_train ") and " B256 " in x for x in l) == 3 and sum(" np1 T4 B256 " in x for x in l) == 6,
}
# The cases that reproduce themselves by design and must carry a digest: the register-resident launch alone (01) or behind a beat path
# whose products are single-range gemv launches (03).  Two more were expected to and did not in the recorded revision's own two runs:
# 02 (its beat-path products of 4 x 4 = 16 rows are split over K, "s4", with f32 atomics: only a SAMPLED call asks for one k range)
# and 09 (a sampled call's beat-path products keep one range, but its per-tick logits product "M17 N48 K512 ... s4" is split as well).
# Both stay "digest": null -- labels alone -- as tests/golden/draw_launches.json already holds the B = 17 truncated calls.
REPRODUCIBLE = ("01 B1 inference", "03 B2 beat mask inference")


def test_the_fixture_covers_the_cases_and_shows_their_routes():
    fx = DL.fixture()["cases"]
    assert list(fx) == [name for name, _ in CASES] == list(ROUTE)
    for name, want in fx.items():
        assert ROUTE[name](want["labels"]), (name, want["labels"])
        assert (want["bwd_labels"] is not None) == bool(dict(DL.CASES)[name].get("save")), name
    for name in REPRODUCIBLE:
        assert fx[name]["digest"] is not None, name


@pytest.mark.parametrize("name,run", CASES, ids=[name.replace(" ", "-") for name, _ in CASES])
def test_launches_and_bits(name, run):
    want = DL.fixture()["cases"][name]
    labels, bwd, digest = run(ops, synthetic)
    assert labels == want["labels"], name
    assert bwd == want["bwd_labels"], name
    if want["digest"] is not None:
        assert digest == want["digest"], name


def test_fused_chunks_behind_row_chunked_beat_chains_reproduce_themselves():
    """Case 05 (three fused launches of 256 rows behind beat chains in three row chunks): in the recorded revision layer 1's second beat
    chunk left the fused launches' counters counted up and the first fused launch took them for zeroed, so workgroups read hand-offs
    nobody had written yet -- its two recorded runs differ, and on recycled memory a stale token index reads outside the gather table.
    The route now has that launch zero its counters: every kernel of the call is deterministic, so two calls agree bit for bit.
    Case 16 is the same odd-chunk form in training (decode_chain_train, with saves and both masks, and the backward call behind it): the
    fused launches take area 2 from the call's ledger (csrc/sync_areas.h), which knows that beat layer 1 counted on it."""
    for name in ("05 B768 inference", "16 B768 free-running train"):
        run, want = dict(CASES)[name], DL.fixture()["cases"][name]
        (l1, b1, d1), (l2, b2, d2) = run(ops, synthetic), run(ops, synthetic)
        assert l1 == l2 == want["labels"] and b1 == b2 == want["bwd_labels"], name
        assert d1 == d2, name
