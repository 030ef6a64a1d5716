"""The launches of the sampling calls, pinned to the recorded ones (tests/draw_launches.py, tests/golden/draw_launches.json; DESIGN.md
section 21): per case and request the same launch labels in the same order -- a request routed to a higher level's kernel returns the
same tokens and fails here alone -- and, where the recording reproduced itself, the same tokens and log-probabilities bit for bit."""
import pytest
import torch

from tests import draw_launches as DL

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic

CASES = DL.cases()


def test_the_fixture_covers_the_cases():
    assert list(DL.fixture()["cases"]) == [name for name, _ in CASES]


@pytest.mark.parametrize("name,run", CASES, ids=[name.replace(" ", "-") for name, _ in CASES])
def test_launches_and_bits(name, run):
    want = DL.fixture()["cases"][name]
    labels, digest = run(ops, synthetic)
    assert labels == want["labels"], name
    if want["digest"] is not None:
        assert digest == want["digest"], name


def test_truncation_off_still_files_a_trunc_label():
    labels, _ = DL.rows_case(ops, synthetic, "trunc_off")
    assert labels == [f"trunc_sample B{DL.ROWS} V{DL.ROWS_V}"]
