"""The optimizer step against bits recorded before its three kernels became one: every C entry point --
inet_adam_step_ex, inet_adam_step_clip, inet_adam_step_w -- in seven forms at thirteen sizes, one SHA-256 per (form, size) over p, m,
v, ema and the report words of every parameter combination (tests/adam_bits.py), compared with tests/golden/adam_step_bits.json as
tools/record_adam_bits.py wrote it.  With one kernel behind all entry points a comparison between them compares the kernel with itself;
this file is what says the arithmetic has not moved."""
import pytest
import torch

from tests import adam_bits as AB

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops

FIX = AB.load_fixture()


def test_the_inputs_are_the_recorded_ones():
    moved = [n for n in AB.SIZES if AB.inputs_digest(n) != FIX["inputs"][str(n)]]
    assert not moved, f"the INPUTS of tests/adam_bits.py, not the kernel, differ from the recorded ones at n = {moved}"


# the plain forms twice: through their own entry points and through ops.adamw_step
@pytest.mark.parametrize("form,through_w", [(f, False) for f in AB.FORMS] + [(f, True) for f in AB.PLAIN])
def test_the_step_computes_the_recorded_bits(form, through_w):
    moved = [n for n in AB.SIZES
             if AB.digest(ops, form, n, FIX["max_norm_half"][str(n)], through_w) != FIX["digests"][form][str(n)]]
    assert not moved, f"form {form}{' through adamw_step' if through_w else ''}: other bits than {FIX['revision']} at n = {moved}"


def test_a_step_without_partials_leaves_words_four_to_seven_alone():
    """What makes the four-word records of inet_adam_step_ex callers safe: without partials the kernel stores to words 0..3 only."""
    for n in (5, 4 * 10007 + 3):
        for kw in ({}, dict(weight_decay=AB.WEIGHT_DECAY)):
            c = AB.combos(n)[5]
            p, g, m, v, _ = (torch.tensor(a, device=AB.DEV) for a in AB.inputs(n, *c))
            rep = torch.tensor([0, 0, 0, 0, -1717986919, -1717986919, -1717986919, -1717986919], dtype=torch.int32).pin_memory()
            ops.adamw_step(p, g, m, v, AB.LR, c[0], gscale=c[1], step_flag=torch.zeros(2, device=AB.DEV), report=rep, **kw)
            torch.cuda.synchronize()
            assert rep.tolist() == [1, 0, 0, 0] + [-1717986919] * 4, (n, kw, rep)
