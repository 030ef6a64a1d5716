#!/usr/bin/env python3
"""Golden vectors of the reference's per-measure attribute extractors.  TEST INFRASTRUCTURE.

Runs where oracle/gen_golden.py runs (the upstream reference importable behind its stub modules) and writes
tests/golden/attr_reference.npz: tokens [B, 24] (tests/attr_ref.py's vocabulary and draws, every row with at least one non-slur tick,
and its edge rows but the all-slur one) and what the reference's own FolkMeasuresDataset.get_num_notes_in_measure,
get_rhythmic_entropy and get_beat_strength (DatasetManager/the_session/folk_dataset.py:607-708) return on them.  The methods are called
on a small stand-in `self` that carries the two attributes they read, and on COPIES of the tokens: two of them overwrite their
argument.  get_note_range_of_measure needs music21 and is pinned to hand-worked rows in tests/test_attr_host.py instead.

    python tools/gen_golden_attr.py
"""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.gen_golden as gg  # noqa: E402  (stubs music21 & co. and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _more_stubs():
    """What the dataset modules import beyond oracle/gen_golden.py's stubs and this machine may lack; none of it is called here."""
    for name in ("tqdm", "music21.corpus", "music21.key", "music21.analysis", "music21.analysis.floatingKey"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = types.ModuleType(name)
                m.tqdm = lambda it=None, *a, **k: it
                sys.modules[name] = m
                parent, _, leaf = name.rpartition(".")
                if parent in sys.modules:
                    setattr(sys.modules[parent], leaf, m)


_more_stubs()
from DatasetManager.the_session import folk_dataset as fd  # noqa: E402
from tests import attr_ref as R  # noqa: E402
from tools.gen_golden_arnn_generate import save_npz  # noqa: E402

B, T = 40, 24


def main():
    tok = R.draw_tokens("golden", B, T)
    edges = R.edge_rows(T)
    tok = np.concatenate([tok] + [edges[k][None] for k in ("all_rest", "no_pitch", "one_pitch", "full_range")], 0)
    tok = tok[(tok != R.SPEC["slur_index"]).sum(1) >= 1]
    NOTES = 0
    me = types.SimpleNamespace(NOTES=NOTES, note2index_dicts=[{name: i for i, name in enumerate(R.VOCAB)}])
    assert fd.SLUR_SYMBOL == "__"
    t = torch.from_numpy(tok)
    fx = {"tokens": tok,
          "num_notes": fd.FolkMeasuresDataset.get_num_notes_in_measure(me, t.clone()).cpu().numpy(),
          "rhy_entropy": fd.FolkMeasuresDataset.get_rhythmic_entropy(me, t.clone()).cpu().numpy(),
          "beat_strength": fd.FolkMeasuresDataset.get_beat_strength(me, t.clone()).cpu().numpy()}
    assert np.array_equal(t.numpy(), tok)
    for k, v in fx.items():
        print(k, v.dtype, v.shape, v[:4])
    path = os.path.join(gg.OUT, "attr_reference.npz")
    save_npz(path, fx)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(fx), os.path.getsize(path)))


if __name__ == "__main__":
    main()
