"""The per-measure attributes of the reference's dataset (DatasetManager/the_session/folk_dataset.py:607-708) as data: which
symbols of the vocabulary are the slur, the rest and None, and which MIDI pitch every other token carries.

ops.measure_attributes(tokens, spec) computes the four columns ATTRIBUTES on the device; VAETrainer(attr_reg=...) ties them to latent
dimensions (AR-VAE, Pati & Lerch 2020).  Pitch names are parsed here: music21 is not needed."""
import re

import numpy as np

ATTRIBUTES = ("num_notes", "note_range", "rhy_entropy", "beat_strength")

SLUR_SYMBOL = "__"
REST_SYMBOL = "rest"
_STEP = {"C": 0, "D": 2, "E": 4, "F": 5, "G": 7, "A": 9, "B": 11}
_NAME = re.compile(r"^([A-Ga-g])(#*|-*)(\d+)$")           # (a '-' is always a flat, as in music21: 'C-1' is C flat 1)


def pitch_midi(name):
    """'G3' -> 55, 'F#4' -> 66, 'B-4' -> 70 (music21's spelling: '#' sharpens, '-' flattens, C4 = 60); None for anything that is not a
    pitch name."""
    m = _NAME.match(name) if isinstance(name, str) else None
    if m is None:
        return None
    acc = m.group(2)
    return 12 * (int(m.group(3)) + 1) + _STEP[m.group(1).upper()] + (len(acc) if acc.startswith("#") else -len(acc))


class AttributeSpec(object):
    """What inet_measure_attrs needs to know about a vocabulary: num_tokens = V; slur_index, rest_index, none_index in [0, V) or -1
    (the vocabulary has none); midi, V ints, -1 for a token without a pitch (the three symbols always read as -1); pitch_range =
    (midi_lo, midi_hi), the reference's [55, 84], by which note_range is normalised."""

    def __init__(self, num_tokens, slur_index, rest_index, none_index, midi, pitch_range=(55, 84)):
        if isinstance(num_tokens, bool) or not isinstance(num_tokens, (int, np.integer)) or num_tokens < 1:
            raise ValueError(f"AttributeSpec: num_tokens must be an integer >= 1, got {num_tokens!r}")
        V = int(num_tokens)
        idx = []
        for name, v in (("slur_index", slur_index), ("rest_index", rest_index), ("none_index", none_index)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -1 <= v < V:
                raise ValueError(f"AttributeSpec: {name} must be an integer in [-1, {V}), got {v!r}")
            idx.append(int(v))
        table = np.asarray(midi)
        if table.shape != (V,) or not np.issubdtype(table.dtype, np.integer):
            raise ValueError(f"AttributeSpec: midi must hold {V} integers, got shape {table.shape} of {table.dtype}")
        if table.min() < -1 or table.max() > 127:
            raise ValueError("AttributeSpec: midi values must lie in [-1, 127]")
        try:
            lo, hi = (int(v) for v in pitch_range)
        except (TypeError, ValueError):
            raise ValueError(f"AttributeSpec: pitch_range must be (midi_lo, midi_hi), got {pitch_range!r}")
        if not lo < hi:
            raise ValueError(f"AttributeSpec: pitch_range must be (midi_lo, midi_hi) with midi_lo < midi_hi, got {pitch_range!r}")
        table = table.astype(np.int32)
        for i in idx:
            if i >= 0:
                table[i] = -1
        self.num_tokens, (self.slur_index, self.rest_index, self.none_index) = V, idx
        self.midi, self.pitch_range = table, (lo, hi)
        self._tables = {}

    @classmethod
    def from_dataset(cls, dataset, pitch_range=None):
        """Reads dataset.note2index_dicts[0]: the keys '__', 'rest' and None, every other key a pitch name ('G3', 'F#4', 'B-4') or a
        symbol without a pitch ('START', 'END', ...).  pitch_range None: the dataset's own, else the reference's (55, 84).  A
        vocabulary without a single pitch name -- the synthetic dataset's integer keys -- is refused."""
        dicts = getattr(dataset, "note2index_dicts", None)
        if not dicts:
            raise ValueError("AttributeSpec.from_dataset: the dataset has no note2index_dicts")
        n2i = dicts[0]
        V = len(n2i)
        midi = np.full(V, -1, np.int64)
        for name, i in n2i.items():
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < V:
                raise ValueError(f"AttributeSpec.from_dataset: index {i!r} of {name!r} is outside [0, {V})")
            m = pitch_midi(name)
            if m is not None:
                if not 0 <= m <= 127:
                    raise ValueError(f"AttributeSpec.from_dataset: {name!r} is MIDI pitch {m}, outside [0, 127]")
                midi[i] = m
        if not (midi >= 0).any():
            raise ValueError("AttributeSpec.from_dataset: no key of note2index_dicts[0] is a pitch name such as 'G3' "
                             f"(the keys are {sorted(map(repr, n2i))[:4]}...): pass an AttributeSpec built by hand as attr_spec / spec")
        if pitch_range is None:
            pitch_range = getattr(dataset, "pitch_range", None) or (55, 84)
        return cls(V, n2i.get(SLUR_SYMBOL, -1), n2i.get(REST_SYMBOL, -1), n2i.get(None, -1), midi, pitch_range)

    def state(self):
        """Plain values that rebuild the spec: AttributeSpec(**spec.state())."""
        return dict(num_tokens=self.num_tokens, slur_index=self.slur_index, rest_index=self.rest_index, none_index=self.none_index,
                    midi=[int(v) for v in self.midi], pitch_range=tuple(self.pitch_range))

    def __eq__(self, other):
        return isinstance(other, AttributeSpec) and self.state() == other.state()

    __hash__ = None

    def __repr__(self):
        return (f"AttributeSpec(V={self.num_tokens}, slur={self.slur_index}, rest={self.rest_index}, none={self.none_index}, "
                f"pitched={int((self.midi >= 0).sum())}, pitch_range={self.pitch_range})")

    def midi_table(self, device):
        """The table as a device int32 tensor, made once per device."""
        import torch
        key = str(device)
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self.midi).to(device)
        return self._tables[key]
