"""Test surface of the AnticipationRNN (AnticipationRNN/anticipation_rnn_tester.py of the reference): inpainting loss /
accuracy over a loader, and generation of a window of measures with ConstraintModelGaussianReg.generate (temperature 1.5).

The tensor -> music21 score conversions (dataset.tensor_to_score, dataset.transposed_score_and_metadata_tensors) are outside
the hot path: they are used when the dataset offers them, otherwise the score slots of the return tuples are None and
`generation` takes the metadata from its caller (tensor_metadata=) or raises ValueError naming what is missing.
"""
import os
from random import randint

import numpy as np
import torch

from . import ops
from .arnn import AnticipationRNNGaussianRegTrainer
from .helpers import to_cuda_variable_long


def _num_variations(n):
    if isinstance(n, bool) or n != n or int(n) != n or n < 1:
        raise ValueError(f"generation: num_variations {n!r} is not a positive integer")
    return int(n)


def _fixed_ticks(fixed_tokens, W, measure_seq_len, V):
    """generation()'s fixed_tokens as a flat int64 (W,) host tensor, -1 = a free tick; ValueError for a wrong shape, dtype or range"""
    fixed = torch.as_tensor(fixed_tokens).cpu()
    if fixed.is_floating_point() or fixed.dtype == torch.bool or fixed.numel() != W or \
            (fixed.dim() != 1 and tuple(fixed.shape) != (W // measure_seq_len, measure_seq_len)):
        raise ValueError(f"fixed_tokens must be an int tensor of shape {(W // measure_seq_len, measure_seq_len)} or "
                         f"{(W,)}, got {fixed.dtype} {tuple(fixed.shape)}")
    fixed = fixed.long().reshape(W)
    if bool(((fixed < -1) | (fixed >= V)).any()):
        raise ValueError(f"fixed_tokens: token indices in [0, {V}), or -1 for a free tick")
    return fixed


class AnticipationRNNTester(object):
    def __init__(self, dataset, model):
        self.dataset = dataset
        self.model = model
        self.model.eval()
        if self.model.flat.is_cuda:
            ops.preload()                            # no generation call pays a kernel's first launch (csrc/preload.hip)
        self.filepath = os.path.join('models/', self.model.__repr__())
        self.batch_size = 1
        self.measure_seq_len = 24                    # (:16-18: set from the dataset, then fixed to 24)
        self.last_logp = None                        # generation(top_k= / top_p=): (num_variations, num_measures_gen)
        self.last_tick_logp = None                   # score(): (N, num_measures_gen, measure_seq_len)

    def _to_score(self, tensor):
        fn = getattr(self.dataset, "tensor_to_score", None)
        return fn(tensor.cpu()) if fn is not None else None

    def test_model(self, batch_size=512):
        """Loss / accuracy of inpainting on the test split (:20-42)."""
        (_, gen_val, gen_test) = self.dataset.data_loaders(batch_size=batch_size, split=(0.01, 0.01))
        print('Num Test Batches: ', len(gen_test))
        mean_loss_test, mean_accuracy_test = self.loss_and_acc_test(gen_test)
        print(f'Test Epoch: {1}/{1}')
        print(f'\tTest Loss: {mean_loss_test}'
              f'\tTest Accuracy: {mean_accuracy_test * 100} %')
        return mean_loss_test, mean_accuracy_test

    def loss_and_acc_test(self, data_loader):
        """Mean loss / accuracy of forward_inpaint over the loader, targets = the unconstrained ticks (:44-86)."""
        mean_loss = mean_accuracy = 0.0
        for batch in data_loader:
            score_tensor, metadata_tensor, constraints_loc, start_tick, end_tick = self.process_batch_data(batch)
            with torch.no_grad():
                weights, _ = self.model.forward_inpaint(score_tensor=score_tensor, metadata_tensor=metadata_tensor,
                                                        constraints_loc=constraints_loc, start_tick=start_tick, end_tick=end_tick)
                targets = score_tensor[:, :, (constraints_loc[0, 0, :] == 0).nonzero().squeeze(-1)].transpose(0, 1)
                loss = self.mean_crossentropy_loss(weights=weights, targets=targets)
                accuracy = self.mean_accuracy(weights=weights, targets=targets)
            mean_loss += float(loss)
            mean_accuracy += float(accuracy)
            ops.check_chains("AnticipationRNNTester.loss_and_acc_test")
        return mean_loss / len(data_loader), mean_accuracy / len(data_loader)

    def loss_and_acc_test_alt(self, data_loader):
        """Loss / accuracy of the training objective at one tick near the middle, t = seq_size_in_beats * subdivision / 2 +
        np.random.randint(-5, 5) per batch (:88-130)."""
        mean_loss = mean_accuracy = 0.0
        for batch in data_loader:
            score_tensor, metadata_tensor, _, _, _ = self.process_batch_data(batch)
            with torch.no_grad():
                # the reference's call passes no constraints_loc (:101-104): here the tensor's ticks are all unconstrained, so
                # forward() returns every tick and `t` indexes ticks as in the reference's intent
                loc = torch.zeros_like(score_tensor)
                weights, _ = self.model(score_tensor=score_tensor, metadata_tensor=metadata_tensor, constraints_loc=loc, train=False)
                t = int(self.dataset.seq_size_in_beats * self.dataset.subdivision / 2) + np.random.randint(-5, 5)
                targets = score_tensor[:, :, t].transpose(0, 1)
                w = [wv[:, t, :] for wv in weights]
                loss = self.mean_crossentropy_loss(weights=[x[:, None] for x in w], targets=targets[:, :, None])
                accuracy = self.mean_accuracy(weights=[x[:, None] for x in w], targets=targets[:, :, None])
            mean_loss += float(loss)
            mean_accuracy += float(accuracy)
            ops.check_chains("AnticipationRNNTester.loss_and_acc_test_alt")
        return mean_loss / len(data_loader), mean_accuracy / len(data_loader)

    def generation_test(self):
        """Inpainting of measures 8 and 9 on a random sample of the test split (:132-183) -> (gen_score | None, gen_score_tensor
        (1, L): past | generated | future, original_score | None).  (The reference unpacks process_batch_data's five values into
        two, :149; here the batch's score and metadata are taken directly.)"""
        (_, gen_val, gen_test) = self.dataset.data_loaders(batch_size=1, split=(0.70, 0.20))
        gen_it_test = iter(gen_test)
        batch = next(gen_it_test)
        for _ in range(randint(0, len(gen_test)) - 1):
            batch = next(gen_it_test)
        tensor_score, tensor_metadata = to_cuda_variable_long(batch[0]), to_cuda_variable_long(batch[1])
        batch_size, num_voices, seq_len, num_metadata = tensor_metadata.size()
        assert batch_size == 1
        return self._generate_window(tensor_score.view(num_voices, seq_len),
                                     tensor_metadata.view(num_voices, seq_len, num_metadata), start_measure=8, num_measures_gen=2)

    def generation(self, tensor_score, start_measure, num_measures_gen, tensor_metadata=None, temperature=1.5, num_variations=1,
                   top_k=None, top_p=None, banned_tokens=None, fixed_tokens=None, clamp_context=False, score_fixed=False):
        """Generates measures start_measure .. start_measure + num_measures_gen - 1 (1-based) of a score with temperature 1.5
        (:185-243) -> (gen_score | None, gen_score_tensor (1, L): past | generated | future, original_score | None).

        num_variations fillings of the one gap come from ONE batched generate() call over num_variations copies of the score, its
        metadata and its constraints: gen_score_tensor is (num_variations, L), past and future the input's in every row.  top_k /
        top_p: generate()'s truncation; with one of them self.last_logp is (num_variations, num_measures_gen) float32, the sum of the
        window's log-probabilities per measure (NaN where a tick took the argmax rule) -- what to rank the fillings by; else None.

        banned_tokens (a list of token indices): never returned at any tick of the window -- START, END or a padding symbol in the
        middle of a piece.  fixed_tokens (an int tensor (num_measures_gen, measure_seq_len) or flat, -1 = a free tick): the notes to
        keep; a fixed tick wins over a ban.  clamp_context=True fixes every tick OUTSIDE the window to the score's own token: generate()
        draws every tick, so without it the generation LSTMs reach the gap behind their own drawn version of the past; with it they
        reach it behind the true past.  All three act inside the launch (generate()'s `allowed`): the token fed into tick t + 1 is the
        constrained one.  Every variation gets the same mask, and with one of the three given the batched call is taken for
        num_variations=1 too.  ValueError for an index outside [0, V) (fixed: other than -1), a ban of the whole vocabulary, or -- with
        clamp_context -- a score token outside [0, V).  A fixed tick adds exactly 0 to last_logp.

        score_fixed=True: the fixed ticks become FORCED ticks under a mask of all ones (generate()'s `forced`): the
        same notes are kept and fed back -- a fixed tick still wins over a ban --, and last_logp, which such a call always leaves,
        includes what the model thinks of the kept notes instead of exactly 0.

        tensor_score (1, L) tokens (None: a random score of dataset.iterator_gen()); its metadata come from
        dataset.transposed_score_and_metadata_tensors where the dataset has it and a score can be built, else from
        `tensor_metadata` (1, L, M).  Where the reference trims a score whose length is not a multiple of a measure it indexes
        one tick (`tensor_score[:, n * len]`, :211-212) and compares a tick count with 16 measures (`min(16, size(1))`, :213):
        here the score is cut to whole measures and to at most 16 of them."""
        num_variations = _num_variations(num_variations)
        if tensor_score is None:
            if not hasattr(self.dataset, "iterator_gen"):
                raise ValueError("generation: tensor_score is None and the dataset has no iterator_gen()")
            score_gen = iter(self.dataset.iterator_gen())
            original_score = next(score_gen)
            for _ in range(randint(0, 100) - 1):
                original_score = next(score_gen)
        else:
            original_score = self._to_score(tensor_score) if tensor_metadata is None else None
        if original_score is not None and hasattr(self.dataset, "transposed_score_and_metadata_tensors"):
            trans_interval = self.dataset.get_transpostion_interval_from_semitone(0)
            tensor_score, tensor_metadata = self.dataset.transposed_score_and_metadata_tensors(original_score, trans_interval)
        elif tensor_metadata is None:
            raise ValueError("generation: pass tensor_metadata= (the dataset cannot derive it: no tensor_to_score / "
                             "transposed_score_and_metadata_tensors)")
        tensor_score = to_cuda_variable_long(torch.as_tensor(tensor_score))
        tensor_metadata = to_cuda_variable_long(torch.as_tensor(tensor_metadata))
        num_measures = min(16, tensor_score.size(1) // self.measure_seq_len)
        tensor_score = tensor_score[:, :num_measures * self.measure_seq_len]
        tensor_metadata = tensor_metadata[:, :num_measures * self.measure_seq_len]
        return self._generate_window(tensor_score, tensor_metadata, start_measure, num_measures_gen, temperature, num_variations,
                                     top_k, top_p, banned_tokens, fixed_tokens, clamp_context, score_fixed)

    def score(self, tensor_score, start_measure, num_measures_gen, fillings, tensor_metadata=None, temperature=1.0, top_k=None,
              top_p=None, banned_tokens=None):
        """The model's log-probability of GIVEN fillings of measures start_measure .. start_measure + num_measures_gen - 1 (1-based) --
        the user's, the original measures, an InpaintNet filling -- on the scale of generation()'s last_logp: -> float32 (N,
        num_measures_gen), the window's log-probabilities summed per measure under softmax(temperature * logits) behind the same top_k
        / top_p truncation and bans a draw would have seen.  -inf where a note is banned or truncated away, NaN where the rule does not
        apply; both propagate.

        fillings: an int tensor (N, num_measures_gen, measure_seq_len) with every value in [0, V).  The score is expanded to N rows as
        generation() expands it for variations; every tick of the window is forced to the filling and every tick outside it to the
        score's own token, the true context (ValueError for a token outside [0, V) there, as under clamp_context) -- ONE forced
        generate() call with uniforms of zeros: np.random is not touched.  banned_tokens act inside the window only, as in generation().
        Leaves self.last_tick_logp (N, num_measures_gen, measure_seq_len) and model.last_weights (N, L, V).  tensor_score and
        tensor_metadata as generation() takes them (tensor_score is required)."""
        measure_seq_len = self.dataset.subdivision * self.dataset.num_beats_per_bar
        V = int(self.model.num_notes_per_voice[0])
        fill = torch.as_tensor(fillings)
        if fill.is_floating_point() or fill.is_complex() or fill.dtype == torch.bool or fill.dim() != 3 or fill.size(0) < 1 or \
                tuple(fill.shape[1:]) != (num_measures_gen, measure_seq_len):
            raise ValueError(f"score: fillings must be an int tensor of shape (N, {num_measures_gen}, {measure_seq_len}), got {fill.dtype} "
                             f"{tuple(fill.shape)}")
        fill = fill.cpu().long()
        if bool(((fill < 0) | (fill >= V)).any()):
            raise ValueError(f"score: fillings hold a token outside [0, {V})")
        if tensor_score is None:
            raise ValueError("score: tensor_score is required")
        original_score = self._to_score(tensor_score) if tensor_metadata is None else None
        if original_score is not None and hasattr(self.dataset, "transposed_score_and_metadata_tensors"):
            trans_interval = self.dataset.get_transpostion_interval_from_semitone(0)
            tensor_score, tensor_metadata = self.dataset.transposed_score_and_metadata_tensors(original_score, trans_interval)
        elif tensor_metadata is None:
            raise ValueError("score: pass tensor_metadata= (the dataset cannot derive it: no tensor_to_score / "
                             "transposed_score_and_metadata_tensors)")
        tensor_score, tensor_metadata = torch.as_tensor(tensor_score), torch.as_tensor(tensor_metadata)
        num_measures = min(16, tensor_score.size(1) // self.measure_seq_len)
        tensor_score = tensor_score[:, :num_measures * self.measure_seq_len]
        tensor_metadata = tensor_metadata[:, :num_measures * self.measure_seq_len]
        n, L = fill.size(0), tensor_score.size(1)
        start_tick = (start_measure - 1) * measure_seq_len
        end_tick = start_tick + num_measures_gen * measure_seq_len
        if start_tick < 0 or end_tick > L:
            raise ValueError(f"score: measures {start_measure} .. {start_measure + num_measures_gen - 1} lie outside the score's {L} ticks")
        allowed = self._allowed(tensor_score, start_tick, end_tick, measure_seq_len, banned_tokens, None, False)
        own = tensor_score[0].cpu().long()
        outside = torch.ones(L, dtype=torch.bool)
        outside[start_tick:end_tick] = False
        if bool(((own < 0) | (own >= V))[outside].any()):
            raise ValueError(f"score: the score has tokens outside [0, {V}) outside the window")
        forced = own.unsqueeze(0).repeat(n, 1)
        forced[:, start_tick:end_tick] = fill.reshape(n, -1)
        tensor_score = to_cuda_variable_long(tensor_score)
        tensor_metadata = to_cuda_variable_long(tensor_metadata)
        self.last_logp = self.last_tick_logp = None
        self.model.generate(tensor_score=tensor_score[:1].unsqueeze(0).expand(n, 1, L).contiguous(),
                            tensor_metadata=tensor_metadata[:1].unsqueeze(0).expand(n, 1, L, -1).contiguous(),
                            constraints_location=self._window_location(tensor_score, start_tick, end_tick)[:1].unsqueeze(0)
                            .expand(n, 1, L).contiguous(),
                            temperature=temperature, top_k=top_k, top_p=top_p, keep_weights=True, forced=forced,
                            uniforms=np.zeros((n, L), dtype=np.float64),
                            **({} if allowed is None else {"allowed": allowed.unsqueeze(0).expand(n, -1, -1)}))
        self.last_tick_logp = self.model.last_logp[:, 0, start_tick:end_tick].reshape(n, num_measures_gen, measure_seq_len)
        return self.last_tick_logp.sum(-1)

    @staticmethod
    def _window_location(tensor_score, start_tick, end_tick):
        """1 = constrained tick, 0 = to be generated: the window [start_tick, end_tick) of generation()"""
        constraints_location = torch.zeros_like(tensor_score)
        if start_tick > 0:
            constraints_location[:, :start_tick] = 1
        if end_tick < constraints_location.size(1) - 1:
            constraints_location[:, end_tick:] = 1
        return constraints_location

    def _allowed(self, tensor_score, start_tick, end_tick, measure_seq_len, banned_tokens, fixed_tokens, clamp_context):
        """generation()'s constraints as one row of generate()'s mask: bool (L, V) on the host, or None without constraints.  The bans
        and the fixed tokens act on the window [start_tick, end_tick); clamp_context fixes every tick outside it to the score's token."""
        if banned_tokens is None and fixed_tokens is None and not clamp_context:
            return None
        V, L, W = int(self.model.num_notes_per_voice[0]), int(tensor_score.shape[1]), end_tick - start_tick
        allow = torch.ones(L, V, dtype=torch.bool)
        if banned_tokens is not None:
            banned = [int(b) for b in banned_tokens]
            if any(b != b0 for b, b0 in zip(banned, banned_tokens)) or any(not 0 <= b < V for b in banned):
                raise ValueError(f"banned_tokens {list(banned_tokens)!r}: token indices in [0, {V})")
            if len(set(banned)) == V:
                raise ValueError("banned_tokens bans the whole vocabulary")
            allow[start_tick:end_tick, banned] = False
        if fixed_tokens is not None:
            fixed = _fixed_ticks(fixed_tokens, W, measure_seq_len, V)
            one = torch.zeros(W, V, dtype=torch.bool)
            one.scatter_(1, fixed.clamp(min=0).unsqueeze(-1), True)
            allow[start_tick:end_tick] = torch.where((fixed >= 0).unsqueeze(-1), one, allow[start_tick:end_tick])
        if clamp_context:
            own = torch.as_tensor(tensor_score)[0].cpu().long()
            outside = torch.ones(L, dtype=torch.bool)
            outside[start_tick:end_tick] = False
            if bool(((own < 0) | (own >= V))[outside].any()):
                raise ValueError(f"clamp_context: the score has tokens outside [0, {V}) outside the window")
            one = torch.zeros(L, V, dtype=torch.bool)
            one.scatter_(1, own.clamp(0, V - 1).unsqueeze(-1), True)
            allow = torch.where(outside.unsqueeze(-1), one, allow)
        return allow

    def _generate_window(self, tensor_score, tensor_metadata, start_measure, num_measures_gen, temperature=1.5, num_variations=1,
                         top_k=None, top_p=None, banned_tokens=None, fixed_tokens=None, clamp_context=False, score_fixed=False):
        num_variations = _num_variations(num_variations)
        self.last_logp = None
        measure_seq_len = self.dataset.subdivision * self.dataset.num_beats_per_bar
        start_tick = (start_measure - 1) * measure_seq_len
        end_tick = start_tick + num_measures_gen * measure_seq_len
        forced = None
        if score_fixed and fixed_tokens is not None:
            # the fixed ticks as forced ticks under a mask of all ones: the bans and the clamp alone make the mask
            V, L = int(self.model.num_notes_per_voice[0]), int(tensor_score.shape[1])
            fixed = _fixed_ticks(fixed_tokens, end_tick - start_tick, measure_seq_len, V)
            allowed = self._allowed(tensor_score, start_tick, end_tick, measure_seq_len, banned_tokens, None, clamp_context)
            forced = torch.full((L,), -1, dtype=torch.int64)
            forced[start_tick:end_tick] = fixed
            if allowed is not None:
                allowed[forced >= 0] = True
        else:
            allowed = self._allowed(tensor_score, start_tick, end_tick, measure_seq_len, banned_tokens, fixed_tokens, clamp_context)   # (the argument errors first)
        constraints_location = torch.zeros_like(tensor_score)
        if start_tick > 0:
            constraints_location[:, :start_tick] = 1
        if end_tick < constraints_location.size(1) - 1:
            constraints_location[:, end_tick:] = 1
        tensor_past = tensor_score[:, :start_tick]
        tensor_future = tensor_score[:, end_tick:]
        tensor_target = tensor_score[:, start_tick:end_tick]
        original_tensor = torch.cat((tensor_past, tensor_target, tensor_future), 1)
        if num_variations == 1 and top_k is None and top_p is None and allowed is None and forced is None:
            _, gen_target, _ = self.model.generate(tensor_score=tensor_score, tensor_metadata=tensor_metadata,
                                                   constraints_location=constraints_location, temperature=temperature)
            gen_target = gen_target[:, start_tick:end_tick]
            gen_score_tensor = torch.cat((tensor_past, gen_target, tensor_future), 1)
            return self._to_score(gen_score_tensor), gen_score_tensor, self._to_score(original_tensor)
        # the one row as num_variations rows of ONE batched call: (B, 1, L), (B, 1, L, M), (B, 1, L)
        n, L = num_variations, tensor_score.size(1)
        _, gen, _ = self.model.generate(tensor_score=tensor_score[:1].unsqueeze(0).expand(n, 1, L).contiguous(),
                                        tensor_metadata=tensor_metadata[:1].unsqueeze(0).expand(n, 1, L, -1).contiguous(),
                                        constraints_location=constraints_location[:1].unsqueeze(0).expand(n, 1, L).contiguous(),
                                        temperature=temperature, top_k=top_k, top_p=top_p,
                                        **({} if allowed is None else {"allowed": allowed.unsqueeze(0).expand(n, -1, -1)}),
                                        **({} if forced is None else {"forced": forced.unsqueeze(0).expand(n, -1)}))
        gen_target = gen[:, 0, start_tick:end_tick].to(tensor_score.dtype)
        gen_score_tensor = torch.cat((tensor_past.expand(n, -1), gen_target, tensor_future.expand(n, -1)), 1)
        if self.model.last_logp is not None:
            self.last_logp = self.model.last_logp[:, 0, start_tick:end_tick].reshape(n, num_measures_gen, measure_seq_len).sum(-1)
        scores = [self._to_score(row[None]) for row in gen_score_tensor]
        return (scores[0] if n == 1 else scores) if scores[0] is not None else None, gen_score_tensor, self._to_score(original_tensor)

    def process_batch_data(self, batch):
        """(score, metadata) -> device tensors, the default constraint window (measures 8 and 9), start / end tick (:245-260)."""
        tensor_score, tensor_metadata = batch
        tensor_score = to_cuda_variable_long(tensor_score)
        tensor_metadata = to_cuda_variable_long(tensor_metadata)
        constraints_location, start_tick, end_tick = self.get_constraints_location(tensor_score, is_stochastic=False)
        return tensor_score, tensor_metadata, constraints_location, start_tick, end_tick

    def get_constraints_location(self, tensor_score, is_stochastic, start_measure=None, num_measures=None):
        """1 = constrained tick, 0 = to be generated (:262-316).  The stochastic branch draws the window from torch's global
        generator (5+ measures of past and of future, 2+ to generate).  As in the reference, start_tick = start_measure * 24
        here, while generation() puts its window at (start_measure - 1) * 24."""
        constraints_location = torch.zeros_like(tensor_score)
        measure_seq_len = self.dataset.subdivision * self.dataset.num_beats_per_bar
        if is_stochastic:
            min_num_measures_past = min_num_measures_future = 5
            min_num_measures_target = 2
            num_measures = int(tensor_score.size(2) / measure_seq_len)
            assert num_measures == self.dataset.n_bars
            num_target = int(torch.randint(low=min_num_measures_target,
                                           high=num_measures - min_num_measures_past - min_num_measures_future, size=(1,)).item())
            num_past = int(torch.randint(low=min_num_measures_past, high=num_measures - num_target - min_num_measures_future,
                                         size=(1,)).item())
            assert num_measures - num_past - num_target >= min_num_measures_future
            start_measure = num_past + 1
            num_measures = num_target
        else:
            if start_measure is None:
                start_measure = 8
            if num_measures is None:
                num_measures = 2
        start_tick = start_measure * measure_seq_len
        end_tick = start_tick + num_measures * measure_seq_len
        if start_tick > 0:
            constraints_location[:, :, :start_tick] = 1
        if end_tick < constraints_location.size(2) - 1:
            constraints_location[:, :, end_tick:] = 1
        return constraints_location, start_tick, end_tick

    @staticmethod
    def mean_crossentropy_loss(weights, targets):
        """Mean over voices of nn.CrossEntropyLoss (mean) of weights[i] (B, T, V) against targets[i] (B, T) (:318-336)."""
        return AnticipationRNNGaussianRegTrainer.mean_crossentropy_loss_and_accuracy_voices(weights, targets)[0]

    @staticmethod
    def mean_accuracy(weights, targets):
        """Mean over voices of the fraction of ticks whose argmax is the target (:338-356)."""
        return AnticipationRNNGaussianRegTrainer.mean_crossentropy_loss_and_accuracy_voices(weights, targets)[1]

