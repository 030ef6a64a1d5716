"""Inference surface of the LatentRNN: B = 1 inpainting (LatentRNN/latent_rnn_tester.py:13-300 of the reference).

`generate` fills `num_target_measures` measures between a past and a future context with the model's free-running path
(train=False: no teacher forcing, no dropout) and returns the full token tensor past | generated | future.  The
tensor -> music21 score conversion of the reference (dataset.tensor_to_score) is outside the hot path: it is called when
the dataset offers it, otherwise the score slots of the return tuple are None.  The reference's call omits the `target`
argument of LatentRNN.forward (latent_rnn_tester.py:231-236, a TypeError as written); here forward() accepts
target=None.
"""
import math
import os

import torch

from . import ops
from .helpers import to_cuda_variable_long
from .trainer import Trainer, class_report_from_counts, class_stats_add, index_to_note_names


class LatentRNNTester(object):
    def __init__(self, dataset, model):
        self.dataset = dataset
        self.model = model
        self.model.eval()
        if self.model.flat.is_cuda:
            ops.preload()                            # no generation call pays a kernel's first launch (csrc/preload.hip)
        self.filepath = os.path.join('models/', self.model.__repr__())
        self.min_num_measures_target = 1
        self.max_num_measure_target = 4
        assert self.dataset.n_bars > self.max_num_measure_target >= self.min_num_measures_target
        self.measure_seq_len = self.dataset.subdivision * self.dataset.num_beats_per_bar
        self.batch_size = 1

    def _to_score(self, tensor):
        fn = getattr(self.dataset, "tensor_to_score", None)
        return fn(tensor.cpu()) if fn is not None else None

    def generate(self, tensor_past, tensor_future, tensor_target, num_target_measures, eval=False, temperature=None,
                 num_variations=1, top_k=None, top_p=None, banned_tokens=None, fixed_tokens=None, score_fixed=False):
        """-> (gen_score | None, gen_score_tensor (B, n_past + n_target + n_future, 24), original_score | None)
        (latent_rnn_tester.py:197-266)
        temperature (a finite float): `num_variations` fillings of the same gap -- the (one-row) contexts are expanded to that many
        rows, every row's tokens are drawn from softmax(temperature * weights) with its own uniforms (one
        np.random.random_sample((num_variations, n_target, 24)) call: np.random.seed reproduces a call) and gen_score_tensor has
        num_variations rows.  Up to sixteen decoder rows (variations x target measures on the non-auto-regressive path) are one
        register-resident launch.  temperature None: one filling by the argmax, as before.
        top_k / top_p (with a temperature only: ValueError without; top_p in (0, 1]): every token is drawn behind top-k / nucleus
        truncation (HierarchicalDecoder.forward) -- the remedy for the mass the many zero logits of a post-ReLU head carry.  Such a call
        leaves self.last_logp (num_variations, n_target): per generated measure the sum of its 24 drawn tokens' log-probabilities
        under the truncated distribution, NaN where a tick fell back to the argmax -- the score to rank the variations by (top_p=1.0
        scores them without truncating); every other call leaves it None.  The return tuple is the same.
        banned_tokens (a list of token indices): never returned at any generated tick -- START, END or a padding symbol in the middle
        of a piece.  fixed_tokens (an int tensor (n_target, 24), -1 = a free tick): the notes to keep; applied to every variation, and a
        fixed tick wins over a ban.  Both are applied inside the decode launch (HierarchicalDecoder.forward's `allowed`), so the notes
        behind a constrained tick are generated from it.  ValueError for an index outside [0, V) (fixed: other than -1) or a ban of
        the whole vocabulary.  With a temperature last_logp is as above (a fixed tick adds exactly 0); without one the single filling
        is the argmax over the allowed tokens and last_logp stays None.
        score_fixed=True (needs a temperature: ValueError without): the fixed ticks become FORCED ticks with an all-ones mask
        (HierarchicalDecoder.forward's `forced`) -- a fixed tick still wins over a ban -- and last_logp then
        includes what the model thinks of the kept notes instead of 0 for each of them.  The default is the behaviour above."""
        if score_fixed and temperature is None:
            raise ValueError("score_fixed needs a temperature")
        if temperature is None and (top_k is not None or top_p is not None):
            raise ValueError("top_k / top_p need a temperature")
        if top_p is not None and not (0.0 < float(top_p) <= 1.0):
            raise ValueError(f"top_p {top_p!r} outside (0, 1]")
        ops._top_k(top_k)                                          # (ValueError for a top_k that is no integer)
        if tensor_target is not None:
            if num_target_measures is not None:
                assert num_target_measures == tensor_target.size(1)
            num_target_measures = tensor_target.size(1)
        elif num_target_measures is None:
            raise ValueError
        allowed = self._allowed(banned_tokens, fixed_tokens, num_target_measures)      # (the argument errors, before any work)
        forced = None
        if score_fixed and fixed_tokens is not None:
            forced = torch.as_tensor(fixed_tokens).cpu().long()                        # (checked by _allowed above)
            allowed = self._allowed(banned_tokens, None, num_target_measures)
            if allowed is not None:                                                    # a fixed tick wins over a ban: its mask is all ones
                allowed = allowed | (forced >= 0).unsqueeze(-1)
        if tensor_past is None:
            tensor_past = self.create_empty_context('start')
        if tensor_future is None:
            tensor_future = self.create_empty_context('end')
        if temperature is None:
            if num_variations != 1:
                raise ValueError("several variations need a temperature: the argmax has one answer per latent")
        else:
            if num_variations < 1:
                raise ValueError("num_variations must be at least 1")
            if tensor_past.size(0) != 1 or tensor_future.size(0) != 1:
                raise ValueError("variations are drawn for one context (batch size 1)")
            tensor_past = tensor_past.expand(num_variations, -1, -1).contiguous()
            tensor_future = tensor_future.expand(num_variations, -1, -1).contiguous()
            if tensor_target is not None:
                tensor_target = tensor_target.expand(num_variations, -1, -1).contiguous()
        if allowed is not None:                                     # every row -- every variation -- under the same constraints
            allowed = allowed.unsqueeze(0).expand(tensor_past.size(0), -1, -1, -1).contiguous()
        extra = {} if allowed is None else {"allowed": allowed}
        if forced is not None:
            extra["forced"] = forced.unsqueeze(0).expand(tensor_past.size(0), -1, -1).contiguous()
        with torch.no_grad():
            weights, gen_target, _ = self.model(past_context=tensor_past, future_context=tensor_future, target=None,
                                                measures_to_generate=num_target_measures, train=False, temperature=temperature,
                                                top_k=top_k, top_p=top_p, **extra)
        self.last_weights = weights
        lp = getattr(self.model, "last_logp", None)
        self.last_logp = lp.sum(-1) if lp is not None else None
        torch.cuda.synchronize()
        ops.check_chains("LatentRNNTester.generate")                   # persistent kernels: never hand back results of a failed launch
        if tensor_target is not None and eval:
            loss, accuracy = Trainer.mean_crossentropy_loss_and_accuracy(weights, tensor_target)
            self.last_eval = (float(loss), float(accuracy))
            print('Accuracy for Test Case:')
            print(f'\tLoss: {self.last_eval[0]}\tAccuracy: {self.last_eval[1] * 100} %')
        batch_size = gen_target.size(0)
        gen_target = gen_target.view(batch_size, num_target_measures, self.measure_seq_len)
        gen_score_tensor = torch.cat((tensor_past, gen_target, tensor_future), 1)
        original = None
        if tensor_target is not None:
            original = self._to_score(torch.cat((tensor_past, tensor_target, tensor_future), 1))
        return self._to_score(gen_score_tensor), gen_score_tensor, original

    def score(self, tensor_past, tensor_future, fillings, temperature=1.0, top_k=None, top_p=None, banned_tokens=None):
        """What the model thinks of given fillings of one gap -> (N, n_target): per measure the sum of its 24 tokens' log-probabilities
        under softmax(temperature * weights) behind the same ban and top-k / nucleus truncation a generate() call with these
        arguments draws from.  fillings: an int tensor (N, n_target, 24) of token indices in [0, V) -- the
        user's own filling, the original measures, another model's, or generate()'s own gen_score_tensor slice -- for ONE context
        (tensor_past / tensor_future of batch size 1, None: the empty contexts of generate()), which is expanded to N rows as generate
        expands it for variations.  Every tick is forced: the tokens are fed back one by one inside the decode launch (up to
        sixteen decoder rows are one register-resident launch), the uniforms are zeros and np.random is not touched.  -inf (a banned or
        truncated token) and NaN (a tick outside the rule) propagate into the sums.  Scoring generate()'s fillings with its
        temperature, top_k, top_p and bans returns its last_logp bit for bit.  Leaves self.last_tick_logp (N, n_target, 24) and
        self.last_weights (N, n_target, 24, V)."""
        if temperature is None or not math.isfinite(float(temperature)):
            raise ValueError(f"score: temperature {temperature!r} must be a finite float")
        if top_p is not None and not (0.0 < float(top_p) <= 1.0):
            raise ValueError(f"top_p {top_p!r} outside (0, 1]")
        ops._top_k(top_k)                                          # (ValueError for a top_k that is no integer)
        V, L = int(self.model.vae_model.decoder.cfg.num_notes), self.measure_seq_len
        fillings = torch.as_tensor(fillings)
        if fillings.is_floating_point() or fillings.is_complex() or fillings.dtype == torch.bool or fillings.dim() != 3 or \
                fillings.size(0) < 1 or fillings.size(1) < 1 or fillings.size(2) != L:
            raise ValueError(f"fillings must be an int tensor of shape (N, n_target, {L}), got {fillings.dtype} {tuple(fillings.shape)}")
        fillings = fillings.cpu().long()
        if bool(((fillings < 0) | (fillings >= V)).any()):
            raise ValueError(f"fillings: token indices in [0, {V})")
        n, n_target = fillings.size(0), fillings.size(1)
        allowed = self._allowed(banned_tokens, None, n_target)
        if tensor_past is None:
            tensor_past = self.create_empty_context('start')
        if tensor_future is None:
            tensor_future = self.create_empty_context('end')
        if tensor_past.size(0) != 1 or tensor_future.size(0) != 1:
            raise ValueError("fillings are scored for one context (batch size 1)")
        tensor_past = tensor_past.expand(n, -1, -1).contiguous()
        tensor_future = tensor_future.expand(n, -1, -1).contiguous()
        extra = {} if allowed is None else {"allowed": allowed.unsqueeze(0).expand(n, -1, -1, -1).contiguous()}
        with torch.no_grad():
            weights, _, _ = self.model(past_context=tensor_past, future_context=tensor_future, target=None,
                                       measures_to_generate=n_target, train=False, temperature=float(temperature),
                                       uniforms=torch.zeros(n, n_target, L, dtype=torch.float64), top_k=top_k, top_p=top_p,
                                       forced=fillings, **extra)
        self.last_weights = weights
        self.last_tick_logp = self.model.last_logp
        torch.cuda.synchronize()
        ops.check_chains("LatentRNNTester.score")                      # persistent kernels: never hand back results of a failed launch
        return self.last_tick_logp.sum(-1)

    def _allowed(self, banned_tokens, fixed_tokens, n_target):
        """generate()'s constraints as one row of the model's mask: bool (n_target, 24, V) on the host, or None without constraints"""
        if banned_tokens is None and fixed_tokens is None:
            return None
        V, L = int(self.model.vae_model.decoder.cfg.num_notes), self.measure_seq_len
        allow = torch.ones(n_target, L, V, dtype=torch.bool)
        if banned_tokens is not None:
            banned = [int(b) for b in banned_tokens]
            if any(b != b0 for b, b0 in zip(banned, banned_tokens)) or any(not 0 <= b < V for b in banned):
                raise ValueError(f"banned_tokens {list(banned_tokens)!r}: token indices in [0, {V})")
            allow[:, :, banned] = False
            if banned and not bool(allow.any(-1).all()):
                raise ValueError("banned_tokens bans the whole vocabulary")
        if fixed_tokens is not None:
            fixed = torch.as_tensor(fixed_tokens).cpu()
            if fixed.is_floating_point() or fixed.dtype == torch.bool or tuple(fixed.shape) != (n_target, L):
                raise ValueError(f"fixed_tokens must be an int tensor of shape {(n_target, L)}, got {fixed.dtype} {tuple(fixed.shape)}")
            fixed = fixed.long()
            if bool(((fixed < -1) | (fixed >= V)).any()):
                raise ValueError(f"fixed_tokens: token indices in [0, {V}), or -1 for a free tick")
            keep = fixed >= 0
            one = torch.zeros(n_target, L, V, dtype=torch.bool)
            one.scatter_(2, fixed.clamp(min=0).unsqueeze(-1), True)
            allow = torch.where(keep.unsqueeze(-1), one, allow)
        return allow

    def create_empty_context(self, type):
        """(1, num_measures, 24) of one symbol: 3 START measures, 1 END measure or 1 rest measure (:268-296)."""
        notes = self.dataset.note2index_dicts[getattr(self.dataset, "NOTES", 0)]
        if type == 'start':
            num_measures, symbol = 3, notes[getattr(self.dataset, "START_SYMBOL", "START")]
        elif type == 'end':
            num_measures, symbol = 1, notes[getattr(self.dataset, "END_SYMBOL", "END")]
        elif type == 'rest':
            num_measures, symbol = 1, notes['rest']
        else:
            raise ValueError('Invalid argument "type"')
        return to_cuda_variable_long(torch.full((1, num_measures, self.measure_seq_len), int(symbol), dtype=torch.int32))

    def class_report(self, data_loader, fix_num_target=4):
        """The per-class report of VAETester.class_report for inpainting: the eval-mode forward and fixed split of
        loss_and_acc_test, statistics and confusion matrix accumulated on the device over the loader."""
        from .latent_rnn_trainer import LatentRNNTrainer
        stats = conf = None
        for score_tensor, _ in data_loader:
            n_meas = score_tensor.size(-1) // self.measure_seq_len
            n_past = (n_meas - fix_num_target) // 2
            past, future, target = LatentRNNTrainer.split_score(score_tensor, n_past, n_meas - n_past - fix_num_target,
                                                                fix_num_target, self.measure_seq_len)
            with torch.no_grad():
                w, _, _ = self.model(past, future, target, fix_num_target, train=False)
            if stats is None:
                V = w.size(-1)
                stats = torch.zeros(V, 3, dtype=torch.int64, device=w.device)
                conf = torch.zeros(V, V, dtype=torch.int64, device=w.device)
            class_stats_add(w, target, stats, conf)
            ops.check_chains("LatentRNNTester.class_report")
        if stats is None:
            raise ValueError("class_report: the loader is empty")
        return class_report_from_counts(stats, conf, index_to_note_names(self.dataset, stats.shape[0]))

    def loss_and_acc_test(self, data_loader, fix_num_target=4):
        """Mean loss / accuracy of inpainting over a loader, fixed split as the reference's test loop (:298-340)."""
        from .latent_rnn_trainer import LatentRNNTrainer
        tot = torch.zeros(3)
        for score_tensor, _ in data_loader:
            n_meas = score_tensor.size(-1) // self.measure_seq_len
            n_past = (n_meas - fix_num_target) // 2
            past, future, target = LatentRNNTrainer.split_score(score_tensor, n_past, n_meas - n_past - fix_num_target,
                                                                fix_num_target, self.measure_seq_len)
            with torch.no_grad():
                w, _, _ = self.model(past, future, target, fix_num_target, train=False)
                loss, acc = Trainer.mean_crossentropy_loss_and_accuracy(w, target)
            tot += torch.tensor([float(loss), float(acc), 1.0])
            ops.check_chains("LatentRNNTester.loss_and_acc_test")
        n = max(float(tot[2]), 1.0)
        return float(tot[0]) / n, float(tot[1]) / n
