"""Inference surface of the MeasureVAE: latent interpolation (MeasureVAE/vae_tester.py:17-160 of the reference).

decode_mid_point decodes z1, n evenly spaced points between z1 and z2, and z2 with the free-running decoder (eval mode,
argmax) -- n + 2 small-batch decodes, here ONE decoder call of batch n + 2 (the rows are independent).  Score rendering
(music21) stays outside the hot path.
"""
import os

import torch

from . import ops
from .attributes import ATTRIBUTES, AttributeSpec
from .helpers import to_cuda_variable_long
from .trainer import Trainer, class_report_from_counts, class_stats_add, index_to_note_names


class VAETester(object):
    def __init__(self, dataset, model):
        self.dataset = dataset
        self.model = model
        self.model.eval()
        if self.model.flat.is_cuda:
            ops.preload()                            # no generation call pays a kernel's first launch (csrc/preload.hip)
        self.filepath = os.path.join('models/', self.model.__repr__())
        self.decoder = self.model.decoder
        self.train = False
        self.z_dim = self.decoder.z_dim
        self.batch_size = 1
        self.measure_seq_len = 24

    def decode_mid_point(self, z1, z2, n):
        """z1, z2 (1, z_dim) -> token tensor (1, (n + 2) * 24): z1 | n interpolated | z2   (vae_tester.py:72-93)"""
        assert n >= 1 and isinstance(n, int)
        # z1 and z2 themselves are decoded at the ends (vae_tester.py:82-91), not z1 + (z2 - z1) * 1.0, which is not
        # bit-equal to z2 in fp32 and could flip a near-tie argmax of the last measure
        ks = torch.arange(1, n + 1, device=z1.device, dtype=z1.dtype).view(-1, 1)
        z = torch.cat((z1, z1 + (z2 - z1) * ks / (n + 1), z2), 0)      # same operation order as the reference's loop
        dummy = torch.zeros(n + 2, self.measure_seq_len, device=z1.device)
        with torch.no_grad():
            _, samples = self.decoder(z.contiguous(), dummy, self.train)
        torch.cuda.synchronize()
        ops.check_chains("VAETester.decode_mid_point")             # never hand back tokens of a failed persistent launch
        return samples.reshape(1, -1)

    def test_interpolation(self, tensor_score1, tensor_score2, n=1):
        """(1, 24) x 2 -> interpolation through the encoder means (vae_tester.py:95-111); returns the token tensor
        (and the rendered score when the dataset can render)."""
        with torch.no_grad():
            z1 = self.model.encoder(tensor_score1).loc
            z2 = self.model.encoder(tensor_score2).loc
        tensor_score = self.decode_mid_point(z1, z2, n)
        fn = getattr(self.dataset, "tensor_to_score", None)
        return (fn(tensor_score.cpu()) if fn is not None else None), tensor_score

    def kl_per_dim(self, data_loader):
        """(Z,) float64 on the device: the mean over all measures of the loader of KL[., d] = 0.5(sigma^2 + mu^2 - 1) - log sigma, the
        plain KL of the encoder's posterior against N(0, 1) per latent dimension -- which dimensions the model uses (DESIGN.md section
        22).  The column sums come from the 'dim' forward kernel with free_nats = 0, accumulated over the batches in float64."""
        total, count = None, 0
        n_bars = getattr(self.dataset, "n_bars", None)
        for score_tensor, _ in data_loader:
            if n_bars is not None and score_tensor.dim() == 3:
                score_tensor = score_tensor.reshape(score_tensor.size(0) * n_bars, -1)
            score = to_cuda_variable_long(score_tensor)
            with torch.no_grad():
                z_dist = self.model.encoder(score)
                parts = ops.reparam_kl_fb(z_dist.loc.contiguous(), z_dist.log_scale.contiguous(), None, 0.0, 'dim', want_z=False)[1]
            total = parts.double() if total is None else total + parts.double()
            count += int(score.shape[0])
            ops.check_chains("VAETester.kl_per_dim")
        if total is None:
            raise ValueError("kl_per_dim: the loader is empty")
        return total / count

    def active_units(self, data_loader, threshold=0.01):
        """How many latent dimensions carry more than `threshold` nats of KL per measure on average (Burda et al. 2016 count active
        units by a threshold of 0.01 on a posterior statistic; this is the KL form of that count)."""
        return int((self.kl_per_dim(data_loader) > threshold).sum())

    def mmd(self, data_loader, kernel='gaussian', bandwidth=None, estimator='unbiased', generator=None):
        """The mean over the loader's batches of the MMD (ops.mmd, DESIGN.md section 25: coeff = 1) between a draw rsample() of the
        encoder's posterior for every measure of the batch and as many draws of the prior N(0, 1) -- whether the AGGREGATE posterior
        matches the prior, which the per-measure KL of kl_per_dim / active_units cannot say.  bandwidth None: 2 * z_dim.  A 0-dim
        float64 tensor on the device.  generator: the device torch.Generator of the 2 B Z normal draws per batch (eps first, then
        the prior's), None: the default one.  Only the value launches run."""
        total, count = None, 0
        n_bars = getattr(self.dataset, "n_bars", None)
        for score_tensor, _ in data_loader:
            if n_bars is not None and score_tensor.dim() == 3:
                score_tensor = score_tensor.reshape(score_tensor.size(0) * n_bars, -1)
            score = to_cuda_variable_long(score_tensor)
            with torch.no_grad():
                z_dist = self.model.encoder(score)
                draws = torch.randn((2,) + tuple(z_dist.loc.shape), dtype=z_dist.loc.dtype, device=z_dist.loc.device,
                                    generator=generator)
                z = z_dist.rsample(eps=draws[0])
                value = ops.mmd(z.contiguous(), draws[1], kernel, bandwidth, estimator)[0][0].double()
            total = value if total is None else total + value
            count += 1
            ops.check_chains("VAETester.mmd")
        if total is None:
            raise ValueError("mmd: the loader is empty")
        return total / count

    LL_COLUMNS = ops.IW_COLUMNS                      # ('iwae', 'elbo', 'ess', 'rec', 'kl')

    def measure_log_likelihood(self, score_tensor, num_samples=64, eps=None, generator=None, max_rows=4096):
        """score_tensor (N, 24) -> float64 (N, 5) on the device, the columns LL_COLUMNS per measure: iwae, the
        importance-weighted bound on log p(x) from num_samples draws of the encoder's posterior (Burda et al. 2016; tight as
        num_samples grows); elbo, the single-sample bound averaged over the same draws; ess, the effective sample size in [1,
        num_samples]; rec and kl, the Monte-Carlo reconstruction and KL terms, rec + kl = -elbo.  In nats per measure; comparable
        between models whatever beta, floor or MMD term they were trained with.  eps / generator / max_rows: MeasureVAE.log_weights."""
        score = to_cuda_variable_long(score_tensor)
        logw, nll = self.model.log_weights(score, num_samples, eps=eps, generator=generator, max_rows=max_rows)
        return ops.iw_finish(logw, nll)

    def log_likelihood(self, data_loader, num_samples=64, generator=None, max_rows=4096):
        """The means over all measures of the loader of measure_log_likelihood's columns: {iwae, elbo, ess, rec, kl, measures,
        nats_per_tick}, nats_per_tick = -iwae / 24.  Accumulated in float64 on the device, read once at the end."""
        total, count = None, 0
        n_bars = getattr(self.dataset, "n_bars", None)
        for score_tensor, _ in data_loader:
            if n_bars is not None and score_tensor.dim() == 3:
                score_tensor = score_tensor.reshape(score_tensor.size(0) * n_bars, -1)
            cols = self.measure_log_likelihood(score_tensor, num_samples, generator=generator, max_rows=max_rows).sum(0)
            total = cols if total is None else total + cols
            count += int(score_tensor.shape[0])
        if total is None:
            raise ValueError("log_likelihood: the loader is empty")
        means = (total / count).tolist()
        out = dict(zip(self.LL_COLUMNS, means))
        out["measures"] = count
        out["nats_per_tick"] = -out["iwae"] / self.measure_seq_len
        return out

    ATTRIBUTES = ATTRIBUTES                          # ('num_notes', 'note_range', 'rhy_entropy', 'beat_strength')

    def _spec(self, spec):
        if spec is None:
            if getattr(self, "_attr_spec", None) is None:
                self._attr_spec = AttributeSpec.from_dataset(self.dataset)
            spec = self._attr_spec
        return spec

    def measure_attributes(self, score_tensor, spec=None):
        """score_tensor (B, 24) -> float32 (B, 4) on the device, the columns ATTRIBUTES of every measure (ops.measure_attributes,
        DESIGN.md section 27).  spec None: AttributeSpec.from_dataset(self.dataset)."""
        return ops.measure_attributes(to_cuda_variable_long(score_tensor).contiguous(), self._spec(spec))

    def attribute_concordance(self, data_loader, dims=None, spec=None):
        """float64 (Z or len(dims), 4) on the device: for latent dimension d (dims None: all of them) and attribute k, (concordant -
        discordant) / (concordant + discordant) over the ordered pairs i != j of measures WITHIN each batch of the loader whose
        attributes differ -- concordant where the posterior mean's dimension d orders the pair as the attribute does.  +1: the
        dimension sorts the measures by the attribute; 0: it knows nothing of it; NaN where no pair differs.  The number that says
        whether the regularisation took.  The counts come from ops.attr_reg's value launches, 8 dimensions a
        call, and are accumulated over the batches as integers."""
        spec = self._spec(spec)
        Z = self.z_dim
        dims = list(range(Z)) if dims is None else list(dims)
        if not dims:
            raise ValueError("attribute_concordance: no dimensions")
        for i0 in range(0, len(dims), ops.ATTR_MAX_DIMS):
            ops.attr_dims(dims[i0:i0 + ops.ATTR_MAX_DIMS], Z)
        total = None
        n_bars = getattr(self.dataset, "n_bars", None)
        for score_tensor, _ in data_loader:
            if n_bars is not None and score_tensor.dim() == 3:
                score_tensor = score_tensor.reshape(score_tensor.size(0) * n_bars, -1)
            score = to_cuda_variable_long(score_tensor).contiguous()
            with torch.no_grad():
                loc = self.model.encoder(score).loc.contiguous()
                attrs = ops.measure_attributes(score, spec)
                counts = torch.empty(len(dims), len(ATTRIBUTES), 3, dtype=torch.int64, device=loc.device)
                for k in range(len(ATTRIBUTES)):
                    for i0 in range(0, len(dims), ops.ATTR_MAX_DIMS):
                        chunk = dims[i0:i0 + ops.ATTR_MAX_DIMS]
                        counts[i0:i0 + len(chunk), k] = ops.attr_reg(loc, chunk, attrs[:, k:k + 1].expand(-1, len(chunk)).contiguous())[1]
            total = counts if total is None else total + counts
            ops.check_chains("VAETester.attribute_concordance")
        if total is None:
            raise ValueError("attribute_concordance: the loader is empty")
        c, d = total[..., 0].double(), total[..., 1].double()
        return (c - d) / (c + d)

    def attribute_sweep(self, score_tensor, dim, values, spec=None):
        """Encodes score_tensor (B, 24), sets the posterior mean's dimension `dim` to each of `values` in turn and decodes by argmax
        (eval mode, the free-running decoder: ONE decoder call of batch len(values) * B) -> (attrs, tokens): the decoded measures'
        attributes float32 (len(values), B, 4) and their tokens int64 (len(values), B, 24).  On a model trained with attr_reg the
        attribute tied to `dim` rises along `values`."""
        spec = self._spec(spec)
        values = [float(v) for v in values]
        if isinstance(dim, bool) or not isinstance(dim, int) or not 0 <= dim < self.z_dim:
            raise ValueError(f"attribute_sweep: dim must be an int in [0, {self.z_dim}), got {dim!r}")
        if not values:
            raise ValueError("attribute_sweep: no values")
        score = to_cuda_variable_long(score_tensor).contiguous()
        B, T = score.shape
        with torch.no_grad():
            loc = self.model.encoder(score).loc
            z = loc.unsqueeze(0).repeat(len(values), 1, 1)
            z[:, :, dim] = torch.tensor(values, dtype=z.dtype, device=z.device).view(-1, 1)
            dummy = torch.zeros(len(values) * B, T, device=z.device)
            _, samples = self.decoder(z.reshape(len(values) * B, -1).contiguous(), dummy, self.train)
        torch.cuda.synchronize()
        ops.check_chains("VAETester.attribute_sweep")               # never hand back tokens of a failed persistent launch
        tokens = samples.reshape(len(values) * B, T).long().contiguous()
        attrs = ops.measure_attributes(tokens, spec)
        return attrs.view(len(values), B, len(ATTRIBUTES)), tokens.view(len(values), B, T)

    def class_report(self, data_loader):
        """How well the model reconstructs each token, as opposed to the hold that fills most ticks: the eval-mode forward of
        loss_and_acc_test over a loader, its per-class statistics and confusion matrix accumulated on the device (DESIGN.md
        section 28), read once at the end.  -> dict: counts, predicted, hits (V,) int64; recall, precision, f1 (V,) float64, NaN
        where undefined; accuracy; balanced_accuracy, the mean recall over the classes present; confusion (V, V) int64 indexed
        [target, argmax]; names, the dataset's index-to-note table or None."""
        V = self.model.num_notes
        dev = self.model.flat.device
        stats = torch.zeros(V, 3, dtype=torch.int64, device=dev)
        conf = torch.zeros(V, V, dtype=torch.int64, device=dev)
        n_bars = getattr(self.dataset, "n_bars", None)
        for score_tensor, _ in data_loader:
            if n_bars is not None and score_tensor.dim() == 3:
                score_tensor = score_tensor.reshape(score_tensor.size(0) * n_bars, -1)
            score = to_cuda_variable_long(score_tensor)
            with torch.no_grad():
                class_stats_add(self.model(measure_score_tensor=score, train=False)[0], score, stats, conf)
            ops.check_chains("VAETester.class_report")
        return class_report_from_counts(stats, conf, index_to_note_names(self.dataset, V))

    def loss_and_acc_test(self, data_loader):
        """vae_tester.py:113-160: mean reconstruction CE / accuracy over a loader (eval mode, no teacher forcing)."""
        tot = torch.zeros(3)
        n_bars = getattr(self.dataset, "n_bars", None)
        for score_tensor, _ in data_loader:
            if n_bars is not None and score_tensor.dim() == 3:
                score_tensor = score_tensor.reshape(score_tensor.size(0) * n_bars, -1)
            score = to_cuda_variable_long(score_tensor)
            with torch.no_grad():
                weights = self.model(measure_score_tensor=score, train=False)[0]
                loss, acc = Trainer.mean_crossentropy_loss_and_accuracy(weights, score)
            tot += torch.tensor([float(loss), float(acc), 1.0])
            ops.check_chains("VAETester.loss_and_acc_test")
        n = max(float(tot[2]), 1.0)
        return float(tot[0]) / n, float(tot[1]) / n
