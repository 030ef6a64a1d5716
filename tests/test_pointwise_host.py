"""What can be said about the helper kernels' entry points without a GPU: the statistics and the (seed, offset) contract of the
dropout stream on its numpy mirror (tests/pointwise_ref.py; tests/test_gpu_pointwise.py holds the kernel bit-equal to that mirror),
and the argument checks of the C-ABI, which answer before any launch."""
import ctypes as C

import numpy as np
import pytest

from inpaintnet_amd import _lib
from tests import pointwise_ref as R

N = 1 << 22
PS = [0.0, 0.1, 0.2, 0.5, 0.999]


# ------------------------------------------------------------------------------- the dropout stream
@pytest.mark.parametrize("p", PS)
def test_kept_fraction_follows_p(p):
    """n Bernoulli(1 - p) draws: the kept fraction lies within five sigma of 1 - float32(p), sigma = sqrt(p (1 - p) / n)."""
    p32 = float(np.float32(p))
    m = R.dropout_mask_ref(N, p, 0x5eed, 0)
    kept = m != 0
    assert np.all(m[kept] == R.dropout_keep_value(p))
    sigma = np.sqrt(p32 * (1.0 - p32) / N)
    dev = abs(float(kept.mean()) - (1.0 - p32))
    print(f"p={p}: kept {kept.mean():.6f}, {dev / sigma if sigma else 0.0:.2f} sigma")
    assert dev <= 5.0 * sigma
    if p == 0.0:
        assert kept.all() and np.all(m == np.float32(1.0))


@pytest.mark.parametrize("offset", [0, 12345, (1 << 32) + 7, (1 << 64) - 1000, (1 << 64) - 1])
def test_a_mask_continues_across_offsets(offset):
    """mask(n, off)[k:] == mask(n - k, off + k): `offset` continues one stream, also across the wrap at 2^64."""
    n = 5000
    whole = R.dropout_mask_ref(n, 0.5, 0x5eed, offset)
    for k in (1, 999, 1000, 1001, 4999):
        assert np.array_equal(whole[k:], R.dropout_mask_ref(n - k, 0.5, 0x5eed, offset + k)), (offset, k)
    assert not np.array_equal(whole[1:], whole[:-1])


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_consecutive_call_seeds_give_independent_masks(p):
    """Decoder.forward derives one sampling seed per call from the dropout seed and the call counter (measure_vae.py: seed * golden
    + counter + 1); masks drawn under two consecutive ones agree where two independent Bernoulli(1 - p) draws agree: on
    p^2 + (1 - p)^2 = 1 - 2 p (1 - p) of the elements, within five sigma."""
    p32 = float(np.float32(p))
    T, B = 24, 256
    seeds = [((0x5eed * 0x9E3779B97F4A7C15 + call * T * B + 1) & (2 ** 64 - 1)) or 1 for call in (0, 1)]
    a, b = (R.dropout_mask_ref(N, p, s, 0) for s in seeds)
    agree = float(((a != 0) == (b != 0)).mean())
    want = 1.0 - 2.0 * p32 * (1.0 - p32)
    sigma = np.sqrt(want * (1.0 - want) / N)
    print(f"p={p}: agree {agree:.6f}, want {want:.6f}, {abs(agree - want) / sigma:.2f} sigma")
    assert abs(agree - want) <= 5.0 * sigma


def test_mix64_known_values():
    """The splitmix64 finaliser as published (Steele, Lea, Flood 2014; the first outputs of the generator seeded with 0 and with
    1234567 are printed in many places): a slip in a shift or a constant of the mirror would otherwise be a slip in every mask test."""
    assert int(R.mix64(0)) == 0xE220A8397B1DCDAF
    assert int(R.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    assert int(R.mix64(1234567)) == 6457827717110365317
    assert int(R.mix64((1 << 64) - 1)) == int(R.mix64(-1))


@pytest.mark.parametrize("p", PS)
def test_the_threshold_is_inclusive(p):
    """An element whose hash has a high word EQUAL to the threshold is kept, one below it is dropped: aimed with the inverse hash."""
    thr = R.dropout_threshold(p)
    for h in (0, 1, 0xE220A8397B1DCDAF, (1 << 64) - 1):
        assert int(R.mix64(R.unmix64(h))) == h
    for hi in [thr, thr + 1] + ([thr - 1, 0] if thr > 0 else []):
        off = (R.offset_with_hash(0x5eed, (hi << 32) | 0x9abcdef0) - 1) & (2 ** 64 - 1)
        m = R.dropout_mask_ref(3, p, 0x5eed, off)
        assert (m[1] != 0) == (hi >= thr), (p, hi, thr, m)


def test_the_aimed_uniforms():
    """The counters tests/test_gpu_pointwise.py aims the sampler at: the two with the largest 24-bit uniform and the one with the
    smallest (0) among the first 2^26 counters of seed 1234 (found by running uniform24_ref over all of them)."""
    assert R.uniform24_ref(1234, 22982038) == 0xFFFFFF and R.uniform24_ref(1234, 50007773) == 0xFFFFFF
    assert R.uniform24_ref(1234, 63355030) == 0
    k = R.uniform24_ref(1234, np.arange(1 << 16, dtype=np.uint64))
    assert k.dtype == np.uint32 and int(k.max()) < (1 << 24)


# ------------------------------------------------------------------------------- argument rejection
@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


# A pointer that is never followed: every call below is refused by the checks in front of the launch, and a call that were not
# would fail on it at once instead of reading memory that happens to be mapped.
X = C.c_void_p(16)
NULL = None


def test_entries_reject_null_pointers_and_empty_sizes(L):
    calls = {
        "argmax w": L.inet_argmax(NULL, 4, 1, 4, X, 1, NULL),
        "argmax out": L.inet_argmax(X, 4, 1, 4, NULL, 1, NULL),
        "argmax rows": L.inet_argmax(X, 4, 0, 4, X, 1, NULL),
        "argmax V": L.inet_argmax(X, 4, 1, 0, X, 1, NULL),
        "argmax V<0": L.inet_argmax(X, 4, 1, -3, X, 1, NULL),
        "ce weights": L.inet_cross_entropy(NULL, 4, 1, 4, X, X, 4, 1.0, 1.0, X, X, NULL),
        "ce targets": L.inet_cross_entropy(X, 4, 1, 4, NULL, X, 4, 1.0, 1.0, X, X, NULL),
        "ce loss_sum": L.inet_cross_entropy(X, 4, 1, 4, X, X, 4, 1.0, 1.0, NULL, X, NULL),
        "ce correct": L.inet_cross_entropy(X, 4, 1, 4, X, X, 4, 1.0, 1.0, X, NULL, NULL),
        "ce rows": L.inet_cross_entropy(X, 4, 0, 4, X, X, 4, 1.0, 1.0, X, X, NULL),
        "ce V": L.inet_cross_entropy(X, 4, 1, 0, X, X, 4, 1.0, 1.0, X, X, NULL),
        "ce_ex weights": L.inet_cross_entropy_ex(NULL, 4, 1, 4, X, X, 4, 1.0, NULL, 1.0, X, X, NULL, 0.0, NULL, 0.0, NULL),
        "ce_ex targets": L.inet_cross_entropy_ex(X, 4, 1, 4, NULL, X, 4, 1.0, NULL, 1.0, X, X, NULL, 0.0, NULL, 0.0, NULL),
        "ce_ex rows": L.inet_cross_entropy_ex(X, 4, -1, 4, X, X, 4, 1.0, NULL, 1.0, X, X, NULL, 0.0, NULL, 0.0, NULL),
        "ce_ex V": L.inet_cross_entropy_ex(X, 4, 1, 0, X, X, 4, 1.0, NULL, 1.0, X, X, NULL, 0.0, NULL, 0.0, NULL),
        "ce_ex no output": L.inet_cross_entropy_ex(X, 4, 1, 4, X, NULL, 4, 1.0, NULL, 1.0, NULL, NULL, NULL, 0.0, NULL, 0.0, NULL),
        "ce_ex fwd_out without scale_dev": L.inet_cross_entropy_ex(X, 4, 1, 4, X, X, 4, 1.0, NULL, 1.0, X, X, NULL, 0.0, X, 1.0, NULL),
        "sample weights": L.inet_sample_multinomial(NULL, 4, 1, 4, X, 1, 1, 0, NULL),
        "sample out": L.inet_sample_multinomial(X, 4, 1, 4, NULL, 1, 1, 0, NULL),
        "sample rows": L.inet_sample_multinomial(X, 4, 0, 4, X, 1, 1, 0, NULL),
        "sample V": L.inet_sample_multinomial(X, 4, 1, 0, X, 1, 1, 0, NULL),
        "reparam mu": L.inet_reparam_kl(NULL, X, X, X, X, 4, X, NULL),
        "reparam logsigma": L.inet_reparam_kl(X, NULL, X, X, X, 4, X, NULL),
        "reparam n": L.inet_reparam_kl(X, X, X, X, X, 0, X, NULL),
        "latent_bwd mu": L.inet_latent_bwd(X, NULL, X, X, 1.0, NULL, X, X, 4, NULL),
        "latent_bwd logsigma": L.inet_latent_bwd(X, X, NULL, X, 1.0, NULL, X, X, 4, NULL),
        "latent_bwd dmu": L.inet_latent_bwd(X, X, X, X, 1.0, NULL, NULL, X, 4, NULL),
        "latent_bwd dlogsigma": L.inet_latent_bwd(X, X, X, X, 1.0, NULL, X, NULL, 4, NULL),
        "latent_bwd n": L.inet_latent_bwd(X, X, X, X, 1.0, NULL, X, X, 0, NULL),
        "step_flag_export dst": L.inet_step_flag_export(NULL, NULL),
        "epoch_stats sums": L.inet_epoch_stats_add_ex(NULL, X, X, X, NULL),
        "epoch_stats loss": L.inet_epoch_stats_add_ex(X, NULL, X, X, NULL),
        "epoch_stats (plain) sums": L.inet_epoch_stats_add(NULL, X, X, NULL),
        "epoch_stats (plain) loss": L.inet_epoch_stats_add(X, NULL, X, NULL),
        "dropout out": L.inet_dropout_mask(NULL, 4, 0.5, 1, 0, NULL),
        "dropout n": L.inet_dropout_mask(X, 0, 0.5, 1, 0, NULL),
        "dropout p < 0": L.inet_dropout_mask(X, 4, -0.001, 1, 0, NULL),
        "dropout p = 1": L.inet_dropout_mask(X, 4, 1.0, 1, 0, NULL),
        "dropout p > 1": L.inet_dropout_mask(X, 4, 1.5, 1, 0, NULL),
        "embedding_fwd table": L.inet_embedding_fwd(NULL, X, 4, 4, X, NULL, NULL),
        "embedding_fwd idx": L.inet_embedding_fwd(X, NULL, 4, 4, X, NULL, NULL),
        "embedding_fwd out": L.inet_embedding_fwd(X, X, 4, 4, NULL, NULL, NULL),
        "embedding_fwd rows": L.inet_embedding_fwd(X, X, 0, 4, X, NULL, NULL),
        "embedding_fwd E": L.inet_embedding_fwd(X, X, 4, 0, X, NULL, NULL),
        "embedding_bwd dout": L.inet_embedding_bwd(NULL, X, 4, 4, X, NULL, 8, NULL),
        "embedding_bwd idx": L.inet_embedding_bwd(X, NULL, 4, 4, X, NULL, 8, NULL),
        "embedding_bwd dtable": L.inet_embedding_bwd(X, X, 4, 4, NULL, NULL, 8, NULL),
        "embedding_bwd rows": L.inet_embedding_bwd(X, X, 0, 4, X, NULL, 8, NULL),
        "embedding_bwd E": L.inet_embedding_bwd(X, X, 4, 0, X, NULL, 8, NULL),
        "embedding_bwd num_embeddings": L.inet_embedding_bwd(X, X, 4, 4, X, NULL, -1, NULL),
        "relu_bwd dy": L.inet_relu_bwd(NULL, X, X, 4, NULL),
        "relu_bwd y": L.inet_relu_bwd(X, NULL, X, 4, NULL),
        "relu_bwd dpre": L.inet_relu_bwd(X, X, NULL, 4, NULL),
        "relu_bwd n": L.inet_relu_bwd(X, X, X, 0, NULL),
        "linear_fwd x": L.inet_linear_fwd(NULL, X, X, X, 4, 4, 4, 0, NULL),
        "linear_fwd W": L.inet_linear_fwd(X, NULL, X, X, 4, 4, 4, 0, NULL),
        "linear_fwd y": L.inet_linear_fwd(X, X, X, NULL, 4, 4, 4, 0, NULL),
        "linear_fwd M": L.inet_linear_fwd(X, X, X, X, 0, 4, 4, 0, NULL),
        "linear_fwd N": L.inet_linear_fwd(X, X, X, X, 4, 0, 4, 0, NULL),
        "linear_fwd K": L.inet_linear_fwd(X, X, X, X, 4, 4, 0, 0, NULL),
        "linear_fwd epi -1": L.inet_linear_fwd(X, X, X, X, 4, 4, 4, -1, NULL),
        "linear_fwd epi 3": L.inet_linear_fwd(X, X, X, X, 4, 4, 4, 3, NULL),
        "linear_bwd dy": L.inet_linear_bwd(NULL, X, X, X, X, X, 4, 4, 4, NULL),
        "linear_bwd M": L.inet_linear_bwd(X, X, X, X, X, X, 0, 4, 4, NULL),
        "linear_bwd N": L.inet_linear_bwd(X, X, X, X, X, X, 4, 0, 4, NULL),
        "linear_bwd K": L.inet_linear_bwd(X, X, X, X, X, X, 4, 4, 0, NULL),
        "linear_bwd dx without W": L.inet_linear_bwd(X, X, NULL, X, NULL, NULL, 4, 4, 4, NULL),
    }
    wrong = {k: v for k, v in calls.items() if v != -1}
    assert not wrong, wrong


@pytest.mark.parametrize("ex", [False, True])
def test_adam_rejects_null_pointers_empty_sizes_and_step_zero(L, ex):
    def call(p=X, g=X, m=X, v=X, n=4, step=1):
        if ex:
            return L.inet_adam_step_ex(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, step, 1.0, NULL, NULL, NULL)
        return L.inet_adam_step(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, step, 1.0, NULL)
    got = {"p": call(p=NULL), "g": call(g=NULL), "m": call(m=NULL), "v": call(v=NULL), "n = 0": call(n=0), "n < 0": call(n=-4),
           "step 0": call(step=0), "step < 0": call(step=-1)}
    assert all(v == -1 for v in got.values()), got
