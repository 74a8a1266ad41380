"""The identities behind folding the MotionAdaptor's normalisation passes into its convs
(runtime.cpp adaptor / ln_conv, conv_x3.hip AFF), in numpy fp64 on random inputs:

1. extrapolator: with hn = (x - mean) / std and the conv's zero padding in the normalised domain,
   (conv3x3(hn) + hn) * std + mean  ==  std * conv3x3(hn) + x;
2. statistics: (count, mean, M2) of frame chunks 2 | 2 | 4 combined by Chan's formula, always as
   (earlier, chunk), give the two-pass mean and unbiased std (+ 1e-5 under the root, the reference's
   calc_mean_std) over the first 2, 4 and 8 frames; the chunk's one-pass M2 about its first element
   holds up when |mean| >> std;
3. PreNorm: conv1x1(W diag(gamma), (x - m) r) == conv1x1(W, LN(x)), LN(x) = (x - m) / sqrt(var +
   1e-5) * gamma with the biased variance over channels and r = 1 / sqrt(var + 1e-5), for one source
   and for two concatenated ones.

fp64 rounding only: the bound is 1e-12 relative to the largest magnitude on either side."""
import numpy as np
import pytest

RTOL = 1e-12


def close(a, b):
    scale = max(np.abs(a).max(), np.abs(b).max(), 1.0)
    assert np.abs(a - b).max() <= RTOL * scale, np.abs(a - b).max() / scale


def conv3x3(x, w):
    """x [C][T][H][W], w [Co][C][3][3], zero padding 1 per frame"""
    C, T, H, W = x.shape
    xp = np.zeros((C, T, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], T, H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum('oc,cthw->othw', w[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])
    return out


def mean_std(x):
    """per channel over (T, H, W): mean and sqrt(unbiased var + 1e-5)"""
    f = x.reshape(x.shape[0], -1)
    return f.mean(axis=1), np.sqrt(f.var(axis=1, ddof=1) + 1e-5)


@pytest.mark.parametrize('offset', [0.0, 50.0])
def test_extrapolator_residual_form(offset):
    rng = np.random.default_rng(11)
    C, T, H, W = 6, 4, 5, 7
    x = rng.standard_normal((C, T, H, W)) * rng.uniform(0.5, 3.0, (C, 1, 1, 1)) + offset
    w = rng.standard_normal((C, C, 3, 3)) * 0.2
    assert np.abs(w).min() > 0
    m, sd = mean_std(x)
    m, sd = m[:, None, None, None], sd[:, None, None, None]
    hn = (x - m) / sd
    ref = (conv3x3(hn, w) + hn) * sd + m
    # the folded form: the affine as a subtract and a reciprocal multiply, the conv term scaled alone
    hn_r = (x - m) * (1.0 / sd)
    close(sd * conv3x3(hn_r, w) + x, ref)


def chunk_stats(x):
    """one pass over a chunk [C][n]: count, mean, M2 from sums about the first element"""
    k = x[:, :1]
    d = x - k
    n = x.shape[1]
    s, q = d.sum(axis=1), (d * d).sum(axis=1)
    return n, k[:, 0] + s / n, q - s * s / n


def chan(a, b):
    (na, ma, qa), (nb, mb, qb) = a, b
    n, delta = na + nb, mb - ma
    return n, ma + delta * nb / n, qa + qb + delta * delta * na * nb / n


@pytest.mark.parametrize('offset,scale', [(0.0, 1.0), (50.0, 1.0), (1e4, 1e-2)])
def test_chan_combined_chunks_match_two_pass(offset, scale):
    rng = np.random.default_rng(12)
    C, HW = 5, 48
    x = rng.standard_normal((C, 8, HW)) * scale * rng.uniform(0.5, 2.0, (C, 1, 1)) + offset
    # later frames drift, as extrapolated frames do
    x += np.arange(8)[None, :, None] * 0.1 * scale
    carried = None
    for lo, hi in ((0, 2), (2, 4), (4, 8)):
        c = chunk_stats(x[:, lo:hi].reshape(C, -1))
        carried = c if carried is None else chan(carried, c)
        n, mean, m2 = carried
        assert n == hi * HW
        m_ref, sd_ref = mean_std(x[:, :hi])
        close(mean, m_ref)
        # the variance loses log2(|mean| / std)^2 bits to the data's own rounding in any formula;
        # about the first element the one-pass form loses no more than the two-pass one
        sd = np.sqrt(m2 / (n - 1) + 1e-5)
        assert np.abs(sd - sd_ref).max() <= 1e-9 * sd_ref.max(), np.abs(sd - sd_ref).max() / sd_ref.max()


def layer_norm(x, g):
    """x [C][N]: channel LayerNorm, biased variance, gamma only"""
    m = x.mean(axis=0, keepdims=True)
    var = ((x - m) ** 2).mean(axis=0, keepdims=True)
    return (x - m) / np.sqrt(var + 1e-5) * g[:, None], m, 1.0 / np.sqrt(var + 1e-5)


@pytest.mark.parametrize('c0,c1', [(8, 0), (8, 8), (16, 4)])
def test_gamma_folds_into_the_1x1_weight(c0, c1):
    rng = np.random.default_rng(13)
    C, Co, N = c0 + c1, 7, 33
    # two sources concatenated along channels (the fuser), or one (the predictor, the qkv conv)
    x = np.concatenate([rng.standard_normal((c0, N)) * 2.0 + 1.0, rng.standard_normal((c1, N)) * 0.3 - 4.0])
    g = rng.uniform(-1.5, 1.5, C)
    w = rng.standard_normal((Co, C))
    ln, m, r = layer_norm(x, g)
    close((w * g[None, :]) @ ((x - m) * r), w @ ln)
