"""NumPy restatements of the two significance tests of block Granger causality (`Engine.block_granger_significance`,
`Engine.block_granger_pseudo_dyad_significance`) for tests/test_block_gc_significance_cpu.py and
tests/test_gpu_block_gc_significance.py: the oracle's fit of every window written out, the textbook block values of
tests/block_gc_restated.py on it, NumPy statistics.  NumPy only: importable without a GPU, nothing here is the code under test.

A window's values are a (2, nv) array: row 0 is A -> B, row 1 is B -> A; the columns are the time-domain value (if asked
for), then the band sums of the spectral decomposition."""
import numpy as np

from hyperscanning_signal_analysis_amd import surrogates as sg
from oracle import mvar_oracle as O
from tests import block_gc_restated as G

STATS = ("p", "p_fwe", "null_mean", "null_std")


def window_values(xw, split, p, freqs, fs, lo, hi, values=("time", "bands")):
    """-> ((2, nv) tested values, (4,) time-domain values) of one window (m, n)."""
    ar, V = O.ar_coeff(xw, p)
    t = G.time_domain(O.lag_covariances(xw, p), V, split, p)
    cols = [t[:2, None]] if "time" in values else []
    if "bands" in values:
        f = G.definition(ar, V, split, freqs, fs)
        cols.append(np.stack([f[:, a:b].sum(-1) for a, b in zip(lo, hi)], axis=-1))
    return np.concatenate(cols, axis=1), t


def null_stats(obs, v):
    """obs (..., 2, nv) against its null values v (K, ..., 2, nv): counting with >=, (1 + count) / (1 + K), the maximum over
    the two directions per column, mean and sample std; and the smallest relative gap of a comparison."""
    K = v.shape[0]
    M = v.max(axis=-2, keepdims=True)
    out = {"p": (1.0 + (v >= obs).sum(0)) / (1.0 + K), "p_fwe": (1.0 + (M >= obs).sum(0)) / (1.0 + K),
           "null_mean": v.mean(0), "null_std": v.std(0, ddof=1)}
    gap = min((np.abs(v - obs) / np.abs(obs)).min(), (np.abs(M - obs) / np.abs(obs)).min())
    return out, float(gap)


def surrogate_windows(null, x, pos, n, S, seed, split, min_shift=None):
    """The surrogate windows of `block_granger_significance` written out from the documented draws: (S, n_rec * W, m, n),
    window r * W + w."""
    n_rec, m, T = x.shape
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    out = np.empty((S, n_rec * len(pos), m, n))
    if null == "shift":
        d = sg.shift_offsets(rng, S, n_rec, T, n if min_shift is None else min_shift)
    else:
        phi = sg.phase_draws(rng, S, m, n)
    for r in range(n_rec):
        for w, st in enumerate(pos):
            xw = x[r, :, st:st + n]
            for s in range(S):
                if null == "shift":
                    xs = xw.copy()
                    xs[split:] = x[r, split:][:, (st + t + d[s, r]) % T]
                else:
                    xs = np.fft.irfft(np.fft.rfft(xw, axis=-1) * np.exp(1j * phi[s]), n, axis=-1)
                out[s, r * len(pos) + w] = xs
    return out


def restate_surrogates(null, x, pos, n, p, freqs, fs, lo, hi, S, seed, split, min_shift=None, values=("time", "bands")):
    """The surrogate test on the host -> (dict: observed, p, p_fwe, null_mean, null_std (N, 2, nv), observed_time (N, 4),
    null (S, N, 2, nv), n_valid (N,); the smallest relative gap of a comparison).  Every fit must succeed."""
    n_rec = x.shape[0]
    sur = surrogate_windows(null, x, pos, n, S, seed, split, min_shift)
    args = (split, p, freqs, fs, lo, hi, values)
    both = [window_values(x[r, :, st:st + n], *args) for r in range(n_rec) for st in pos]
    obs, obs_t = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    v = np.stack([np.stack([window_values(xs, *args)[0] for xs in sur[s]]) for s in range(S)])
    out, gap = null_stats(obs, v)
    out.update(observed=obs, observed_time=obs_t, null=v, n_valid=np.full(len(obs), S))
    return out, gap


def pseudo_window(x, a, b, s, n, split):
    """The window written out: rows < split of recording a, rows >= split of recording b, samples s .. s + n."""
    w = x[a][:, s:s + n].copy()
    w[split:] = x[b][split:, s:s + n]
    return w


def restate_pseudo_dyads(x, starts, n, p, freqs, fs, lo, hi, split, partners, values=("time", "bands")):
    """The pseudo-dyad test on the host -> (per-dyad dict (D, W, 2, nv) with null (2 S, D, W, 2, nv), group dict (W, 2, nv)
    with null (S, W, 2, nv), the smallest relative gap).  Null value 2 s of dyad d is A-anchored (A_d with B_pi(d)), 2 s + 1
    B-anchored (A_{pi^-1(d)} with B_d); the group value is the mean over the dyads."""
    D, W, S = x.shape[0], len(starts), len(partners)
    args = (split, p, freqs, fs, lo, hi, values)
    both = [[window_values(pseudo_window(x, d, d, s0, n, split), *args) for s0 in starts] for d in range(D)]
    obs = np.array([[b[0] for b in row] for row in both])
    obs_t = np.array([[b[1] for b in row] for row in both])
    sur = np.array([[[window_values(pseudo_window(x, d, partners[s][d], s0, n, split), *args)[0] for s0 in starts]
                     for d in range(D)] for s in range(S)])
    v = np.empty((2 * S,) + obs.shape)
    for s in range(S):
        v[2 * s] = sur[s]
        v[2 * s + 1] = sur[s][np.argsort(partners[s])]
    dyad, gap_d = null_stats(obs, v)
    dyad.update(observed=obs, observed_time=obs_t, null=v, n_valid=np.full((D, W), 2 * S))
    gobs = obs.mean(0)
    group, gap_g = null_stats(gobs, sur.mean(1))
    group.update(observed=gobs, null=sur.mean(1), n_valid=np.full(W, S))
    return dyad, group, min(gap_d, gap_g)


def planted_dyads():
    """The data of test_planted_coupling_is_found_against_every_pseudo_dyad (tests/test_gpu_pseudo_dyads.py): 5 dyads of 3 + 3
    channels of white noise, B's channel 0 follows its own partner's A channel 0 by one sample."""
    D, T = 5, 520
    x = np.empty((D, 6, T))
    for d in range(D):
        e = np.random.default_rng(300 + d).standard_normal((6, T))
        b0 = e[3].copy()
        e[3] = 0.5 * b0
        e[3, 1:] += 0.9 * e[0, :-1]
        x[d] = e
    return x


PLANTED = dict(split=3, n=256, hop=264, starts=(0, 264), p=2, fs=128.0, freqs=np.linspace(1.0, 60.0, 16), lo=[0], hi=[16])
