"""Seeded synthetic workloads -- the build's own generator, not reference code.

Used by bench.py, the parity tests and tests/golden/make_golden.py.  NumPy only (no GPU, no oracle), except
`band_limited_dyad`, which filters with SciPy as `eeg_io` does.
"""
from __future__ import annotations

import numpy as np

__all__ = ["synthetic_var_dyad", "mixed_order_recording", "band_limited_dyad", "northstar_freqs", "NORTHSTAR"]

NORTHSTAR = dict(m=64, fs=500.0, window=1000, hop=500, p=8, F=256, T=300_000)


def northstar_freqs(F: int = 256):
    """0.5 Hz grid 0.5 .. 128 Hz (the reference's default 0.5-Hz step, mtmvar.py:1014)."""
    return 0.5 * np.arange(1, F + 1)

def synthetic_var_dyad(dyad: int, m: int = 64, p: int = 8, T: int = 300_000, fs: float = 500.0,
                       burn: int = 2000, density: float = 0.05, coupling: float = 0.05,
                       target_radius: float = 0.95):
    """Seeded stable VAR(p) recording used by bench and parity tests.

    Diagonal AR(2) resonators (f0 ~ U(4, 40) Hz, r ~ U(0.80, 0.95)), sparse N(0,1)*coupling
    off-diagonal terms on every lag, companion spectral radius rescaled to `target_radius`
    (A_k <- A_k * g**k), unit-variance innovations, burn-in discarded, each channel z-scored.
    This is the build's own workload generator, not reference code.
    """
    rng = np.random.default_rng(1234 + dyad)
    A = np.zeros((p, m, m))
    f0 = rng.uniform(4.0, 40.0, m)
    r = rng.uniform(0.80, 0.95, m)
    idx = np.arange(m)
    A[0, idx, idx] = 2 * r * np.cos(2 * np.pi * f0 / fs)
    if p > 1:
        A[1, idx, idx] = -r ** 2
    mask = rng.random((p, m, m)) < density
    off = coupling * rng.standard_normal((p, m, m)) * mask
    off[:, idx, idx] = 0.0
    A += off
    comp = np.zeros((m * p, m * p))
    comp[:m, :] = np.concatenate(list(A), axis=1)
    comp[m:, :-m] = np.eye(m * (p - 1))
    rho = np.max(np.abs(np.linalg.eigvals(comp)))
    g = min(1.0, target_radius / rho)
    A = A * (g ** np.arange(1, p + 1))[:, None, None]
    n_tot = T + burn
    e = rng.standard_normal((n_tot, m))
    x = np.zeros((n_tot, m))
    # x[t] = e[t] + [x[t-1], ..., x[t-p]] @ W,  W = vstack_k A_k^T  (one (p*m) x m mat-vec per sample)
    W = np.ascontiguousarray(np.concatenate([A[k].T for k in range(p)], axis=0))
    for t in range(p, n_tot):
        x[t] = e[t] + x[t - p:t][::-1].reshape(-1) @ W
    x = x[burn:].T
    x = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
    return np.ascontiguousarray(x)


def mixed_order_recording(seed: int, m: int, orders, seg: int, burn: int = 500):
    """Recording (m, len(orders) * seg) whose windows need DIFFERENT model orders: one stable VAR(q) stretch of `seg`
    samples per entry q of `orders`, concatenated.  `synthetic_var_dyad` is AR(2)-dominated -- the model-order criterion
    picks order 2 for every window of it -- and cannot test a selection.  Stretch i, seeded default_rng(seed + i): lag-1
    diagonal U(0.1, 0.3); -0.5 * U(0.7, 1.0) added to the lag-q diagonal; lag-q coupling i <- i + 1 (mod m) of +0.15; unit
    innovations; `burn` samples dropped.  The whole recording is z-scored per channel."""
    idx = np.arange(m)
    parts = []
    for i, q in enumerate(orders):
        q = int(q)
        rng = np.random.default_rng(seed + i)
        A = np.zeros((q, m, m))
        A[0, idx, idx] = rng.uniform(0.1, 0.3, m)
        A[q - 1, idx, idx] += -0.5 * rng.uniform(0.7, 1.0, m)
        A[q - 1, idx, (idx + 1) % m] = 0.15
        n_tot = seg + burn
        e = rng.standard_normal((n_tot, m))
        x = np.zeros((n_tot, m))
        W = np.ascontiguousarray(np.concatenate([A[k].T for k in range(q)], axis=0))
        x[:q] = e[:q]
        for t in range(q, n_tot):
            x[t] = e[t] + x[t - q:t][::-1].reshape(-1) @ W
        parts.append(x[burn:].T)
    x = np.concatenate(parts, axis=1)
    x = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
    return np.ascontiguousarray(x)


def band_limited_dyad(seed: int, m: int, T: int, fs: float = 500.0, high_cutoff_hz: float = 45.0, p: int = 8,
                      burn: int = 2000):
    """`synthetic_var_dyad(seed, m, p, T, fs, burn)` through a zero-phase Butterworth-4 low-pass at `high_cutoff_hz`
    (`scipy.signal.filtfilt`, what `eeg_io.bandpass_filter` applies to a recording), z-scored per channel again: the
    ill-conditioned regime of filtered recordings.  The lagged samples of a signal without power above the cut-off are
    nearly dependent -- at fs = 500 the order-8 normal equations of a 64-channel window reach cond ~ 4e15 at 45 Hz and
    ~ 2e18 at 30 Hz -- and the unpivoted Yule-Walker solvers refuse such windows (`Engine(pivoted_yw=True)`)."""
    from scipy.signal import butter, filtfilt
    if not 0.0 < float(high_cutoff_hz) < 0.5 * float(fs):
        raise ValueError(f"high_cutoff_hz must be in (0, fs / 2) = (0, {0.5 * float(fs)}), got {high_cutoff_hz}")
    x = synthetic_var_dyad(seed, m=m, p=p, T=T, fs=fs, burn=burn)
    b, a = butter(4, float(high_cutoff_hz) / (0.5 * float(fs)), btype="low")
    x = filtfilt(b, a, x, axis=1)
    x = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
    return np.ascontiguousarray(x)
