"""NumPy restatement of the decimation formula of include/hypermvar.h (hmv_decimate_fir_f64) and the rounding bound the
decimation tests hold results to.  No GPU, no SciPy: shared by tests/test_decimate_cpu.py and tests/test_gpu_decimate.py.

    y[..., k] = sum_{j=0}^{n_taps-1} h[j] x[..., k q + H - j],    H = (n_taps - 1) / 2,    k = 0 .. ceil(T / q) - 1,

samples outside [0, T) counting as zero."""
import numpy as np

EPS = 2.0 ** -52
T_CASES = (1, 7, 39, 40, 41, 1003)
Q_CASES = (2, 3, 4, 5, 8, 13)


def _gathered(x, q, n_taps):
    """(.., T_out, n_taps): x[..., k q + H - j] with zeros outside the recording."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    H = (n_taps - 1) // 2
    T_out = -(-T // q)
    idx = np.arange(T_out)[:, None] * q + H - np.arange(n_taps)[None, :]
    ok = (idx >= 0) & (idx < T)
    return np.where(ok, x[..., np.clip(idx, 0, T - 1)], 0.0)


def decimate_restated(x, q, h):
    """The formula, summed by NumPy (pairwise, not the kernel's order: equal to it to `rounding_bound` only)."""
    h = np.asarray(h, dtype=np.float64)
    return (_gathered(x, q, len(h)) * h).sum(axis=-1)


def rounding_bound(x, q, h):
    """Per output: two summations of the same n_taps products in different orders, each product rounded once or fused,
    differ by at most 2 n_taps 2^-52 sum_j |h_j| |x_{kq+H-j}| (each side's error is below n u sum |terms| with
    u = 2^-53, to first order; the factor 2 n eps = 4 n u leaves the higher-order terms ample room)."""
    h = np.asarray(h, dtype=np.float64)
    return 2.0 * len(h) * EPS * (np.abs(_gathered(x, q, len(h))) * np.abs(h)).sum(axis=-1)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the outputs whose bound is not zero; outputs with a zero bound must agree exactly."""
    err = np.abs(np.asarray(got) - np.asarray(want))
    zero = bound == 0.0
    assert not err[zero].any(), "outputs that no non-zero product reaches must be exactly zero"
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
