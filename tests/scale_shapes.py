"""Shapes and small helpers shared by tests/test_scale_equivariance_cpu.py, tests/test_gpu_amplitude.py and
tests/test_gpu_high_order.py.  NumPy only: importable without a GPU.

The lever of the amplitude tests: x * 2**k changes no mantissa, so every product, sum, reciprocal and square root of an
implementation without an absolute constant scales by an exact power of two -- lag covariances and residual covariances
by 4**k bit for bit, coefficients, transfer functions and the normalised measures not at all."""
import numpy as np

from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

EPS = np.finfo(np.float64).eps

# k = -20: volts (1e-6 .. 1e-5); 4**12 = 1.7e7 is the smallest power of four beyond 1 / HMV_LWR_GUARD = 1e7
POWERS = (-20, -12, 12, 20)

# (m, p, n) of the high-order tests, inputs synthetic_var_dyad(31, m=m, p=4, T=n, burn=300); the condition number of the
# oracle's normal matrix lies between 6e3 and 8.2e4 (the tests compute it and bound it)
HIGH_ORDER_SEED = 31
HIGH_ORDER_SHAPES = [(4, 20, 160), (4, 32, 400), (5, 32, 600), (19, 24, 1500), (19, 32, 2000), (33, 17, 2000),
                     (48, 32, 4000), (64, 17, 3000), (64, 32, 6000)]
COND_TOL_CAP = 2e-9          # 1e2 * cond * eps must stay below this on the shapes above

# (m, p, n, n_windows) of the amplitude tests: padded sizes 16 / 32 / 48 / 64 with and without padded channels, p in
# {3, 8}, and the reference's default order on the small-window configuration.  Windows start every n // 2 samples.
AMPLITUDE_SEED = 61
PADDED_M = (4, 19, 33, 50)
AMPLITUDE_SHAPES = [(4, 3, 200, 8), (4, 8, 240, 5), (19, 3, 300, 4), (19, 8, 400, 4), (33, 3, 300, 3), (33, 8, 400, 3),
                    (50, 3, 400, 3), (50, 8, 600, 3), (16, 3, 200, 5), (16, 8, 300, 4), (48, 3, 400, 3), (48, 8, 600, 3),
                    (64, 3, 400, 3), (64, 8, 600, 3), (4, 20, 160, 6)]
# automatic order: (m, pmax, n, n_windows); the oracle's criterion gap is asserted in the tests
AUTO_HIGH_ORDER_SHAPES = [(4, 32, 400), (19, 32, 2000), (4, 20, 160)]          # (m, pmax, n), one window each
AUTO_AMPLITUDE_SHAPES = [(4, 20, 160, 6), (19, 8, 400, 4), (33, 6, 300, 3), (50, 6, 600, 3), (64, 8, 600, 3)]
GAP = 1e-6


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


def high_order_input(m, p, n):
    return synthetic_var_dyad(HIGH_ORDER_SEED, m=m, p=4, T=n, burn=300)


def amplitude_input(m, p, n, n_windows, seed=AMPLITUDE_SEED):
    """(x (m, T), starts): n_windows windows of n samples every n // 2 samples (a regular grid of two hops per window)."""
    hop = n // 2
    T = n + hop * (n_windows - 1)
    x = synthetic_var_dyad(seed, m=m, p=min(p, 4), T=T, burn=300)
    return x, hop * np.arange(n_windows, dtype=np.int64)


def normal_matrix_cond(O, x, p):
    """2-norm condition number of the oracle's block-Toeplitz normal matrix of one window."""
    r_left, _, _ = O.count_corr(x[:, :, None], p, 1)
    assert np.array_equal(r_left, r_left.T)                       # block Toeplitz of R_0 = R_0^T and R_l / R_l^T
    ev = np.linalg.eigvalsh(r_left)
    return float(ev[-1] / ev[0])


def criterion_gap(c):
    """(first arg-min + 1, runner-up's value minus the minimum) of one criterion curve."""
    order = np.argsort(c, kind="stable")
    return int(np.argmin(c)) + 1, (float(c[order[1]] - c[order[0]]) if len(c) > 1 else np.inf)


def minors_power(m):
    """Largest |k| at which the oracle's (and the reference's) dDTF / partial coherence can be asked about x * 2**k: they
    divide minors of the spectral matrix by sqrt(M_ii M_jj), a product that carries 4**(2 k (m - 1)); 600 binary orders of
    it leave the determinants themselves 400 more inside float64.  Beyond it the product underflows to 0 or overflows
    (measured at 19 channels: kappa 10 % off at k = -12, all zero at k = -20, not finite at k = 20)."""
    return min(20, 600 // (4 * (m - 1)))


def ddtf_restated(O, xw, freqs, fs, p):
    """dDTF of one window from the oracle's fit by the algebra of the kernels (tests/test_gpu_auto_order.py's
    restatement): |kappa_ij| = |W_ji| / sqrt(|W_ii| |W_jj|), W = A^T V^-1 A, kappa_ii = 1.  No minors: no amplitude limit."""
    ar, V = O.ar_coeff(xw, p)
    _, A = O.mvar_transfer_function(ar, freqs, fs)
    Vi = np.linalg.inv(V)
    ff = O.full_freq_dtf(xw, freqs, fs, p)
    out = np.empty_like(ff)
    m = xw.shape[0]
    for k in range(len(freqs)):
        W = A[:, :, k].T @ Vi @ A[:, :, k]
        d = np.abs(np.diag(W))
        kap = np.abs(W.T) / np.sqrt(np.outer(d, d))
        kap[np.arange(m), np.arange(m)] = 1.0
        out[:, :, k] = ff[:, :, k] * kap
    return out


def i64(eng, a):
    """int64 device tensor of an index list (imports torch only when a GPU test calls it)."""
    import torch
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)


class tuning:
    """`with tuning(eng, knob, value):` -- hmv_set_tuning for the block, back to the default behind it."""
    def __init__(self, eng, knob, value):
        self.eng, self.knob, self.value = eng, knob, value

    def __enter__(self):
        assert self.eng.lib.hmv_set_tuning(self.knob, self.value) == 0

    def __exit__(self, *exc):
        assert self.eng.lib.hmv_set_tuning(self.knob, 0) == 0


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
