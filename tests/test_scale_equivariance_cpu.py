"""The premise of tests/test_gpu_amplitude.py, pinned on the NumPy oracle (no GPU): scaling every sample by a power of
two changes no mantissa, so the Yule-Walker fit returns the SAME coefficient bits and the residual covariance times
4**k bit for bit (the dense solve's partial pivoting compares magnitudes that all carry the same factor), and the
normalised measures built from them do not move.  ffDTF and GPDC are bitwise; dDTF and the partial coherence go through
determinants of minors, whose LU pivot choice sees entries scaled by different powers of the factor in different
minors only through exact scalings too, but NumPy's complex arithmetic is allowed its last bits there: 1e-13 relative.

Also the conditioning of the high-order inputs: 1e2 * cond * eps of every shape stays below the cap the GPU tests use."""
import numpy as np
import pytest

from oracle import mvar_oracle as O
from tests import scale_shapes as SS


@pytest.mark.parametrize("shape", SS.HIGH_ORDER_SHAPES, ids=SS.shape_id)
def test_yule_walker_fit_is_power_of_two_equivariant(shape):
    m, p, n = shape
    x = SS.high_order_input(m, p, n)
    ar, V = O.ar_coeff(x, p)
    assert np.isfinite(ar).all() and np.isfinite(V).all()
    for k in SS.POWERS:
        ark, Vk = O.ar_coeff(x * 2.0 ** k, p)
        assert np.array_equal(ark, ar), k
        assert np.array_equal(Vk, V * 4.0 ** k), k


@pytest.mark.parametrize("shape", SS.HIGH_ORDER_SHAPES, ids=SS.shape_id)
def test_high_order_inputs_are_well_conditioned(shape):
    m, p, n = shape
    cond = SS.normal_matrix_cond(O, SS.high_order_input(m, p, n), p)
    print(shape, f"cond {cond:.3g}, tolerance {1e2 * cond * SS.EPS:.3g}")
    assert 1e3 < cond < 1e5
    assert 1e2 * cond * SS.EPS <= SS.COND_TOL_CAP


def test_lag_covariances_scale_by_four_to_the_k():
    x = SS.high_order_input(19, 32, 2000)
    R = O.lag_covariances(x, 32)
    for k in SS.POWERS:
        assert np.array_equal(O.lag_covariances(x * 2.0 ** k, 32), R * 4.0 ** k)


def test_ffdtf_and_gpdc_are_bitwise_scale_free():
    x, _ = SS.amplitude_input(19, 8, 400, 1)
    freqs = np.linspace(1.0, 45.0, 16)
    ff = O.full_freq_dtf(x, freqs, 128.0, 8)
    gp = O.gen_partial_directed_coherence(x, freqs, 128.0, 8)
    S = O.multivariate_spectra(x, freqs, 128.0, 8)
    for k in SS.POWERS:
        y = x * 2.0 ** k
        assert np.array_equal(O.full_freq_dtf(y, freqs, 128.0, 8), ff), k
        assert np.array_equal(O.gen_partial_directed_coherence(y, freqs, 128.0, 8), gp), k
        assert np.array_equal(O.multivariate_spectra(y, freqs, 128.0, 8), S * 4.0 ** k), k


def test_ddtf_and_partial_coherence_are_scale_free_to_rounding():
    x, _ = SS.amplitude_input(8, 5, 400, 1)
    freqs = np.linspace(1.0, 45.0, 8)
    dd = O.direct_dtf(x, freqs, 128.0, 5)
    kap = O.partial_coherence(O.multivariate_spectra(x, freqs, 128.0, 5))
    for k in SS.POWERS:
        y = x * 2.0 ** k
        assert SS.rel(O.direct_dtf(y, freqs, 128.0, 5), dd) <= 1e-13, k
        assert SS.rel(O.partial_coherence(O.multivariate_spectra(y, freqs, 128.0, 5)), kap) <= 1e-13, k


def test_per_channel_scaling_of_the_fit():
    """D = diag(2**s_i): ar -> D ar D^-1 and V -> D V D, GPDC unchanged -- on the oracle only to the conditioning rule
    1e2 * cond * eps: its dense solve pivots on magnitudes, which per-channel factors reorder (the kernels, which do not
    pivot, keep the bits: tests/test_gpu_amplitude.py)."""
    x, _ = SS.amplitude_input(19, 8, 400, 1)
    s = (np.arange(19) % 7) - 3
    d = 2.0 ** s
    freqs = np.linspace(1.0, 45.0, 16)
    ar, V = O.ar_coeff(x, 8)
    ard, Vd = O.ar_coeff(x * d[:, None], 8)
    assert SS.rel(ard, ar * (d[:, None] / d[None, :])[:, :, None]) <= 1e2 * SS.normal_matrix_cond(O, x, 8) * SS.EPS
    assert SS.rel(Vd, V * np.outer(d, d)) <= 1e2 * SS.normal_matrix_cond(O, x, 8) * SS.EPS
    assert SS.rel(O.gen_partial_directed_coherence(x * d[:, None], freqs, 128.0, 8),
                  O.gen_partial_directed_coherence(x, freqs, 128.0, 8)) <= 1e-9


@pytest.mark.parametrize("case", SS.AUTO_AMPLITUDE_SHAPES, ids=SS.shape_id)
def test_criterion_gap_of_the_automatic_order_inputs(case):
    """Every window the GPU test selects an order for has its criterion minimum at least GAP below the runner-up, under
    all three criteria, and the selection does not move with the amplitude (log det V shifts by 2 k m ln 2 at every order)."""
    m, pmax, n, nw = case
    x, starts = SS.amplitude_input(m, pmax, n, nw)
    for crit in ("AIC", "HQ", "SC"):
        for s in starts:
            c = O.mvar_criterion(x[:, s:s + n], pmax, crit)[0]
            q, gap = SS.criterion_gap(c)
            assert gap >= SS.GAP, (crit, int(s), q, gap)
    # The oracle (like the reference) takes log(det V): det V * 4**(k m) leaves the float64 range once 2 |k| m > ~1000, and
    # its criterion is then -inf / inf at every order.  The kernels add up log pivots and have no such limit, which is why
    # the GPU tests compare the scaled run with the UNSCALED one and ask the oracle at unit scale only.
    c0 = O.mvar_criterion(x[:, :n], pmax, "AIC")[0]
    for k in (-20, 20):
        if 2 * abs(k) * m > 900:
            continue
        ck = O.mvar_criterion(x[:, :n] * 2.0 ** k, pmax, "AIC")[0]
        assert SS.criterion_gap(ck)[0] == SS.criterion_gap(c0)[0]
        assert np.allclose(ck - c0, 2 * k * m * np.log(2.0), rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", SS.AUTO_HIGH_ORDER_SHAPES, ids=SS.shape_id)
def test_criterion_gap_of_the_high_order_inputs(case):
    m, pmax, n = case
    x = SS.high_order_input(m, pmax, n)
    for crit in ("AIC", "HQ", "SC"):
        q, gap = SS.criterion_gap(O.mvar_criterion(x, pmax, crit)[0])
        assert gap >= SS.GAP, (crit, q, gap)


@pytest.mark.parametrize("m,p,n", [(19, 3, 300), (16, 3, 200), (4, 3, 200)])
def test_amplitudes_the_minors_based_ddtf_can_take(m, p, n):
    """The oracle's dDTF and partial coherence on x * 2**k agree with those on x up to |k| = SS.minors_power(m) -- the
    amplitude at which tests/test_gpu_amplitude.py asks them -- and at 19 channels they no longer do at k = -20 (the
    product of two minors has underflowed), which is why that test does not ask them there."""
    x, _ = SS.amplitude_input(m, p, n, 1)
    freqs = np.linspace(1.0, 60.0, 32)
    dd = O.direct_dtf(x, freqs, 128.0, p)
    kap = np.abs(O.partial_coherence(O.multivariate_spectra(x, freqs, 128.0, p)))
    for k in (-SS.minors_power(m), SS.minors_power(m)):
        y = x * 2.0 ** k
        assert SS.rel(O.direct_dtf(y, freqs, 128.0, p), dd) <= 1e-12, k
        assert SS.rel(np.abs(O.partial_coherence(O.multivariate_spectra(y, freqs, 128.0, p))), kap) <= 1e-12, k
    if m == 19:
        assert SS.minors_power(m) == 8
        with np.errstate(all="ignore"):
            assert SS.rel(O.direct_dtf(x * 2.0 ** -20, freqs, 128.0, p), dd) > 1e-2
