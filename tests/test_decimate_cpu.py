"""FIR decimation without a GPU: the formula of hmv_decimate_fir_f64 restated in NumPy equals SciPy's two decimators, the
taps are SciPy's, the C ABI refuses bad arguments before any launch, and escan_batch's argument checks."""
import os
import subprocess

import numpy as np
import pytest

from tests import decimate_restated as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


@pytest.mark.parametrize("q", DR.Q_CASES)
def test_restatement_equals_scipy(q):
    """Both SciPy decimators are the formula with their own taps, to the bound of two summation orders of the same
    products (decimate_restated.rounding_bound); printed: the worst observed share of that bound."""
    from scipy.signal import decimate, resample_poly
    from hyperscanning_signal_analysis_amd.eeg_io import decimation_taps
    rng = np.random.default_rng(100 + q)
    worst = 0.0
    for T in DR.T_CASES:
        x = 50e-6 * rng.standard_normal((2, 3, T))
        for design, want in (("decimate", decimate(x, q, ftype="fir", zero_phase=True, axis=-1)),
                             ("resample_poly", resample_poly(x, 1, q, axis=-1))):
            h = decimation_taps(q, design)
            got = DR.decimate_restated(x, q, h)
            assert got.shape == want.shape == (2, 3, -(-T // q))
            r = DR.worst_ratio(got, want, DR.rounding_bound(x, q, h))
            worst = max(worst, r)
            assert r <= 1.0, (design, T, q, r)
    print(f"q={q}: worst |restated - scipy| / bound = {worst:.3g}")


def test_decimation_taps_are_scipys():
    from scipy.signal import firwin
    from hyperscanning_signal_analysis_amd.eeg_io import decimation_taps
    for q in (2, 3, 4, 13, 32):
        assert np.array_equal(decimation_taps(q), firwin(20 * q + 1, 1.0 / q, window="hamming"))
        assert np.array_equal(decimation_taps(q, "decimate"), firwin(20 * q + 1, 1.0 / q, window="hamming"))
        assert np.array_equal(decimation_taps(q, "resample_poly"), firwin(20 * q + 1, 1.0 / q, window=("kaiser", 5.0)))
    own = np.array([0.25, 0.5, 0.25])
    assert np.array_equal(decimation_taps(2, own), own) and decimation_taps(2, [1, 2, 1]).dtype == np.float64
    for q, design, msg in ((1, "decimate", "factor"), (33, "decimate", "factor"), (4, "iir", "design"),
                           (4, np.ones(4), "odd length"), (4, np.ones(643), "odd length"), (4, np.ones((3, 3)), "1-D")):
        with pytest.raises(ValueError, match=msg):
            decimation_taps(q, design)


def test_out_len_and_tile(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    assert f"#define HMV_MAX_DECIMATE {_lib.MAX_DECIMATE}\n" in hdr
    assert f"#define HMV_MAX_DECIMATE_TAPS {_lib.MAX_DECIMATE_TAPS} " in hdr and _lib.MAX_DECIMATE_TAPS == 20 * 32 + 1
    for T, q, want in ((1, 2, 1), (7, 2, 4), (8, 2, 4), (9, 2, 5), (1003, 13, 78), (1000, 32, 32), (31, 32, 1),
                       (1 << 40, 3, ((1 << 40) + 2) // 3), (0, 2, -1), (-5, 2, -1), (10, 1, -1), (10, 33, -1), (10, 0, -1)):
        assert lib.hmv_decimate_out_len(T, q) == want, (T, q)
    # outputs per workgroup: whole multiples of the 256 lanes, smaller where the staged samples would not fit
    assert lib.hmv_decimate_tile(4, 81) == 1024 and lib.hmv_decimate_tile(2, 41) == 1024
    assert lib.hmv_decimate_tile(32, 641) == 256 and lib.hmv_decimate_tile(16, 321) == 512
    assert lib.hmv_decimate_tile(1, 41) == -1 and lib.hmv_decimate_tile(4, 80) == -1 and lib.hmv_decimate_tile(4, 643) == -1


def test_refusals_without_gpu(lib):
    """Every refusal of hmv_decimate_fir_f64 has its own code and text and comes before any launch (no GPU here); the
    pointers are never dereferenced on the host."""
    P = 4096                                                     # a non-null "device pointer"

    def call(x=P, rec_stride=3000, ld=1000, T=1000, n_rec=2, m=3, q=4, h=P, n_taps=81, y=P, y_rec_stride=750, y_ld=250):
        return lib.hmv_decimate_fir_f64(x, rec_stride, ld, T, n_rec, m, q, h, n_taps, y, y_rec_stride, y_ld, None)

    for kw, code, text in (
            (dict(q=1), -1, b"decimation factor"), (dict(q=33), -1, b"decimation factor"),
            (dict(n_taps=80), -2, b"taps"), (dict(n_taps=1), -2, b"taps"), (dict(n_taps=643), -2, b"taps"),
            (dict(T=0), -3, b"count"), (dict(n_rec=-1), -3, b"count"), (dict(m=0), -3, b"count"),
            (dict(x=None), -4, b"null pointer"), (dict(h=None), -4, b"null pointer"), (dict(y=None), -4, b"null pointer"),
            (dict(ld=999), -5, b"ld is smaller"),
            (dict(y_ld=249), -6, b"y_ld is smaller"), (dict(T=1001, ld=1001, y_ld=250), -6, b"y_ld is smaller"),
            (dict(T=(1 << 40) + 1, ld=1 << 41, y_ld=1 << 40), -7, b"2^40")):
        assert call(**kw) == code, kw
        assert text in lib.hmv_last_error(), (kw, lib.hmv_last_error())
    # nothing to do is not an error, even with null pointers
    assert call(n_rec=0) == 0 and call(n_rec=0, x=None, h=None, y=None) == 0
    # ... but a bad factor is refused first
    assert call(n_rec=0, q=64) == -1


def test_escan_batch_decimate_argument_checks():
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    assert EB.resolve_decimate(None) is None and EB.resolve_decimate(None, "nonsense") is None
    assert EB.resolve_decimate(4) == (4, "decimate") and EB.resolve_decimate(np.int64(2), "resample_poly") == (2, "resample_poly")
    assert EB.resolve_decimate(3, np.array([0.25, 0.5, 0.25])) == (3, "taps")
    for bad, design in ((1, "decimate"), (33, "decimate"), (4.0, "decimate"), (True, "decimate"), ("4", "decimate"),
                        (4, "iir"), (4, np.ones(4))):
        with pytest.raises(ValueError):
            EB.resolve_decimate(bad, design)
    # 8 channels, 2 s windows, 500 Hz -> 125 Hz: 250 samples against 8 x 8 = 64 unknowns
    assert EB.decimated_segment(4, 500.0, 2.0, 8, 8, np.arange(1.0, 62.5, 0.5)) == (125.0, 250)
    assert EB.decimated_segment(4, 500.0, 2.0, 8, 8, None) == (125.0, 250)
    # a requested frequency must lie below the new Nyquist rate fs / (2 q)
    with pytest.raises(ValueError, match="Nyquist"):
        EB.decimated_segment(4, 500.0, 2.0, 8, 8, np.arange(1.0, 63.0, 0.5))          # reaches 62.5 Hz exactly
    with pytest.raises(ValueError, match="Nyquist"):
        EB.decimated_segment(4, 500.0, 2.0, 8, 8, [10.0, 100.0])
    # the rank trap: 64 channels at order 8 have 512 unknowns per row, a 2 s window at 125 Hz 250 samples
    with pytest.raises(ValueError, match="rank") as ei:
        EB.decimated_segment(4, 500.0, 2.0, 64, 8, np.arange(1.0, 45.0))
    assert "lower model order" in str(ei.value) and "512" in str(ei.value) and "250" in str(ei.value)
    with pytest.raises(ValueError, match="rank"):
        EB.decimated_segment(2, 500.0, 1.0, 25, 10, None)                              # exactly as many samples: still refused
    assert EB.decimated_segment(4, 500.0, 2.0, 64, 2, np.arange(1.0, 45.0)) == (125.0, 250)
    assert issubclass(EB.DecimateConfigError, ValueError)
