"""Phase synchrony without a GPU: `eeg_io.band_response` against SciPy, the frequency-domain definition against the
`sosfiltfilt` + `hilbert` chain away from the ends, the planted couplings on the NumPy restatement, the C ABI's refusals
before any launch, and the host argument checks of the public calls."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import phase_sync_restated as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


@pytest.fixture(scope="module")
def planted():
    """seed -> (x, z of the 8 - 12 Hz band by the restatement), made once for the tests that share them."""
    from hyperscanning_signal_analysis_amd.eeg_io import band_response
    out = {}
    for seed in (0, 1, 2):
        x, fs = PR.planted_dyad(seed)
        out[seed] = (x, PR.analytic_restated(x, band_response(x.shape[1], fs, *PR.BAND)))
    return out


def _hilbert_weights(T):
    w = np.zeros(T)
    w[0] = 1.0
    w[1:(T + 1) // 2] = 2.0
    if T % 2 == 0:
        w[T // 2] = 1.0
    return w


def test_band_response_is_the_squared_butterworth_times_the_hilbert_weights():
    from scipy.signal import butter, sosfreqz
    from hyperscanning_signal_analysis_amd.eeg_io import band_response
    for T, fs, lo, hi, order in ((1000, 250.0, 8.0, 12.0, 4), (997, 250.0, 0.5, 4.0, 4), (4096, 500.0, 13.0, 30.0, 2),
                                 (30011, 250.0, 30.0, 100.0, 6)):
        resp = band_response(T, fs, lo, hi, order)
        assert resp.shape == (T,) and resp.dtype == np.float64
        f = np.abs(np.fft.fftfreq(T, 1.0 / fs))
        sos = butter(order, np.array([lo, hi]) / (fs / 2.0), btype="band", output="sos")
        _, h = sosfreqz(sos, worN=2.0 * np.pi * f / fs)
        assert np.array_equal(resp, np.abs(h) ** 2 * _hilbert_weights(T))
        assert not resp[T // 2 + 1:].any()               # nothing on the negative frequencies (k = T / 2 is Nyquist)
        assert resp.max() <= 2.0 * (1.0 + 1e-12) and resp[np.argmin(np.abs(f - np.sqrt(lo * hi)))] > 1.9
    # the edges 0 and fs / 2: a missing edge is a low-pass or a high-pass
    T, fs = 1000, 250.0
    f = np.abs(np.fft.fftfreq(T, 1.0 / fs))
    _, h_lo = sosfreqz(butter(4, 30.0 / 125.0, btype="low", output="sos"), worN=2.0 * np.pi * f / fs)
    _, h_hi = sosfreqz(butter(4, 30.0 / 125.0, btype="high", output="sos"), worN=2.0 * np.pi * f / fs)
    for lo in (None, 0.0, -1.0):
        assert np.array_equal(band_response(T, fs, lo, 30.0), np.abs(h_lo) ** 2 * _hilbert_weights(T))
    for hi in (None, 125.0, 128.5):                              # DEFAULT_BANDS' gamma edge at fs = 250
        assert np.array_equal(band_response(T, fs, 30.0, hi), np.abs(h_hi) ** 2 * _hilbert_weights(T))
    for T in (1, 2, 7, 8):
        assert np.array_equal(band_response(T, fs), _hilbert_weights(T))
        assert np.array_equal(band_response(T, fs, 0.0, 125.0), _hilbert_weights(T))
    for lo, hi in ((12.0, 8.0), (8.0, 8.0), (130.0, None), (None, -3.0), (float("nan"), 8.0)):
        with pytest.raises(ValueError, match="band_response"):
            band_response(1000, 250.0, lo, hi)
    with pytest.raises(ValueError, match="band_response"):
        band_response(0, 250.0, 8.0, 12.0)


def test_weights_alone_are_scipys_hilbert():
    """resp = w reproduces scipy.signal.hilbert through the restatement to the float64 FFT's own error, 8 eps log2(T)
    relative L2 (observed 4 - 9e-16 for T between 997 and 30011)."""
    from scipy.signal import hilbert
    from hyperscanning_signal_analysis_amd.eeg_io import band_response
    rng = np.random.default_rng(5)
    for T in (997, 1000, 4096, 30011):
        x = 50e-6 * rng.standard_normal((3, T))
        z, want = PR.analytic_restated(x, band_response(T, 250.0)), hilbert(x, axis=-1)
        err = np.linalg.norm(z - want, axis=-1) / np.linalg.norm(want, axis=-1)
        print(f"T={T}: relative L2 |restated - hilbert| = {err.max():.3g} (bound {8 * PR.EPS * np.log2(T):.3g})")
        assert err.max() <= 8 * PR.EPS * np.log2(T)


def test_definition_against_sosfiltfilt_and_hilbert(planted):
    """PLV of the frequency-domain definition against PLV of hilbert(sosfiltfilt(sos, x)) in the 16 interior windows of
    the planted dyad: at most 1e-3 apart (the Butterworth transient of the two edge conventions, not rounding; measured
    3.04e-4 at the most over seeds 0..7).  Printed: the worst value."""
    from scipy.signal import butter, hilbert, sosfiltfilt
    sos = butter(4, np.array(PR.BAND) / (PR.FS / 2.0), btype="band", output="sos")
    worst = 0.0
    for seed, (x, z) in planted.items():
        zs = hilbert(sosfiltfilt(sos, x, axis=-1), axis=-1)
        for s in PR.STARTS:
            worst = max(worst, float(np.abs(PR.plv(z, s, PR.WINDOW) - PR.plv(zs, s, PR.WINDOW)).max()))
    print(f"worst | |R| - |R_scipy| | = {worst:.3g}")
    assert worst <= 1e-3


def test_planted_couplings_on_the_restatement(planted):
    worst = 0.0
    for seed, (x, z) in planted.items():
        for s in PR.STARTS:
            worst = max(worst, PR.check_planted(PR.plv(z, s, PR.WINDOW), PR.ciplv(z, s, PR.WINDOW)))
    print(f"largest PLV outside the planted pairs: {worst:.3f}")


def test_restated_measures_rules():
    """The restatement itself: diagonal and den rules, the zero channel, the non-finite sample."""
    rng = np.random.default_rng(11)
    z = rng.standard_normal((4, 50)) + 1j * rng.standard_normal((4, 50))
    z[3] = 0.0
    u = PR.measures_restated(z, 5, 40, PR.UNIT)
    assert u["info"] == 0 and np.array_equal(u["mag"].diagonal(), [1, 1, 1, 0]) and not u["lagged"].diagonal().any()
    assert not u["mag"][3].any() and not u["lagged"][3].any() and np.array_equal(u["mag"], u["mag"].T)
    assert np.array_equal(u["coherency"][1], -u["coherency"][1].T)
    r = PR.measures_restated(z, 5, 40, PR.RAW)
    assert r["info"] == 2 and np.isnan(r["mag"][3]).all() and np.isnan(r["mag"][:, 3]).all() and np.isfinite(r["mag"][:3, :3]).all()
    z[1, 7] = np.nan
    assert PR.measures_restated(z, 5, 40, PR.UNIT)["info"] == 1 and np.isnan(PR.measures_restated(z, 5, 40, PR.RAW)["mag"]).all()
    assert PR.measures_restated(z, 8, 40, PR.UNIT)["info"] == 0
    one = PR.measures_restated(z[:3], 8, 1, PR.UNIT)                          # n = 1: |R| = 1, den = Im^2
    assert np.allclose(one["mag"], 1.0) and np.allclose(one["lagged"][0, 1], 1.0, atol=1e-6)


def test_header_and_table(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    assert f"#define HMV_PHASE_UNIT {_lib.PHASE_UNIT}\n" in hdr and f"#define HMV_PHASE_RAW  {_lib.PHASE_RAW}\n" in hdr
    assert (_lib.PHASE_UNIT, _lib.PHASE_RAW) == (PR.UNIT, PR.RAW) == (0, 1)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+hmv_phase_sync_c128\s*\(", code)
    assert "hmv_phase_sync_c128" in _lib.SIGNATURES and len(_lib.SIGNATURES["hmv_phase_sync_c128"][1]) == 16
    assert hasattr(lib, "hmv_phase_sync_c128")
    assert not any(s.startswith("hmv_sliding_") and "phase" in s for s in _lib.SIGNATURES)


def test_refusals_without_gpu(lib):
    """Every refusal of hmv_phase_sync_c128 has its own code and text and comes before any launch (no GPU here); the
    pointers are never dereferenced on the host."""
    P = 4096                                                     # a non-null, 16-byte aligned "device pointer"

    def call(z=P, rec_stride=8000, ld=1000, T=1000, n_rec=2, m=8, item_rec=P, item_start=P, n_items=5, n=100, mode=0,
             coherency=P, mag=P, lagged=P, info=P):
        return lib.hmv_phase_sync_c128(z, rec_stride, ld, T, n_rec, m, item_rec, item_start, n_items, n, mode, coherency, mag,
                                       lagged, info, None)

    cases = (
        (dict(m=0), -1, b"channel count"), (dict(m=65, rec_stride=65000), -1, b"channel count"),
        (dict(n=0), -2, b"window length"), (dict(n=1001), -2, b"window length"),
        (dict(T=0, ld=0), -3, b"count"), (dict(n_rec=-1), -3, b"count"), (dict(n_items=-1), -3, b"count"),
        (dict(z=None), -4, b"null pointer"), (dict(item_rec=None), -4, b"null pointer"),
        (dict(item_start=None), -4, b"null pointer"), (dict(info=None), -4, b"null pointer"),
        (dict(z=P + 8), -8, b"16-byte aligned"),
        (dict(ld=999), -5, b"ld is smaller"), (dict(rec_stride=7999), -6, b"rec_stride is smaller"),
        (dict(mode=2), -7, b"mode"), (dict(mode=-1), -7, b"mode"),
        (dict(coherency=None, mag=None, lagged=None), -9, b"no output"),
        (dict(n_items=1 << 31), -10, b"items"))
    for kw, code, text in cases:
        assert call(**kw) == code, kw
        err = lib.hmv_last_error()
        assert text in err and err.startswith(b"hmv_phase_sync_c128: "), (kw, err)
    assert len({code for _, code, _ in cases}) == 10
    # nothing to do is not an error, even with null pointers ...
    assert call(n_items=0) == 0 and call(n_items=0, z=None, item_rec=None, item_start=None, info=None) == 0
    # ... but bad arguments are refused first
    assert call(n_items=0, mode=3) == -7 and call(n_items=0, m=65) == -1
    # any one output is enough
    for keep in ("coherency", "mag", "lagged"):
        kw = {k: None for k in ("coherency", "mag", "lagged") if k != keep}
        assert call(n_items=0, **kw) == 0


def test_host_argument_checks_come_before_any_device(tmp_path):
    """An unknown measure, an empty band list and lo >= hi raise from `sliding.sliding_phase_sync` and
    `escan_batch.run(phase_sync=...)` before an engine exists (there is no GPU here to make one on)."""
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd import sliding
    from hyperscanning_signal_analysis_amd.eeg_io import PHASE_MEASURES, resolve_bands_hz, resolve_phase_measures
    assert PHASE_MEASURES == ("plv", "ciplv", "coh", "imcoh")
    assert resolve_phase_measures("plv") == ("plv",) and resolve_phase_measures(["coh", "plv", "coh"]) == ("coh", "plv")
    assert resolve_bands_hz(((0.5, 4.0), (30.0, 128.5), (None, 8.0), (0, 200)), 250.0) == ((0.5, 4.0), (30.0, None), (None, 8.0),
                                                                                          (None, None))
    x = np.zeros((3, 2000))
    for kw, text in ((dict(measures=("plv", "wpli")), "measures"), (dict(measures=()), "measures"),
                     (dict(bands_hz=()), "empty"), (dict(bands_hz=((12.0, 8.0),)), "lower edge"),
                     (dict(bands_hz=((8.0, 8.0),)), "lower edge"), (dict(bands_hz=((130.0, 140.0),)), "lower edge"),
                     (dict(bands_hz=(8.0, 12.0)), "pairs"), (dict(check="mask"), "check")):
        with pytest.raises(ValueError, match=text):
            sliding.sliding_phase_sync(x, 500, 3, 250.0, **kw)
    for kw, text in ((dict(phase_sync=("plv", "wpli")), "measures"), (dict(phase_sync=()), "measures"),
                     (dict(phase_sync=("plv",), bands=()), "empty"), (dict(phase_sync=("plv",), bands=((12.0, 8.0),)), "lower edge")):
        with pytest.raises(ValueError, match=text):
            EB.run(tmp_path / "no_such_tree", tmp_path / "out", **kw)
    assert not (tmp_path / "out").exists()
