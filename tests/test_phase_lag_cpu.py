"""The phase-lag family without a GPU: the NumPy restatement against a brute-force long-double evaluation of the definitions
and its bound against a sequential float64 summation, the planted dyad (zero-lag mixing cannot raise PLI and wPLI, a
pi/2-lagged coupling drives them to 1), the C ABI's refusals before any launch, and the host argument checks of the public
calls."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import phase_lag_restated as LR
from tests import phase_sync_restated as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
PLI_MEDIAN_MAX, WPLI_MEDIAN_MAX = 0.25, 0.40


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


def test_restatement_against_long_double():
    """The restatement (NumPy's own summation order) and a sequential float64 summation -- the order the kernel documents --
    against the definitions in long double, on the z of the GPU tests (all 64 channels, the five items of every window
    length): PLI equal exactly, wpli and dwpli within `lag_bound` (observed: 0.075 of it at the most), NaN in the same
    cells.  The input's sign margin is 0 pair-samples, and the smallest D / A^2 is printed (1.2e-5)."""
    z = LR.z64_recipe()
    off = ~np.eye(64, dtype=bool)
    worst, doubt, min_d = {"wpli": 0.0, "dwpli": 0.0}, 0, 1.0
    for n in (1, 2) + LR.N_CASES[1:]:
        for r, s in LR.items_for(n):
            want = LR.measures_longdouble(z[r], s, n)
            got, bound = LR.measures_restated(z[r], s, n), LR.lag_bound(z[r], s, n)
            seq = dict(zip(("wpli", "dwpli"), LR.measures_sequential(z[r], s, n)))
            assert got["info"] == 0
            assert np.array_equal(got["pli"], want[0].astype(np.float64))
            doubt += LR.sign_margin(z[r], s, n)
            for k, w in (("wpli", want[1]), ("dwpli", want[2])):
                w64 = w.astype(np.float64)
                for g in (got[k], seq[k]):
                    assert np.array_equal(np.isnan(g[off]), np.isnan(w64[off])), (k, n)
                    ok = off & np.isfinite(w64)
                    if ok.any():
                        ratio = float((np.abs(g - w)[ok] / bound[k][ok]).max())
                        worst[k] = max(worst[k], ratio)
                        assert ratio <= 1.0, (k, n, r, s, ratio)
            if n == 1:
                assert np.isnan(got["dwpli"][off]).all() and (got["wpli"][off] == 1.0).all() and (got["pli"][off] == 1.0).all()
            else:
                min_d = min(min_d, float((bound["D"][off] / bound["A"][off] ** 2).min()))
    print(f"worst |float64 - long double| / lag_bound: wpli {worst['wpli']:.3g}, dwpli {worst['dwpli']:.3g}; "
          f"sign-ambiguous pair-samples {doubt}; min D / A^2 {min_d:.3g}")
    assert doubt == 0 and min_d > 1e-6


def test_restated_rules():
    """Diagonal, split, duplicated / scaled / flat channels, the non-finite sample, a window past the end."""
    rng = np.random.default_rng(11)
    z = rng.standard_normal((6, 50)) + 1j * rng.standard_normal((6, 50))
    r = LR.measures_restated(z, 5, 40)
    for k in LR.MEASURES:
        assert np.array_equal(r[k], r[k].T) and not r[k].diagonal().any()
    off = ~np.eye(6, dtype=bool)
    assert r["info"] == 0 and (r["wpli"][off] <= 1.0).all() and (r["pli"][off] <= 1.0).all() and (r["dwpli"][off] <= 1.0).all()
    s = LR.measures_restated(z, 5, 40, split=2)
    done = LR.computed_pairs(6, 2)
    assert done.sum() == 2 * 2 * 4 and s["info"] == 0
    for k in LR.MEASURES:
        assert np.array_equal(s[k][done], r[k][done]) and np.isnan(s[k][off & ~done]).all() and not s[k].diagonal().any()
    z[3] = 4.0 * z[1]                                              # proportional by a power of two: x = 0 exactly
    z[5] = 0.0
    d = LR.measures_restated(z, 5, 40)
    assert d["info"] == 2 and d["pli"][1, 3] == 0.0 and np.isnan(d["wpli"][1, 3]) and np.isnan(d["dwpli"][3, 1])
    assert not d["pli"][5].any() and np.isnan(d["wpli"][5, :5]).all() and np.isfinite(d["wpli"][:3, :3]).all()
    assert LR.sign_margin(z, 5, 40) > 0
    assert LR.measures_restated(z[:3], 5, 40)["info"] == 0
    assert LR.measures_restated(z, 5, 40, split=5)["info"] == 2 and LR.measures_restated(z[:5], 5, 40, split=1)["info"] == 0
    z[0, 7] = np.inf
    bad = LR.measures_restated(z, 5, 40)
    assert bad["info"] == 1 and all(np.isnan(bad[k]).all() for k in LR.MEASURES)
    assert LR.measures_restated(z, 8, 40)["info"] == 2
    past = LR.x_restated(z[:3], 30, 40)
    assert past.shape == (3, 3, 40) and not past[..., 20:].any()


def test_planted_dyad_zero_lag_mixing_does_not_raise_the_lag_family():
    """The planted dyad of the phase-synchrony tests, band 8 - 12 Hz, the 16 interior windows, seeds 0, 1, 2.
    (0, 5), pi/2-lagged: pli, wpli and dwpli > 0.95 in every window (observed: 1.0000 in every window).
    (2, 6), zero-lag mixing: PLV > 0.9 in every window (observed >= 0.948), yet the median over the windows of pli is below
    0.25 and of wpli below 0.40.  Observed medians per seed: pli 0.124, 0.142, 0.160; wpli 0.253, 0.223, 0.198; worst single
    window pli 0.309, wpli 0.548.  The thresholds are medians because uncoupled pairs of this narrow band reach wpli 0.73
    in single windows; they sit midway between what chance gives and what the measure would have to reach to pass for a
    coupling (PLV there is above 0.9)."""
    from hyperscanning_signal_analysis_amd.eeg_io import band_response
    for seed in (0, 1, 2):
        x, fs = PR.planted_dyad(seed)
        z = PR.analytic_restated(x, band_response(x.shape[1], fs, *PR.BAND))
        rows = []
        for s in PR.STARTS:
            r = LR.measures_restated(z, s, PR.WINDOW)
            assert r["info"] == 0
            for k in LR.MEASURES:
                assert r[k][0, 5] > 0.95, (seed, s, k, r[k][0, 5])
            assert PR.plv(z, s, PR.WINDOW)[2, 6] > 0.9
            rows.append((r["pli"][2, 6], r["wpli"][2, 6]))
        med, worst = np.median(rows, axis=0), np.max(rows, axis=0)
        print(f"seed {seed}: (2, 6) median pli {med[0]:.3f} wpli {med[1]:.3f}; worst window pli {worst[0]:.3f} wpli {worst[1]:.3f}")
        assert med[0] < PLI_MEDIAN_MAX and med[1] < WPLI_MEDIAN_MAX, (seed, med)


def test_header_and_table(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.search(r"\bint\s+hmv_phase_lag_c128\s*\(([^)]*)\)", code)
    assert found and len(found.group(1).split(",")) == 16
    assert "hmv_phase_lag_c128" in _lib.SIGNATURES and len(_lib.SIGNATURES["hmv_phase_lag_c128"][1]) == 16
    assert hasattr(lib, "hmv_phase_lag_c128")
    assert "Stam" in hdr and "Vinck" in hdr and "NOT A FUNCTION OF THE REFERENCE" in hdr
    assert not any(s.startswith("hmv_sliding_") and "phase" in s for s in _lib.SIGNATURES)


def test_refusals_without_gpu(lib):
    """Every refusal of hmv_phase_lag_c128 has its own code and text and comes before any launch (no GPU here); the
    pointers are never dereferenced on the host."""
    P = 4096                                                     # a non-null, 16-byte aligned "device pointer"

    def call(z=P, rec_stride=8000, ld=1000, T=1000, n_rec=2, m=8, split=0, item_rec=P, item_start=P, n_items=5, n=100,
             pli=P, wpli=P, dwpli=P, info=P):
        return lib.hmv_phase_lag_c128(z, rec_stride, ld, T, n_rec, m, split, item_rec, item_start, n_items, n, pli, wpli, dwpli,
                                      info, None)

    cases = (
        (dict(m=0), -1, b"channel count"), (dict(m=65, rec_stride=65000), -1, b"channel count"),
        (dict(n=0), -2, b"window length"), (dict(n=1001), -2, b"window length"),
        (dict(T=0, ld=0), -3, b"count"), (dict(n_rec=-1), -3, b"count"), (dict(n_items=-1), -3, b"count"),
        (dict(z=None), -4, b"null pointer"), (dict(item_rec=None), -4, b"null pointer"),
        (dict(item_start=None), -4, b"null pointer"), (dict(info=None), -4, b"null pointer"),
        (dict(z=P + 8), -8, b"16-byte aligned"),
        (dict(ld=999), -5, b"ld is smaller"), (dict(rec_stride=7999), -6, b"rec_stride is smaller"),
        (dict(pli=None, wpli=None, dwpli=None), -9, b"no output"),
        (dict(n_items=1 << 31), -10, b"items"),
        (dict(split=-1), -11, b"split"), (dict(split=8), -11, b"split"), (dict(m=1, split=1), -11, b"split"))
    for kw, code, text in cases:
        assert call(**kw) == code, kw
        err = lib.hmv_last_error()
        assert text in err and err.startswith(b"hmv_phase_lag_c128: "), (kw, err)
    assert len({code for _, code, _ in cases}) == 10
    # nothing to do is not an error, even with null pointers ...
    assert call(n_items=0) == 0 and call(n_items=0, z=None, item_rec=None, item_start=None, info=None) == 0
    assert call(n_items=0, split=7) == 0 and call(n_items=0, m=1) == 0
    # ... but bad arguments are refused first
    assert call(n_items=0, split=9) == -11 and call(n_items=0, m=65) == -1
    # any one output is enough
    for keep in ("pli", "wpli", "dwpli"):
        kw = {k: None for k in ("pli", "wpli", "dwpli") if k != keep}
        assert call(n_items=0, **kw) == 0


def test_host_argument_checks_come_before_any_device(tmp_path):
    """Unknown measures, a bad split and bad bands raise from `sliding.sliding_phase_lag` and `escan_batch.run(phase_lag=...)`
    before an engine exists (there is no GPU here to make one on); the synchrony family keeps refusing the new names."""
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd import sliding
    from hyperscanning_signal_analysis_amd.eeg_io import (PHASE_LAG_MEASURES, PHASE_MEASURES, resolve_phase_lag_measures,
                                                          resolve_phase_measures)
    assert PHASE_LAG_MEASURES == ("pli", "wpli", "dwpli") and PHASE_MEASURES == ("plv", "ciplv", "coh", "imcoh")
    assert resolve_phase_lag_measures("wpli") == ("wpli",)
    assert resolve_phase_lag_measures(["dwpli", "pli", "dwpli"]) == ("dwpli", "pli")
    with pytest.raises(ValueError, match="measures"):
        resolve_phase_measures(("plv", "wpli"))
    x = np.zeros((3, 2000))
    for kw, text in ((dict(measures=("wpli", "plv")), "measures"), (dict(measures=()), "measures"),
                     (dict(measures=("wPLI",)), "measures"),
                     (dict(split=3), "split"), (dict(split=-1), "split"), (dict(split=1.0), "split"), (dict(split=True), "split"),
                     (dict(bands_hz=()), "empty"), (dict(bands_hz=((12.0, 8.0),)), "lower edge"),
                     (dict(bands_hz=((130.0, 140.0),)), "lower edge"), (dict(bands_hz=(8.0, 12.0)), "pairs"),
                     (dict(check="mask"), "check")):
        with pytest.raises(ValueError, match=text):
            sliding.sliding_phase_lag(x, 500, 3, 250.0, **kw)
    with pytest.raises(ValueError, match="x must be"):
        sliding.sliding_phase_lag(np.zeros(2000), 500, 3, 250.0)
    for kw, text in ((dict(phase_lag=("wpli", "plv")), "measures"), (dict(phase_lag=()), "measures"),
                     (dict(phase_lag=("wpli",), bands=()), "empty"), (dict(phase_lag=("pli",), bands=((12.0, 8.0),)), "lower edge"),
                     (dict(phase_sync=("plv", "wpli")), "measures"),
                     (dict(phase_sync=("plv", "wpli"), phase_lag=("wpli",)), "measures")):
        with pytest.raises(ValueError, match=text):
            EB.run(tmp_path / "no_such_tree", tmp_path / "out", **kw)
    with pytest.raises(ValueError, match="measures"):
        sliding.sliding_phase_sync(x, 500, 3, 250.0, measures=("plv", "wpli"))
    assert not (tmp_path / "out").exists()
    stub = types.SimpleNamespace(pivoted_yw=False)
    cfg, _ = EB.resolve_settings(stub, model_order=3, phase_lag=["wpli", "pli", "wpli"])
    assert cfg.phase_lag == ("wpli", "pli") and cfg.phase_sync is None
    assert EB.resolve_settings(stub, model_order=3)[0].phase_lag is None
