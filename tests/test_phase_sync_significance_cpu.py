"""The null tests of phase synchrony without a GPU: the new C entry in the header and the ctypes table with its refusals
before any launch, the commutation of the analytic signal with a circular shift that the shift null rests on, the planted
dyad through the NumPy restatement of the whole test, and the host argument checks and planners."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import phase_sync_restated as PR
from tests import phase_sync_significance_restated as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
ENTRY = "hmv_phase_sync_pairs_c128"


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


@pytest.fixture(scope="module")
def planted():
    """seed -> (x, z of the 8 - 12 Hz band by the restatement, the band response)."""
    from hyperscanning_signal_analysis_amd.eeg_io import band_response
    out = {}
    for seed in (0, 1, 2):
        x, fs = PR.planted_dyad(seed)
        resp = band_response(x.shape[1], fs, *PR.BAND)
        out[seed] = (x, PR.analytic_restated(x, resp), resp)
    return out


def test_header_and_table(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", code)
    assert proto and len(proto.group(1).split(",")) == 20
    assert ENTRY in _lib.SIGNATURES and len(_lib.SIGNATURES[ENTRY][1]) == 20
    assert hasattr(lib, ENTRY)


def test_refusals_without_gpu(lib):
    """Every refusal of the entry has its code and text and comes before any launch (no GPU here); the pointers are never
    dereferenced on the host."""
    P = 4096                                                     # a non-null, 16-byte aligned "device pointer"

    def call(z=P, rec_stride=8000, ld=1000, T=1000, n_rec=2, m=8, split=4, rec_a=P, rec_b=P, item_start=P, shift_b=P, n_items=5,
             n=100, mode=0, values=P, val_stride=4, col_mag=0, col_lagged=1, info=P):
        return getattr(lib, ENTRY)(z, rec_stride, ld, T, n_rec, m, split, rec_a, rec_b, item_start, shift_b, n_items, n, mode,
                                   values, val_stride, col_mag, col_lagged, info, None)

    cases = (
        (dict(m=0), -1, b"channel count"), (dict(m=65, rec_stride=65000, split=32), -1, b"channel count"),
        (dict(n=0), -2, b"window length"), (dict(n=1001), -2, b"window length"),
        (dict(T=0, ld=0), -3, b"count"), (dict(n_rec=-1), -3, b"count"), (dict(n_items=-1), -3, b"count"),
        (dict(n_items=1 << 31), -10, b"items"),
        (dict(mode=2), -7, b"mode"), (dict(mode=-1), -7, b"mode"),
        (dict(ld=999), -5, b"ld is smaller"), (dict(rec_stride=7999), -6, b"rec_stride is smaller"),
        (dict(ld=1 << 58, rec_stride=(1 << 63) - 1, m=64, split=32), -6, b"rec_stride is smaller"),
        (dict(z=None), -4, b"null pointer"), (dict(rec_a=None), -4, b"null pointer"), (dict(rec_b=None), -4, b"null pointer"),
        (dict(item_start=None), -4, b"null pointer"), (dict(values=None), -4, b"null pointer"),
        (dict(info=None), -4, b"null pointer"),
        (dict(z=P + 8), -8, b"16-byte aligned"),
        (dict(split=0), -11, b"split"), (dict(split=8), -11, b"split"), (dict(split=-3), -11, b"split"),
        (dict(m=1, split=1), -11, b"split"),
        (dict(val_stride=0), -12, b"val_stride"), (dict(col_mag=4), -12, b"val_stride"), (dict(col_lagged=-2), -12, b"val_stride"),
        (dict(col_mag=-1, col_lagged=-1), -12, b"val_stride"), (dict(col_mag=2, col_lagged=2), -12, b"val_stride"))
    for kw, code, text in cases:
        assert call(**kw) == code, kw
        err = lib.hmv_last_error()
        assert text in err and err.startswith(ENTRY.encode() + b": "), (kw, err)
    assert {code for _, code, _ in cases} == {-1, -2, -3, -10, -7, -5, -6, -4, -8, -11, -12}
    # nothing to do is not an error, even with null pointers; a missing shift table is a shift of 0, not an error ...
    assert call(n_items=0) == 0
    assert call(n_items=0, z=None, rec_a=None, rec_b=None, item_start=None, shift_b=None, values=None, info=None) == 0
    # ... but bad arguments are refused first
    assert call(n_items=0, mode=3) == -7 and call(n_items=0, split=8) == -11 and call(n_items=0, col_mag=1) == -12
    # one column is enough, in either place
    assert call(n_items=0, col_mag=-1, col_lagged=0, val_stride=1) == 0 and call(n_items=0, col_mag=3, col_lagged=-1) == 0


def test_analytic_signal_commutes_with_a_circular_shift(planted):
    """analytic(roll(x, -d)) against roll(analytic(x), -d): at most 1e-13 of each row's largest |z| apart (measured 1.2e-15
    to 1.4e-15 at d = 3333).  Printed: the worst ratio."""
    worst = 0.0
    for seed, (x, z, resp) in planted.items():
        T = x.shape[1]
        for d in (1, 3333, T - 1):
            a, b = PR.analytic_restated(np.roll(x, -d, axis=-1), resp), np.roll(z, -d, axis=-1)
            rel = np.abs(a - b).max(axis=-1) / np.abs(z).max(axis=-1)
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-13, (seed, d, rel)
    print(f"worst |analytic(roll x) - roll(analytic x)| / max |z| per row = {worst:.3g}")


def test_planted_dyad_on_the_restatement(planted):
    """Split 4, S = 19, 8 - 12 Hz, the 16 windows of 2500 samples: the lagged pair (0, 5) reaches the smallest possible p in
    every window for all four measures, the zero-lag pair (2, 6) for PLV and coherence, and nothing else is significant
    family-wise."""
    from hyperscanning_signal_analysis_amd import surrogates as sg
    S, split = 19, 4
    for seed, (x, z, _) in planted.items():
        d = sg.shift_offsets(np.random.default_rng(100 + seed), S, 1, x.shape[1], PR.WINDOW)[:, 0]
        res = SR.shift_test(z, PR.STARTS, PR.WINDOW, split, d, SR.MEASURES)
        SR.check_planted_significance(res["p"], res["p_fwe"], res["n_valid"], S, seed)


def test_restated_null_statistics():
    """The restatement's own rules: a bad surrogate is left out of everything, a NaN value out of its cell only."""
    rng = np.random.default_rng(4)
    tested = SR.tested_mask(4, 2)
    obs = rng.random((3, 4, 4, 2))
    surr = rng.random((5, 3, 4, 4, 2))
    surr[2, 1, 0, 3, 0] = np.nan
    bad = np.zeros((5, 3), dtype=bool)
    bad[4, 2] = True
    out = SR.null_stats(obs, surr, tested, bad)
    assert out["n_valid"].tolist() == [5, 5, 4]
    assert np.isnan(out["p"][:, ~tested]).all() and np.isfinite(out["p"][:, tested]).all()
    v = surr[[0, 1, 3, 4], 1, 0, 3, 0]
    assert out["p"][1, 0, 3, 0] == (1.0 + (v >= obs[1, 0, 3, 0]).sum()) / 6.0
    assert np.isclose(out["null_mean"][1, 0, 3, 0], v.mean()) and np.isclose(out["null_std"][1, 0, 3, 0], v.std(ddof=1))
    v = surr[:4, 2, 1, 2, 1]
    assert out["p"][2, 1, 2, 1] == (1.0 + (v >= obs[2, 1, 2, 1]).sum()) / 5.0
    M = surr[:4, 2][:, tested][..., 1].max(axis=1)
    assert out["p_fwe"][2, 1, 2, 1] == (1.0 + (M >= obs[2, 1, 2, 1]).sum()) / 5.0


def test_argument_checks_and_planners(tmp_path):
    """`phase_significance_args` / `phase_pseudo_dyad_args` refuse before anything is drawn or launched, the sliding calls
    refuse before an engine exists (there is no GPU here to make one on), and the planners used are the integer ones."""
    from hyperscanning_signal_analysis_amd import _lib, significance, sliding
    from hyperscanning_signal_analysis_amd import surrogates as sg
    ok = dict(measures=("plv", "imcoh"), n_surrogates=19, m=8, T=12000, n=2500)
    assert sg.phase_significance_args(**ok) == (("plv", "imcoh"), 19, 4, 2500)
    assert sg.phase_significance_args(**dict(ok, measures="coh", split=3, min_shift=0, check="nan")) == (("coh",), 19, 3, 0)
    for kw, text in ((dict(measures=("plv", "wpli")), "measures"), (dict(measures=()), "measures"),
                     (dict(n_surrogates=0), "n_surrogates"), (dict(n_surrogates=2.5), "n_surrogates"),
                     (dict(m=7), "odd channel count"), (dict(split=0), "split"), (dict(split=8), "split"),
                     (dict(split=True), "split"), (dict(min_shift=-1), "min_shift"), (dict(T=4999), "2 min_shift"),
                     (dict(min_shift=6001), "2 min_shift"), (dict(check="mask"), "check")):
        with pytest.raises(ValueError, match=text):
            sg.phase_significance_args(**dict(ok, **kw))
    okd = dict(measures=("ciplv",), D=3, m=8, n_surrogates=None, seed=None)
    assert sg.phase_pseudo_dyad_args(**okd) == (("ciplv",), None, 4)
    assert sg.phase_pseudo_dyad_args(**dict(okd, n_surrogates=7, seed=1, split=5)) == (("ciplv",), 7, 5)
    for kw, text in ((dict(measures=("dtf",)), "measures"), (dict(D=1), "at least 2 dyads"), (dict(n_surrogates=4), "need a seed"),
                     (dict(n_surrogates=0, seed=1), "n_surrogates"), (dict(m=5), "odd channel count"), (dict(split=8), "split"),
                     (dict(check=False), "check")):
        with pytest.raises(ValueError, match=text):
            sg.phase_pseudo_dyad_args(**dict(okd, **kw))
    # the calls that fill the value columns: one per mode in use, -1 for a measure that was not asked for
    assert significance.phase_calls(("plv", "ciplv", "coh", "imcoh")) == [(_lib.PHASE_UNIT, (0, 1)), (_lib.PHASE_RAW, (2, 3))]
    assert significance.phase_calls(("imcoh", "plv")) == [(_lib.PHASE_UNIT, (1, -1)), (_lib.PHASE_RAW, (-1, 0))]
    assert significance.phase_calls(("coh",)) == [(_lib.PHASE_RAW, (0, -1))]
    # surrogate blocks: whole surrogates where one fits in the chunk, else one surrogate in ranges of rows; ascending
    assert significance.sliding_plan(5, 12, 30) == (2, 12) and significance.sliding_plan(5, 12, 7) == (1, 7)
    blocks = list(significance.surrogate_blocks(5, 2, significance.window_ranges(12, 12)))
    assert blocks == [(0, 2, 0, 12, False), (2, 2, 0, 12, False), (4, 1, 0, 12, True)]
    assert significance.phase_chunk(64, 2, 8 << 30) == (2 << 30) // (8 * 64 * 64 * 2 + 64)
    assert significance.phase_chunk(64, 4, 1) == 1
    # the public calls: the arguments first
    x = np.zeros((8, 6000))
    for kw, text in ((dict(measures=("plv", "wpli")), "measures"), (dict(n_surrogates=0), "n_surrogates"),
                     (dict(bands_hz=()), "empty"), (dict(bands_hz=((12.0, 8.0),)), "lower edge"), (dict(split=8), "split"),
                     (dict(min_shift=3001), "2 min_shift"), (dict(check="mask"), "check")):
        with pytest.raises(ValueError, match=text):
            sliding.sliding_phase_sync_significance(x, 2500, 3, 250.0, **dict(dict(n_surrogates=5, seed=0), **kw))
    with pytest.raises(ValueError, match="odd channel count"):
        sliding.sliding_phase_sync_significance(x[:7], 2500, 3, 250.0, n_surrogates=5, seed=0)
    xd = np.zeros((3, 8, 6000))
    for xx, kw, text in ((xd[:1], {}, "at least 2 dyads"), (xd, dict(n_surrogates=4), "need a seed"),
                         (xd[0], {}, "dyads, channels"), (xd, dict(measures=()), "measures"), (xd, dict(bands_hz=((8.0, 8.0),)), "lower edge")):
        with pytest.raises(ValueError, match=text):
            sliding.sliding_phase_sync_pseudo_dyad_significance(xx, 2500, 3, 250.0, **kw)
