"""CPU-side checks of the per-window automatic model order: the new C-ABI entries are declared, bound and refuse bad
arguments before anything touches a GPU; the Python layer refuses bad arguments before it touches one; the penalty
formulas are the reference's; and the mixed-order workload of the GPU tests really needs a selection.

The workload (`synthetic.mixed_order_recording(100, m, orders, seg)`, windows every `hop` samples), as the oracle's
`mvar_criterion` sees it -- re-derived by `test_workload_needs_a_selection` below:

    m   n     hop  pmax  crit  orders            seg   windows  picked per order 1, 2, ...                  smallest gap
    4   160   80   20    AIC   [1,2,3,5,8,12]    1600  119      35, 20, 23, 0, 18, 0, 0, 19, 1, 0, 0, 3     1.7e-3
    4   160   80   20    HQ    same              1600  119      75, 20, 19, 0, 5                            2.6e-3
    4   160   80   20    SC    same              1600  119      83, 20, 16                                  1.6e-2
    19  1000  500  12    AIC   [1,2,4,6,9]       6000  59       11, 11, 1, 12, 0, 12, 0, 0, 12              3.6e-3
    32  1000  500  10    AIC   [1,3,5,8]         5000  39       10, 0, 10, 0, 10, 0, 0, 9                   0.13
    64  1000  500  8     AIC   [1,2,4,6]         4000  31       9, 8, 0, 7, 0, 5, 0, 2                      3.1e-2

(gap: best criterion value against the runner-up of the same window; every criterion value is finite).  The GPU tests
accept a different order only for a window whose gap is below 1e-6; this workload has none."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import mvar_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")

# (m, n, hop, pmax, crit, orders, seg, picked per order) -- shared with tests/test_gpu_auto_order.py by value
WORKLOADS = [
    (4, 160, 80, 20, "AIC", [1, 2, 3, 5, 8, 12], 1600, [35, 20, 23, 0, 18, 0, 0, 19, 1, 0, 0, 3]),
    (4, 160, 80, 20, "HQ", [1, 2, 3, 5, 8, 12], 1600, [75, 20, 19, 0, 5]),
    (4, 160, 80, 20, "SC", [1, 2, 3, 5, 8, 12], 1600, [83, 20, 16]),
    (19, 1000, 500, 12, "AIC", [1, 2, 4, 6, 9], 6000, [11, 11, 1, 12, 0, 12, 0, 0, 12]),
    (32, 1000, 500, 10, "AIC", [1, 3, 5, 8], 5000, [10, 0, 10, 0, 10, 0, 0, 9]),
    (64, 1000, 500, 8, "AIC", [1, 2, 4, 6], 4000, [9, 8, 0, 7, 0, 5, 0, 2]),
]
GAP = 1e-6


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


P = 0x1000          # a fake non-zero device address: the checks must refuse before any pointer is read


def test_header_and_ctypes_table_agree_on_the_new_entries(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    assert int(re.search(r"#define HMV_VERSION (\d+)", hdr).group(1)) == 160 == lib.hmv_version()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("hmv_yw_solve_auto_f64", "hmv_sliding_auto_workspace_bytes", "hmv_sliding_auto_f64"):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name)
    for k, v in (("FFDTF", 0), ("DDTF", 1), ("GPDC", 2)):
        assert re.search(r"#define HMV_MEASURE_%s %d\b" % (k, v), hdr)
        assert getattr(_lib, "MEASURE_" + k) == v
    assert _lib.CRITERIA == {"AIC": 0, "HQ": 1, "SC": 2}


def _yw(lib, m=8, pmax=5, n=100, crit=0, R=P, order=P, flags=0, items=2):
    return lib.hmv_yw_solve_auto_f64(R, items, m, pmax, n, crit, P, P, P, order, 0, 0, P, flags, 0)


def _sl(lib, measure=0, m=8, n=100, pmax=5, crit=0, F=4, out=P, nb=0, S=0, order=P, flags=0, items=2, ws=1 << 40, lo=0, hi=0,
        info_tf=P):
    return lib.hmv_sliding_auto_f64(measure, P, 1000, 1000, P, P, items, m, n, pmax, crit, P, F, 100.0, out, lo, hi, nb, S, 0,
                                    0, order, 0, P, info_tf, P, ws, 2, 1.0, flags, 0, 0, 0, 0, 0, 0)


def test_entries_refuse_bad_arguments(lib):
    cases = [
        (_yw, b"hmv_yw_solve_auto_f64", [(dict(m=0), -1, b"channel count"), (dict(m=65), -1, b"channel count"),
                                         (dict(pmax=0), -2, b"model order"), (dict(pmax=33), -2, b"model order"),
                                         (dict(n=5), -3, b"window shorter"), (dict(crit=3), -5, b"criterion"),
                                         (dict(crit=-1), -5, b"criterion"), (dict(flags=2), -6, b"LDL"),
                                         (dict(R=0), -4, b"null pointer"), (dict(order=0), -4, b"null pointer")]),
        (_sl, b"hmv_sliding_auto_f64", [(dict(measure=3), -4, b"measure"), (dict(measure=-1), -4, b"measure"),
                                        (dict(m=0), -1, b"channel count"), (dict(m=65), -1, b"channel count"),
                                        (dict(pmax=0), -2, b"model order"), (dict(pmax=33), -2, b"model order"),
                                        (dict(n=5), -3, b"window shorter"), (dict(crit=3), -5, b"criterion"),
                                        (dict(crit=-1), -5, b"criterion"), (dict(nb=-1), -4, b"n_bands"),
                                        (dict(out=0), -4, b"null pointer"), (dict(order=0), -4, b"null pointer"),
                                        (dict(nb=2), -4, b"band bins"), (dict(S=P, measure=1), -4, b"spectra"),
                                        (dict(S=P, nb=2, lo=P, hi=P), -4, b"spectra"), (dict(flags=4), -6, b"LDL"),
                                        (dict(ws=16), -7, b"workspace too small"),
                                        (dict(measure=1, info_tf=0), -4, b"null pointer")]),
    ]
    for fn, name, cs in cases:
        for kw, code, text in cs:
            assert fn(lib, **kw) == code, (name, kw)
            err = lib.hmv_last_error()
            assert err.startswith(name) and text in err, (name, kw, err)
    # an empty batch is not an error, whatever the pointers
    assert _sl(lib, items=0, out=0, order=0) == 0
    assert _yw(lib, items=0) == 0


def test_workspace_sizing(lib):
    f = lib.hmv_sliding_auto_workspace_bytes
    # the fixed-order layouts at p = pmax: the automatic order needs no scratch of its own (the snapshots go to the outputs)
    assert f(0, 7, 19, 12, 30, 0) == lib.hmv_sliding_workspace_bytes(7, 19, 12, 30)
    assert f(0, 7, 19, 12, 30, 3) == lib.hmv_sliding_bands_workspace_bytes(7, 19, 12, 30)
    assert f(0, 7, 19, 12, 30, -1) == lib.hmv_sliding_spectra_workspace_bytes(7, 19, 12, 30)
    assert f(1, 7, 19, 12, 30, 0) == lib.hmv_sliding_ddtf_workspace_bytes(7, 19, 12, 30, 0)
    assert f(1, 7, 19, 12, 30, 2) == lib.hmv_sliding_ddtf_workspace_bytes(7, 19, 12, 30, 2)
    assert f(2, 7, 19, 12, 30, 2) == lib.hmv_sliding_gpdc_workspace_bytes(7, 19, 12, 30, 2)
    for bad in ((3, 7, 19, 12, 30, 0), (0, 0, 19, 12, 30, 0), (0, 7, 65, 12, 30, 0), (0, 7, 19, 33, 30, 0), (0, 7, 19, 12, 0, 0),
                (1, 7, 19, 12, 30, -1), (0, 7, 19, 12, 30, -2)):
        assert f(*bad) == -1, bad


def test_python_refusals_before_the_gpu():
    from hyperscanning_signal_analysis_amd import sliding
    from hyperscanning_signal_analysis_amd.engine import Engine, auto_order_args
    assert auto_order_args(20, "AIC", 160) == (20, 0) and auto_order_args(1, "SC", 2) == (1, 2)
    with pytest.raises(ValueError, match=re.escape("Invalid criterion type. Choose from 'AIC', 'HQ', 'SC'.")):
        auto_order_args(20, "BIC", 160)
    for bad in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_model_order must be an integer in 1..32"):
            auto_order_args(bad, "AIC", 160)
    with pytest.raises(ValueError, match=r"window length \(20\) must exceed max_model_order \(20\)"):
        auto_order_args(20, "AIC", 20)
    x = np.zeros((4, 400))
    f = np.linspace(1.0, 40.0, 8)
    # the host wrappers refuse before they ask for an engine (there is no GPU here: reaching the engine would raise
    # RuntimeError, not ValueError)
    for fn in (sliding.sliding_ffdtf, sliding.sliding_ddtf, sliding.sliding_gpdc):
        with pytest.raises(ValueError, match="Invalid criterion type"):
            fn(x, 100, 4, None, f, 100.0, crit_type="FPE")
        with pytest.raises(ValueError, match="max_model_order must be"):
            fn(x, 100, 4, None, f, 100.0, max_model_order=40)
    with pytest.raises(ValueError, match="not offered here yet"):
        sliding.sliding_significance(x, 100, 4, None, f, 100.0, (np.array([0]), np.array([4])), measure="ffdtf",
                                     null="shift", n_surrogates=10, seed=0)
    with pytest.raises(ValueError, match="sliding_significance: the automatic model order"):
        Engine.sliding_significance(None, None, None, None, 100, None, f, 100.0, None, measure="ffdtf", null="shift",
                                    n_surrogates=10, seed=0)
    with pytest.raises(ValueError, match="stream_dyads: the automatic model order"):
        Engine.stream_dyads(None, [], 100, [0], None, f, 100.0)


def test_escan_refuses_before_the_tree(tmp_path):
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    with pytest.raises(ValueError, match="Invalid criterion type"):
        EB.run(tmp_path / "nope", tmp_path / "out", model_order=None, crit_type="BIC", engine=object())
    with pytest.raises(ValueError, match="max_model_order must be"):
        EB.run(tmp_path / "nope", tmp_path / "out", model_order=None, max_model_order=0, engine=object())
    with pytest.raises(ValueError, match="not offered here yet"):
        EB.run(tmp_path / "nope", tmp_path / "out", model_order=None, engine=object(),
               significance=dict(null="shift", n_surrogates=10, seed=0))


def test_penalties_are_the_reference_s():
    """crit_q - log det V_q of the oracle (the reference's arithmetic) is c q m^2 / n with c = 2, 2 log log n, log n --
    the three constants `hmv_yw_solve_auto_f64` is given -- and the order is the FIRST arg-min."""
    from hyperscanning_signal_analysis_amd.synthetic import mixed_order_recording
    m, n, pmax = 4, 160, 12
    x = mixed_order_recording(100, m, [3], 400)[:, 100:100 + n]
    logdet = np.array([np.log(np.linalg.det(O.ar_coeff(x, q)[1])) for q in range(1, pmax + 1)])
    q = np.arange(1, pmax + 1)
    for crit, c in (("AIC", 2.0), ("HQ", 2.0 * np.log(np.log(n))), ("SC", np.log(n))):
        curve, rng, popt = O.mvar_criterion(x, pmax, crit)
        assert np.array_equal(rng, q)
        assert np.allclose(curve - logdet, ((c * q) * (m * m)) / n, rtol=1e-13, atol=1e-15)
        assert popt == 1 + int(np.argmin(logdet + ((c * q) * (m * m)) / n))


@pytest.mark.parametrize("case", WORKLOADS, ids=lambda c: f"m{c[0]}-{c[4]}")
def test_workload_needs_a_selection(case):
    """The property the GPU tests lean on, shown without a GPU: the oracle picks several different orders on the
    mixed-order recording, no window's best and second-best criterion are closer than 1e-6, every value is finite."""
    from hyperscanning_signal_analysis_amd.sliding import hop_positions
    from hyperscanning_signal_analysis_amd.synthetic import mixed_order_recording
    m, n, hop, pmax, crit, orders, seg, picked = case
    x = mixed_order_recording(100, m, orders, seg)
    assert x.shape == (m, len(orders) * seg)
    assert np.allclose(x.mean(axis=1), 0.0, atol=1e-12) and np.allclose(x.std(axis=1), 1.0)
    pos = hop_positions(x.shape[1], n, hop)
    picks, gaps = [], []
    for s in pos:
        curve, _, popt = O.mvar_criterion(x[:, s:s + n], pmax, crit)
        assert np.isfinite(curve).all()
        two = np.sort(curve)[:2]
        gaps.append(two[1] - two[0])
        picks.append(int(popt))
    counts = np.bincount(picks, minlength=pmax + 1)[1:]
    assert counts.tolist() == picked + [0] * (pmax - len(picked))
    assert min(gaps) > GAP
    if crit == "AIC":
        assert np.count_nonzero(counts) >= 4
    assert np.count_nonzero(counts) >= 3


def test_generator_is_seeded_and_per_stretch():
    from hyperscanning_signal_analysis_amd.synthetic import mixed_order_recording
    a = mixed_order_recording(7, 5, [1, 4], 300)
    assert np.array_equal(a, mixed_order_recording(7, 5, [1, 4], 300))
    assert not np.array_equal(a, mixed_order_recording(8, 5, [1, 4], 300))
    assert np.isfinite(a).all() and np.abs(a).max() < 10.0
