"""K2's pivoted fallback (csrc/yw_lu.hip) without a GPU: its NumPy restatement (tests/yw_lu_restated.py) against
`numpy.linalg.solve`, the refusals of the C ABI, the constants, the scratch it lives in, and the host logic of the Python
options.

The restatement walks the kernel's blocking and pivot rule; what separates the two is the order of accumulation inside a
step.  For every input below `test_restatement_against_numpy` prints eta_restated / eta_numpy, eta = ||B - G X||_F /
(||G||_F ||X||_F + ||B||_F) on the real channels' rows and columns.  Printed here (NumPy 2 on OpenBLAS): between 0.35 and
0.99 over the 48 collinear windows (cond 1e16 .. 2e18; eta_numpy 0.12 .. 0.38 eps, eta_restated 0.06 .. 0.17 eps), 0.41
and 0.44 on the two band-limited windows, 0.77 .. 1.21 on the g6 fixtures.  The largest over the collinear windows, 0.992,
is `MAX_RATIO_PRINTED`; tests/test_gpu_yw_pivoted.py allows the kernel c = 4 x that = 3.97 times numpy's backward error."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import yw_lu_restated as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
MAX_RATIO_PRINTED = 0.992
P = 0x1000          # a fake non-zero device address: the checks must refuse before any pointer is read


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


def _etas(x, p):
    m = x.shape[0]
    R = Y.padded_lagcov(x, p)
    G, B = Y.build_system(R)
    idx = Y.real_index(m, p)
    ar, V, info, X = Y.lu_solve(R)
    Xn = np.linalg.solve(G, B)                       # (the padded system is block diagonal: the real block is G's own)
    return info, Y.eta(G, B, X, idx), Y.eta(G, B, Xn, idx), len(idx), ar, V, X


def test_restatement_against_numpy(golden):
    g = golden("g6_errors.npz")
    cases = [(f"g6 {k}", g[f"{k}_x"] if k.startswith("nc") else g[k], 3) for k in ("nc0", "nc1", "nc2", "xs")]
    cases += list(Y.ratio_cases())
    worst = 0.0
    for name, x, p in cases:
        info, er, en, N, ar, V, X = _etas(x, p)
        print(f"{name:36s} N={N:4d} eta_restated={er / Y.EPS:.3f} eps  eta_numpy={en / Y.EPS:.3f} eps  ratio={er / en:.3f}")
        assert info == 0, name
        assert er <= N * Y.EPS, (name, er)           # the textbook bound
        if name.startswith("collinear"):
            worst = max(worst, er / en)
    print(f"largest ratio over the collinear windows: {worst:.3f} (recorded: {MAX_RATIO_PRINTED})")
    assert worst <= 1.5 * MAX_RATIO_PRINTED          # the figure the GPU test's c is built on still describes this walk


def test_restatement_on_the_fixtures_with_an_answer(golden):
    """Where the conditioning leaves an answer to compare: the project's contract 1e2 cond eps against the reference's
    recorded ar / V (nc0, nc1, nc2), V = R_0 - X^T B; the dead channel is dgesv's info > 0."""
    g = golden("g6_errors.npz")
    for k in ("nc0", "nc1", "nc2"):
        x = g[f"{k}_x"]
        m = x.shape[0]
        ar, V, info, X = Y.lu_solve(Y.padded_lagcov(x, 3))
        tol = 1e2 * float(g[f"{k}_cond"]) * Y.EPS
        assert info == 0
        assert np.abs(ar[:m, :m] - g[f"{k}_ar"]).max() / np.abs(g[f"{k}_ar"]).max() < tol, k
        assert np.abs(V[:m, :m] - g[f"{k}_V"]).max() / np.abs(g[f"{k}_V"]).max() < tol, k
        assert not ar[m:].any() and not ar[:, m:].any() and np.array_equal(V[m:, m:], np.eye(16 - m))
    ar, V, info, X = Y.lu_solve(Y.padded_lagcov(g["xz"], 3))
    assert info == 3 and np.isnan(ar).all()          # channel 2 is dead: column 2 is exactly zero
    with pytest.raises(np.linalg.LinAlgError):
        G, B = Y.build_system(Y.padded_lagcov(g["xz"], 3))
        np.linalg.solve(G, B)


def test_restatement_is_scale_free():
    """No absolute constant: samples * 2^k give the same X bit for bit and V * 4^k."""
    x = Y.collinear_window(1, 19, 200, 1e-8)
    ar0, V0, _, _ = Y.lu_solve(Y.padded_lagcov(x, 3))
    for k in (-20, 12):
        ar, V, info, _ = Y.lu_solve(Y.padded_lagcov(x * 2.0 ** k, 3))
        assert info == 0 and np.array_equal(ar, ar0) and np.array_equal(V[:19, :19], V0[:19, :19] * 4.0 ** k)


def test_constants_and_binding(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    assert int(re.search(r"#define HMV_FLAG_YW_PIVOTED (\d+)", hdr).group(1)) == 16 == _lib.FLAG_YW_PIVOTED
    flags = {n: int(v) for n, v in re.findall(r"#define HMV_FLAG_(\w+) (\d+)", hdr)}
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())     # distinct bits
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"\bhmv_yw_routes_i32\s*\(([^)]*)\)", code)
    assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES["hmv_yw_routes_i32"][1]) == 6
    assert hasattr(lib, "hmv_yw_routes_i32")
    # HMV_TUNE_YW_FORM takes the new value 5 and nothing beyond it
    before = lib.hmv_get_tuning(_lib.TUNE_YW_FORM)
    try:
        assert lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 5) == 0 and lib.hmv_get_tuning(_lib.TUNE_YW_FORM) == 5
        assert lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 6) < 0 and lib.hmv_get_tuning(_lib.TUNE_YW_FORM) == 5
    finally:
        assert lib.hmv_set_tuning(_lib.TUNE_YW_FORM, before) == 0


def test_the_system_fits_the_scratch(lib):
    """[G | B] takes p (p + 1) tiles; the scratch has yw_ws_tiles, the last of which holds the route word."""
    for mch in (4, 64):
        mp = lib.hmv_pad(mch)
        for p in range(1, 33):
            tiles = lib.hmv_yw_workspace_doubles(mch, p) // (mp * mp)
            assert tiles * mp * mp == lib.hmv_yw_workspace_doubles(mch, p)
            assert p * (p + 1) <= tiles - 1, (mch, p)
    assert lib.hmv_yw_workspace_doubles(64, 8) == (2 * 45 + 16 + 1) * 64 * 64          # unchanged


def test_c_abi_refusals(lib):
    from hyperscanning_signal_analysis_amd import _lib
    piv = _lib.FLAG_YW_PIVOTED
    # the flag with a criterion curve
    assert lib.hmv_yw_solve_f64(P, 2, 8, 3, P, P, P, P, P, piv, 0) == -6
    assert b"pivoted LU" in lib.hmv_last_error() and b"vq_logdet" in lib.hmv_last_error()
    assert lib.hmv_yw_solve_f64(P, 2, 8, 3, P, P, P, P, P, piv | _lib.FLAG_YW_ONE_LAUNCH, 0) == -6
    # the LU alone (HMV_TUNE_YW_FORM = 5) with a criterion curve
    try:
        assert lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 5) == 0
        assert lib.hmv_yw_solve_f64(P, 2, 8, 3, P, P, P, P, P, 0, 0) == -6 and b"pivoted LU" in lib.hmv_last_error()
    finally:
        assert lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 0) == 0
    # the earlier checks still come first, and an empty batch with the flag is fine
    assert lib.hmv_yw_solve_f64(P, 2, 65, 3, P, P, P, P, P, piv, 0) == -1
    assert lib.hmv_yw_solve_f64(0, 2, 8, 3, P, P, P, 0, P, piv, 0) == -4
    assert lib.hmv_yw_solve_f64(P, 0, 8, 3, P, P, P, 0, P, piv, 0) == 0
    # the automatic order
    assert lib.hmv_yw_solve_auto_f64(P, 2, 8, 5, 100, 0, P, P, P, P, 0, 0, P, piv, 0) == -6
    assert b"hmv_yw_solve_auto_f64" in lib.hmv_last_error() and b"pivoted LU" in lib.hmv_last_error()
    rc = lib.hmv_sliding_auto_f64(0, P, 1000, 1000, P, P, 2, 8, 100, 5, 0, P, 4, 100.0, P, 0, 0, 0, 0, 0, 0, P, 0, P, P, P,
                                  1 << 40, 2, 1.0, piv, 0, 0, 0, 0, 0, 0)
    assert rc == -6 and b"hmv_sliding_auto_f64" in lib.hmv_last_error() and b"pivoted LU" in lib.hmv_last_error()
    # the route call
    assert lib.hmv_yw_routes_i32(P, 2, 0, 3, P, 0) == -1 and lib.hmv_yw_routes_i32(P, 2, 8, 33, P, 0) == -2
    assert lib.hmv_yw_routes_i32(0, 2, 8, 3, P, 0) == -4 and lib.hmv_yw_routes_i32(P, 2, 8, 3, 0, 0) == -4
    assert lib.hmv_yw_routes_i32(P, 0, 8, 3, P, 0) == 0


def test_engine_option_host_logic(monkeypatch):
    from hyperscanning_signal_analysis_amd.engine import no_pivoted_auto_order, resolve_pivoted_yw, route_counts
    monkeypatch.delenv("HYPERMVAR_YW_PIVOTED", raising=False)
    assert resolve_pivoted_yw(None) is False and resolve_pivoted_yw(True) is True and resolve_pivoted_yw(False) is False
    for v, want in (("1", True), ("true", True), ("yes", True), ("0", False), ("", False), ("off", False), (" False ", False)):
        monkeypatch.setenv("HYPERMVAR_YW_PIVOTED", v)
        assert resolve_pivoted_yw(None) is want, v
        assert resolve_pivoted_yw(False) is False and resolve_pivoted_yw(True) is True      # an argument wins
    for bad in (1, "yes", 0.0):
        with pytest.raises(ValueError, match="pivoted_yw must be"):
            resolve_pivoted_yw(bad)
    no_pivoted_auto_order(False, "x")
    with pytest.raises(ValueError, match=r"sliding_ffdtf: the automatic model order \(p=None\) is not available with the pivoted"):
        no_pivoted_auto_order(True, "sliding_ffdtf")
    assert route_counts(np.array([0, 2, 1, 0, 2, 2])) == {"recursion": 2, "ldlt": 1, "lu": 3}
    assert route_counts(np.zeros((0,), dtype=np.int32)) == {"recursion": 0, "ldlt": 0, "lu": 0}


def test_escan_option_host_logic(tmp_path):
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    f = EB.resolve_pivoted_fallback
    assert f(None, False, False) == (False, {}) and f(None, True, False) == (True, {"flags": _lib.FLAG_YW_PIVOTED})
    assert f(True, False, False) == (True, {"flags": 16}) and f(False, False, True) == (False, {})
    with pytest.raises(ValueError, match="pivoted_fallback=False"):
        f(False, True, False)
    with pytest.raises(ValueError, match="automatic model order"):
        f(True, False, True)
    with pytest.raises(ValueError, match="must be True, False or None"):
        f(1, False, False)

    class Eng:
        pivoted_yw = True
    with pytest.raises(ValueError, match="automatic model order"):
        EB.run(tmp_path / "nope", tmp_path / "out", model_order=None, engine=Eng())


def test_yw_routes_refuses_before_the_gpu():
    from hyperscanning_signal_analysis_amd import sliding
    x = np.zeros((4, 300))
    with pytest.raises(ValueError, match="yw_routes"):
        sliding.yw_routes(x, 100, 3, None, engine=object())
    with pytest.raises(ValueError, match="yw_routes"):
        sliding.yw_routes(x, 100, 3, 40, engine=object())
    with pytest.raises(ValueError, match=r"\(m, T\) or \(n_rec, m, T\)"):
        sliding.yw_routes(np.zeros(300), 100, 3, 3, engine=object())
    with pytest.raises(ValueError, match="hop needs a window_size"):
        sliding.yw_routes(x, None, 3, 3, hop=50, engine=object())


def test_band_limited_dyad_is_seeded_and_band_limited():
    from hyperscanning_signal_analysis_amd.synthetic import band_limited_dyad
    a = band_limited_dyad(3, 5, 4000, high_cutoff_hz=45.0, burn=300)
    assert a.shape == (5, 4000) and np.array_equal(a, band_limited_dyad(3, 5, 4000, high_cutoff_hz=45.0, burn=300))
    assert not np.array_equal(a, band_limited_dyad(4, 5, 4000, high_cutoff_hz=45.0, burn=300))
    assert np.allclose(a.mean(axis=1), 0.0, atol=1e-12) and np.allclose(a.std(axis=1), 1.0)
    spec = np.abs(np.fft.rfft(a * np.hanning(4000), axis=1)) ** 2     # (tapered: the window's own leakage is not the filter's)
    f = np.fft.rfftfreq(4000, 1.0 / 500.0)
    assert spec[:, f > 90.0].sum() < 1e-6 * spec.sum()              # Butterworth-4 twice: -48 dB / octave
    with pytest.raises(ValueError, match="high_cutoff_hz"):
        band_limited_dyad(3, 5, 1000, high_cutoff_hz=250.0)
