"""FAD decomposition on the MI355X against the reference's own outputs (tests/golden/g9_fad.npz, written by
tests/golden/make_golden_fad.py from /root/reference/src/mtmvar.py:607-757 and scipy.signal.residuez) and against a
host restatement (NumPy solve + residuez) kept in this file.

Tolerances.  The fit is Levinson-Durbin where the reference solves the Toeplitz system with LAPACK: coefficients
agree to ~kappa * eps, checked at 1e2 * kappa * eps relative.  Poles come from Aberth-Ehrlich iteration where NumPy
takes companion-matrix eigenvalues; roots and everything derived from them are compared as multisets (nearest pole:
the order of poles with equal |z| is not specified by the reference) to 1e-9 relative to max(1, |value|).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
POLE_KEYS = ("poles", "C", "alpha", "freq_hz", "omega_rad_s", "beta", "bandwidth_hz", "phi", "B")
KEYS = {"model_order", "poles", "C", "alpha", "freq_hz", "omega_rad_s", "beta", "phi", "bandwidth_hz", "B",
        "noise_variance", "osc_mask", "ar_coeffs", "paired_components"}
CRIT = ("AIC", "HQ", "SC")

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import mtmvar as M
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import sliding_fad
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad


def close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert np.all(err <= tol), (err.max(), tol)


def match(got_poles, ref_poles):
    """index into got for every reference pole (nearest), and check it is a bijection"""
    idx = np.array([int(np.argmin(np.abs(got_poles - z))) for z in ref_poles], dtype=int)
    assert sorted(idx.tolist()) == list(range(len(ref_poles))) or len(set(np.round(ref_poles, 6))) < len(ref_poles)
    return idx


def check_poles(got, ref, tol=1e-9):
    """per-pole arrays of a result dict (got) against the reference's (ref), matched as multisets"""
    idx = match(got["poles"], ref["poles"])
    for k in POLE_KEYS:
        g = np.asarray(got[k])[idx]
        r = np.asarray(ref[k])
        if k == "phi":                               # an angle: compare on the circle
            g = np.angle(np.exp(1j * (g - r)))
            r = np.zeros_like(r)
        close(g, r, tol)
    np.testing.assert_array_equal(np.asarray(got["osc_mask"])[idx], ref["osc_mask"])


def golden_case(g, c):
    d = {k: g[f"{c}__{k}"] for k in POLE_KEYS + ("osc_mask", "ar_coeffs", "noise_variance", "model_order", "kappa")}
    d["pc"] = {k: g[f"{c}__pc_{k}"] for k in ("pole_index",) + POLE_KEYS}
    return d


CASES = ("ar6_p8", "ar6_aic", "ar6_hq", "ar6_sc", "short", "unpaired", "negpole")


@pytest.mark.parametrize("case", CASES)
def test_fad_parity_with_reference(golden, case, capsys):
    g = golden("g9_fad.npz")
    ref = golden_case(g, case)
    mo = int(g[f"{case}__in_model_order"])
    kw = dict(model_order=None if mo == 0 else mo, max_model_order=int(g[f"{case}__in_max_model_order"]),
              crit_type=CRIT[int(g[f"{case}__in_crit"])], pair_conjugates=bool(g[f"{case}__in_pair"]))
    capsys.readouterr()
    d = M.fad_decomposition(g[f"{case}__in_x"], float(g[f"{case}__in_fs"]), **kw)
    assert capsys.readouterr().out == str(g[f"{case}__printed"])
    assert set(d) == KEYS
    assert set(d["paired_components"]) == set(ref["pc"])
    assert d["model_order"] == int(ref["model_order"])
    p = int(ref["model_order"])
    for k in ("poles", "C", "alpha"):
        assert d[k].dtype == np.complex128 and d[k].shape == (p,)
    assert d["osc_mask"].dtype == bool and d["paired_components"]["pole_index"].dtype == np.int64
    assert isinstance(d["noise_variance"], float)
    close(d["ar_coeffs"], ref["ar_coeffs"], 1e2 * float(ref["kappa"]) * EPS)
    assert abs(d["noise_variance"] - ref["noise_variance"]) <= 1e-12 * abs(ref["noise_variance"])
    check_poles(d, ref)
    pc, rpc = d["paired_components"], ref["pc"]
    assert len(pc["pole_index"]) == len(rpc["pole_index"])
    # element-wise in order; with pair_conjugates=False the list is in pole order, and the reference orders the two
    # poles of a conjugate pair (equal |z|) by whatever NumPy's argsort does with ties (its vectorised quicksort is not
    # stable) -- there the two members of each pair are matched to their nearest counterpart
    order = np.arange(len(rpc["poles"])) if kw["pair_conjugates"] else match(pc["poles"], rpc["poles"])
    if not kw["pair_conjugates"]:
        assert np.all(np.abs(order - np.arange(len(order))) <= 1)
    for k in POLE_KEYS:
        if k == "phi":
            close(np.angle(np.exp(1j * (pc[k][order] - rpc[k]))), np.zeros(len(rpc[k])), 1e-8)
        else:
            close(pc[k][order], rpc[k], 1e-8)
    np.testing.assert_array_equal(d["poles"][pc["pole_index"]], pc["poles"])   # pole_index points at its poles
    if kw["model_order"] is None:
        b = M.fad_decomposition_batch(g[f"{case}__in_x"][None], float(g[f"{case}__in_fs"]), **kw)
        # log V_p inherits the fit's ~kappa * eps relative difference (1.1e-12 absolute measured on criterion values
        # near 8.4 at kappa 9e4): checked at 1e-12 relative to max(1, |crit|)
        close(b["crit"][0], g[f"{case}__crit"], 1e-12)


def test_fad_decompose_only_against_residuez(golden):
    """hmv_fad_decompose_f64 on the coefficient sets of the fixture.  Well-separated poles: 1e-11.  Repeated poles
    (an exact double real pole, a double conjugate pair) and the grouped pair 5e-4 apart: the roots of a repeated
    factor are only determined to ~sqrt(eps) by any root finder (NumPy's companion eigenvalues included), residuez
    averages them, and its polynomial-division route for the repeated-pole residues loses a further ~1e-7 against the
    direct series of this library (both measured on these cases) -- checked at 1e-6."""
    g = golden("g9_fad.npz")
    eng = default_engine()
    names = sorted({k[2:].split("__")[0] for k in g.files if k.startswith("d_")})
    assert len(names) == 11
    for name in names:
        a = g[f"d_{name}__ar"]
        o = eng.fad_decompose(torch.as_tensor(a[None]), 250.0)
        info = int(o["info"][0])
        poles = o["poles"][0].cpu().numpy()
        C = o["C"][0].cpu().numpy()
        rz, rC = g[f"d_{name}__poles"], g[f"d_{name}__C"]
        tol = 1e-6 if name in ("double_real", "double_pair", "grouped") else 1e-11
        if name == "rand32":
            # 32 random poles: residuez's own poles / residues are 6e-11 / 3.5e-10 away from the same quantities
            # computed in 50-digit arithmetic (mpmath, measured on this coefficient set) -- the reference is the
            # less accurate side here
            tol = 1e-9
        assert info & 3 == 0, (name, info)
        assert len(poles) == len(rz)
        # residuez's order: sorted by |z|; within a repeated pole the residues ascend in power -- compared in order
        close(np.abs(poles), np.abs(rz), tol)
        if name in ("double_real", "double_pair", "grouped"):
            close(poles, rz, tol)                    # order inside a group is significant
            close(C, rC, tol)
        else:
            idx = match(poles, rz)                   # conjugate partners (equal |z|) in either order
            close(poles[idx], rz, tol)
            close(C[idx], rC, tol)
        assert np.all(np.imag(poles[np.abs(np.imag(rz)) == 0]) == 0)       # real poles are exactly real


def test_sliding_fad_matches_reference_loop_and_single_calls_bitwise(golden):
    g = golden("g9_fad.npz")
    rec = g["rec__in_x"]
    w = int(g["rec__in_window"])
    out = sliding_fad(rec, 250.0, window_size=w, n_windows=3)
    assert out["model_order"].shape == (3, 8) and out["poles"].shape == (3, 8, 20)
    np.testing.assert_array_equal(out["model_order"], g["rec__model_order"])
    assert np.all(out["info"] == 0)
    close(out["noise_variance"], g["rec__noise_variance"], 1e-12)
    for wi, s0 in enumerate(g["rec__in_starts"]):
        for c in range(8):
            p = int(g["rec__model_order"][wi, c])
            got = {k: out[k][wi, c, :p] for k in POLE_KEYS + ("osc_mask",)}
            ref = {k: g[f"rec__{k}"][wi, c, :p] for k in POLE_KEYS + ("osc_mask",)}
            check_poles(got, ref)
            assert np.all(np.isnan(out["poles"][wi, c, p:])) and not out["osc_mask"][wi, c, p:].any()
            if c in (0, 5):                           # batch row == single call, bit for bit
                d = M.fad_decomposition(rec[c, s0:s0 + w], 250.0)
                for k in POLE_KEYS:
                    np.testing.assert_array_equal(d[k], out[k][wi, c, :p])
                np.testing.assert_array_equal(d["ar_coeffs"], out["ar_coeffs"][wi, c, :p])
                assert d["noise_variance"] == out["noise_variance"][wi, c]


def host_fad(x, fs, pmax=20):
    """host restatement: biased autocovariance, dense Toeplitz solves for every order, AIC, residuez"""
    from scipy.linalg import toeplitz
    from scipy.signal import residuez
    n = len(x)
    r = np.array([x[:n - k] @ x[k:] / n for k in range(pmax + 1)])
    crit, fits = [], []
    for p in range(1, pmax + 1):
        a = np.linalg.solve(toeplitz(r[:p]), r[1:p + 1])
        V = r[0] - a @ r[1:p + 1]
        crit.append(np.log(V) + 2 * p / n)
        fits.append((a, V))
    p = int(np.argmin(crit)) + 1
    a, V = fits[p - 1]
    C, z, _ = residuez([1.0], np.r_[1.0, -a])
    alpha = np.log(z) * fs
    return dict(model_order=p, ar=a, V=V, poles=z, C=C, alpha=alpha, freq_hz=alpha.imag / (2 * np.pi),
                beta=-alpha.real, B=2 * np.abs(C), osc=np.abs(z.imag) > 1e-8)


def test_fad_northstar_shape():
    x = synthetic_var_dyad(0, m=64, p=8)
    fs = 500.0
    out = sliding_fad(x, fs, window_size=1000, hop=500)
    assert out["model_order"].shape == (599, 64)
    assert np.all(out["info"] == 0)
    f = out["paired_components"]["freq_hz"]
    have = out["paired_components"]["pole_index"] >= 0
    assert np.all((f[have] > 0) & (f[have] <= fs / 2))
    rng = np.random.default_rng(5)
    for s in rng.choice(599 * 64, 200, replace=False):
        wi, c = divmod(int(s), 64)
        h = host_fad(x[c, 500 * wi:500 * wi + 1000], fs)
        p = h["model_order"]
        assert out["model_order"][wi, c] == p
        close(out["ar_coeffs"][wi, c, :p], h["ar"], 1e-9)
        got = {k: out[k][wi, c, :p] for k in ("poles", "C", "alpha", "freq_hz", "beta", "B", "osc_mask")}
        idx = match(got["poles"], h["poles"])
        for k in ("poles", "C", "alpha", "freq_hz", "beta", "B"):
            close(got[k][idx], h[k], 1e-9)
        np.testing.assert_array_equal(got["osc_mask"][idx], h["osc"])
    again = sliding_fad(x, fs, window_size=1000, hop=500)
    for k in POLE_KEYS + ("ar_coeffs", "noise_variance", "model_order"):
        np.testing.assert_array_equal(again[k], out[k])


def test_fad_degenerate_input():
    rng = np.random.default_rng(3)
    sig = rng.standard_normal((3, 400))
    sig[1] = 0.0
    b = M.fad_decomposition_batch(sig, 100.0)
    assert b["info"].tolist() == [0, 1, 0]
    assert np.all(np.isnan(b["poles"][1])) and np.all(np.isnan(b["ar_coeffs"][1])) and np.isnan(b["noise_variance"][1])
    assert b["paired_components"]["n_components"][1] == 0 and np.all(b["paired_components"]["pole_index"][1] == -1)
    assert np.isfinite(b["noise_variance"][[0, 2]]).all()
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        M.fad_decomposition(np.zeros(400), 100.0)
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        M.fad_decomposition(np.zeros((1, 400)), 100.0, model_order=4)


def test_fad_imag_tol_and_unpaired(golden):
    g = golden("g9_fad.npz")
    x = g["ar6_p8__in_x"]
    d = M.fad_decomposition(x, 250.0, model_order=8)
    osc = np.abs(d["poles"].imag) > 1e-8
    np.testing.assert_array_equal(d["osc_mask"], osc)
    pi = d["paired_components"]["pole_index"]
    assert np.all(d["poles"][pi].imag > 0) and np.all(np.diff(d["paired_components"]["freq_hz"]) >= 0)
    u = M.fad_decomposition(x, 250.0, model_order=8, pair_conjugates=False)
    np.testing.assert_array_equal(u["paired_components"]["pole_index"], np.where(osc)[0])
    big = M.fad_decomposition(x, 250.0, model_order=8, imag_tol=10.0)
    assert not big["osc_mask"].any() and len(big["paired_components"]["pole_index"]) == 0
    mid_tol = np.sort(np.abs(d["poles"].imag[osc]))[0] * 1.0001          # drops the pair nearest to the real axis
    mid = M.fad_decomposition(x, 250.0, model_order=8, imag_tol=mid_tol)
    assert mid["osc_mask"].sum() == osc.sum() - 2
    assert len(mid["paired_components"]["pole_index"]) == len(pi) - 1
    close(mid["poles"], d["poles"], 0.0)                                   # imag_tol changes only the classification
