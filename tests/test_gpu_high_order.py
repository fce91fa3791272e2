"""Model orders 17 .. 32 on the GPU.  include/hypermvar.h and every entry point accept p in 1..32 and the reference's own
default is max_model_order = 20, but the other GPU tests stop at p = 16 (one automatic-order case reaches 20 on four
channels).  Shapes (m, p, n) and inputs: tests/scale_shapes.py (`synthetic_var_dyad(31, m=m, p=4, T=n, burn=300)`; the
condition number of the oracle's normal matrix lies between 6e3 and 8.2e4).

Tolerance of K2 against the oracle: the project's conditioning rule (test_g6_rank_deficient_and_nearly_collinear_windows),
1e2 * cond * eps with cond computed here from the oracle's matrix, and asserted to be at most 2e-9 so that a badly
conditioned draw cannot loosen the test.  Downstream outputs: the 1e-8 of test_shapes_vs_oracle.  K1: 1e-12 (the sums of
up to 6000 products of O(1) values, both sides rounding).  All @pytest.mark.gpu."""
import functools

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O
from tests import scale_shapes as SS
from tests.scale_shapes import i64, tuning
from tests import validation_restated as VR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import mtmvar as M
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import regular_grid, window_items
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

FS = 250.0
FREQS = np.linspace(1.0, 100.0, 32)
P32_SHAPES = [s for s in SS.HIGH_ORDER_SHAPES if s[1] == 32]         # padded sizes 16, 16, 32, 48, 64


def rel_t(a, b):
    return float((a - b).abs().max() / b.abs().max())


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """The oracle's fit of one shape, computed once: ar, V, the log dets of every order, the conditioning tolerance."""
    m, p, n = shape
    x = SS.high_order_input(m, p, n)
    ar, V = O.ar_coeff(x, p)
    crit = O.mvar_criterion(x, p, "AIC")[0]
    logdet = crit - 2.0 * np.arange(1, p + 1) * m ** 2 / n
    cond = SS.normal_matrix_cond(O, x, p)
    tol = 1e2 * cond * SS.EPS
    for a in (ar, V, logdet):
        a.setflags(write=False)
    return dict(x=x, ar=ar, V=V, logdet=logdet, cond=cond, tol=tol)


@functools.lru_cache(maxsize=None)
def _device(shape):
    eng = default_engine()
    m, p, n = shape
    x = SS.high_order_input(m, p, n)
    xd = eng.to_device(np.stack([x, x[:, ::-1]]))                  # item 1: the window reversed in time (R_l -> R_l^T)
    rec, st = i64(eng, [0, 1]), i64(eng, [0, 0])
    return eng, x, xd, rec, st, eng.lagcov(xd, rec, st, n, p)


# ----------------------------------------------------------------------------------------------------------- K1
@pytest.mark.parametrize("shape", P32_SHAPES, ids=SS.shape_id)
def test_k1_all_33_lags(shape):
    m, p, n = shape
    eng, x, xd, rec, st, R = _device(shape)
    want = O.lag_covariances(x, p)
    assert R.shape == (2, p + 1, eng.pad(m), eng.pad(m))
    assert SS.rel(R[0, :, :m, :m].cpu().numpy(), want) <= 1e-12
    assert SS.rel(R[1, :, :m, :m].cpu().numpy(), want.transpose(0, 2, 1)) <= 1e-12
    mp = R.shape[-1]
    if mp > m:
        assert torch.equal(R[:, 0, m:, m:], torch.eye(mp - m, dtype=torch.float64, device=eng.device).expand(2, -1, -1))
        assert not bool(R[:, 1:, m:, :].any()) and not bool(R[:, :, :m, m:].any()) and not bool(R[:, 0, m:, :m].any())


@pytest.mark.parametrize("m,n,hop", [(19, 330, 33), (64, 330, 33), (5, 400, 40), (50, 400, 40)])
def test_k1_hop_blocks_at_the_edge_of_the_halo(m, n, hop):
    """hop = p + 1 is the shortest hop the shared form takes (every lag's products reach into the next block only); the
    last window ends at the end of the recording."""
    eng = default_engine()
    p, n_win = 32, 5
    T = n + hop * (n_win - 1)
    x = synthetic_var_dyad(SS.HIGH_ORDER_SEED, m=m, p=4, T=T, burn=300)
    xd = eng.to_device(x[None])
    st = hop * torch.arange(n_win, dtype=torch.int64, device=eng.device)
    direct = eng.lagcov(xd, torch.zeros_like(st), st, n, p)
    shared = eng.lagcov_regular(xd[0], 0, hop, n_win, n, p)
    assert rel_t(shared, direct) <= 1e-13
    for w in (0, n_win - 1):
        assert SS.rel(shared[w, :, :m, :m].cpu().numpy(), O.lag_covariances(x[:, w * hop:w * hop + n], p)) <= 1e-12
    mp = shared.shape[-1]
    if mp > m:
        assert torch.equal(shared[:, 0, m:, m:], torch.eye(mp - m, dtype=torch.float64, device=eng.device).expand(n_win, -1, -1))
        assert not bool(shared[:, 1:, m:, :].any()) and not bool(shared[:, :, :m, m:].any())


def test_k1_ensemble_pairs_and_trials_at_p32():
    eng = default_engine()
    m, p, n, hop, E, W = 19, 32, 330, 33, 3, 3
    T = n + hop * (W - 1) + 20 * (E - 1)
    x = synthetic_var_dyad(SS.HIGH_ORDER_SEED, m=m, p=4, T=T, burn=300)
    xd = eng.to_device(np.stack([x, x[::-1, ::-1]]))
    starts, offsets = 20 * np.arange(E), hop * np.arange(W)
    ens = dict(trial_rec=i64(eng, np.zeros(E)), trial_start=i64(eng, starts), group_ptr=i64(eng, [0, E]),
               item_group=i64(eng, np.zeros(W)), item_offset=i64(eng, offsets), n=n, p=p)
    direct = eng.lagcov_ensemble(xd, flags=_lib.FLAG_DIRECT_LAGCOV, **ens)
    shared = eng.lagcov_ensemble(xd, grid=(hop, W), **ens)
    Rt = eng.lagcov_trials(xd, ens["trial_rec"], ens["trial_start"], ens["item_offset"], n, p)
    for w, off in enumerate(offsets):
        trials = np.stack([x[:, s + off:s + off + n] for s in starts], axis=2)
        want = O.lag_covariances(trials, p)
        assert SS.rel(direct[w, :, :m, :m].cpu().numpy(), want) <= 1e-12
        assert SS.rel(shared[w, :, :m, :m].cpu().numpy(), want) <= 1e-12
        for e in range(E):
            assert SS.rel(Rt[e, w, :, :m, :m].cpu().numpy(), O.lag_covariances(trials[:, :, e], p)) <= 1e-12
    split = 9
    pairs = eng.lagcov_pairs(xd, i64(eng, [0, 0]), i64(eng, [1, 1]), i64(eng, [0, 37]), n, p, split)
    both = xd.cpu().numpy()
    for k, s in enumerate((0, 37)):
        glued = np.concatenate([both[0, :split, s:s + n], both[1, split:, s:s + n]])
        assert SS.rel(pairs[k, :, :m, :m].cpu().numpy(), O.lag_covariances(glued, p)) <= 1e-12


# ----------------------------------------------------------------------------------------------------------- K2
@pytest.mark.parametrize("shape", SS.HIGH_ORDER_SHAPES, ids=SS.shape_id)
def test_k2_against_the_oracle(shape):
    """The recursion (default) and its pipelined form (TUNE_YW_FORM = 3): ar, V and every order's log det against
    `O.ar_coeff` / `O.mvar_criterion`; with and without the log dets the same bits; no window trips the guard (the result
    does not carry the LDL^T's bits).  The block LDL^T, the fallback of guarded windows: both launch forms the same bits,
    info 0 and finite; its error against the oracle is printed, not asserted (csrc/yw_lwr.hip and DESIGN.md quote it)."""
    m, p, n = shape
    o = _oracle(shape)
    eng, x, xd, rec, st, R = _device(shape)
    print(shape, f"cond {o['cond']:.3g} tol {o['tol']:.3g}")
    assert o["tol"] <= SS.COND_TOL_CAP
    ar_rev, V_rev = O.ar_coeff(x[:, ::-1], p)
    forms = {}
    forms["default"] = (eng.yw_solve(R, m, True), eng.yw_solve(R, m, False))
    with tuning(eng, _lib.TUNE_YW_FORM, 3):
        forms["form3"] = (eng.yw_solve(R, m, True), eng.yw_solve(R, m, False))
        torch.cuda.synchronize()
    a1, v1, l1, i1 = eng.yw_solve(R, m, True, flags=_lib.FLAG_YW_ONE_LAUNCH)
    a2, v2, l2, i2 = eng.yw_solve(R, m, True, flags=_lib.FLAG_YW_TILED)
    torch.cuda.synchronize()
    for name, ((ar, V, ld, info), (ar_b, V_b, _, info_b)) in forms.items():
        assert not bool(info.any()) and not bool(info_b.any()), name
        assert torch.equal(ar, ar_b) and torch.equal(V, V_b), name
        assert not torch.equal(ar, a1), name
        err = (SS.rel(ar[0, :m, :m].cpu().numpy(), o["ar"]), SS.rel(V[0, :m, :m].cpu().numpy(), o["V"]),
               SS.rel(ar[1, :m, :m].cpu().numpy(), ar_rev), SS.rel(V[1, :m, :m].cpu().numpy(), V_rev))
        print(shape, name, "ar / V / ar reversed / V reversed against the oracle:", " ".join(f"{e:.2e}" for e in err))
        assert max(err) <= o["tol"], (name, err, o["tol"])
        assert np.allclose(ld[0].cpu().numpy(), o["logdet"], rtol=1e-9, atol=1e-9), name
        assert not bool(ar[:, m:, :, :].any()) and not bool(ar[:, :, m:, :].any())
    assert torch.equal(a1, a2) and torch.equal(v1, v2) and torch.equal(l1, l2)
    assert not bool(i1.any()) and not bool(i2.any()) and bool(torch.isfinite(a1).all()) and bool(torch.isfinite(v1).all())
    e_ar, e_V = SS.rel(a1[0, :m, :m].cpu().numpy(), o["ar"]), SS.rel(v1[0, :m, :m].cpu().numpy(), o["V"])
    e_ld = float(np.abs(l1[0].cpu().numpy() - o["logdet"]).max())
    print(shape, f"block LDL^T against the oracle: ar {e_ar:.2e} V {e_V:.2e} log det (abs) {e_ld:.2e}")


@pytest.mark.parametrize("crit", ["AIC", "HQ", "SC"])
@pytest.mark.parametrize("case", SS.AUTO_HIGH_ORDER_SHAPES, ids=SS.shape_id)
def test_k2_automatic_order_up_to_32(case, crit):
    m, pmax, n = case
    eng, x, xd, rec, st, R = _device(case)
    curve = O.mvar_criterion(x, pmax, crit)[0]
    q, gap = SS.criterion_gap(curve)
    assert gap >= SS.GAP, (case, crit, gap)
    ar, V, orders, got_curve, info = eng.yw_solve_auto(R, m, n, crit)
    assert int(info[0]) == 0 and int(orders[0]) == q
    assert np.allclose(got_curve[0].cpu().numpy(), curve, rtol=1e-9, atol=1e-10)
    aro, Vo = O.ar_coeff(x, q)
    tol = 1e2 * SS.normal_matrix_cond(O, x, q) * SS.EPS
    assert tol <= SS.COND_TOL_CAP
    assert SS.rel(ar[0, :m, :m, :q].cpu().numpy(), aro) <= tol and SS.rel(V[0, :m, :m].cpu().numpy(), Vo) <= tol
    assert not bool(ar[0, :, :, q:].any())
    ff, o2, _ = eng.sliding_ffdtf(xd, rec, st, n, None, FREQS, FS, max_model_order=pmax, crit_type=crit, return_orders=True)
    assert int(o2[0]) == q and SS.rel(ff[0].cpu().numpy(), O.full_freq_dtf(x, FREQS, FS, q)) <= 1e-8


# ----------------------------------------------------------------------------------------------------------- K3
@pytest.mark.parametrize("m", [57, 64])
@pytest.mark.parametrize("p", [17, 23, 24, 25, 31, 32])
def test_hand_scheduled_k3_body_equals_compiler_body_at_high_orders(m, p):
    """test_hand_scheduled_k3_body_equals_compiler_body beyond p = 16: whole chunks of eight lags (24, 32), chunks plus
    lag pairs (17, 23, 25, 31: also the zero padding lag of an odd order).  Coefficients N(0, 1/m) * 0.3 * sqrt(16 / p):
    the sum over the lags keeps the size it has at that test's (64, 16, 16, 0.3)."""
    eng = default_engine()
    F, items = 16, 5
    assert eng.pad(m) == 64
    rng = np.random.default_rng(100 * p + m)
    ar = np.zeros((items, 64, 64, p))
    ar[:, :m, :m, :] = 0.3 * np.sqrt(16.0 / p) * rng.standard_normal((items, m, m, p)) / np.sqrt(m)
    ar[:, np.arange(m), np.arange(m), 0] += 0.4
    freqs = np.linspace(1.0, 200.0, F)
    tw = eng.twiddles(freqs, 500.0, p)
    ard = eng.to_device(ar)
    outs = {}
    for form in (1, 2):
        with tuning(eng, _lib.TUNE_K3_FORM, form):
            outs[form] = eng.transfer(ard, m, tw, want_P=True, want_H=True)
            torch.cuda.synchronize()
    a, b = outs[1], outs[2]
    assert not bool(a["info"].any()) and not bool(b["info"].any())
    for k in ("H", "P", "rowsum", "info"):
        assert torch.equal(a[k], b[k]), k
    for it in (0, items - 1):
        H = torch.view_as_complex(b["H"])[it, :, :m, :m].cpu().numpy()
        z = np.exp(-(np.arange(p) + 1) * 2 * np.pi * 1j * freqs[:, None] / 500.0)
        want = np.linalg.inv(np.eye(m)[None] - np.einsum("ijk,fk->fij", ar[it, :m, :m, :], z))
        assert np.abs(H - want).max() / np.abs(want).max() < 1e-9


@pytest.mark.parametrize("m", [19, 33])
def test_transfer_function_at_p32(m):
    rng = np.random.default_rng(m)
    ar = 0.3 * np.sqrt(0.5) * rng.standard_normal((m, m, 32)) / np.sqrt(m)
    ar[np.arange(m), np.arange(m), 0] += 0.4
    H, A = M.mvar_transfer_function(ar, FREQS, FS)
    Ho, Ao = O.mvar_transfer_function(ar, FREQS, FS)
    assert SS.rel(H, Ho) <= 1e-9 and SS.rel(A, Ao) <= 1e-9


# --------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("shape", [(19, 32, 2000), (64, 32, 6000)], ids=SS.shape_id)
def test_sliding_calls_at_p32(shape):
    m, p, n = shape
    eng = default_engine()
    hop, nw = n // 2, 3
    x = synthetic_var_dyad(SS.HIGH_ORDER_SEED, m=m, p=4, T=n + hop * (nw - 1), burn=300)
    xd = eng.to_device(x[None])
    starts = hop * np.arange(nw)
    rec, st = window_items(1, starts, eng.device)
    lo, hi = hd.band_bins(FREQS, ((0.0, 8.0), (8.0, 30.0), (30.0, 101.0)))
    ff = eng.sliding_ffdtf(xd, rec, st, n, p, FREQS, FS)
    ffg = eng.sliding_ffdtf(xd, rec, st, n, p, FREQS, FS, grid=regular_grid(starts, n, p))
    bands = eng.sliding_ffdtf(xd, rec, st, n, p, FREQS, FS, bands=(lo, hi))
    dd = eng.sliding_ddtf(xd, rec, st, n, p, FREQS, FS)
    gp = eng.sliding_gpdc(xd, rec, st, n, p, FREQS, FS)
    torch.cuda.synchronize()
    assert float((ff.sum(dim=(2, 3)) - 1).abs().max()) < 1e-12
    assert torch.equal(bands, eng.band_sums(ff, lo, hi))
    assert rel_t(ffg, ff) <= 1e-8
    for w, s in enumerate(starts):
        xw = x[:, s:s + n]
        assert SS.rel(ff[w].cpu().numpy(), O.full_freq_dtf(xw, FREQS, FS, p)) <= 1e-8
        assert SS.rel(gp[w].cpu().numpy(), O.gen_partial_directed_coherence(xw, FREQS, FS, p)) <= 1e-8
        if m <= 19:
            assert SS.rel(dd[w].cpu().numpy(), O.direct_dtf(xw, FREQS, FS, p)) <= 1e-7
    assert SS.rel(dd[nw - 1].cpu().numpy(), SS.ddtf_restated(O, x[:, starts[-1]:starts[-1] + n], FREQS, FS, p)) <= 1e-8


# ------------------------------------------------------------------------------------------ validation and FAD
def test_model_validation_at_p32_with_32_lags():
    """p = 32 and max_lag = 32: the residual kernel's halo at its edge, on 19 channels (32 padded)."""
    eng = default_engine()
    m, p, n, h = 19, 32, 2000, 32
    _, x, xd, rec, st, R = _device((m, p, n))
    ar, _, _, info = eng.yw_solve(R, m)
    assert not bool(info.any())
    val = eng.model_validation(xd, rec, st, n, ar, h, return_residuals=True)
    arh = ar[:, :m, :m].cpu().numpy()
    for it, xw in enumerate((x, x[:, ::-1])):
        E = val["residuals"][it].cpu().numpy()
        assert np.all(np.abs(E - VR.residuals(xw, arh[it])) <= VR.residual_bound(xw, arh[it]))
        want = VR.validate_window(xw, arh[it], h)
        assert int(val["info"][it]) == 0
        for key in ("s", "q", "q_channel"):
            assert SS.rel(val[key][it].cpu().numpy(), want[key]) <= 1e-9, key
        # C_0 = E E^T / N from residuals within 2 (m p + 2) eps = 2.7e-13 of the restated ones, relative to |x| + sum |A| |x|
        assert SS.rel(val["resid_cov"][it].cpu().numpy(), want["resid_cov"]) <= 1e-11


def test_fad_at_p32_against_residuez():
    """FAD of four channels at model order 32: the scalar fit against a dense Toeplitz solve (1e2 * cond * eps), and the
    decomposition of the kernel's own coefficients against scipy.signal.residuez at the 1e-9 that
    test_fad_decompose_only_against_residuez documents for 32 poles."""
    from scipy.linalg import toeplitz
    from scipy.signal import residuez
    x = SS.high_order_input(4, 32, 400)
    for c in range(4):
        d = M.fad_decomposition(x[c], FS, model_order=32)
        n = x.shape[1]
        r = np.array([x[c, :n - k] @ x[c, k:] / n for k in range(33)])
        T = toeplitz(r[:32])
        a = np.linalg.solve(T, r[1:])
        assert d["model_order"] == 32
        assert SS.rel(d["ar_coeffs"], a) <= 1e2 * np.linalg.cond(T) * SS.EPS
        C, z, _ = residuez([1.0], np.r_[1.0, -d["ar_coeffs"]])
        idx = np.array([int(np.argmin(np.abs(d["poles"] - zz))) for zz in z])
        assert sorted(idx.tolist()) == list(range(32))
        assert np.all(np.abs(d["poles"][idx] - z) <= 1e-9 * np.maximum(1.0, np.abs(z)))
        assert np.all(np.abs(d["C"][idx] - C) <= 1e-9 * np.maximum(1.0, np.abs(C)))
