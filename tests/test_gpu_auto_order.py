"""Per-window automatic model order on the MI355X (`p=None` of `Engine.sliding_ffdtf` / `_ddtf` / `_gpdc` /
`_ffdtf_spectra`, `Engine.yw_solve_auto`, `sliding.sliding_*`, `escan_batch.run(model_order=None)`): pinned to the
reference's golden outputs, every window against the oracle's `mvar_criterion` and the oracle's measure at the oracle's
order, bit-identity with the fixed-order path, the invariants of the fused call, failures and the conditioning guard,
and the ESCan driver.  All @pytest.mark.gpu.

Orders: the GPU order must equal the oracle's for every window whose oracle gap (best criterion against the runner-up)
exceeds 1e-6; a window below it may take the runner-up; at most 2 % of a test's windows may lie below it.  On the
workloads used here none does (tests/test_auto_order_cpu.py shows that without a GPU)."""
import json

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import (hop_positions, regular_grid, sliding_ddtf, sliding_ffdtf,
                                                           sliding_ffdtf_device, sliding_gpdc, window_items)
    from hyperscanning_signal_analysis_amd.synthetic import mixed_order_recording, synthetic_var_dyad
    from tests.test_gpu_escan_batch import _reader, tree  # noqa: F401  (the fixture of the ESCan test, reused)

GUARD = 1e-9          # test_gpu_parity's guard for the golden vectors
GAP = 1e-6
EPS = np.finfo(np.float64).eps

# (m, n, hop, pmax, crit, orders, seg): the table of tests/test_auto_order_cpu.py
WORKLOADS = [
    (4, 160, 80, 20, "AIC", [1, 2, 3, 5, 8, 12], 1600),
    (4, 160, 80, 20, "HQ", [1, 2, 3, 5, 8, 12], 1600),
    (4, 160, 80, 20, "SC", [1, 2, 3, 5, 8, 12], 1600),
    (19, 1000, 500, 12, "AIC", [1, 2, 4, 6, 9], 6000),
    (32, 1000, 500, 10, "AIC", [1, 3, 5, 8], 5000),
    (64, 1000, 500, 8, "AIC", [1, 2, 4, 6], 4000),
]


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def assert_parity(out, ref, guard=GUARD):
    """The rule of tests/test_gpu_parity.py, restated."""
    assert out.shape == ref.shape
    assert rel(out, ref) <= guard, rel(out, ref)
    if np.isrealobj(ref):
        row_max = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).min()
    else:
        row_max = np.abs(ref).max()
    assert np.allclose(out, ref, rtol=1e-5, atol=1e-5 * row_max)


def ddtf_restated(xw, freqs, fs, p):
    """dDTF of one window from the oracle's fit by the algebra of the kernels (tests/test_gpu_sliding_conn.py, restated):
    |kappa_ij| = |W_ji| / sqrt(|W_ii| |W_jj|), W(f) = A(f)^T V^-1 A(f), kappa_ii = 1."""
    ar, V = O.ar_coeff(xw, p)
    _, A = O.mvar_transfer_function(ar, freqs, fs)
    Vi = np.linalg.inv(V)
    ff = O.full_freq_dtf(xw, freqs, fs, p)
    out = np.empty_like(ff)
    m = xw.shape[0]
    for k in range(len(freqs)):
        W = A[:, :, k].T @ Vi @ A[:, :, k]
        d = np.abs(np.diag(W))
        den = np.sqrt(np.outer(d, d))
        with np.errstate(divide="ignore", invalid="ignore"):
            kap = np.where(den != 0, np.abs(W.T) / den, 0.0)
        kap[np.arange(m), np.arange(m)] = 1.0
        out[:, :, k] = ff[:, :, k] * kap
    return out


def oracle_selection(x, pos, n, pmax, crit):
    curves, picks, gaps, runners = [], [], [], []
    for s in pos:
        c, _, popt = O.mvar_criterion(x[:, s:s + n], pmax, crit)
        order = np.argsort(c, kind="stable")
        curves.append(c)
        picks.append(int(popt))
        gaps.append(c[order[1]] - c[order[0]] if pmax > 1 else np.inf)
        runners.append(int(order[1]) + 1 if pmax > 1 else int(popt))
    return np.array(curves), np.array(picks), np.array(gaps), np.array(runners)


def check_selection(orders, crit, curves, picks, gaps, runners):
    """The rule of the module docstring; prints the figures before it asserts."""
    close = gaps <= GAP
    wrong = np.nonzero(orders != picks)[0]
    print(f"windows {len(picks)}, orders picked {np.bincount(picks).tolist()}, smallest gap {gaps.min():.3g}, "
          f"below the gap {int(close.sum())}, different from the oracle {len(wrong)}, "
          f"criterion max abs err {np.abs(crit - curves).max():.3g}")
    assert np.isfinite(curves).all()
    assert close.sum() <= 0.02 * len(picks)
    for w in wrong:
        assert close[w] and orders[w] == runners[w], (w, orders[w], picks[w], gaps[w])
    assert np.allclose(crit, curves, rtol=1e-9, atol=1e-10)


def _workload(case):
    m, n, hop, pmax, crit, orders, seg = case
    eng = default_engine()
    x = mixed_order_recording(100, m, orders, seg)
    pos = hop_positions(x.shape[1], n, hop)
    xd = eng.to_device(x[None])
    rec, st = window_items(1, pos, eng.device)
    return eng, x, xd, pos, rec, st


# ----------------------------------------------------------------------------- golden pins
@pytest.mark.parametrize("crit", ["AIC", "HQ", "SC"])
def test_g1_one_window_automatic_order(golden, crit):
    g = golden("g1_config1.npz")
    x, fs, freqs = g["x"], float(g["fs"]), g["freqs"]
    ff, orders, curve = sliding_ffdtf(x, x.shape[1], 1, None, freqs, fs, max_model_order=10, crit_type=crit, return_orders=True)
    assert ff.shape == (1,) + g["ffdtf_auto"].shape and orders.shape == (1,) and curve.shape == (1, 10)
    assert orders.dtype == np.int32 and int(orders[0]) == int(g[f"crit_{crit}_popt"])
    assert np.allclose(curve[0], g[f"crit_{crit}"], rtol=1e-9, atol=1e-10)
    if crit == "AIC":
        assert_parity(ff[0], g["ffdtf_auto"])


def test_g4_global_window_automatic_order(golden):
    g = golden("g4_config4.npz")
    x, fs, freqs = g["x"], float(g["fs"]), g["freqs"]
    ff, orders, _ = sliding_ffdtf(x, x.shape[1], 1, None, freqs, fs, return_orders=True)     # the defaults: 20, AIC
    assert int(orders[0]) == int(g["p_opt_auto"])
    assert_parity(ff[0], g["ff_global_auto"])


# ----------------------------------------------------------------------------- every window against the oracle
@pytest.mark.parametrize("case", WORKLOADS, ids=lambda c: f"m{c[0]}-{c[4]}")
def test_every_window_vs_oracle(case):
    m, n, hop, pmax, crit, _, _ = case
    eng, x, xd, pos, rec, st = _workload(case)
    fs, F = 250.0, 16
    freqs = np.linspace(1.0, 100.0, F)
    grid = regular_grid(pos, n, pmax)
    kw = dict(max_model_order=pmax, crit_type=crit, return_orders=True, grid=grid)
    ff, orders_t, crit_t = eng.sliding_ffdtf(xd, rec, st, n, None, freqs, fs, **kw)
    dd, o_d, c_d = eng.sliding_ddtf(xd, rec, st, n, None, freqs, fs, **kw)
    gp, o_g, c_g = eng.sliding_gpdc(xd, rec, st, n, None, freqs, fs, **kw)
    assert torch.equal(o_d, orders_t) and torch.equal(o_g, orders_t) and torch.equal(c_d, crit_t) and torch.equal(c_g, crit_t)
    ff, dd, gp, orders, curve = (t.cpu().numpy() for t in (ff, dd, gp, orders_t, crit_t))
    assert orders.dtype == np.int32 and orders.shape == (len(pos),) and curve.shape == (len(pos), pmax)
    curves, picks, gaps, runners = oracle_selection(x, pos, n, pmax, crit)
    check_selection(orders, curve, curves, picks, gaps, runners)
    if crit == "AIC":
        assert len(np.unique(orders)) >= 4
    if m == 19:
        lo, hi = hd.band_bins(freqs, ((1.0, 8.0), (8.0, 30.0), (30.0, 100.0)))
        kb = dict(max_model_order=pmax, crit_type=crit, grid=grid, bands=(lo, hi))
        bands = {"ffdtf": eng.sliding_ffdtf(xd, rec, st, n, None, freqs, fs, **kb).cpu().numpy(),
                 "ddtf": eng.sliding_ddtf(xd, rec, st, n, None, freqs, fs, **kb).cpu().numpy(),
                 "gpdc": eng.sliding_gpdc(xd, rec, st, n, None, freqs, fs, **kb).cpu().numpy()}
        ff2, S, o_s, c_s = eng.sliding_ffdtf_spectra(xd, rec, st, n, None, freqs, fs, max_model_order=pmax, crit_type=crit,
                                                     grid=grid, return_orders=True)
        assert torch.equal(o_s, orders_t) and torch.equal(c_s, crit_t)
        assert np.array_equal(ff2.cpu().numpy(), ff)
        S = S.cpu().numpy()
    for w, s in enumerate(pos):
        if orders[w] != picks[w]:
            continue                                   # (a window below the gap that took the runner-up: none here)
        xw, q = x[:, s:s + n], int(picks[w])
        want_f = O.full_freq_dtf(xw, freqs, fs, q)
        assert_parity(ff[w], want_f, 1e-8)
        want_g = O.gen_partial_directed_coherence(xw, freqs, fs, q)
        assert np.abs(gp[w] - want_g).max() <= 1e-8, (w, np.abs(gp[w] - want_g).max())
        if m <= 19:
            want_d = O.direct_dtf(xw, freqs, fs, q)
            assert np.abs(dd[w] - want_d).max() <= 1e-7, (w, np.abs(dd[w] - want_d).max())
        else:
            want_d = ddtf_restated(xw, freqs, fs, q)
            assert np.abs(dd[w] - want_d).max() <= 1e-10, (w, np.abs(dd[w] - want_d).max())
        if m == 19:
            assert_parity(S[w], O.multivariate_spectra(xw, freqs, fs, q), 1e-8)
            for name, want, tol in (("ffdtf", want_f, 1e-8), ("ddtf", want_d, 1e-7), ("gpdc", want_g, 1e-8)):
                wb = np.stack([want[:, :, a:b].sum(axis=2) for a, b in zip(lo, hi)], axis=2)
                assert bands[name][w].shape == wb.shape
                assert np.abs(bands[name][w] - wb).max() <= tol * (hi - lo).max(), (name, w)


def test_k2_alone_matches_the_fused_call():
    """`Engine.yw_solve_auto` on K1's lag covariances at pmax: the same orders, curves, coefficients and V as the fused call."""
    case = WORKLOADS[3]
    m, n, hop, pmax, crit, _, _ = case
    eng, x, xd, pos, rec, st = _workload(case)
    freqs = np.linspace(1.0, 100.0, 16)
    _, ar, V, (iy, _), orders, curve = eng.sliding_ffdtf(xd, rec, st, n, None, freqs, 250.0, max_model_order=pmax,
                                                         crit_type=crit, return_ar=True, return_orders=True,
                                                         flags=_lib.FLAG_DIRECT_LAGCOV)
    R = eng.lagcov(xd, rec, st, n, pmax)
    ar2, V2, orders2, curve2, info2 = eng.yw_solve_auto(R, m, n, crit)
    assert torch.equal(ar, ar2) and torch.equal(V, V2) and torch.equal(orders, orders2) and torch.equal(curve, curve2)
    assert not bool(info2.any()) and not bool(iy.any())
    # the log determinants of the fixed-order solve at pmax are the criterion's terms
    _, _, logdet, _ = eng.yw_solve(R, m, want_logdet=True)
    pen = 2.0 * np.arange(1, pmax + 1) * m * m / n
    assert np.allclose(logdet.cpu().numpy() + pen, curve.cpu().numpy(), rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match="Invalid criterion type"):
        eng.yw_solve_auto(R, m, n, "BIC")


# ----------------------------------------------------------------------------- same as the fixed-order path
@pytest.mark.parametrize("case", [WORKLOADS[0], WORKLOADS[3], WORKLOADS[5]], ids=lambda c: f"m{c[0]}")
def test_same_bits_as_the_fixed_order_path(case):
    """Windows grouped by selected order q against `sliding_<measure>(..., p=q)` on the same windows.  The recursion to
    order q is a prefix of the recursion to pmax, K1's sum for lag l does not depend on how many lags are asked for, and
    the padded lags are exact zeros in every later stage: with the direct K1 (HMV_FLAG_DIRECT_LAGCOV) the results are
    bit-identical -- observed, and asserted here.  On the regular grid K1 assembles the windows from hop-block sums and
    subtracts the products that reach past the window end; that form is held to the ~1e-16 relative on R its
    documentation gives, propagated as 1e2 cond eps (cond of the order-q normal equations, taken as 1e4 from the
    benchmark's well-conditioned windows: DESIGN.md section 5) on the outputs."""
    m, n, hop, pmax, crit, _, _ = case
    eng, x, xd, pos, rec, st = _workload(case)
    fs = 250.0
    freqs = np.linspace(1.0, 100.0, 32)
    lo, hi = hd.band_bins(freqs, ((1.0, 8.0), (8.0, 30.0)))
    direct = _lib.FLAG_DIRECT_LAGCOV
    for meas in ("ffdtf", "ddtf", "gpdc"):
        fn = getattr(eng, "sliding_" + meas)
        out, ar, V, _, orders, _ = fn(xd, rec, st, n, None, freqs, fs, max_model_order=pmax, crit_type=crit, return_ar=True,
                                      return_orders=True, flags=direct)
        red = fn(xd, rec, st, n, None, freqs, fs, max_model_order=pmax, crit_type=crit, flags=direct, bands=(lo, hi))
        grid = regular_grid(pos, n, pmax)
        out_g = fn(xd, rec, st, n, None, freqs, fs, max_model_order=pmax, crit_type=crit, grid=grid)
        assert int(orders.min()) >= 1
        for q in torch.unique(orders).tolist():
            sel = torch.nonzero(orders == q).flatten()
            o2, a2, V2, _ = fn(xd, rec[sel], st[sel], n, q, freqs, fs, return_ar=True, flags=direct)
            assert torch.equal(ar[sel][..., :q], a2), (meas, q)
            assert not bool(ar[sel][..., q:].any()) and not bool(torch.signbit(ar[sel][..., q:]).any())     # +0.0 exactly
            assert torch.equal(V[sel], V2), (meas, q)
            assert torch.equal(out[sel], o2), (meas, q)
            r2 = fn(xd, rec[sel], st[sel], n, q, freqs, fs, flags=direct, bands=(lo, hi))
            assert torch.equal(red[sel], r2), (meas, q)
            err = float((out_g[sel] - o2).abs().max() / o2.abs().max())
            assert err <= 1e2 * 1e4 * EPS, (meas, q, err)


# ----------------------------------------------------------------------------- invariance
def test_invariants_chunk_grid_and_empty_batch():
    case = WORKLOADS[3]
    m, n, hop, pmax, crit, _, _ = case
    eng, x, xd, pos, rec, st = _workload(case)
    fs = 250.0
    freqs = np.linspace(1.0, 100.0, 32)
    grid = regular_grid(pos, n, pmax)
    assert grid is not None
    lo, hi = hd.band_bins(freqs, ((1.0, 8.0), (8.0, 30.0), (30.0, 100.0)))
    kw = dict(max_model_order=pmax, crit_type=crit, return_orders=True)
    for meas in ("ffdtf", "ddtf", "gpdc"):
        fn = getattr(eng, "sliding_" + meas)
        for bands in (None, (lo, hi)):
            runs = {c: fn(xd, rec, st, n, None, freqs, fs, chunk=c, grid=grid, bands=bands, **kw) for c in (1, 7, None)}
            for c in (1, 7):
                for a, b in zip(runs[c], runs[None]):
                    assert torch.equal(a, b), (meas, c)                      # bit-identical whatever the chunk
        full, orders, curve = fn(xd, rec, st, n, None, freqs, fs, grid=grid, **kw)
        d_full, d_orders, d_curve = fn(xd, rec, st, n, None, freqs, fs, flags=_lib.FLAG_DIRECT_LAGCOV, **kw)
        assert torch.equal(d_orders, orders)
        assert float((d_curve - curve).abs().max()) < 1e-9
        assert rel(d_full.cpu().numpy(), full.cpu().numpy()) < 1e-9          # as the fixed-order entries agree
        e = torch.zeros(0, dtype=torch.int64, device=eng.device)
        out0, o0, c0 = fn(xd, e, e, n, None, freqs, fs, **kw)
        assert tuple(out0.shape) == (0, m, m, 32) and tuple(o0.shape) == (0,) and o0.dtype == torch.int32
        assert tuple(c0.shape) == (0, pmax)
        assert tuple(fn(xd, e, e, n, None, freqs, fs, bands=(lo, hi), max_model_order=pmax).shape) == (0, m, m, 3)
    f0, S0, o0, c0 = eng.sliding_ffdtf_spectra(xd, e, e, n, None, freqs, fs, max_model_order=pmax, return_orders=True)
    assert tuple(f0.shape) == tuple(S0.shape) == (0, m, m, 32) and S0.is_complex() and tuple(o0.shape) == (0,)
    # the wrappers: shapes, and the same bits as the engine
    ffw, ow, cw = sliding_ffdtf_device(xd, n, len(pos), None, freqs, fs, max_model_order=pmax, crit_type=crit,
                                       return_orders=True)
    assert tuple(ffw.shape) == (1, len(pos), m, m, 32) and tuple(ow.shape) == (1, len(pos)) and tuple(cw.shape) == (1, len(pos), pmax)
    hd_ = sliding_ddtf(x, n, None, None, freqs, fs, hop=hop, max_model_order=pmax, crit_type=crit)
    hg, og, _ = sliding_gpdc(x, n, None, None, freqs, fs, hop=hop, max_model_order=pmax, crit_type=crit, return_orders=True)
    assert hd_.shape == hg.shape == (len(pos), m, m, 32) and og.shape == (len(pos),)
    assert np.array_equal(hg, eng.sliding_gpdc(xd, rec, st, n, None, freqs, fs, grid=grid, max_model_order=pmax).cpu().numpy())
    # an integer p is the fixed-order call, whatever the new keywords say
    a = eng.sliding_ffdtf(xd, rec, st, n, 4, freqs, fs, grid=regular_grid(pos, n, 4))
    b = eng.sliding_ffdtf(xd, rec, st, n, 4, freqs, fs, grid=regular_grid(pos, n, 4), max_model_order=2, crit_type="SC",
                          return_orders=True)
    assert isinstance(b, torch.Tensor) and torch.equal(a, b)
    with pytest.raises(ValueError, match="Invalid criterion type"):
        eng.sliding_ffdtf(xd, rec, st, n, None, freqs, fs, crit_type="FPE")
    with pytest.raises(ValueError, match="must exceed max_model_order"):
        eng.sliding_gpdc(xd, rec, st, 20, None, freqs, fs)
    with pytest.raises(ValueError, match="not offered here yet"):
        eng.sliding_significance(xd, rec, st, n, None, freqs, fs, (lo, hi), measure="ffdtf", null="shift", n_surrogates=4,
                                 seed=0, split=9)


# ----------------------------------------------------------------------------- failure and guard
def test_failed_windows_are_masked_and_leave_the_others_alone(golden):
    """Ordinary windows with g6 `xz` (a dead channel) and g6 `xs` (exactly rank deficient) among them: check="mask" flags
    exactly the windows for which the oracle's mvar_criterion raises or returns a non-finite curve, their order is 0, and
    the other windows are the bits of a run without the bad ones."""
    g = golden("g6_errors.npz")
    eng = default_engine()
    m, n = g["xz"].shape
    pmax, fs = 6, 64.0
    freqs = np.linspace(1.0, 30.0, 16)
    good = mixed_order_recording(100, m, [1, 2, 3, 5], n)
    batch = np.stack([good[:, :n], g["xz"], good[:, n:2 * n], good[:, 2 * n:3 * n], g["xs"][:, :n], good[:, 3 * n:4 * n]])
    expect = []
    for xw in batch:
        try:
            with np.errstate(all="ignore"):
                c = O.mvar_criterion(xw, pmax, "AIC")[0]
            expect.append(not np.isfinite(c).all())
        except np.linalg.LinAlgError:
            expect.append(True)
    assert expect == [False, True, False, False, True, False]
    xd = eng.to_device(batch)
    W = len(batch)
    rec = torch.arange(W, dtype=torch.int64, device=eng.device)
    st = torch.zeros(W, dtype=torch.int64, device=eng.device)
    keep = torch.as_tensor([k for k in range(W) if not expect[k]], device=eng.device)
    for meas in ("ffdtf", "ddtf", "gpdc"):
        fn = getattr(eng, "sliding_" + meas)
        out, bad, orders, curve = fn(xd, rec, st, n, None, freqs, fs, max_model_order=pmax, check="mask", return_orders=True)
        assert bad.cpu().tolist() == expect, meas
        assert (orders.cpu().numpy() == 0).tolist() == expect
        ref, ref_orders, ref_curve = fn(xd, rec[keep], st[keep], n, None, freqs, fs, max_model_order=pmax, return_orders=True)
        assert torch.equal(out[keep], ref) and torch.equal(orders[keep], ref_orders) and torch.equal(curve[keep], ref_curve)
        with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
            fn(xd, rec, st, n, None, freqs, fs, max_model_order=pmax)
        assert list(ei.value.items) == [1, 4]
        nan = fn(xd, rec, st, n, None, freqs, fs, max_model_order=pmax, check="nan")
        assert bool(torch.isnan(nan[[1, 4]]).all()) and torch.equal(nan[keep], ref)


def test_guarded_windows_are_re_solved_at_their_own_order(golden):
    """The nearly collinear g6 windows nc0..nc2 (cond 2e5, 2e9, 2e13) with max_model_order=3, against the oracle at the
    selected order, to the 1e2 cond eps that tests/test_gpu_parity.py applies to them; an ordinary window rides along.  The
    windows whose inverses trip the recursion's guard come out with the bits of the block LDL^T at their own order."""
    g = golden("g6_errors.npz")
    eng = default_engine()
    m, n = g["nc0_x"].shape
    pmax = 3
    ordinary = synthetic_var_dyad(43, m=m, p=3, T=n, burn=300)
    batch = np.stack([g["nc0_x"], ordinary, g["nc1_x"], g["nc2_x"]])
    conds = [float(g["nc0_cond"]), None, float(g["nc1_cond"]), float(g["nc2_cond"])]
    xd = eng.to_device(batch)
    W = len(batch)
    rec = torch.arange(W, dtype=torch.int64, device=eng.device)
    st = torch.zeros(W, dtype=torch.int64, device=eng.device)
    R = eng.lagcov(xd, rec, st, n, pmax)
    ar, V, orders, curve, info = eng.yw_solve_auto(R, m, n, "AIC")
    torch.cuda.synchronize()
    orders, info = orders.cpu().numpy(), info.cpu().numpy()
    tripped = 0
    for k in range(W):
        if info[k] != 0:                            # refused: only acceptable far beyond what float64 resolves
            assert conds[k] is not None and conds[k] > 1e12 and orders[k] == 0, (k, conds[k])
            continue
        q = int(orders[k])
        assert 1 <= q <= pmax
        aro, Vo = O.ar_coeff(batch[k], q)
        tol = 1e2 * (conds[k] if conds[k] is not None else 1e4) * EPS
        assert rel(ar[k, :m, :m, :q].cpu().numpy(), aro) <= tol, (k, q, rel(ar[k, :m, :m, :q].cpu().numpy(), aro), tol)
        assert rel(V[k, :m, :m].cpu().numpy(), Vo) <= tol
        assert not bool(ar[k, :, :, q:].any())
        # the block LDL^T and the recursion at this window's order: which one are these bits?
        Rq = R[k:k + 1, :q + 1].contiguous()
        a_ldl, v_ldl, _, _ = eng.yw_solve(Rq, m, flags=_lib.FLAG_YW_ONE_LAUNCH)
        a_fix, v_fix, _, _ = eng.yw_solve(Rq, m)                     # recursion + its own guard at order q
        is_ldl = torch.equal(ar[k:k + 1, :, :, :q], a_ldl) and torch.equal(V[k:k + 1], v_ldl)
        tripped += int(is_ldl)
        if not is_ldl:
            assert torch.equal(ar[k:k + 1, :, :, :q], a_fix) and torch.equal(V[k:k + 1], v_fix), k
    print(f"orders {orders.tolist()}, info {info.tolist()}, windows re-solved by the block LDL^T at their own order: {tripped}")
    assert int(info[0]) == 0 and int(info[1]) == 0 and int(info[2]) == 0       # cond <= 2e9 must not be refused
    assert tripped >= 1                                                        # the per-window-order re-solve ran


# ----------------------------------------------------------------------------- ESCan
def test_escan_automatic_order(tree, tmp_path):  # noqa: F811
    freqs = np.arange(1.0, 33.0, 1.0)
    kw = dict(window_s=2.0, overlap=0.5, freqs=freqs, low_cutoff_hz=1.0, high_cutoff_hz=45.0, reader=_reader, verbose=False)
    auto = EB.run(tree, tmp_path / "auto", model_order=None, max_model_order=6, crit_type="HQ",
                  measures=("ffdtf", "gpdc"), **kw)
    fix_a = EB.run(tree, tmp_path / "fix_a", model_order=8, **kw)
    fix_b = EB.run(tree, tmp_path / "fix_b", model_order=8, max_model_order=3, crit_type="SC", **kw)
    assert auto["done"] == fix_a["done"] == fix_b["done"] == ["W_003", "W_010"]
    eng = default_engine()
    found = EB.discover_dyads(tree)
    lo, hi = hd.band_bins(freqs)
    for dy in auto["done"]:
        z = np.load(tmp_path / "auto" / f"{dy}_ffdtf.npz", allow_pickle=False)
        za = np.load(tmp_path / "fix_a" / f"{dy}_ffdtf.npz", allow_pickle=False)
        zb = np.load(tmp_path / "fix_b" / f"{dy}_ffdtf.npz", allow_pickle=False)
        meta, ma, mb = (json.loads(str(f["meta"])) for f in (z, za, zb))
        assert meta["model_order"] == "auto" and meta["max_model_order"] == 6 and meta["crit_type"] == "HQ"
        # an integer model_order: the same keys, arrays and meta as without the new keywords
        assert ma["model_order"] == mb["model_order"] == 8 and "max_model_order" not in ma and "crit_type" not in ma
        ma.pop("created"); mb.pop("created")
        assert ma == mb and za.files == zb.files
        for k in za.files:
            if k != "meta":
                assert za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f"), k
        assert not [k for k in za.files if k.endswith("/orders")]
        assert set(z.files) - set(za.files) == {f"{s['task']}/{s['event']}/{k}" for s in meta["segments"]
                                                for k in ("orders", "gpdc_bands")}
        for seg in meta["segments"]:
            key = f"{seg['task']}/{seg['event']}"
            recs = {r: _reader(found[dy][seg["task"]][r]) for r in ("ch", "cg")}
            block, _, fs = EB.segment_block(recs["ch"], recs["cg"], seg["start_s"], seg["duration_s"], 1.0, 45.0)
            W = seg["window"]
            xd = eng.to_device(block[None])
            pos = z[f"{key}/starts"]
            rec, st = window_items(1, pos, eng.device)
            grid = regular_grid(pos, W, 6)
            want, orders, _ = eng.sliding_ffdtf(xd, rec, st, W, None, freqs, fs, max_model_order=6, crit_type="HQ", check="nan",
                                                grid=grid, bands=(lo, hi), return_orders=True)
            assert z[f"{key}/orders"].dtype == np.int32 and z[f"{key}/orders"].shape == (len(pos),)
            assert np.array_equal(z[f"{key}/orders"], orders.cpu().numpy())
            assert np.array_equal(z[f"{key}/ffdtf_bands"], want.cpu().numpy(), equal_nan=True)
            gw = eng.sliding_gpdc(xd, rec, st, W, None, freqs, fs, max_model_order=6, crit_type="HQ", check="nan", grid=grid,
                                  bands=(lo, hi))
            assert np.array_equal(z[f"{key}/gpdc_bands"], gw.cpu().numpy(), equal_nan=True)
            # ... and the orders are the oracle's
            curves, picks, gaps, runners = oracle_selection(block, pos, W, 6, "HQ")
            for w_, got in enumerate(z[f"{key}/orders"]):
                assert got == picks[w_] or (gaps[w_] <= GAP and got == runners[w_]), (key, w_, got, picks[w_], gaps[w_])
