"""Sliding-window dDTF and GPDC on the MI355X (`Engine.sliding_ddtf` / `sliding_gpdc`, `sliding.sliding_ddtf` /
`sliding_gpdc`, `escan_batch.run(measures=...)`): pinned to the reference's golden outputs, every window against the
oracle (and, where the oracle's minors are too slow, against a NumPy restatement of W = A^T V^-1 A), the invariants
of the fused path, the failure modes and the ESCan driver.  All @pytest.mark.gpu."""
import json

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd import mtmvar as M
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import (hop_positions, regular_grid, sliding_ddtf, sliding_ddtf_device,
                                                           sliding_gpdc, sliding_gpdc_device,
                                                           window_items, window_positions)
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad
    from tests.test_gpu_escan_batch import _reader, tree  # noqa: F401  (the fixture of the ESCan test, reused)

GUARD = 1e-9          # test_gpu_parity's guard for the golden vectors


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _signal(n_rec, m, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rec, m, T))
    x[..., 1:] += 0.5 * x[..., :-1]
    x[:, 1:] += 0.3 * x[:, :-1]
    return x


def ddtf_restated(xw, freqs, fs, p):
    """dDTF of one window from the oracle's fit, by the algebra of the kernels: |kappa_ij| = |W_ji| / sqrt(|W_ii| |W_jj|)
    with W(f) = A(f)^T V^-1 A(f) (plain transpose), kappa_ii = 1, 0 where the denominator vanishes."""
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


def test_g7_one_window_covers_the_signal(golden):
    """One window over the whole signal reproduces the reference's direct_dtf / gen_partial_directed_coherence."""
    g = golden("g7_connectivity.npz")
    for tag in "abc":
        x, fs, freqs, p = g[f"x_{tag}"], float(g[f"fs_{tag}"]), g[f"freqs_{tag}"], int(g[f"p_{tag}"])
        T = x.shape[1]
        dd = sliding_ddtf(x, T, 1, p, freqs, fs)[0]
        gp = sliding_gpdc(x, T, 1, p, freqs, fs)[0]
        for got, want in ((dd, g[f"ddtf_{tag}"]), (gp, g[f"gpdc_{tag}"])):
            assert got.shape == want.shape
            assert rel(got, want) <= GUARD, (tag, rel(got, want))
            assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


@pytest.mark.parametrize("m,p,F", [(3, 1, 16), (8, 5, 30), (19, 8, 16)])
@pytest.mark.parametrize("grid", ["even", "hop"])
def test_every_window_vs_oracle(m, p, F, grid):
    fs, n = 100.0, 400
    x = _signal(2, m, 1200, 11 * m + p)
    freqs = np.linspace(1.0, 45.0, F)
    if grid == "even":
        pos, w = window_positions(1200, 4, n)
        dd = sliding_ddtf(x, n, 4, p, freqs, fs)
        gp = sliding_gpdc(x, n, 4, p, freqs, fs)
    else:
        pos, w = hop_positions(1200, n, n // 2), n
        dd = sliding_ddtf(x, n, None, p, freqs, fs, hop=n // 2)
        gp = sliding_gpdc(x, n, None, p, freqs, fs, hop=n // 2)
    assert dd.shape == gp.shape == (2, len(pos), m, m, F)
    for r in range(2):
        for k, s in enumerate(pos):
            xw = x[r, :, s:s + w]
            want_g = O.gen_partial_directed_coherence(xw, freqs, fs, p)
            assert np.abs(gp[r, k] - want_g).max() <= 1e-8, (r, k, np.abs(gp[r, k] - want_g).max())
            assert np.abs((gp[r, k] ** 2).sum(axis=0) - 1.0).max() < 1e-12          # columns of GPDC^2 sum to one
            want_d = O.direct_dtf(xw, freqs, fs, p)
            assert np.abs(dd[r, k] - want_d).max() <= 1e-7, (r, k, np.abs(dd[r, k] - want_d).max())
            if r == 0 and k == 0:
                assert np.abs(dd[r, k] - ddtf_restated(xw, freqs, fs, p)).max() <= 1e-10


@pytest.mark.parametrize("m,p", [(32, 5), (64, 8)])
def test_large_windows_vs_restatement_and_chain(m, p):
    """At 32 / 64 channels the oracle's minors are O(m^5 F): the NumPy restatement of the same algebra (1e-10) and the
    existing chain of batched calls, which inverts S (1e2 cond(S) eps)."""
    fs, n, F = 500.0, 1000, 16
    x = synthetic_var_dyad(5, m=m, p=p, T=2000, burn=500)
    freqs = np.linspace(1.0, 120.0, F)
    dd = sliding_ddtf(x, n, 2, p, freqs, fs)
    gp = sliding_gpdc(x, n, 2, p, freqs, fs)
    eps = np.finfo(np.float64).eps
    for k, s in enumerate(window_positions(2000, 2, n)[0]):
        xw = x[:, s:s + n]
        assert np.abs(dd[k] - ddtf_restated(xw, freqs, fs, p)).max() <= 1e-10
        assert np.abs(gp[k] - O.gen_partial_directed_coherence(xw, freqs, fs, p)).max() <= 1e-8
        S = O.multivariate_spectra(xw, freqs, fs, p)
        cond = max(np.linalg.cond(S[:, :, f]) for f in range(F))
        chain = M.mvar_analysis(xw, freqs, fs, p, want=("ddtf",))["ddtf"]
        assert np.abs(dd[k] - chain).max() <= 1e2 * cond * eps, (np.abs(dd[k] - chain).max(), cond)


def _device_case(m=8, p=4, T=1600, n=400, n_rec=2, seed=3):
    eng = default_engine()
    x = _signal(n_rec, m, T, seed)
    xd = eng.to_device(x)
    pos = hop_positions(T, n, n // 2)
    rec, st = window_items(n_rec, pos, eng.device)
    return eng, x, xd, pos, rec, st


def test_invariants_chunks_bands_grid():
    eng, x, xd, pos, rec, st = _device_case()
    n, p, fs = 400, 4, 128.0
    freqs = np.arange(1.0, 33.0)                                  # F = 32: K3's fused normalisation and band path
    grid = regular_grid(pos, n, p)
    assert grid is not None
    ff = eng.sliding_ffdtf(xd, rec, st, n, p, freqs, fs, grid=grid).cpu().numpy()
    runs = {}
    for meas, fn in (("ddtf", eng.sliding_ddtf), ("gpdc", eng.sliding_gpdc)):
        full = {c: fn(xd, rec, st, n, p, freqs, fs, chunk=c, grid=grid).cpu().numpy() for c in (1, 7, None)}
        for c in (1, 7):
            assert np.array_equal(full[c], full[None]), (meas, c)             # bit-identical whatever the chunk
        runs[meas] = full[None]
        direct = fn(xd, rec, st, n, p, freqs, fs).cpu().numpy()             # K1 without the shared overlap
        assert rel(direct, full[None]) < 1e-9
        lo, hi = hd.band_bins(freqs, ((1.0, 4.0), (4.0, 8.0), (8.0, 13.0), (13.0, 30.0)))
        red = fn(xd, rec, st, n, p, freqs, fs, grid=grid, bands=(lo, hi)).cpu().numpy()
        want = eng.band_sums(torch.as_tensor(full[None], device=eng.device), lo, hi).cpu().numpy()
        assert red.shape == want.shape == (len(rec), 8, 8, 4)
        assert np.abs(red - want).max() <= 1e-13 * np.abs(want).max()
        red7 = fn(xd, rec, st, n, p, freqs, fs, grid=grid, bands=(lo, hi), chunk=7).cpu().numpy()
        assert np.array_equal(red7, red)
    d = np.arange(8)
    assert np.array_equal(runs["ddtf"][:, d, d], ff[:, d, d])                 # kappa_ii = 1: ffDTF's diagonal, bitwise
    assert np.abs((runs["gpdc"] ** 2).sum(axis=1) - 1.0).max() < 1e-12
    # the device wrappers: shapes and the same bits as the engine
    dv = sliding_ddtf_device(xd, n, None, p, freqs, fs, hop=n // 2)
    gv = sliding_gpdc_device(xd, n, None, p, freqs, fs, hop=n // 2)
    assert dv.shape == gv.shape == (2, len(pos), 8, 8, 32)
    assert np.array_equal(dv.reshape(-1, 8, 8, 32).cpu().numpy(), runs["ddtf"])
    assert np.array_equal(gv.reshape(-1, 8, 8, 32).cpu().numpy(), runs["gpdc"])
    # return_ar: the fit of the ffDTF path
    _, ar, V, (iy, itf) = eng.sliding_ddtf(xd, rec, st, n, p, freqs, fs, grid=grid, return_ar=True)
    _, ar2, V2, iy2 = eng.sliding_gpdc(xd, rec, st, n, p, freqs, fs, grid=grid, return_ar=True)
    _, ar0, V0, _ = eng.sliding_ffdtf(xd, rec, st, n, p, freqs, fs, grid=grid, return_ar=True)
    assert torch.equal(ar, ar0) and torch.equal(V, V0) and torch.equal(ar2, ar0) and torch.equal(V2, V0)
    assert not iy.any() and not itf.any() and not iy2.any()


def test_singular_window_and_empty_batch():
    eng = default_engine()
    m, n, p, fs = 6, 300, 3, 100.0
    x = _signal(1, m, 4 * n, 21)
    x[0, 3, 2 * n:3 * n] = x[0, 0, 2 * n:3 * n] + x[0, 1, 2 * n:3 * n]      # window 2: collinear channels
    xd = eng.to_device(x)
    pos = np.arange(4) * n
    rec, st = window_items(1, pos, eng.device)
    freqs = np.linspace(1.0, 40.0, 16)
    for fn in (eng.sliding_ddtf, eng.sliding_gpdc):
        with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
            fn(xd, rec, st, n, p, freqs, fs)
        assert list(ei.value.items) == [2] and "item 2" in str(ei.value.args[1])
        nan = fn(xd, rec, st, n, p, freqs, fs, check="nan").cpu().numpy()
        assert np.isnan(nan[2]).all() and np.isfinite(nan[[0, 1, 3]]).all()
        out, bad = fn(xd, rec, st, n, p, freqs, fs, check="mask")
        assert bad.is_cuda and bad.cpu().tolist() == [False, False, True, False]
        assert torch.equal(out[bad == 0], torch.as_tensor(nan[[0, 1, 3]], device=eng.device))
        good = fn(xd, rec[[0, 1, 3]], st[[0, 1, 3]], n, p, freqs, fs).cpu().numpy()
        assert rel(good, nan[[0, 1, 3]]) < 1e-12
        e = torch.zeros(0, dtype=torch.int64, device=eng.device)
        assert tuple(fn(xd, e, e, n, p, freqs, fs).shape) == (0, m, m, 16)
        assert tuple(fn(xd, e, e, n, p, freqs, fs, bands=([0, 4], [4, 16])).shape) == (0, m, m, 2)


def test_escan_measures(tree, tmp_path):  # noqa: F811
    freqs = np.arange(1.0, 33.0, 1.0)
    kw = dict(window_s=2.0, overlap=0.5, model_order=3, freqs=freqs, low_cutoff_hz=1.0, high_cutoff_hz=45.0, reader=_reader,
              verbose=False)
    base = EB.run(tree, tmp_path / "plain", **kw)
    allm = EB.run(tree, tmp_path / "all", measures=("ffdtf", "ddtf", "gpdc"), save_full=False, **kw)
    full = EB.run(tree, tmp_path / "full", measures=("ffdtf", "gpdc"), save_full=True, **kw)
    assert base["done"] == allm["done"] == full["done"] == ["W_003", "W_010"]
    eng = default_engine()
    found = EB.discover_dyads(tree)
    for dy in base["done"]:
        z0 = np.load(tmp_path / "plain" / f"{dy}_ffdtf.npz", allow_pickle=False)
        z1 = np.load(tmp_path / "all" / f"{dy}_ffdtf.npz", allow_pickle=False)
        z2 = np.load(tmp_path / "full" / f"{dy}_ffdtf.npz", allow_pickle=False)
        m0, m1 = json.loads(str(z0["meta"])), json.loads(str(z1["meta"]))
        assert m0["measures"] == ["ffdtf"] and m1["measures"] == ["ffdtf", "ddtf", "gpdc"]
        assert set(z1.files) - set(z0.files) == {f"{s['task']}/{s['event']}/{k}" for s in m0["segments"]
                                                  for k in ("ddtf_bands", "gpdc_bands")}
        for seg in m1["segments"]:
            key = f"{seg['task']}/{seg['event']}"
            assert np.array_equal(z1[f"{key}/ffdtf_bands"], z0[f"{key}/ffdtf_bands"], equal_nan=True)
            recs = {r: _reader(found[dy][seg["task"]][r]) for r in ("ch", "cg")}
            block, _, fs = EB.segment_block(recs["ch"], recs["cg"], seg["start_s"], seg["duration_s"], 1.0, 45.0)
            W = seg["window"]
            lo, hi = hd.band_bins(freqs)
            xd = eng.to_device(block[None])
            pos = z1[f"{key}/starts"]
            rec, st = window_items(1, pos, eng.device)
            grid = regular_grid(pos, W, 3)
            for meas, fn in (("ddtf", eng.sliding_ddtf), ("gpdc", eng.sliding_gpdc)):
                want = fn(xd, rec, st, W, 3, freqs, fs, check="nan", grid=grid, bands=(lo, hi)).cpu().numpy()
                assert np.array_equal(z1[f"{key}/{meas}_bands"], want, equal_nan=True)
            gfull = eng.sliding_gpdc(xd, rec, st, W, 3, freqs, fs, check="nan", grid=grid).cpu().numpy()
            assert np.array_equal(z2[f"{key}/gpdc"], gfull, equal_nan=True)
            assert np.allclose(z2[f"{key}/gpdc_bands"], z1[f"{key}/gpdc_bands"], rtol=1e-13, atol=0.0, equal_nan=True)
    with pytest.raises(ValueError, match="measures"):
        EB.run(tree, tmp_path / "bad", measures=("ffdtf", "pdc"), **kw)
    assert not (tmp_path / "bad").exists()
