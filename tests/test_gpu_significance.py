"""Surrogate significance of the sliding-window measures on the MI355X (`Engine.sliding_significance`,
`sliding.sliding_significance`, `escan_batch.run(significance=...)`): the surrogate windows against NumPy, every statistic
against a NumPy restatement on the oracle, the observed values against `sliding_<measure>`, determinism and block
invariance, a planted inter-brain link, failed surrogates and windows, and the ESCan driver.  All @pytest.mark.gpu."""
import json

import numpy as np
import pytest
import torch

from hyperscanning_signal_analysis_amd import surrogates as sg
from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import (hop_positions, sliding_ddtf, sliding_gpdc, sliding_significance,
                                                           window_items)
    from hyperscanning_signal_analysis_amd import sliding as SL
    from tests.test_gpu_escan_batch import _reader, tree  # noqa: F401  (the fixture of the ESCan test, reused)

ORACLE = {"ffdtf": O.full_freq_dtf, "ddtf": O.direct_dtf, "gpdc": O.gen_partial_directed_coherence}
STATS = ("observed", "p", "p_fwe", "null_mean", "null_std", "n_valid")


def _signal(n_rec, m, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rec, m, T))
    x[..., 1:] += 0.5 * x[..., :-1]
    x[:, 1:] += 0.3 * x[:, :-1]
    return x


def planted_dyad(T, seed, weight=0.6):
    """Two independent 4-channel VAR(2) participants A (channels 0-3) and B (4-7) with one inter-brain link
    A0 -> B1 at lag 1."""
    rng = np.random.default_rng(seed)
    A1 = np.diag([0.55, 0.5, 0.6, 0.45])
    A1[1, 0] = A1[2, 1] = A1[3, 0] = 0.25                   # intra-brain flows, the same pattern in both participants
    A2 = np.diag([-0.35, -0.3, -0.4, -0.25])
    burn = 500
    e = rng.standard_normal((8, T + burn))
    x = np.zeros((8, T + burn))
    for t in range(2, T + burn):
        for off in (0, 4):
            s = slice(off, off + 4)
            x[s, t] = A1 @ x[s, t - 1] + A2 @ x[s, t - 2] + e[s, t]
        x[5, t] += weight * x[0, t - 1]
    return x[:, burn:]


def band_values(measure, xw, freqs, fs, p, lo, hi):
    v = ORACLE[measure](xw, freqs, fs, p)
    return np.stack([v[..., a:b].sum(-1) for a, b in zip(lo, hi)], axis=-1)


def restate(measure, null, x, pos, n, p, freqs, fs, lo, hi, S, seed, split, min_shift=None, tie=1e-9):
    """The whole test on the host from the documented draws and the oracle: (stats dict shaped (n_rec * W, m, m, nb),
    ties mask of the cells whose nearest surrogate value -- or maximum -- lies within `tie` relative of T_obs)."""
    n_rec, m, T = x.shape
    min_shift = n if min_shift is None else min_shift
    rng = np.random.default_rng(seed)
    if null == "shift":
        d = sg.shift_offsets(rng, S, n_rec, T, min_shift)
    else:
        phi = sg.phase_draws(rng, S, m, n)
    tested = sg.tested_mask(m, null, split)
    out = {k: [] for k in STATS}
    ties = []
    t = np.arange(n)
    for r in range(n_rec):
        for st in pos:
            xw = x[r, :, st:st + n]
            obs = band_values(measure, xw, freqs, fs, p, lo, hi)
            vals = []
            for s in range(S):
                if null == "shift":
                    xs = xw.copy()
                    xs[split:] = x[r, split:][:, (st + t + d[s, r]) % T]
                else:
                    xs = np.fft.irfft(np.fft.rfft(xw, axis=-1) * np.exp(1j * phi[s]), n, axis=-1)
                try:
                    vals.append(band_values(measure, xs, freqs, fs, p, lo, hi))
                except np.linalg.LinAlgError:
                    pass
            v = np.stack(vals)                                       # (n_valid, m, m, nb)
            M = np.where(tested[None, :, :, None], v, -np.inf).max(axis=(1, 2))      # (n_valid, nb)
            nv = len(vals)
            pv = (1.0 + (v >= obs).sum(0)) / (1.0 + nv)
            pf = (1.0 + (M[:, None, None, :] >= obs).sum(0)) / (1.0 + nv)
            mask = np.where(tested[:, :, None], 1.0, np.nan)
            out["observed"].append(obs)
            out["p"].append(pv * mask)
            out["p_fwe"].append(pf * mask)
            out["null_mean"].append(v.mean(0) * mask)
            out["null_std"].append(v.std(0, ddof=1) * mask)
            out["n_valid"].append(nv)
            scale = np.maximum(np.abs(obs), 1e-300)
            near = np.abs(v - obs).min(0) <= tie * scale
            near |= np.abs(M[:, None, None, :] - obs).min(0) <= tie * scale
            ties.append(near & tested[:, :, None])
    return {k: np.asarray(v) for k, v in out.items()}, np.asarray(ties)


def _same(a, b):
    """Bitwise equality, NaN == NaN for the float arrays."""
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind in "fc")


def _flat(res):
    return {k: (v.reshape((-1,) + v.shape[2:]) if k != "tested" else v) for k, v in res.items()}


# ---------------------------------------------------------------------------------------------------- 1. construction
def test_surrogate_construction():
    eng = default_engine()
    m, T, split = 6, 600, 3
    x = _signal(2, m, T, 5)
    xd = eng.to_device(x)
    for n in (200, 201):
        pos = hop_positions(T, n, 100)
        rec, st = window_items(2, pos, eng.device)
        W = len(rec)
        # shift: bitwise a NumPy gather, windows wrapping past T included
        d = sg.shift_offsets(np.random.default_rng(2), 4, 2, T, n)
        got = eng.surrogate_shift(xd, rec, st, n, torch.as_tensor(d).to(eng.device), split).cpu().numpy()
        want = np.empty((4 * W, m, n))
        wraps = 0
        rh, sh = rec.cpu().numpy(), st.cpu().numpy()
        for s in range(4):
            for w in range(W):
                r, s0 = rh[w], sh[w]
                want[s * W + w, :split] = x[r, :split, s0:s0 + n]
                idx = (s0 + np.arange(n) + d[s, r]) % T
                wraps += int(idx[-1] < idx[0])
                want[s * W + w, split:] = x[r, split:][:, idx]
        assert wraps > 0 and np.array_equal(got, want)
        # phase: irfft(rfft(window) e^{i phi}) of every window, the same phases for every window and recording
        phi = sg.phase_draws(np.random.default_rng(4), 3, m, n)
        spec = eng.window_spectra(xd, rec, st, n)
        phd = torch.as_tensor(phi).to(eng.device)
        got = eng.surrogate_phase(spec, phd, n).cpu().numpy()
        wins = np.stack([x[r, :, s0:s0 + n] for r, s0 in zip(rh, sh)])
        F = np.fft.rfft(wins, axis=-1)
        want = np.stack([np.fft.irfft(F * np.exp(1j * phi[s]), n, axis=-1) for s in range(3)]).reshape(3 * W, m, n)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), np.abs(got - want).max()
        amp = np.abs(np.fft.rfft(got, axis=-1))
        amp0 = np.tile(np.abs(F), (3, 1, 1))
        assert np.abs(amp - amp0).max() <= 1e-12 * amp0.max()
        Z = eng.surrogate_phase_spectra(spec, phd, n).cpu().numpy().reshape(3, W, m, -1)
        sp = spec.cpu().numpy()
        real_bins = [0] + ([n // 2] if n % 2 == 0 else [])
        for b in real_bins:
            assert np.array_equal(Z[..., b], np.broadcast_to(sp[..., b], Z[..., b].shape))
        assert np.abs(sp - F).max() <= 1e-12 * np.abs(F).max()


# ------------------------------------------------------------------------- 2. + 3. statistics, observed values
@pytest.mark.parametrize("null", ["shift", "phase"])
@pytest.mark.parametrize("measure", ["ffdtf", "ddtf", "gpdc"])
def test_statistics_vs_restatement(measure, null):
    m, n, p, fs, S, seed = 6, 200, 3, 100.0, 24, 11
    x = _signal(2, m, 600, 17)
    freqs = np.linspace(1.0, 45.0, 24)
    lo, hi = hd.band_bins(freqs, ((0.0, 8.0), (8.0, 20.0), (20.0, 50.0)))
    res = sliding_significance(x, n, None, p, freqs, fs, (lo, hi), measure=measure, null=null, n_surrogates=S, seed=seed,
                               split=3, hop=100)
    pos = hop_positions(600, n, 100)
    assert res["p"].shape == (2, len(pos), m, m, 3) and res["n_valid"].shape == (2, len(pos))
    assert np.array_equal(res["tested"], sg.tested_mask(m, null, 3))
    # 3. the observed values are what sliding_<measure>(bands=...) returns, bit for bit
    plain = {"ffdtf": SL.sliding_ffdtf_device, "ddtf": sliding_ddtf, "gpdc": sliding_gpdc}[measure]
    if measure == "ffdtf":
        eng = default_engine()
        rec, st = window_items(2, pos, eng.device)
        want_obs = eng.sliding_ffdtf(eng.to_device(x), rec, st, n, p, freqs, fs, bands=(lo, hi),
                                     grid=SL.regular_grid(pos, n, p)).cpu().numpy().reshape(res["observed"].shape)
    else:
        want_obs = plain(x, n, None, p, freqs, fs, hop=100, bands=(lo, hi))
    assert np.array_equal(res["observed"], want_obs)
    # 2. the NumPy restatement on the oracle
    want, ties = restate(measure, null, x, pos, n, p, freqs, fs, lo, hi, S, seed, 3)
    got = _flat(res)
    assert np.array_equal(got["n_valid"], want["n_valid"]) and (want["n_valid"] == S).all()
    tested = np.broadcast_to(sg.tested_mask(m, null, 3)[None, :, :, None], got["p"].shape)
    for k in ("null_mean", "null_std"):
        assert np.array_equal(np.isnan(got[k]), ~tested)
        scale = np.abs(want[k][tested]).max()
        assert np.abs(got[k][tested] - want[k][tested]).max() <= 1e-10 * max(scale, 1.0), k
    keep = tested & ~ties
    excluded = int((tested & ties).sum())
    print(f"{measure}/{null}: {excluded} of {int(tested.sum())} tested cells excluded as near-ties")
    assert excluded <= 0.02 * tested.sum()
    for k in ("p", "p_fwe"):
        assert np.array_equal(np.isnan(got[k]), ~tested)
        assert np.array_equal(got[k][keep], want[k][keep]), k
        assert (got[k][tested] > 0).all() and (got[k][tested] <= 1).all()


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("null", ["shift", "phase"])
def test_determinism_and_block_invariance(null):
    eng = default_engine()
    m, n, p, fs, S = 6, 200, 3, 100.0, 24
    x = eng.to_device(_signal(1, m, 1300, 23))
    pos = hop_positions(1300, n, 100)
    rec, st = window_items(1, pos, eng.device)
    W = len(pos)
    freqs = np.arange(1.0, 33.0)
    lo, hi = hd.band_bins(freqs, ((0.0, 8.0), (8.0, 20.0), (20.0, 40.0)))
    kw = dict(measure="ffdtf", null=null, n_surrogates=S, split=3)

    def run(seed, chunk=None):
        r = eng.sliding_significance(x, rec, st, n, p, freqs, fs, (lo, hi), seed=seed, chunk=chunk, **kw)
        return {k: v.cpu().numpy() for k, v in r.items()}
    base = run(3)
    assert W == 12 and (base["n_valid"] == S).all()
    for chunk in (None, W, 7, 5 * W, S * W, 1):                 # all at once, one surrogate, odd window tiles, odd blocks
        again = run(3, chunk)
        for k in STATS:
            assert _same(again[k], base[k]), (chunk, k)
    other = run(4)
    assert np.array_equal(other["observed"], base["observed"])
    assert not np.array_equal(other["null_mean"], base["null_mean"], equal_nan=True)
    assert not np.array_equal(other["p"], base["p"], equal_nan=True)


# --------------------------------------------------------------------------------------------- 5. planted coupling
def test_planted_coupling():
    fs, n, p, S = 100.0, 500, 2, 99
    x = planted_dyad(6000, seed=8)
    freqs = np.linspace(1.0, 48.0, 32)
    lo, hi = hd.band_bins(freqs, ((0.0, 50.0),))
    kw = dict(measure="ffdtf", n_surrogates=S, seed=21, split=4, hop=250)
    sh = sliding_significance(x, n, None, p, freqs, fs, (lo, hi), null="shift", **kw)
    pv, pf = sh["p"][:, 5, 0, 0], sh["p_fwe"][:, 5, 0, 0]            # cell [target B1, source A0]
    W = len(pv)
    frac_min, frac_fwe = np.mean(pv == 0.01), np.mean(pf <= 0.05)
    null_cells = sh["p"][:, :4, 4:, 0]                                  # B -> A: no flow at all
    frac_null = np.mean(null_cells <= 0.05)
    print(f"planted link: {W} windows, p = 0.01 in {frac_min:.3f}, p_fwe <= 0.05 in {frac_fwe:.3f}; "
          f"B -> A cells with p <= 0.05: {frac_null:.3f}")
    assert frac_min >= 0.95 and frac_fwe >= 0.90
    assert 0.01 <= frac_null <= 0.12
    ph = sliding_significance(x, n, None, p, freqs, fs, (lo, hi), null="phase", **kw)
    assert np.mean(ph["p"][:, 5, 0, 0] <= 0.05) >= 0.95


# ------------------------------------------------------------------------------------------------------ 6. failures
@pytest.mark.parametrize("measure", ["ffdtf", "ddtf", "gpdc"])
def test_failed_surrogates_and_windows(measure):
    eng = default_engine()
    m, n, p, fs, S, seed, T = 6, 200, 3, 100.0, 12, 9, 1200
    x = _signal(1, m, T, 31)
    d00 = sg.shift_offsets(np.random.default_rng(seed), S, 1, T, n)[0, 0]
    x[0, 3] = np.roll(x[0, 0], d00)          # B0 = A0 delayed by d[0, 0]: surrogate 0 shifts it back onto A0
    xd = eng.to_device(x)
    pos = hop_positions(T, n, 100)
    rec, st = window_items(1, pos, eng.device)
    freqs = np.linspace(1.0, 45.0, 16)
    lo, hi = hd.band_bins(freqs, ((0.0, 10.0), (10.0, 50.0)))
    kw = dict(measure=measure, null="shift", n_surrogates=S, seed=seed, split=3)
    r = eng.sliding_significance(xd, rec, st, n, p, freqs, fs, (lo, hi), **kw)
    assert (r["n_valid"].cpu().numpy() == S - 1).all()
    t = r["tested"].cpu().numpy()
    for k in ("p", "p_fwe", "null_mean", "null_std"):
        v = r[k].cpu().numpy()
        assert np.isfinite(v[:, t]).all() and np.isnan(v[:, ~t]).all(), k
    assert (r["p"].cpu().numpy()[:, t] >= 1.0 / S).all()
    # a singular observed window: LinAlgError under check=True, NaN statistics under "nan"
    y = _signal(1, m, T, 32)
    y[0, 2, 400:600] = y[0, 0, 400:600] + y[0, 1, 400:600]              # window 4 (start 400): collinear channels
    yd = eng.to_device(y)
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
        eng.sliding_significance(yd, rec, st, n, p, freqs, fs, (lo, hi), **kw)
    assert 4 in list(ei.value.items)
    r = eng.sliding_significance(yd, rec, st, n, p, freqs, fs, (lo, hi), check="nan", **kw)
    bad = np.zeros(len(pos), bool)
    bad[list(ei.value.items)] = True
    for k in ("observed", "p", "p_fwe", "null_mean", "null_std"):
        v = r[k].cpu().numpy()
        assert np.isnan(v[bad]).all() and np.isfinite(v[~bad][:, t]).all(), k
    # zero windows
    e = torch.zeros(0, dtype=torch.int64, device=eng.device)
    r = eng.sliding_significance(xd, e, e, n, p, freqs, fs, (lo, hi), **kw)
    for k in ("observed", "p", "p_fwe", "null_mean", "null_std"):
        assert tuple(r[k].shape) == (0, m, m, 2)
    assert tuple(r["n_valid"].shape) == (0,) and tuple(r["tested"].shape) == (m, m)


# -------------------------------------------------------------------------------------------------------- 7. ESCan
def test_escan_significance(tree, tmp_path):  # noqa: F811
    freqs = np.arange(1.0, 33.0, 1.0)
    kw = dict(window_s=2.0, overlap=0.5, model_order=3, freqs=freqs, low_cutoff_hz=1.0, high_cutoff_hz=45.0, reader=_reader,
              verbose=False, measures=("ffdtf", "gpdc"))
    sig = dict(null="shift", n_surrogates=19, seed=5)
    plain = EB.run(tree, tmp_path / "plain", **kw)
    withs = EB.run(tree, tmp_path / "sig", significance=sig, **kw)
    assert plain["done"] == withs["done"] == ["W_003", "W_010"]
    new = ("p", "p_fwe", "null_mean", "null_std", "n_valid")
    for dy in plain["done"]:
        z0 = np.load(tmp_path / "plain" / f"{dy}_ffdtf.npz", allow_pickle=False)
        z1 = np.load(tmp_path / "sig" / f"{dy}_ffdtf.npz", allow_pickle=False)
        m0, m1 = json.loads(str(z0["meta"])), json.loads(str(z1["meta"]))
        segs = [f"{s['task']}/{s['event']}" for s in m0["segments"]]
        today = {"channels", "freqs", "bands", "meta"} | {f"{k}/{a}" for k in segs
                                                          for a in ("ffdtf_bands", "gpdc_bands", "starts")}
        assert set(z0.files) == today and "significance" not in m0
        assert m1["significance"] == dict(sig, min_shift=None)
        assert set(z1.files) - set(z0.files) == {f"{k}/{meas}_bands_{a}" for k in segs for meas in ("ffdtf", "gpdc")
                                                  for a in new}
        for f_ in z0.files:
            if f_ != "meta":
                assert _same(z0[f_], z1[f_]), f_
        names = list(z1["channels"])
        split = sum(c.endswith("_ch") for c in names)
        tested = sg.tested_mask(len(names), "shift", split)
        for k in segs:
            nw = len(z1[f"{k}/starts"])
            for meas in ("ffdtf", "gpdc"):
                pv = z1[f"{k}/{meas}_bands_p"]
                assert pv.shape == z1[f"{k}/{meas}_bands"].shape == (nw, 16, 16, 5)
                assert z1[f"{k}/{meas}_bands_n_valid"].shape == (nw,)
                assert (z1[f"{k}/{meas}_bands_n_valid"] == 19).all()
                for a in ("p", "p_fwe", "null_mean", "null_std"):
                    v = z1[f"{k}/{meas}_bands_{a}"]
                    assert np.isnan(v[:, ~tested]).all() and np.isfinite(v[:, tested]).all(), (k, meas, a)
                for a in ("p", "p_fwe"):
                    v = z1[f"{k}/{meas}_bands_{a}"][:, tested]
                    assert (v > 0).all() and (v <= 1).all()
