"""Pseudo-dyad (shuffled-partner) significance on the MI355X (`Engine.lagcov_pairs`, `Engine.sliding_pairs`,
`Engine.pseudo_dyad_significance`, `sliding.sliding_pseudo_dyad_significance`, `escan_batch.run_pseudo_dyads`): the pair K1
and the fused pair call bit for bit against the single-recording calls on the pseudo recordings written out, every statistic
of both levels against a NumPy restatement on the oracle, a planted coupling, chunk independence, a failing participant and
the batch front-end.  All @pytest.mark.gpu."""
import json

import numpy as np
import pytest
import torch

from hyperscanning_signal_analysis_amd import surrogates as sg
from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad
from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd.engine import SingularMatrixError, default_engine
    from hyperscanning_signal_analysis_amd.sliding import sliding_pseudo_dyad_significance
    from tests.test_gpu_escan_batch import _reader, _write

ORACLE = {"ffdtf": O.full_freq_dtf, "ddtf": O.direct_dtf, "gpdc": O.gen_partial_directed_coherence}
MEASURES = ("ffdtf", "ddtf", "gpdc")
STATS = ("observed", "p", "p_fwe", "null_mean", "null_std")
EPS = np.finfo(np.float64).eps
FREQS = np.arange(1.0, 33.0)          # F = 32 at fs = 128: K3 adds the bands up itself


def band_bins(freqs, edges):
    """Half-open [lo, hi) bands on an ascending grid -> bin tables (`distributed.band_bins`, restated)."""
    lo = [int(np.searchsorted(freqs, a, side="left")) for a, _ in edges]
    hi = [int(np.searchsorted(freqs, b, side="left")) for _, b in edges]
    return np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32)


def coloured(rng, shape):
    x = rng.standard_normal(shape)
    x[..., 1:] += 0.5 * x[..., :-1]
    x[..., 1:, :] += 0.3 * x[..., :-1, :]
    return x


def i64(eng, a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)


def pseudo_window(x, a, b, s, n, split):
    """The window written out: rows < split of recording a, rows >= split of recording b, samples s .. s + n."""
    w = x[a][:, s:s + n].copy()
    w[split:] = x[b][split:, s:s + n]
    return w


# ------------------------------------------------------------------------------------------------------------ 1. K1 bits
PAIRS3 = [(a, b) for a in range(3) for b in range(3)]          # the 6 ordered pairs and the 3 real dyads


@pytest.mark.parametrize("m,split,n,p", [(64, 32, 200, 8), (38, 19, 90, 3), (33, 17, 128, 6), (5, 2, 66, 2), (16, 6, 67, 2)])
def test_k1_bits(m, split, n, p):
    """Every pair of 3 recordings at 2 starts (one window ending at T), R poisoned with NaN before each call: with the base,
    without it, and for rec_a == rec_b, the whole stack -- padding included -- is `Engine.lagcov` of the window written out."""
    eng = default_engine()
    T = n + 41
    x = eng.to_device(coloured(np.random.default_rng(7 * m + n), (3, m, T)))
    starts = (5, T - n)
    mat = torch.stack([torch.cat([x[a, :split], x[b, split:]], dim=0) for a, b in PAIRS3])        # (9, m, T)
    rec_a = i64(eng, [a for a, b in PAIRS3 for _ in starts])
    rec_b = i64(eng, [b for a, b in PAIRS3 for _ in starts])
    st = i64(eng, [s for _ in PAIRS3 for s in starts])
    want = eng.lagcov(mat, i64(eng, np.repeat(np.arange(9), 2)), st, n, p)
    mp = want.shape[-1]
    assert tuple(want.shape) == (18, p + 1, mp, mp)
    # the base: the real recordings' own covariances, item r * 2 + k
    base = eng.lagcov(x, i64(eng, np.repeat(np.arange(3), 2)), i64(eng, np.tile(starts, 3)), n, p)
    k = i64(eng, np.tile(np.arange(2), 9))
    poison = lambda: torch.full_like(want, float("nan"))  # noqa: E731
    got = eng.lagcov_pairs(x, rec_a, rec_b, st, n, p, split, out=poison())
    assert torch.equal(got, want)
    got = eng.lagcov_pairs(x, rec_a, rec_b, st, n, p, split, R_base=base, base_a=rec_a * 2 + k, base_b=rec_b * 2 + k,
                           out=poison())
    assert torch.equal(got, want)
    real = torch.nonzero(rec_a == rec_b).flatten()
    got = eng.lagcov_pairs(x, rec_a[real], rec_a[real], st[real], n, p, split, out=poison()[:len(real)])
    assert torch.equal(got, eng.lagcov(x, rec_a[real], st[real], n, p))
    # a recognisable base addressed backwards: the within-participant elements are copies, whatever they hold
    r = torch.arange(mp, device=eng.device)
    in_a = ((r < split)[:, None] & (r < split)[None, :]).expand(18, p + 1, mp, mp)
    in_b = ((r >= split)[:, None] & (r >= split)[None, :]).expand(18, p + 1, mp, mp)
    pattern = torch.arange(7 * (p + 1) * mp * mp, dtype=torch.float64, device=eng.device).view(7, p + 1, mp, mp)
    ba, bb = 6 - (rec_a * 2 + k), 5 - (rec_b * 2 + k)
    got = eng.lagcov_pairs(x, rec_a, rec_b, st, n, p, split, R_base=pattern, base_a=ba, base_b=bb, out=poison())
    assert torch.equal(got[in_a], pattern[ba][in_a]) and torch.equal(got[in_b], pattern[bb][in_b])
    assert torch.equal(got[~(in_a | in_b)], want[~(in_a | in_b)])
    for kw, msg in [(dict(split=0), "split"), (dict(split=m), "split"), (dict(R_base=base), "go together"),
                    (dict(R_base=base, base_a=bb, base_b=bb + 1), "base_b must lie"),
                    (dict(R_base=base, base_a=bb - 1, base_b=bb), "base_a must lie"),
                    (dict(R_base=base[:, :p], base_a=bb, base_b=bb), "R_base must be")]:
        with pytest.raises(ValueError, match=msg):
            eng.lagcov_pairs(x, rec_a, rec_b, st, n, p, **dict(dict(split=split), **kw))
    with pytest.raises(ValueError, match="item_rec must lie"):
        eng.lagcov_pairs(x, rec_a, rec_b + 3, st, n, p, split)


# --------------------------------------------------------------------------------------------------------- 2. fused bits
@pytest.mark.parametrize("m,split", [(8, 4), (6, 2)])
@pytest.mark.parametrize("F", [32, 24])
def test_fused_bits(m, split, F):
    """`sliding_pairs` with bands = `sliding_<measure>` with bands on the pseudo recordings written out, bit for bit: F = 32
    (the bands summed in the kernel) and F = 24 (full array, then band sums), with the base and a chunk that cuts the
    base tables, and without either."""
    eng = default_engine()
    n, p, fs, T = 128, 3, 128.0, 500
    x = eng.to_device(coloured(np.random.default_rng(100 * m + F), (3, m, T)))
    starts = (0, 100, 201, T - n)
    mat = torch.stack([torch.cat([x[a, :split], x[b, split:]], dim=0) for a, b in PAIRS3])
    rec_a = i64(eng, [a for a, b in PAIRS3 for _ in starts])
    rec_b = i64(eng, [b for a, b in PAIRS3 for _ in starts])
    st = i64(eng, [s for _ in PAIRS3 for s in starts])
    rec_m = i64(eng, np.repeat(np.arange(9), 4))
    k = i64(eng, np.tile(np.arange(4), 9))
    freqs = np.linspace(1.0, 60.0, F)
    bands = ([0, 8], [8, F])
    base = eng.lagcov(x, i64(eng, np.repeat(np.arange(3), 4)), i64(eng, np.tile(starts, 3)), n, p)
    based = dict(R_base=base, base_a=rec_a * 4 + k, base_b=rec_b * 4 + k, chunk=5)
    run = {"ffdtf": eng.sliding_ffdtf, "ddtf": eng.sliding_ddtf, "gpdc": eng.sliding_gpdc}
    for meas in MEASURES:
        want = run[meas](mat, rec_m, st, n, p, freqs, fs, bands=bands)
        assert tuple(want.shape) == (36, m, m, 2)
        for kw in (based, {}):
            got = eng.sliding_pairs(x, rec_a, rec_b, st, n, p, freqs, fs, measure=meas, split=split, bands=bands, **kw)
            assert torch.equal(got, want), (meas, sorted(kw))
    if F == 32:
        w_out, w_ar, w_V, _ = eng.sliding_ddtf(mat, rec_m, st, n, p, freqs, fs, return_ar=True)
        out, ar, V, (iy, itf) = eng.sliding_pairs(x, rec_a, rec_b, st, n, p, freqs, fs, measure="ddtf", split=split,
                                                  return_ar=True, **based)
        assert torch.equal(out, w_out) and torch.equal(ar, w_ar) and torch.equal(V, w_V) and not iy.any() and not itf.any()
        with pytest.raises(ValueError, match="not offered"):
            eng.sliding_pairs(x, rec_a, rec_b, st, n, None, freqs, fs, measure="ddtf", split=split)
        with pytest.raises(ValueError, match="windows .* must lie"):
            eng.sliding_pairs(x, rec_a, rec_b, st + 1, n, p, freqs, fs, measure="ddtf", split=split)


# ------------------------------------------------------------------------------------------------- 3. the statistics
CASES = {
    "A": dict(D=4, m=6, split=3, T=600, n=200, starts=(0, 200, 400), p=2, fs=128.0, edges=((2.0, 10.0), (10.0, 24.0)),
              seed0=100, n_surrogates=None, seed=None),
    "B": dict(D=3, m=5, split=2, T=400, n=128, starts=(0, 100, 272), p=3, fs=128.0, edges=((0.0, 16.0), (16.0, 32.0)),
              seed0=200, n_surrogates=5, seed=17),
}
_data, _restated = {}, {}


def case_data(tag):
    if tag not in _data:
        c = CASES[tag]
        _data[tag] = np.stack([synthetic_var_dyad(c["seed0"] + d, m=c["m"], p=c["p"], T=c["T"], burn=300, fs=c["fs"])
                               for d in range(c["D"])])
    return _data[tag]


def band_values(measure, w, freqs, fs, p, lo, hi):
    v = ORACLE[measure](w, freqs, fs, p)
    return np.stack([v[..., a:b].sum(-1) for a, b in zip(lo, hi)], axis=-1)


def null_stats(obs, v, tested):
    """observed (..., m, m, nb) against its null values v (K, ..., m, m, nb): counting with >=, (1 + count) / (1 + K), the
    maximum over the tested pairs, mean and sample std.  Also the smallest relative gap of a comparison."""
    K = v.shape[0]
    t4 = tested[:, :, None]
    M = np.where(t4, v, -np.inf).max(axis=(-3, -2))                              # (K, ..., nb)
    mask = np.where(t4, 1.0, np.nan)
    Mb = M[..., None, None, :]
    out = {"p": (1.0 + (v >= obs).sum(0)) / (1.0 + K) * mask, "p_fwe": (1.0 + (Mb >= obs).sum(0)) / (1.0 + K) * mask,
           "null_mean": v.mean(0) * mask, "null_std": v.std(0, ddof=1) * mask}
    sel = np.broadcast_to(t4, obs.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = min((np.abs(v - obs) / np.abs(obs)).min(0)[sel].min(), (np.abs(Mb - obs) / np.abs(obs)).min(0)[sel].min())
    return out, float(gap)


def restate(x, measure, n, p, starts, freqs, fs, lo, hi, split, partners):
    """The whole test on the host: the oracle on every window written out, NumPy statistics.  Returns (per-dyad dict
    (D, W, ...), group dict (W, ...), cond of the normal equations per observed (D, W) and surrogate (S, D, W) item, the
    smallest relative gap between a compared pair of values)."""
    D, m = x.shape[:2]
    W, S = len(starts), len(partners)
    tested = sg.tested_mask(m, "shift", split)
    obs = np.empty((D, W, m, m, len(lo)))
    sur = np.empty((S, D, W, m, m, len(lo)))
    c_obs, c_sur = np.empty((D, W)), np.empty((S, D, W))
    for d in range(D):
        for w, s0 in enumerate(starts):
            win = pseudo_window(x, d, d, s0, n, split)
            obs[d, w] = band_values(measure, win, freqs, fs, p, lo, hi)
            c_obs[d, w] = np.linalg.cond(O.count_corr(win, p)[0])
            for s in range(S):
                win = pseudo_window(x, d, partners[s][d], s0, n, split)
                sur[s, d, w] = band_values(measure, win, freqs, fs, p, lo, hi)
                c_sur[s, d, w] = np.linalg.cond(O.count_corr(win, p)[0])
    assert np.isfinite(obs).all() and np.isfinite(sur).all()
    v = np.empty((2 * S,) + obs.shape)
    for s in range(S):
        v[2 * s] = sur[s]                                    # A-anchored: A_d with B_pi(d)
        v[2 * s + 1] = sur[s][np.argsort(partners[s])]       # B-anchored: A_{pi^-1(d)} with B_d
    dyad, gap_d = null_stats(obs, v, tested)
    dyad.update(observed=obs, n_valid=np.full((D, W), 2 * S))
    gobs = obs.mean(0)
    group, gap_g = null_stats(gobs, sur.mean(1), tested)
    group.update(observed=gobs, n_valid=np.full(W, S))
    return dyad, group, c_obs, c_sur, min(gap_d, gap_g)


def restated(tag, measure):
    key = (tag, measure)
    if key not in _restated:
        c = CASES[tag]
        lo, hi = band_bins(FREQS, c["edges"])
        rng = None if c["n_surrogates"] is None else np.random.default_rng(c["seed"])
        partners = sg.partner_derangements(rng, c["n_surrogates"], c["D"])
        _restated[key] = (partners,) + restate(case_data(tag), measure, c["n"], c["p"], c["starts"], FREQS, c["fs"], lo, hi,
                                               c["split"], partners)
    return _restated[key]


def run_case(tag, measure, x=None, **kw):
    c = CASES[tag]
    lo, hi = band_bins(FREQS, c["edges"])
    eng = default_engine()
    xd = eng.to_device(case_data(tag) if x is None else x)
    res = eng.pseudo_dyad_significance(xd, i64(eng, c["starts"]), c["n"], c["p"], FREQS, c["fs"], (lo, hi), measure=measure,
                                       split=c["split"], n_surrogates=c["n_surrogates"], seed=c["seed"], **kw)
    out = {k: v.cpu().numpy() for k, v in res.items() if k != "group"}
    out["group"] = {k: v.cpu().numpy() for k, v in res["group"].items()}
    return out


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("tag", ["A", "B"])
def test_statistics_vs_restatement(tag, measure):
    """observed, null_mean, null_std of both levels within 1e2 cond eps of the restatement -- the bound
    test_gpu_sliding_conn.py applies to these measures, cond being that of the oracle's normal equations, the largest over
    the windows a number is made of.  p, p_fwe, n_valid and partners exactly: on the oracle every fit is
    finite, cond is 604 at the most (73 in case A) and no compared pair of values is closer than 1e-7 relative (asserted here on the restatement's own
    values), so no cell is left out."""
    c = CASES[tag]
    partners, dyad, group, c_obs, c_sur, gap = restated(tag, measure)
    D, W, m, S = c["D"], len(c["starts"]), c["m"], len(partners)
    cmax = max(c_obs.max(), c_sur.max())
    print(f"{tag}/{measure}: S = {S}, cond <= {cmax:.3g}, smallest relative gap {gap:.3g}")
    assert cmax < 605 and gap > 1e-7                          # (on the host: 73 for case A, 604 for case B)
    got = run_case(tag, measure)
    assert np.array_equal(got["partners"], partners) and got["partners"].dtype == np.int64
    tested = sg.tested_mask(m, "shift", c["split"])
    assert np.array_equal(got["tested"], tested) and tested.sum() == 2 * c["split"] * (m - c["split"])
    assert np.array_equal(got["n_valid"], dyad["n_valid"]) and np.array_equal(got["group"]["n_valid"], group["n_valid"])
    assert got["n_valid"].dtype == np.int32 and got["observed"].shape == (D, W, m, m, 2)
    assert got["group"]["observed"].shape == (W, m, m, 2)
    # cond per number: an observed value its own window's; a null statistic of (d, w) the 2 S windows behind it and the
    # observed one; a group number all windows at w
    c_null = np.maximum(c_obs, np.maximum(c_sur, np.stack([c_sur[s][np.argsort(partners[s])] for s in range(S)])).max(0))
    c_group = np.maximum(c_obs.max(0), c_sur.max((0, 1)))
    t5 = np.broadcast_to(tested[:, :, None], got["observed"].shape)
    for level, g, w, cond_obs, cond_null in (("dyad", got, dyad, c_obs, c_null), ("group", got["group"], group, c_group, c_group)):
        sel = t5 if level == "dyad" else t5[0]
        for k in STATS[1:]:
            assert np.array_equal(np.isnan(g[k]), ~sel), (level, k)
        for k, cond in (("observed", cond_obs), ("null_mean", cond_null), ("null_std", cond_null)):
            full = np.ones_like(sel) if k == "observed" else sel
            err = np.where(full, np.abs(g[k] - w[k]), 0.0).max(axis=(-3, -2, -1))
            tol = 1e2 * cond * EPS
            print(f"  {level:5s} {k:9s} max err / tol = {(err / tol).max():.3g} (err {err.max():.3g})")
            assert (err <= tol).all(), (level, k, err.max(), tol.min())
        for k in ("p", "p_fwe"):
            assert np.array_equal(g[k][sel], w[k][sel]), (level, k)


# -------------------------------------------------------------------------------------------------- 4. planted coupling
def test_planted_coupling_is_found_against_every_pseudo_dyad():
    """5 dyads of 3 + 3 channels of white noise; B's channel 0 follows its own partner's A channel 0 by one sample.  Every
    pseudo dyad lacks the link: the cell (split, 0) has the smallest possible p at both levels, in every window."""
    D, split, T, n, p, fs = 5, 3, 520, 256, 2, 128.0
    x = np.empty((D, 6, T))
    for d in range(D):
        e = np.random.default_rng(300 + d).standard_normal((6, T))
        b0 = e[3].copy()
        e[3] = 0.5 * b0
        e[3, 1:] += 0.9 * e[0, :-1]
        x[d] = e
    bands = ([0], [32])
    for measure in MEASURES:
        res = sliding_pseudo_dyad_significance(x, n, None, p, FREQS, fs, bands, measure=measure, hop=264)
        assert res["p"].shape == (D, 2, 6, 6, 1) and (res["n_valid"] == 2 * (D - 1)).all() and (res["group"]["n_valid"] == D - 1).all()
        assert np.array_equal(res["partners"], [(np.arange(D) + k) % D for k in range(1, D)])
        assert (res["p"][:, :, split, 0, 0] == 1.0 / 9.0).all(), (measure, res["p"][:, :, split, 0, 0])
        assert (res["group"]["p"][:, split, 0, 0] == 1.0 / 5.0).all(), (measure, res["group"]["p"][:, split, 0, 0])


# ------------------------------------------------------------------------------------------------- 5. chunk independence
def test_chunk_independence():
    """A chunk that cuts one surrogate (12 items) into several fused calls, evenly and not: the same bits."""
    base = run_case("A", "ffdtf")
    for chunk in (5, 4, 1, 100):
        again = run_case("A", "ffdtf", chunk=chunk)
        for k in STATS + ("n_valid", "partners"):
            assert np.array_equal(again[k], base[k], equal_nan=True), (chunk, k)
            if k != "partners":
                assert np.array_equal(again["group"][k], base["group"][k], equal_nan=True), (chunk, "group", k)


# ------------------------------------------------------------------------------------------------ 6. a failing participant
@pytest.mark.parametrize("measure", ["ffdtf", "gpdc"])
def test_failing_participant(measure):
    c = CASES["A"]
    D, W, split = c["D"], len(c["starts"]), c["split"]
    x = case_data("A").copy()
    x[2, split + 1] = 0.0                                      # a dead channel of B of dyad 2: no fit with it succeeds
    with pytest.raises(SingularMatrixError):
        run_case("A", measure, x=x)
    res = run_case("A", measure, x=x, check="nan")
    tested = sg.tested_mask(c["m"], "shift", split)
    others = [d for d in range(D) if d != 2]
    for k in STATS:
        assert np.isnan(res[k][2]).all(), k
        cells = res[k][others] if k == "observed" else res[k][others][:, :, tested]
        assert np.isfinite(cells).all(), k
        assert np.isnan(res["group"][k]).all(), k
    # dyad d != 2 loses the one A-anchored surrogate that gives it B of dyad 2; B-anchored it keeps all (A of dyad 2 is fine)
    assert (res["n_valid"][others] == 2 * (D - 1) - 1).all() and (res["group"]["n_valid"] == 0).all()
    p = res["p"][others][:, :, tested]
    assert (p >= 1.0 / (2 * (D - 1))).all() and (p <= 1.0).all()


# ------------------------------------------------------------------------------------------------------------ 7. batch
def test_batch_front_end(tmp_path, capsys):
    root = tmp_path / "tree"
    film = [("Peppa", 1.0, 5.0)]
    dyads = ["W_001", "W_002", "W_003"]
    for d, dy in enumerate(dyads):
        for r, (code, role) in enumerate((("ch", "child"), ("cg", "caregiver"))):
            _write(root / "EEG" / dy / role / f"{dy}_EEG_{code}_movies.nc", 50 + 10 * d + r, 9.0, film, r == 0)
    _write(root / "EEG" / "W_004" / "child" / "W_004_EEG_ch_movies.nc", 99, 9.0, film, True)            # no caregiver
    subset = ["Fp1", "F3", "O1"]
    out = tmp_path / "out"
    res = EB.run_pseudo_dyads(root, out, "movies", "Peppa", model_order=3, freqs=FREQS, channel_subset=subset,
                              measures=("ffdtf", "gpdc"), reader=_reader)
    assert res["dyads"] == dyads and [d for d, _ in res["skipped"]] == ["W_004"]
    assert "[SKIP] W_004 movies/Peppa: missing caregiver file" in capsys.readouterr().out
    z = np.load(out / "pseudo_dyads_movies_Peppa.npz", allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    blocks = []
    found = EB.discover_dyads(root)
    for dy in dyads:
        recs = {r: _reader(found[dy]["movies"][r]) for r in ("ch", "cg")}
        blocks.append(EB.segment_block(recs["ch"], recs["cg"], 1.0, 5.0, channel_subset=subset)[0])
    T = min(b.shape[1] for b in blocks)
    starts = np.arange((T - 256) // 128 + 1) * 128
    W, nb = len(starts), z["bands"].shape[0]
    assert meta["samples"] == T and meta["split"] == 3 and meta["window"] == 256 and meta["dyads"] == dyads
    assert list(z["dyads"]) == dyads and list(z["channels"]) == [f"{c}_{r}" for r in ("ch", "cg") for c in subset]
    assert np.array_equal(z["starts"], starts) and np.array_equal(z["freqs"], FREQS)
    assert np.array_equal(z["partners"], [[1, 2, 0], [2, 0, 1]])
    for meas in ("ffdtf", "gpdc"):
        for k in ("bands", "p", "p_fwe", "null_mean", "null_std"):
            assert z[f"{meas}_{k}"].shape == (3, W, 6, 6, nb) and z[f"group_{meas}_{k}"].shape == (W, 6, 6, nb), (meas, k)
        assert z[f"{meas}_n_valid"].shape == (3, W) and z[f"group_{meas}_n_valid"].shape == (W,)
        assert (z[f"{meas}_n_valid"] == 4).all() and (z[f"group_{meas}_n_valid"] == 2).all()
    eng = default_engine()
    from hyperscanning_signal_analysis_amd import distributed as hd
    lo, hi = hd.band_bins(FREQS)
    want = eng.pseudo_dyad_significance(eng.to_device(np.stack([b[:, :T] for b in blocks])), i64(eng, starts), 256, 3, FREQS,
                                        128.0, (lo, hi), measure="gpdc", split=3)
    assert np.array_equal(z["gpdc_p"][1], want["p"][1].cpu().numpy(), equal_nan=True)
    assert np.array_equal(z["group_gpdc_p"], want["group"]["p"].cpu().numpy(), equal_nan=True)
