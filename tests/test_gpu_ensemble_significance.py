"""Trial-shuffle significance of event-locked connectivity on the MI355X (`Engine.lagcov_ensemble_split`,
`Engine.ensemble_significance`, `sliding.sliding_ensemble_significance` / `sliding_ensemble_epochs_significance`): K1 with
the second trial table against a NumPy restatement on the oracle, with and without the copied within-participant
blocks, the identity permutation against the direct form, every statistic against a restatement from the documented
draws, determinism and block invariance, a planted same-trial coupling, and failed fits.  All @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

from hyperscanning_signal_analysis_amd import surrogates as sg
from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import (hop_positions, sliding_ensemble_epochs,
                                                           sliding_ensemble_epochs_significance,
                                                           sliding_ensemble_significance)

ORACLE = {"ffdtf": O.full_freq_dtf, "ddtf": O.direct_dtf, "gpdc": O.gen_partial_directed_coherence}
STATS = ("observed", "p", "p_fwe", "null_mean", "null_std", "n_valid")
DIRECT = 8            # _lib.FLAG_DIRECT_LAGCOV


def band_bins(freqs, edges):
    """`distributed.band_bins` restated for half-open [lo, hi) bands on an ascending grid (so that the restatement below
    also runs where the package's GPU half cannot be imported)."""
    lo = [int(np.searchsorted(freqs, a, side="left")) for a, _ in edges]
    hi = [int(np.searchsorted(freqs, b, side="left")) for _, b in edges]
    return np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32)


def coloured(rng, shape):
    """Noise with a little memory along the samples (axis 1) and a little mixing across the channels (axis 0)."""
    x = rng.standard_normal(shape)
    x[:, 1:] += 0.5 * x[:, :-1]
    x[1:] += 0.3 * x[:-1]
    return x


def band_values(measure, stack, freqs, fs, p, lo, hi):
    v = ORACLE[measure](stack, freqs, fs, p)
    return np.stack([v[..., a:b].sum(-1) for a, b in zip(lo, hi)], axis=-1)


def shuffled(ep, pi, split, off, n):
    """(m, n, E) window of one group of epochs (m, L, E): rows < split of trial e, rows >= split of trial pi[e]."""
    st = ep[:, off:off + n, :].copy()
    st[split:] = ep[split:, off:off + n, :][:, :, pi]
    return st


def restate(measure, groups, offsets, n, p, freqs, fs, lo, hi, S, seed, split, tie=1e-9):
    """The whole test on the host from the documented draws and the oracle: (stats dict shaped (G * W, ...), mask of the
    cells whose nearest surrogate value -- or maximum -- lies within `tie` relative of T_obs)."""
    m = groups[0].shape[0]
    counts = [g.shape[2] for g in groups]
    perms = sg.trial_permutations(np.random.default_rng(seed), S, counts)
    tested = sg.tested_mask(m, "trial", split)
    out = {k: [] for k in STATS}
    ties = []
    for g, ep in enumerate(groups):
        ident = np.arange(counts[g])
        for off in offsets:
            obs = band_values(measure, shuffled(ep, ident, split, off, n), freqs, fs, p, lo, hi)
            vals = []
            for s in range(S):
                try:
                    vals.append(band_values(measure, shuffled(ep, perms[s][g], split, off, n), freqs, fs, p, lo, hi))
                except np.linalg.LinAlgError:
                    pass
            v = np.stack(vals)
            M = np.where(tested[None, :, :, None], v, -np.inf).max(axis=(1, 2))
            nv = len(vals)
            mask = np.where(tested[:, :, None], 1.0, np.nan)
            out["observed"].append(obs)
            out["p"].append((1.0 + (v >= obs).sum(0)) / (1.0 + nv) * mask)
            out["p_fwe"].append((1.0 + (M[:, None, None, :] >= obs).sum(0)) / (1.0 + nv) * mask)
            out["null_mean"].append(v.mean(0) * mask)
            out["null_std"].append(v.std(0, ddof=1) * mask)
            out["n_valid"].append(nv)
            scale = np.maximum(np.abs(obs), 1e-300)
            near = np.abs(v - obs).min(0) <= tie * scale
            near |= np.abs(M[:, None, None, :] - obs).min(0) <= tie * scale
            ties.append(near & tested[:, :, None])
    return {k: np.asarray(v) for k, v in out.items()}, np.asarray(ties)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind in "fc")


# ------------------------------------------------------------------------------------------------------------ K1
# (m, split, p, n, group sizes)
K1_SHAPES = [
    (6, 3, 3, 70, [2, 5]),          # NT = 1, nothing skippable, n not a multiple of 4, two chunks
    (38, 19, 6, 100, [6, 7]),       # split inside a 4-row strip and inside a 16-column tile
    (40, 8, 8, 64, [3]),            # asymmetric, exactly one chunk
    (20, 16, 4, 40, [5]),           # split on a tile boundary, B = 4 channels + padding
    (64, 32, 8, 100, [4, 6]),       # every accumulator pure or cross, three full lag groups
    (64, 48, 2, 129, [2]),          # one lag group, a 1-sample third chunk
]
K1_OFFSETS = (0, 7)
_k1_cache = {}


def k1_case(m, split, p, n, counts):
    """Recordings, both trial tables, items and the NumPy restatement of one K1 shape, built once.  Every trial is a
    recording of its own that starts 0..13 samples in; every group slides the offsets 0 and 7."""
    key = (m, split, p, n, tuple(counts))
    if key in _k1_cache:
        return _k1_cache[key]
    rng = np.random.default_rng(1000 * m + 10 * p + n)
    E = sum(counts)
    T = n + max(K1_OFFSETS) + 13
    x = np.stack([coloured(rng, (m, T)) for _ in range(E)])
    start = rng.integers(0, 14, E)
    gp = np.concatenate([[0], np.cumsum(counts)])
    src = np.concatenate([gp[g] + sg.trial_permutations(rng, 1, [c])[0][0] for g, c in enumerate(counts)])
    G, W = len(counts), len(K1_OFFSETS)
    want = np.empty((G * W, p + 1, m, m))
    for g in range(G):
        for w, off in enumerate(K1_OFFSETS):
            tr = np.arange(gp[g], gp[g + 1])
            st = np.stack([x[e, :, start[e] + off:start[e] + off + n] for e in tr], axis=2)
            sb = np.stack([x[e, :, start[e] + off:start[e] + off + n] for e in src[tr]], axis=2)
            st[split:] = sb[split:]
            want[g * W + w] = O.lag_covariances(st, p)
    case = dict(x=x, rec=np.arange(E), start=start, rec_b=src, start_b=start[src], group_ptr=gp,
                item_group=np.repeat(np.arange(G), W), item_offset=np.tile(K1_OFFSETS, G), want=want)
    _k1_cache[key] = case
    return case


def k1_device(eng, c):
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
    idx = dict(group_ptr=i64(c["group_ptr"]), item_group=i64(c["item_group"]), item_offset=i64(c["item_offset"]))
    a = dict(trial_rec=i64(c["rec"]), trial_start=i64(c["start"]))
    b = dict(trial_rec_b=i64(c["rec_b"]), trial_start_b=i64(c["start_b"]))
    return eng.to_device(c["x"]), idx, a, b


def check_padding(R, m, pattern=None):
    """Rows and columns >= m as K1 writes them: zeros, identity at lag 0 (or, where they are copied, the base's)."""
    mp = R.shape[-1]
    if mp == m:
        return
    eye = torch.eye(mp - m, dtype=torch.float64, device=R.device).expand(R.shape[0], -1, -1)
    if pattern is None:
        assert torch.equal(R[:, 0, m:, m:], eye) and not bool(R[:, 1:, m:, m:].any())
    else:
        assert torch.equal(R[:, :, m:, m:], pattern[:, :, m:, m:])


@pytest.mark.parametrize("m,split,p,n,counts", K1_SHAPES)
def test_k1_against_restatement(m, split, p, n, counts):
    """Error <= 1e-13 max|R| (the bound of test_gpu_ensemble.py for the direct form); with R_base the within-participant
    elements are the base's bits and the cross elements those of the call without it; the padding is K1's."""
    eng = default_engine()
    c = k1_case(m, split, p, n, counts)
    xd, idx, ta, tb = k1_device(eng, c)
    N = len(c["item_group"])
    kw = dict(n=n, p=p, split=split, **idx, **ta, **tb)
    full = eng.lagcov_ensemble_split(xd, **kw)
    mp = full.shape[-1]
    assert tuple(full.shape) == (N, p + 1, mp, mp)
    want = c["want"]
    scale = np.abs(want).max()
    err = np.abs(full[:, :, :m, :m].cpu().numpy() - want).max()
    print(f"K1 split m={m} split={split} p={p} n={n} E={counts}: err {err / scale:.2e} of max|R|")
    assert err <= 1e-13 * scale
    check_padding(full, m)
    assert not bool(full[:, :, m:, :m].any()) and not bool(full[:, :, :m, m:].any())
    r = torch.arange(mp, device=eng.device)
    within = ((r < split)[:, None] == (r < split)[None, :]).expand(N, p + 1, mp, mp)
    # the real base: the observed arrangement's covariances, here in the direct form
    base = eng.lagcov_ensemble(xd, n=n, p=p, **idx, **ta)
    it = torch.arange(N, dtype=torch.int64, device=eng.device)
    got = eng.lagcov_ensemble_split(xd, R_base=base, item_base=it, **kw)
    assert torch.equal(got[within], base[within])
    assert torch.equal(got[~within], full[~within])
    assert np.abs(got[:, :, :m, :m].cpu().numpy() - want).max() <= 1e-13 * scale
    check_padding(got, m)
    # a recognisable base, one stack more than there are items, addressed backwards
    k, l, i, j = torch.meshgrid(torch.arange(N + 1), torch.arange(p + 1), torch.arange(mp), torch.arange(mp), indexing="ij")
    pattern = (1e6 * (k + 1) + 1e4 * l + 100.0 * i + j).to(torch.float64).to(eng.device).contiguous()
    back = (N - it).contiguous()
    got = eng.lagcov_ensemble_split(xd, R_base=pattern, item_base=back, **kw)
    assert torch.equal(got[within], pattern[back][within])
    assert torch.equal(got[~within], full[~within])
    check_padding(got, m, pattern[back])


@pytest.mark.parametrize("m,split,p,n,counts", [K1_SHAPES[1], K1_SHAPES[4]])
def test_identity_permutation_is_the_direct_form(m, split, p, n, counts):
    eng = default_engine()
    c = k1_case(m, split, p, n, counts)
    xd, idx, ta, _ = k1_device(eng, c)
    same = dict(trial_rec_b=ta["trial_rec"], trial_start_b=ta["trial_start"])
    want = eng.lagcov_ensemble(xd, n=n, p=p, flags=DIRECT, **idx, **ta)
    assert torch.equal(eng.lagcov_ensemble_split(xd, n=n, p=p, split=split, **idx, **ta, **same), want)


def test_k1_refusals():
    eng = default_engine()
    m, split, p, n, counts = K1_SHAPES[0]
    c = k1_case(m, split, p, n, counts)
    xd, idx, ta, tb = k1_device(eng, c)
    kw = dict(n=n, p=p, **idx, **ta)
    N = len(c["item_group"])
    base = eng.lagcov_ensemble(xd, **kw)
    it = torch.arange(N, dtype=torch.int64, device=eng.device)
    for s in (0, m, -1):
        with pytest.raises(ValueError, match="split"):
            eng.lagcov_ensemble_split(xd, split=s, **kw, **tb)
    with pytest.raises(ValueError, match="go together"):
        eng.lagcov_ensemble_split(xd, split=split, R_base=base, **kw, **tb)
    with pytest.raises(ValueError, match="item_base must lie"):
        eng.lagcov_ensemble_split(xd, split=split, R_base=base, item_base=it + 1, **kw, **tb)
    with pytest.raises(ValueError, match="R_base must be"):
        eng.lagcov_ensemble_split(xd, split=split, R_base=base[:, :p], item_base=it, **kw, **tb)
    with pytest.raises(ValueError, match="trial_rec must lie"):
        eng.lagcov_ensemble_split(xd, split=split, **kw, **dict(tb, trial_rec_b=tb["trial_rec_b"] + len(c["rec"])))
    # the C entry itself: split (-5), a null second table (-4), R_base without item_base (-4)
    P, lib = xd.data_ptr(), eng.lib
    call = lambda rb, sb, sp, Rb, ib: lib.hmv_lagcov_ensemble_split_f64(  # noqa: E731
        P, xd.stride(0), xd.stride(1), xd.shape[2], P, P, P, 2, P, P, N, m, n, p, P, rb, sb, sp, Rb, ib, 0, 0)
    assert call(P, P, 0, 0, 0) == -5 and call(P, P, m, 0, 0) == -5 and b"split" in lib.hmv_last_error()
    assert call(0, P, split, 0, 0) == -4 and call(P, 0, split, 0, 0) == -4
    assert call(P, P, split, P, 0) == -4 and call(P, P, split, 0, P) == -4 and b"go together" in lib.hmv_last_error()


# ---------------------------------------------------------------------------------------------------- statistics
def stat_groups(seed=41, m=6, L=120, counts=(8, 9)):
    rng = np.random.default_rng(seed)
    groups = []
    for E in counts:
        ep = np.stack([coloured(rng, (m, L)) for _ in range(E)], axis=2)
        ep[3, 1:, :] += 0.5 * ep[0, :-1, :]                       # a same-trial link A0 -> B0, so that not every cell is null
        groups.append(ep)
    return groups


STAT = dict(n=60, hop=30, p=3, fs=100.0, S=24, seed=11, split=3)
STAT_FREQS = np.linspace(1.0, 45.0, 24)
STAT_EDGES = ((0.0, 8.0), (8.0, 20.0), (20.0, 50.0))


@pytest.mark.parametrize("measure", ["ffdtf", "ddtf", "gpdc"])
def test_statistics_vs_restatement(measure):
    """Modelled on test_gpu_significance.test_statistics_vs_restatement.  Near-ties of the restatement alone with this
    seed (CPU, before any GPU run): 0 of 324 tested cells for each of the three measures."""
    n, hop, p, fs, S, seed, split = (STAT[k] for k in ("n", "hop", "p", "fs", "S", "seed", "split"))
    groups = stat_groups()
    m, L = groups[0].shape[:2]
    lo, hi = band_bins(STAT_FREQS, STAT_EDGES)
    assert np.array_equal(lo, hd.band_bins(STAT_FREQS, STAT_EDGES)[0]) and np.array_equal(hi, hd.band_bins(STAT_FREQS, STAT_EDGES)[1])
    offsets = hop_positions(L, n, hop)
    res = sliding_ensemble_epochs_significance(groups, n, hop, p, STAT_FREQS, fs, (lo, hi), measure=measure, n_surrogates=S,
                                               seed=seed, split=split)
    G, W = len(groups), len(offsets)
    assert res["p"].shape == (G, W, m, m, 3) and res["n_valid"].shape == (G, W)
    assert np.array_equal(res["tested"], sg.tested_mask(m, "trial", split))
    assert np.array_equal(res["observed"], sliding_ensemble_epochs(groups, n, hop, p, STAT_FREQS, fs, measure=measure, bands=(lo, hi)))
    want, ties = restate(measure, groups, offsets, n, p, STAT_FREQS, fs, lo, hi, S, seed, split)
    got = {k: (v.reshape((-1,) + v.shape[2:]) if k != "tested" else v) for k, v in res.items()}
    assert np.array_equal(got["n_valid"], want["n_valid"]) and (want["n_valid"] == S).all()
    tested = np.broadcast_to(sg.tested_mask(m, "trial", split)[None, :, :, None], got["p"].shape)
    for k in ("null_mean", "null_std"):
        assert np.array_equal(np.isnan(got[k]), ~tested)
        scale = np.abs(want[k][tested]).max()
        assert np.abs(got[k][tested] - want[k][tested]).max() <= 1e-10 * max(scale, 1.0), k
    keep = tested & ~ties
    excluded = int((tested & ties).sum())
    print(f"{measure}/trial: {excluded} of {int(tested.sum())} tested cells excluded as near-ties")
    assert excluded <= 0.02 * tested.sum()
    for k in ("p", "p_fwe"):
        assert np.array_equal(np.isnan(got[k]), ~tested)
        assert np.array_equal(got[k][keep], want[k][keep]), k
        assert (got[k][tested] > 0).all() and (got[k][tested] <= 1).all()


# --------------------------------------------------------------------------------------- determinism and blocking
def test_determinism_and_block_invariance():
    eng = default_engine()
    n, hop, p, fs, S, split = 60, 30, 3, 100.0, 12, 3
    groups = stat_groups(seed=43, counts=(5, 7, 4))
    m, L = groups[0].shape[:2]
    counts = [g.shape[2] for g in groups]
    offsets = hop_positions(L, n, hop)
    G, W = len(groups), len(offsets)
    N = G * W
    xd = eng.to_device(np.concatenate([np.moveaxis(e, 2, 0) for e in groups], axis=0))
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
    E = sum(counts)
    d = dict(trial_rec=i64(np.arange(E)), trial_start=i64(np.zeros(E)), group_ptr=i64(np.concatenate([[0], np.cumsum(counts)])),
             item_group=i64(np.repeat(np.arange(G), W)), item_offset=i64(np.tile(offsets, G)))
    freqs = np.arange(1.0, 33.0)
    lo, hi = hd.band_bins(freqs, ((0.0, 8.0), (8.0, 20.0), (20.0, 40.0)))

    def run(seed, chunk=None, **over):
        r = eng.ensemble_significance(xd, n=n, p=p, freqs=freqs, fs=fs, bands=(lo, hi), measure="ffdtf", n_surrogates=S,
                                      seed=seed, split=split, chunk=chunk, grid=(hop, W), **dict(d, **over))
        return {k: v.cpu().numpy() for k, v in r.items()}
    base = run(3)
    assert (base["n_valid"] == S).all() and base["p"].shape == (N, m, m, 3)
    # again; one surrogate per block; several; all; blocks of one group, of two groups, and a chunk below one group's items
    for chunk in (None, N, 3 * N + 1, S * N, W, 2 * W, 1):
        again = run(3, chunk)
        for k in STATS:
            assert _same(again[k], base[k]), (chunk, k)
    other = run(4)
    assert np.array_equal(other["observed"], base["observed"])
    assert not np.array_equal(other["null_mean"], base["null_mean"], equal_nan=True)
    # items in another order (no grid then; the direct form for the base run too): the same statistics, reordered
    plain = eng.ensemble_significance(xd, n=n, p=p, freqs=freqs, fs=fs, bands=(lo, hi), measure="gpdc", n_surrogates=S, seed=3,
                                      split=split, **d)
    mix = torch.as_tensor(np.random.default_rng(0).permutation(N)).to(eng.device)
    mixed = eng.ensemble_significance(xd, n=n, p=p, freqs=freqs, fs=fs, bands=(lo, hi), measure="gpdc", n_surrogates=S, seed=3,
                                      split=split, chunk=W, **dict(d, item_group=d["item_group"][mix].contiguous(),
                                                                   item_offset=d["item_offset"][mix].contiguous()))
    for k in STATS:
        assert _same(mixed[k].cpu().numpy(), plain[k][mix].cpu().numpy()), k


# ----------------------------------------------------------------------------------------------- planted coupling
PLANT = dict(n=100, hop=50, p=2, fs=100.0, S=99, E=40, L=200)
PLANT_FREQS = np.linspace(1.0, 48.0, 32)
PLANT_DATA_SEED, PLANT_SEED = 5, 21          # checked on the CPU restatement (`restate` above): both assertions hold


def planted_epochs(seed=PLANT_DATA_SEED, E=PLANT["E"], L=PLANT["L"], weight=0.8):
    """2 + 2 channels (A: 0, 1; B: 2, 3), E trials.  B's channel 2 is driven by A's channel 0 of the same trial at lag 1;
    channels 1 and 3 share only a stimulus-locked waveform that is the same in every trial."""
    rng = np.random.default_rng(seed)
    burn = 50
    t = np.arange(L + burn)
    evoked = 1.5 * np.exp(-0.5 * ((t - burn - 60.0) / 15.0) ** 2) * np.sin(2 * np.pi * t / 25.0)
    ep = np.empty((4, L, E))
    for e in range(E):
        w = rng.standard_normal((4, L + burn))
        x = np.zeros((4, L + burn))
        for k in range(2, L + burn):
            x[:, k] = 0.5 * x[:, k - 1] - 0.3 * x[:, k - 2] + w[:, k]
            x[2, k] += weight * x[0, k - 1]
        x[1] += evoked
        x[3] += np.roll(evoked, 3)
        ep[:, :, e] = x[:, burn:]
    return ep


def test_planted_coupling():
    n, hop, p, fs, S = (PLANT[k] for k in ("n", "hop", "p", "fs", "S"))
    ep = planted_epochs()
    lo, hi = hd.band_bins(PLANT_FREQS, ((0.0, 50.0),))
    r = sliding_ensemble_epochs_significance(ep, n, hop, p, PLANT_FREQS, fs, (lo, hi), measure="ffdtf", n_surrogates=S,
                                             seed=PLANT_SEED, split=2)
    W = len(hop_positions(PLANT["L"], n, hop))
    assert r["p"].shape == (W, 4, 4, 1) and W == 3
    print("planted: p_fwe[2,0]", r["p_fwe"][:, 2, 0, 0], "p[3,1]", r["p"][:, 3, 1, 0], "p[1,3]", r["p"][:, 1, 3, 0])
    assert (r["p_fwe"][:, 2, 0, 0] <= 0.05).all()
    assert (r["p"][:, 3, 1, 0] > 0.05).all() and (r["p"][:, 1, 3, 0] > 0.05).all()


# ------------------------------------------------------------------------------------------------------ failures
@pytest.mark.parametrize("measure", ["ffdtf", "ddtf", "gpdc"])
def test_failed_surrogates_and_items(measure):
    eng = default_engine()
    n, hop, p, fs, S, seed, split = 60, 30, 3, 100.0, 12, 9, 3
    groups = stat_groups(seed=47)
    counts = [g.shape[2] for g in groups]
    m, L = groups[0].shape[:2]
    # surrogate 0 pairs trial e of group 0 with trial pi[e]: make B0 of trial pi[e] a copy of A0 of trial e, so that in
    # this one arrangement two channels of every trial coincide (as test_gpu_significance does with the shift)
    # Group 0 is rounded to small integers first: every product and sum of K1 is then exact, so the coinciding channels
    # give exactly equal rows of the covariances whatever the order in which the copied and the computed blocks were summed.
    pi = sg.trial_permutations(np.random.default_rng(seed), S, counts)[0][0]
    groups[0] = np.round(4.0 * groups[0])
    groups[0][3][:, pi] = groups[0][0]
    offsets = hop_positions(L, n, hop)
    W = len(offsets)
    freqs = np.linspace(1.0, 45.0, 16)
    lo, hi = hd.band_bins(freqs, ((0.0, 10.0), (10.0, 50.0)))
    kw = dict(measure=measure, n_surrogates=S, seed=seed, split=split, share_overlap=False)
    r = sliding_ensemble_epochs_significance(groups, n, hop, p, freqs, fs, (lo, hi), **kw)
    assert (r["n_valid"][0] == S - 1).all() and (r["n_valid"][1] == S).all()
    t = r["tested"]
    for k in ("p", "p_fwe", "null_mean", "null_std"):
        assert np.isfinite(r[k][:, :, t]).all() and np.isnan(r[k][:, :, ~t]).all(), k
    # the smallest p a cell can have is 1 / (1 + n_valid): 1 / S where one surrogate failed, 1 / (S + 1) where none did
    assert (r["p"][0][:, t] >= 1.0 / S).all() and (r["p"][1][:, t] >= 1.0 / (S + 1)).all()
    # a failed observed item: group 1 has a channel that is zero in every trial
    bad = [g.copy() for g in stat_groups(seed=48)]
    bad[1][4] = 0.0
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
        sliding_ensemble_epochs_significance(bad, n, hop, p, freqs, fs, (lo, hi), **kw)
    assert list(ei.value.items) == list(range(W, 2 * W))
    r = sliding_ensemble_epochs_significance(bad, n, hop, p, freqs, fs, (lo, hi), check="nan", **kw)
    for k in ("observed", "p", "p_fwe", "null_mean", "null_std"):
        assert np.isnan(r[k][1]).all() and np.isfinite(r[k][0][:, t]).all(), k
    assert (r["n_valid"][0] == S).all()
    # no items, a group of one trial, no automatic order
    xd = eng.to_device(np.moveaxis(groups[1], 2, 0))
    E = counts[1]
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
    e = i64([])
    d = dict(trial_rec=i64(np.arange(E)), trial_start=i64(np.zeros(E)), group_ptr=i64([0, E]), item_group=e, item_offset=e)
    args = dict(n=n, p=p, freqs=freqs, fs=fs, bands=(lo, hi), measure=measure, n_surrogates=S, seed=seed, split=split)
    r = eng.ensemble_significance(xd, **d, **args)
    assert tuple(r["p"].shape) == (0, m, m, 2) and tuple(r["n_valid"].shape) == (0,) and tuple(r["tested"].shape) == (m, m)
    with pytest.raises(ValueError, match="at least 2 trials"):
        eng.ensemble_significance(xd, **dict(d, group_ptr=i64([0, 1, E]), item_group=i64([0, 1]), item_offset=i64([0, 0])), **args)
    with pytest.raises(ValueError, match="integer model order"):
        eng.ensemble_significance(xd, **d, **dict(args, p=None))


def test_onsets_front_end_matches_the_epochs_front_end():
    n, hop, p, fs, S = 60, 30, 3, 100.0, 8
    rng = np.random.default_rng(3)
    x = coloured(rng, (6, 3000))
    onsets = np.sort(rng.choice(np.arange(100, 2800), 9, replace=False))
    pre, L = 20, 120
    ep = np.stack([x[:, s - pre:s - pre + L] for s in onsets], axis=2)
    freqs = np.arange(1.0, 33.0)
    lo, hi = hd.band_bins(freqs, ((0.0, 12.0), (12.0, 40.0)))
    kw = dict(measure="gpdc", n_surrogates=S, seed=2, split=3, share_overlap=False)
    a = sliding_ensemble_significance(x, onsets, n, p, freqs, fs, (lo, hi), pre=pre, post=L - pre, hop=hop, **kw)
    b = sliding_ensemble_epochs_significance(ep, n, hop, p, freqs, fs, (lo, hi), **kw)
    assert a["p"].shape == (len(hop_positions(L, n, hop)), 6, 6, 2)
    for k in STATS:
        assert _same(a[k], b[k]), k
