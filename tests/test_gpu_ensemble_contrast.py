"""Condition-contrast permutation test of event-locked connectivity on the MI355X (`Engine.lagcov_trials`,
`Engine.lagcov_mix`, `Engine.sliding_mix`, `Engine.ensemble_contrast`, `sliding.sliding_ensemble_contrast` /
`sliding_ensemble_epochs_contrast`): the mix kernel against numpy.einsum, label rows against the ensemble K1, bits that do
not depend on the batch, the mix route against the relabelled-epochs route, every statistic against the restatement from
the documented draws, determinism and block invariance, a planted contrast, failed fits, and the two front-ends against
each other.  All @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

from hyperscanning_signal_analysis_amd import surrogates as sg
from tests.contrast_restated import PLANT, PLANT_FREQS, band_bins, coloured, planted_conditions, restate

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd.engine import Engine, default_engine
    from hyperscanning_signal_analysis_amd.sliding import (hop_positions, sliding_ensemble_contrast, sliding_ensemble_epochs,
                                                           sliding_ensemble_epochs_contrast)

EPS = np.finfo(np.float64).eps
DIRECT = 8            # _lib.FLAG_DIRECT_LAGCOV


def _i64(eng, a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind in "fc")


def _flat(r):
    """A result dict (tensors or arrays) as {key: array}, the group sub-dict under "group/<key>"."""
    h = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
    out = {k: h(v) for k, v in r.items() if k != "group"}
    out.update({"group/" + k: h(v) for k, v in r.get("group", {}).items()})
    return out


# ---------------------------------------------------------------------------------------------------- the kernel
# (m, p, E, W, n_mix): trial counts that are and are not multiples of the kernel's unroll, row counts below, at and above one
# 16-row tile, every channel padding (MP = 16, 32, 48, 64)
MIX_SHAPES = [(6, 3, 1, 1, 1), (6, 3, 5, 3, 2), (20, 4, 9, 2, 17), (38, 6, 4, 1, 16), (64, 8, 7, 2, 3)]


@pytest.mark.parametrize("m,p,E,W,rows", MIX_SHAPES)
def test_mix_against_einsum(m, p, E, W, rows):
    """Random stack, random general weights (negative ones included) and a scale.  Elementwise tolerance
    (E + 2) eps |scale_k| sum_e |W_ke| |Rt_e|: E fused multiply-adds and one multiplication, each within eps / 2 of a
    partial result that the sum of the absolute terms bounds.  The padding of the stack is poisoned with NaN: the kernel
    writes the padding of the output (zero, identity at lag 0) without reading it."""
    eng = default_engine()
    mp = eng.pad(m)
    rng = np.random.default_rng(1000 * m + 10 * E + rows)
    Rt = np.full((E, W, p + 1, mp, mp), np.nan)
    Rt[..., :m, :m] = rng.standard_normal((E, W, p + 1, m, m))
    Wt = rng.standard_normal((rows, E))
    scale = rng.uniform(0.2, 2.0, rows) * rng.choice([-1.0, 1.0], rows)
    assert (Wt < 0).any()
    got = eng.lagcov_mix(eng.to_device(Rt), eng.to_device(Wt), eng.to_device(scale), m=m)
    assert tuple(got.shape) == (rows * W, p + 1, mp, mp)
    g = got.view(rows, W, p + 1, mp, mp).cpu().numpy()
    real = Rt[..., :m, :m]
    want = np.einsum("ke,ewlij->kwlij", Wt, real) * scale[:, None, None, None, None]
    tol = (E + 2) * EPS * np.abs(scale)[:, None, None, None, None] * np.einsum("ke,ewlij->kwlij", np.abs(Wt), np.abs(real))
    err = np.abs(g[..., :m, :m] - want)
    print(f"mix m={m} p={p} E={E} W={W} rows={rows}: max err / tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    pad = np.zeros((p + 1, mp, mp))
    pad[0] = np.eye(mp)
    mask = np.ones((mp, mp), dtype=bool)
    mask[:m, :m] = False
    assert np.array_equal(g[..., mask], np.broadcast_to(pad[:, mask], g[..., mask].shape))
    # without a scale: the same chains, multiplied by 1
    one = eng.lagcov_mix(eng.to_device(Rt), eng.to_device(Wt), None, m=m)
    ones = eng.lagcov_mix(eng.to_device(Rt), eng.to_device(Wt), eng.to_device(np.ones(rows)), m=m)
    assert torch.equal(one, ones)


@pytest.mark.parametrize("m,n,p,counts", [(6, 70, 3, (3, 5)), (64, 100, 8, (4, 6))])
def test_label_rows_are_the_ensemble_estimator(m, n, p, counts):
    """0 / 1 label rows with scale = 1 / E_c on the stack of `lagcov_trials` against `lagcov_ensemble` in the direct form on
    the same trials as one group per condition, at offsets 0 and 7.  Two orders of the same E_c n products per element: the
    bound of tests/test_ensemble_contrast_cpu.py, (E_c n + n + E_c + 6) eps / 2 mean_e sqrt(d_e[i] d_e[j])."""
    eng = default_engine()
    rng = np.random.default_rng(10 * m + n)
    E, offs = sum(counts), (0, 7)
    x = np.stack([coloured(rng, (m, n + 7 + 5)) for _ in range(E)])
    start = rng.integers(0, 6, E)
    xd, rec, st, off = eng.to_device(x), _i64(eng, np.arange(E)), _i64(eng, start), _i64(eng, offs)
    Rt = eng.lagcov_trials(xd, rec, st, off, n, p)
    mp = eng.pad(m)
    assert tuple(Rt.shape) == (E, 2, p + 1, mp, mp)
    labels = np.zeros((2, E))
    labels[0, :counts[0]] = 1.0
    labels[1, counts[0]:] = 1.0
    got = eng.lagcov_mix(Rt, eng.to_device(labels), eng.to_device([1.0 / counts[0], 1.0 / counts[1]]), m=m)
    want = eng.lagcov_ensemble(xd, rec, st, _i64(eng, [0, counts[0], E]), _i64(eng, [0, 0, 1, 1]), _i64(eng, offs * 2), n, p,
                               flags=DIRECT)
    assert torch.equal(got[..., m:, :], want[..., m:, :]) and torch.equal(got[..., :, m:], want[..., :, m:])       # the padding
    g = got.view(2, 2, p + 1, mp, mp)[..., :m, :m].cpu().numpy()
    w = want.view(2, 2, p + 1, mp, mp)[..., :m, :m].cpu().numpy()
    d = np.diagonal(Rt[:, :, 0, :m, :m].cpu().numpy(), axis1=-2, axis2=-1)            # (E, W, m): lag-0 diagonal of every trial
    for c, sel in enumerate((slice(0, counts[0]), slice(counts[0], E))):
        root = np.sqrt(d[sel][:, :, :, None] * d[sel][:, :, None, :]).mean(axis=0)     # (W, m, m)
        bound = (counts[c] * n + n + counts[c] + 6) * EPS / 2 * root[:, None]
        err = np.abs(g[c] - w[c])
        print(f"labels m={m} n={n} E_c={counts[c]}: max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()


def test_bits_do_not_depend_on_the_batch():
    """A row computed alone, inside a 17-row call, and through `sliding_mix` with chunks that cut rows (1, W - 1, W + 1, all)."""
    eng = default_engine()
    m, p, n, E, W, rows = 20, 4, 80, 6, 3, 17
    rng = np.random.default_rng(3)
    x = np.stack([coloured(rng, (m, n + 40)) for _ in range(E)])
    Rt = eng.lagcov_trials(eng.to_device(x), _i64(eng, np.arange(E)), _i64(eng, np.zeros(E)), _i64(eng, [0, 20, 40]), n, p)
    Wt = rng.uniform(0.0, 1.0, (rows, E))
    scale = 1.0 / Wt.sum(axis=1)
    Wd, sd = eng.to_device(Wt), eng.to_device(scale)
    full = eng.lagcov_mix(Rt, Wd, sd, m=m).view(rows, W, p + 1, 32, 32)
    for k in (0, 5, 15, 16):
        alone = eng.lagcov_mix(Rt, Wd[k:k + 1].contiguous(), sd[k:k + 1].contiguous(), m=m)
        assert torch.equal(alone.view(W, p + 1, 32, 32), full[k]), k
    assert torch.equal(eng.lagcov_mix(Rt, Wd[3:9].contiguous(), sd[3:9].contiguous(), m=m).view(6, W, p + 1, 32, 32), full[3:9])
    # one window of the stack: the other windows of the call do not matter either
    for w in range(W):
        sub = eng.lagcov_mix(Rt[:, w:w + 1].contiguous(), Wd, sd, m=m)
        assert torch.equal(sub.view(rows, p + 1, 32, 32), full[:, w]), w
    freqs = np.linspace(1.0, 45.0, 32)
    lo, hi = band_bins(freqs, ((0.0, 10.0), (10.0, 50.0)))
    for measure in ("ffdtf", "gpdc"):
        base = eng.sliding_mix(Rt, Wd, sd, n, freqs, 100.0, m=m, measure=measure, bands=(lo, hi), return_ar=True)
        assert tuple(base[0].shape) == (rows * W, m, m, 2)
        for chunk in (1, W - 1, W + 1, rows * W):
            again = eng.sliding_mix(Rt, Wd, sd, n, freqs, 100.0, m=m, measure=measure, bands=(lo, hi), return_ar=True, chunk=chunk)
            for a, b in zip(base[:3], again[:3]):                          # band values, ar, V
                assert torch.equal(a, b), (measure, chunk)
        alone = eng.sliding_mix(Rt, Wd[16:17].contiguous(), sd[16:17].contiguous(), n, freqs, 100.0, m=m, measure=measure,
                                bands=(lo, hi), return_ar=True)
        for a, b in zip(base[:3], alone[:3]):
            assert torch.equal(a[16 * W:], b), measure


# ------------------------------------------------------------------------------------------- the existing route
@pytest.mark.parametrize("measure", ["ffdtf", "ddtf", "gpdc"])
def test_sliding_mix_against_relabelled_epochs(measure):
    """Three label draws: the band values of both conditions through `sliding_mix` against `sliding_ensemble_epochs` on the
    explicitly relabelled epoch arrays.  Tolerance 1e-10 max(largest value, 1), the one the significance tests use for
    quantities that agree to rounding."""
    eng = default_engine()
    m, L, n, hop, p, fs, EA, EB = 6, 120, 60, 30, 3, 100.0, 5, 4
    rng = np.random.default_rng(17)
    pool = coloured(rng, (m, L, EA + EB))
    freqs = np.linspace(1.0, 45.0, 24)
    lo, hi = band_bins(freqs, ((0.0, 8.0), (8.0, 20.0), (20.0, 50.0)))
    offsets = hop_positions(L, n, hop)
    W = len(offsets)
    draws = sg.label_draws(np.random.default_rng(5), 3, [EA], [EB])
    xd = eng.to_device(np.moveaxis(pool, 2, 0))
    Rt = eng.lagcov_trials(xd, _i64(eng, np.arange(EA + EB)), _i64(eng, np.zeros(EA + EB)), _i64(eng, offsets), n, p, grid=(hop, W))
    labels = np.zeros((6, EA + EB))
    for s in range(3):
        labels[2 * s, draws[s][0]] = 1.0
        labels[2 * s + 1] = 1.0 - labels[2 * s]
    got = eng.sliding_mix(Rt, eng.to_device(labels), eng.to_device(np.tile([1.0 / EA, 1.0 / EB], 3)), n, freqs, fs, m=m,
                          measure=measure, bands=(lo, hi)).view(3, 2, W, m, m, 3).cpu().numpy()
    for s in range(3):
        a = draws[s][0]
        b = np.setdiff1d(np.arange(EA + EB), a)
        want = sliding_ensemble_epochs([pool[:, :, a], pool[:, :, b]], n, hop, p, freqs, fs, measure=measure, bands=(lo, hi))
        err = np.abs(got[s] - want).max()
        print(f"{measure} draw {s}: err {err:.2e}, largest value {np.abs(want).max():.3f}")
        assert err <= 1e-10 * max(np.abs(want).max(), 1.0)


# ---------------------------------------------------------------------------------------------------- statistics
STAT = dict(n=60, hop=30, p=3, fs=100.0, S=24, seed=11)
STAT_FREQS = np.linspace(1.0, 45.0, 24)
STAT_EDGES = ((0.0, 8.0), (8.0, 20.0), (20.0, 50.0))


def stat_groups():
    rng = np.random.default_rng(41)
    a = [coloured(rng, (6, 120, c)) for c in (8, 9)]
    b = [coloured(rng, (6, 120, c)) for c in (7, 9)]
    return a, b


def _check_statistics(got, want, ties, tested, S, what):
    """got / want: one level of the result (the cells, or the group sub-dict); ties: its near-tie mask."""
    assert np.array_equal(got["n_valid"], want["n_valid"]) and (want["n_valid"] == S).all()
    t = np.broadcast_to(tested[:, :, None], got["p"].shape)
    for k in [k for k in ("observed", "observed_a", "observed_b") if k in got]:
        scale = np.abs(want[k]).max()
        assert np.abs(got[k] - want[k]).max() <= 1e-10 * max(scale, 1.0), (what, k)
    for k in ("null_mean", "null_std"):
        assert np.array_equal(np.isnan(got[k]), ~t), (what, k)
        scale = np.abs(want[k][t]).max()
        assert np.abs(got[k][t] - want[k][t]).max() <= 1e-10 * max(scale, 1.0), (what, k)
    keep = t & ~ties
    excluded = int((t & ties).sum())
    print(f"{what}: {excluded} of {int(t.sum())} tested cells excluded as near-ties")
    assert excluded <= 0.02 * t.sum()
    for k in ("p", "p_fwe"):
        assert np.array_equal(np.isnan(got[k]), ~t), (what, k)
        assert np.array_equal(got[k][keep], want[k][keep]), (what, k)
        assert (got[k][t] > 0).all() and (got[k][t] <= 1).all()


@pytest.mark.parametrize("measure,tail", [("ffdtf", "two-sided"), ("ddtf", "two-sided"), ("gpdc", "two-sided"), ("ffdtf", "greater")])
def test_statistics_vs_restatement(measure, tail):
    """Every statistic, per dyad and in `group`, against tests/contrast_restated.py.  Near-ties of the restatement alone with
    these seeds (CPU, before any GPU run): 0 of 540 tested cells for each of the three measures, 0 of 270 at the group level."""
    n, hop, p, fs, S, seed = (STAT[k] for k in ("n", "hop", "p", "fs", "S", "seed"))
    ga, gb = stat_groups()
    m, L = ga[0].shape[:2]
    lo, hi = band_bins(STAT_FREQS, STAT_EDGES)
    offsets = hop_positions(L, n, hop)
    res = sliding_ensemble_epochs_contrast(ga, gb, n, hop, p, STAT_FREQS, fs, (lo, hi), measure=measure, n_surrogates=S, seed=seed,
                                           tail=tail)
    G, W = 2, len(offsets)
    assert res["p"].shape == (G, W, m, m, 3) and res["n_valid"].shape == (G, W) and res["group"]["p"].shape == (W, m, m, 3)
    tested = ~np.eye(m, dtype=bool)
    assert np.array_equal(res["tested"], tested)
    assert np.array_equal(res["observed"], res["observed_a"] - res["observed_b"])
    want, ties = restate(measure, ga, gb, offsets, n, p, STAT_FREQS, fs, lo, hi, S, seed, tail=tail)
    _check_statistics(res, want, ties["cells"], tested, S, f"{measure}/{tail} cells")
    _check_statistics(res["group"], want["group"], ties["group"], tested, S, f"{measure}/{tail} group")


def test_split_tests_the_inter_brain_pairs_and_less_mirrors_greater():
    ga, gb = stat_groups()
    lo, hi = band_bins(STAT_FREQS, STAT_EDGES)
    kw = dict(measure="gpdc", n_surrogates=6, seed=2, split=2)
    up = sliding_ensemble_epochs_contrast(ga[0], gb[0], 60, 30, 3, STAT_FREQS, 100.0, (lo, hi), tail="greater", **kw)
    dn = sliding_ensemble_epochs_contrast(gb[0], ga[0], 60, 30, 3, STAT_FREQS, 100.0, (lo, hi), tail="less", **kw)
    t = sg.tested_mask(6, "shift", 2)
    assert np.array_equal(up["tested"], t) and "group" not in up and up["p"].shape == (3, 6, 6, 3)
    assert np.isnan(up["p"][:, ~t]).all() and np.isfinite(up["p"][:, t]).all()
    # B - A under "less" of the swapped conditions is A - B under "greater" only where the draws coincide: the observed
    # values do, whatever the draws
    assert np.array_equal(up["observed_a"], dn["observed_b"]) and np.array_equal(up["observed"], -dn["observed"])


# --------------------------------------------------------------------------------------- determinism and blocking
def test_determinism_and_block_invariance():
    eng = default_engine()
    n, hop, p, fs, S = 60, 30, 3, 100.0, 10
    rng = np.random.default_rng(43)
    ca, cb = (5, 7), (6, 4)
    ga = [coloured(rng, (6, 120, c)) for c in ca]
    gb = [coloured(rng, (6, 120, c)) for c in cb]
    m, L = 6, 120
    offsets = hop_positions(L, n, hop)
    W = len(offsets)
    # the pools: A's trials of a group, then its B's; every trial a recording of its own
    xs, cond, counts = [], [], []
    for g in range(2):
        xs += [np.moveaxis(ga[g], 2, 0), np.moveaxis(gb[g], 2, 0)]
        cond += [0] * ca[g] + [1] * cb[g]
        counts.append(ca[g] + cb[g])
    x = np.concatenate(xs, axis=0)
    E = len(cond)
    freqs = np.arange(1.0, 33.0)
    lo, hi = band_bins(freqs, ((0.0, 8.0), (8.0, 20.0), (20.0, 40.0)))

    def run(engine, seed, chunk=None, grid=(hop, W)):
        d = dict(trial_rec=_i64(engine, np.arange(E)), trial_start=_i64(engine, np.zeros(E)),
                 group_ptr=_i64(engine, np.concatenate([[0], np.cumsum(counts)])), cond=_i64(engine, cond),
                 offsets=_i64(engine, offsets))
        r = engine.ensemble_contrast(engine.to_device(x), n=n, p=p, freqs=freqs, fs=fs, bands=(lo, hi), measure="ffdtf",
                                     n_surrogates=S, seed=seed, chunk=chunk, grid=grid, **d)
        return _flat(r)
    base = run(eng, 3)
    assert (base["n_valid"] == S).all() and base["p"].shape == (2, W, m, m, 3) and base["group/p"].shape == (W, m, m, 3)
    # again; one surrogate per block; several; all; one window; a single item
    for chunk in (None, 2 * W, 3 * 2 * W + 1, S * 2 * W, W, 1):
        again = run(eng, 3, chunk)
        for k in base:
            assert _same(again[k], base[k]), (chunk, k)
    # the stack of a group built in two blocks of windows: 11 trials x 8 KiB per window, two windows fit into half of this
    small = Engine(max_workspace_bytes=400_000)
    assert 2 * 11 * 4 * 256 * 8 <= small.max_workspace_bytes // 2 < 3 * 11 * 4 * 256 * 8
    split = run(small, 3)
    for k in base:
        assert _same(split[k], base[k]), ("window blocks", k)
    plain = run(eng, 3, grid=None)                        # the direct form of K1: equal to rounding, and block-invariant alike
    split = run(small, 3, grid=None)
    for k in base:
        assert _same(split[k], plain[k]), ("window blocks, direct form", k)
    assert np.abs(plain["observed"] - base["observed"]).max() <= 1e-10
    other = run(eng, 4)
    for k in ("observed", "observed_a", "observed_b", "group/observed"):
        assert np.array_equal(other[k], base[k]), k
    assert not np.array_equal(other["null_mean"], base["null_mean"], equal_nan=True)
    assert not np.array_equal(other["group/null_mean"], base["group/null_mean"], equal_nan=True)


# ----------------------------------------------------------------------------------------------- planted contrast
def test_planted_contrast():
    """The data and the three assertions of tests/test_ensemble_contrast_cpu.py::test_planted_contrast_on_the_restatement.
    The other cells of row 2 are not asserted on: the row normalisation of the ffDTF makes them significant too."""
    n, hop, p, fs, S, seed = (PLANT[k] for k in ("n", "hop", "p", "fs", "S", "seed"))
    ep_a, ep_b = planted_conditions()
    lo, hi = band_bins(PLANT_FREQS, ((0.0, 50.0),))
    r = sliding_ensemble_epochs_contrast(ep_a, ep_b, n, hop, p, PLANT_FREQS, fs, (lo, hi), measure="ffdtf", n_surrogates=S, seed=seed)
    assert r["p"].shape == (3, 4, 4, 1) and "group" not in r
    print("planted: D[2,0]", r["observed"][:, 2, 0, 0], "p_fwe[2,0]", r["p_fwe"][:, 2, 0, 0], "p[3,1]", r["p"][:, 3, 1, 0],
          "p[0,2]", r["p"][:, 0, 2, 0])
    assert (r["p_fwe"][:, 2, 0, 0] <= 0.05).all()
    assert (r["p"][:, 3, 1, 0] > 0.05).all() and (r["p"][:, 0, 2, 0] > 0.05).all()


# ------------------------------------------------------------------------------------------------------ failures
@pytest.mark.parametrize("measure", ["ffdtf", "ddtf", "gpdc"])
def test_failed_fits(measure):
    n, hop, p, fs, S, seed = 60, 30, 3, 100.0, 12, 9
    rng = np.random.default_rng(47)
    ca, cb = (4, 5), (2, 4)
    ga = [coloured(rng, (6, 120, c)) for c in ca]
    gb = [coloured(rng, (6, 120, c)) for c in cb]
    freqs = np.linspace(1.0, 45.0, 16)
    lo, hi = band_bins(freqs, ((0.0, 10.0), (10.0, 50.0)))
    W = len(hop_positions(120, n, hop))
    kw = dict(measure=measure, n_surrogates=S, seed=seed)
    good = sliding_ensemble_epochs_contrast(ga, gb, n, hop, p, freqs, fs, (lo, hi), **kw)
    assert (good["n_valid"] == S).all()
    t = good["tested"]
    # a failed observed fit: group 1 has a channel that is zero in every trial of condition B
    bad_b = [g.copy() for g in gb]
    bad_b[1][4] = 0.0
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
        sliding_ensemble_epochs_contrast(ga, bad_b, n, hop, p, freqs, fs, (lo, hi), **kw)
    assert "group 1" in str(ei.value) and "condition B" in str(ei.value) and "window 0" in str(ei.value)
    assert ei.value.group == 1 and list(ei.value.windows) == list(range(W))
    r = sliding_ensemble_epochs_contrast(ga, bad_b, n, hop, p, freqs, fs, (lo, hi), check="nan", **kw)
    for k in ("observed", "observed_a", "observed_b", "p", "p_fwe", "null_mean", "null_std"):
        assert np.isnan(r[k][1]).all(), k
        assert _same(r[k][0], good[k][0]), k               # the other group: the same draws, the same bits
    assert np.array_equal(r["n_valid"][0], good["n_valid"][0])
    for k in ("observed", "p", "p_fwe", "null_mean", "null_std"):
        assert np.isnan(r["group"][k]).all(), k
    # surrogate-only failures: channel 4 is zero in all but the first of group 0's A trials, so a relabelling fails exactly
    # when its B set lies inside the three zero trials -- the observed labels do not
    bad_a = [g.copy() for g in ga]
    bad_a[0][4, :, 1:] = 0.0
    draws = sg.label_draws(np.random.default_rng(seed), S, ca, cb)
    failing = [s for s in range(S) if set(range(ca[0] + cb[0])) - set(draws[s][0].tolist()) <= {1, 2, 3}]
    assert 1 <= len(failing) < S
    r = sliding_ensemble_epochs_contrast(bad_a, gb, n, hop, p, freqs, fs, (lo, hi), **kw)
    assert (r["n_valid"][0] == S - len(failing)).all() and (r["n_valid"][1] == S).all()
    assert (r["group"]["n_valid"] == S - len(failing)).all()
    for k in ("p", "p_fwe", "null_mean", "null_std"):
        assert np.isfinite(r[k][:, :, t]).all() and np.isnan(r[k][:, :, ~t]).all(), k
        assert np.isfinite(r["group"][k][:, t]).all(), k
        assert _same(r[k][1], good[k][1]), k
    assert (r["p"][0][:, t] >= 1.0 / (1 + S - len(failing))).all()


def test_engine_refusals():
    eng = default_engine()
    rng = np.random.default_rng(0)
    x = eng.to_device(rng.standard_normal((5, 6, 100)))
    d = dict(trial_rec=_i64(eng, np.arange(5)), trial_start=_i64(eng, np.zeros(5)), group_ptr=_i64(eng, [0, 5]),
             cond=_i64(eng, [0, 0, 1, 1, 1]), offsets=_i64(eng, [0, 20, 40]))
    freqs = np.linspace(1.0, 45.0, 8)
    lo, hi = band_bins(freqs, ((0.0, 50.0),))
    args = dict(n=60, p=3, freqs=freqs, fs=100.0, bands=(lo, hi), measure="ffdtf", n_surrogates=4, seed=0)
    r = eng.ensemble_contrast(x, **d, **args)
    assert tuple(r["p"].shape) == (1, 3, 6, 6, 1) and "group" not in r
    assert tuple(eng.ensemble_contrast(x, **d, **args, group=True)["group"]["p"].shape) == (3, 6, 6, 1)
    with pytest.raises(ValueError, match="integer model order"):
        eng.ensemble_contrast(x, **d, **dict(args, p=None))
    with pytest.raises(ValueError, match="at least one trial of each condition"):
        eng.ensemble_contrast(x, **dict(d, cond=_i64(eng, [0] * 5)), **args)
    with pytest.raises(ValueError, match="0 .condition A. or 1"):
        eng.ensemble_contrast(x, **dict(d, cond=_i64(eng, [0, 0, 1, 2, 1])), **args)
    with pytest.raises(ValueError, match="one entry per trial"):
        eng.ensemble_contrast(x, **dict(d, cond=_i64(eng, [0, 1])), **args)
    with pytest.raises(ValueError, match="must lie in"):
        eng.ensemble_contrast(x, **dict(d, offsets=_i64(eng, [0, 41])), **args)
    with pytest.raises(ValueError, match="grid"):
        eng.ensemble_contrast(x, **d, **args, grid=(10, 3))
    Rt = eng.lagcov_trials(x, d["trial_rec"], d["trial_start"], d["offsets"], 60, 3)
    W = eng.to_device(np.ones((2, 5)))
    with pytest.raises(ValueError, match="W must be"):
        eng.lagcov_mix(Rt, W[:, :4].contiguous(), None, m=6)
    with pytest.raises(ValueError, match="scale must be"):
        eng.lagcov_mix(Rt, W, eng.to_device(np.ones(3)), m=6)
    with pytest.raises(ValueError, match="Rt must be"):
        eng.lagcov_mix(Rt, W, None, m=20)
    with pytest.raises(ValueError, match="integer model order"):
        eng.lagcov_trials(x, d["trial_rec"], d["trial_start"], d["offsets"], 60, None)


# ---------------------------------------------------------------------------------------------------- front-ends
def test_onsets_front_end_matches_the_epochs_front_end():
    n, hop, p, fs, S = 60, 30, 3, 100.0, 8
    rng = np.random.default_rng(3)
    x = np.stack([coloured(rng, (6, 3000)) for _ in range(2)])
    pre, L = 20, 120
    on = [np.sort(rng.choice(np.arange(100, 2800), 9, replace=False)) for _ in range(2)]
    oa, ob = [o[::2] for o in on], [o[1::2] for o in on]
    cut = lambda r, o: np.stack([x[r][:, s - pre:s - pre + L] for s in o], axis=2)  # noqa: E731
    freqs = np.arange(1.0, 33.0)
    lo, hi = band_bins(freqs, ((0.0, 12.0), (12.0, 40.0)))
    kw = dict(measure="gpdc", n_surrogates=S, seed=2, share_overlap=False)
    a = sliding_ensemble_contrast(x, oa, ob, n, p, freqs, fs, (lo, hi), pre=pre, post=L - pre, hop=hop, **kw)
    b = sliding_ensemble_epochs_contrast([cut(0, oa[0]), cut(1, oa[1])], [cut(0, ob[0]), cut(1, ob[1])], n, hop, p, freqs, fs,
                                         (lo, hi), **kw)
    assert a["p"].shape == (2, len(hop_positions(L, n, hop)), 6, 6, 2)
    fa, fb = _flat(a), _flat(b)
    assert sorted(fa) == sorted(fb) and "group/p" in fa
    for k in fa:
        assert _same(fa[k], fb[k]), k
    # a single recording: no group level, no leading axis
    one = sliding_ensemble_contrast(x[0], oa[0], ob[0], n, p, freqs, fs, (lo, hi), pre=pre, post=L - pre, hop=hop, **kw)
    assert one["p"].shape == a["p"].shape[1:] and "group" not in one
    assert np.array_equal(one["observed"], a["observed"][0])
