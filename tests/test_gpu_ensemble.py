"""Event-locked multi-trial sliding-window connectivity on the MI355X (`Engine.lagcov_ensemble` / `sliding_ensemble`,
`sliding.sliding_ensemble` / `sliding_ensemble_epochs`): the trial-averaged lag covariances in both K1 forms, the
reference's golden outputs on (channels, samples, trials) input, every window of every shape against the oracle on the
stacked trials, bit identity with the single-trial engine for groups of one trial, batch invariance, the two front ends
against each other, and the failure modes.  All @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd.engine import SingularMatrixError, default_engine
    from hyperscanning_signal_analysis_amd.sliding import (hop_positions, sliding_ensemble, sliding_ensemble_epochs)
    from tests.test_gpu_sliding_conn import _device_case, _signal, ddtf_restated

GUARD = 1e-9          # test_gpu_parity's guard for the golden vectors
EPS = np.finfo(np.float64).eps
FS = 100.0
FREQS = np.linspace(1.0, 45.0, 8)
# (m, p, n, trials, hop, epoch length): hop > p and k = n / hop = 4..6 everywhere, so both K1 forms apply
SHAPES = [(3, 1, 24, 12, 6, 120), (8, 4, 60, 40, 10, 200), (19, 8, 80, 60, 16, 240), (64, 8, 100, 100, 20, 300)]


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


def workload(m, p, n, E, hop, L):
    T = E * L + 500
    x = _signal(1, m, T, 7 * m + p)[0]
    onsets = np.sort(np.random.default_rng(1).choice(np.arange(50, T - L - 50), E, replace=False))
    return x, onsets, hop_positions(L, n, hop)


def stack_of(x, starts, off, n):
    return np.stack([x[:, s + off:s + off + n] for s in starts], axis=2)


def describe(eng, starts_per_group, recs_per_group, offsets):
    """Device index tensors of groups that all slide the same offsets; items group-major, window-minor."""
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
    counts = [len(s) for s in starts_per_group]
    G, W = len(counts), len(offsets)
    return dict(trial_rec=i64(np.concatenate(recs_per_group)), trial_start=i64(np.concatenate(starts_per_group)),
                group_ptr=i64(np.concatenate([[0], np.cumsum(counts)])), item_group=i64(np.repeat(np.arange(G), W)),
                item_offset=i64(np.tile(offsets, G)))


def one_group(eng, onsets, offsets):
    return describe(eng, [onsets], [np.zeros(len(onsets), dtype=np.int64)], offsets)


DIRECT = 8            # _lib.FLAG_DIRECT_LAGCOV (restated: the module imports the library only where a GPU is present)


@pytest.mark.parametrize("m,p,n,E,hop,L", SHAPES + [
    (5, 3, 40, 9, 20, 120),        # k = 2
    (5, 3, 48, 9, 4, 100),         # k = 12, above the single-trial limit of 8
    (6, 2, 35, 11, 7, 91),         # a hop that is no multiple of the 4-sample MFMA step, odd k
    (33, 5, 96, 5, 3 * 4, 180),    # 48 padded channels
    (7, 4, 640, 3, 20, 700),       # k = 32, the limit of the shared form
])
def test_lagcov_ensemble_both_forms(m, p, n, E, hop, L):
    """K1: the trial-averaged lag covariances against the oracle on the stacked trials (1e-12, assert_parity), the
    shared-overlap form against the direct form (< 1e-13 of the maximum, as test_lag_covariances_from_shared_hop_blocks),
    the padded channels' identity block, and a last window that ends exactly at the end of the recording."""
    eng = default_engine()
    x, onsets, offsets = workload(m, p, n, E, hop, L)
    T = x.shape[1]
    onsets = np.sort(np.r_[onsets[:-1], T - (offsets[-1] + n)])       # the last window of one trial ends at T
    assert onsets[-1] + offsets[-1] + n == T
    xd = eng.to_device(x[None])
    d = one_group(eng, onsets, offsets)
    direct = eng.lagcov_ensemble(xd, n=n, p=p, **d)
    direct2 = eng.lagcov_ensemble(xd, n=n, p=p, grid=(hop, len(offsets)), flags=DIRECT, **d)
    shared = eng.lagcov_ensemble(xd, n=n, p=p, grid=(hop, len(offsets)), **d)
    assert int(eng.lib.hmv_lagcov_ensemble_workspace_doubles(len(offsets), m, n, p, hop, len(offsets))) > 0   # the shared form ran
    mp = direct.shape[-1]
    assert tuple(direct.shape) == tuple(shared.shape) == (len(offsets), p + 1, mp, mp)
    assert torch.equal(direct, direct2)
    err = float((shared - direct).abs().max() / direct.abs().max())
    print(f"K1 m={m} p={p} n={n} E={E} hop={hop}: shared vs direct {err:.2e}")
    assert err < 1e-13
    for R in (direct, shared):
        if mp > m:
            eye = torch.eye(mp - m, dtype=torch.float64, device=eng.device).expand(len(offsets), -1, -1)
            assert torch.equal(R[:, 0, m:, m:], eye)
            assert not bool(R[:, 1:, m:, :].any()) and not bool(R[:, :, :m, m:].any()) and not bool(R[:, 0, m:, :m].any())
        Rh = R.cpu().numpy()
        for w in sorted({0, len(offsets) // 2, len(offsets) - 1}):
            assert_parity(Rh[w, :, :m, :m], O.lag_covariances(stack_of(x, onsets, offsets[w], n), p), 1e-12)


def test_lagcov_ensemble_every_window_of_the_large_shape():
    m, p, n, E, hop, L = SHAPES[3]
    eng = default_engine()
    x, onsets, offsets = workload(m, p, n, E, hop, L)
    xd = eng.to_device(x[None])
    d = one_group(eng, onsets, offsets)
    for grid in (None, (hop, len(offsets))):
        R = eng.lagcov_ensemble(xd, n=n, p=p, grid=grid, **d).cpu().numpy()
        for w, off in enumerate(offsets):
            assert_parity(R[w], O.lag_covariances(stack_of(x, onsets, off, n), p), 1e-12)


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("form", ["direct", "shared"])
def test_g10_reference_outputs_on_trial_stacks(golden, case, form):
    """The reference's own outputs for `np.stack(trial windows, axis=2)` with `optimal_model_order=p`."""
    g = golden("g10_ensemble.npz")
    x, onsets, freqs, fs = g[f"{case}__x"], g[f"{case}__onsets"], g[f"{case}__freqs"], float(g[f"{case}__fs"])
    p, n, hop, L = (int(g[f"{case}__{k}"]) for k in ("p", "n", "hop", "L"))
    keep = g[f"{case}__windows"]
    kw = dict(pre=0, post=L, hop=hop, share_overlap=(form == "shared"))
    ff, S = sliding_ensemble(x, onsets, n, p, freqs, fs, spectra=True, **kw)
    dd = sliding_ensemble(x, onsets, n, p, freqs, fs, measure="ddtf", **kw)
    gp = sliding_ensemble(x, onsets, n, p, freqs, fs, measure="gpdc", **kw)
    assert ff.shape == (len(hop_positions(L, n, hop)),) + g[f"{case}__ffdtf"].shape[1:]
    for got, key in ((ff, "ffdtf"), (S, "spectra"), (dd, "ddtf"), (gp, "gpdc")):
        want = g[f"{case}__{key}"]
        for k, w in enumerate(keep):
            assert rel(got[w], want[k]) <= GUARD, (key, w, rel(got[w], want[k]))
            assert_parity(got[w], want[k])
    eng = default_engine()
    off = hop_positions(L, n, hop)
    m = x.shape[0]
    _, ar, V, _ = eng.sliding_ensemble(eng.to_device(x[None]), n=n, p=p, freqs=freqs, fs=fs, return_ar=True,
                                       grid=(hop, len(off)) if form == "shared" else None, **one_group(eng, onsets, off))
    for k, w in enumerate(keep):
        assert_parity(ar[w, :m, :m].cpu().numpy(), g[f"{case}__ar"][k])
        assert_parity(V[w, :m, :m].cpu().numpy(), g[f"{case}__V"][k])


@pytest.mark.parametrize("m,p,n,E,hop,L", SHAPES)
@pytest.mark.parametrize("form", ["direct", "shared"])
def test_every_window_vs_oracle(m, p, n, E, hop, L, form):
    """Every window of every shape against the oracle on the stacked trials, full and band output, both K1 forms.
    cond(r_left) of the ensemble fits is 3.3 / 15.7 / 29.7 / 35.2 on these shapes: no window is near K2's guard and none
    may be skipped."""
    eng = default_engine()
    x, onsets, offsets = workload(m, p, n, E, hop, L)
    xd = eng.to_device(x[None])
    d = one_group(eng, onsets, offsets)
    W = len(offsets)
    grid = (hop, W) if form == "shared" else None
    lo, hi = [0, 2, 5], [2, 5, 8]
    kw = dict(n=n, p=p, freqs=FREQS, fs=FS, grid=grid, **d)
    ff, S, ar, V, infos = eng.sliding_ensemble(xd, spectra=True, return_ar=True, **kw)
    dd = eng.sliding_ensemble(xd, measure="ddtf", **kw)
    gp = eng.sliding_ensemble(xd, measure="gpdc", **kw)
    assert not bool(infos[0].any()) and not bool(infos[1].any())
    for meas, full in (("ffdtf", eng.sliding_ensemble(xd, **kw)), ("ddtf", dd), ("gpdc", gp)):
        band = eng.sliding_ensemble(xd, measure=meas, bands=(lo, hi), **kw)
        assert tuple(band.shape) == (W, m, m, 3)
        assert torch.equal(band, eng.band_sums(full, lo, hi)), meas
    ff, S, dd, gp, ar, V = (a.cpu().numpy() for a in (ff, S, dd, gp, ar, V))
    assert ff.shape == dd.shape == gp.shape == S.shape == (W, m, m, len(FREQS))
    worst = dict(ff=0.0, gp=0.0, dd=0.0, S=0.0, ar=0.0, V=0.0)
    for w, off in enumerate(offsets):
        st = stack_of(x, onsets, off, n)
        want = O.full_freq_dtf(st, FREQS, FS, p)
        worst["ff"] = max(worst["ff"], rel(ff[w], want))
        assert_parity(ff[w], want)
        assert np.abs(ff[w].sum(axis=(1, 2)) - 1.0).max() < 1e-12
        e = np.abs(gp[w] - O.gen_partial_directed_coherence(st, FREQS, FS, p)).max()
        worst["gp"] = max(worst["gp"], e)
        assert e <= 1e-8, (w, e)
        if m <= 19:
            e, tol = np.abs(dd[w] - O.direct_dtf(st, FREQS, FS, p)).max(), 1e-7
        else:
            e, tol = np.abs(dd[w] - ddtf_restated(st, FREQS, FS, p)).max(), 1e-10
        worst["dd"] = max(worst["dd"], e)
        assert e <= tol, (w, e)
        want_S = O.multivariate_spectra(st, FREQS, FS, p)
        worst["S"] = max(worst["S"], rel(S[w], want_S))
        assert_parity(S[w], want_S)
        assert np.array_equal(S[w], S[w].transpose(1, 0, 2))
        want_ar, want_V = O.ar_coeff(st, p)
        tol = 1e2 * np.linalg.cond(O.count_corr(st, p)[0]) * EPS
        worst["ar"], worst["V"] = max(worst["ar"], rel(ar[w, :m, :m], want_ar)), max(worst["V"], rel(V[w, :m, :m], want_V))
        assert rel(ar[w, :m, :m], want_ar) <= tol and rel(V[w, :m, :m], want_V) <= tol, (w, tol)
    print(f"m={m} {form}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_bands_inside_k3_are_the_band_sums_of_the_full_output():
    """F = 32: K3's row workers add the ffDTF bands themselves (`bands_in_kernel`); same bits as the full array's sums."""
    m, p, n, E, hop, L = SHAPES[1]
    eng = default_engine()
    x, onsets, offsets = workload(m, p, n, E, hop, L)
    xd = eng.to_device(x[None])
    freqs = np.arange(1.0, 33.0)
    assert eng.bands_in_kernel(m, 32)
    kw = dict(n=n, p=p, freqs=freqs, fs=FS, **one_group(eng, onsets, offsets))
    for grid in (None, (hop, len(offsets))):
        full = eng.sliding_ensemble(xd, grid=grid, **kw)
        band = eng.sliding_ensemble(xd, grid=grid, bands=([0, 8, 20], [8, 20, 32]), **kw)
        assert torch.equal(band, eng.band_sums(full, [0, 8, 20], [8, 20, 32]))


def test_one_trial_is_the_existing_engine():
    """Groups of exactly one trial in the direct form: the bits of `Engine.lagcov` / `sliding_ffdtf` / `_ddtf` / `_gpdc` on
    the same windows (m = 8, p = 4, n = 400, hop 200: one realisation is enough for the fit)."""
    eng, x, xd, pos, rec, st = _device_case()
    n, p, fs = 400, 4, 128.0
    freqs = np.arange(1.0, 33.0)
    N = int(rec.numel())
    ar = torch.arange(N + 1, dtype=torch.int64, device=eng.device)
    # (a) every window a trial and a group of its own, offset 0; (b) one trial per recording at sample 0, the window
    # positions as offsets
    a = dict(trial_rec=rec, trial_start=st, group_ptr=ar, item_group=ar[:N], item_offset=torch.zeros_like(st))
    b = describe(eng, [[0], [0]], [[0], [1]], pos)
    for d in (a, b):
        assert torch.equal(eng.lagcov_ensemble(xd, n=n, p=p, flags=DIRECT, **d), eng.lagcov(xd, rec, st, n, p))
        for meas, fn in (("ffdtf", eng.sliding_ffdtf), ("ddtf", eng.sliding_ddtf), ("gpdc", eng.sliding_gpdc)):
            want = fn(xd, rec, st, n, p, freqs, fs, flags=DIRECT)
            got = eng.sliding_ensemble(xd, n=n, p=p, freqs=freqs, fs=fs, measure=meas, flags=DIRECT, **d)
            assert torch.equal(got, want), meas
            wb = fn(xd, rec, st, n, p, freqs, fs, flags=DIRECT, bands=([0, 8], [8, 32]))
            gb = eng.sliding_ensemble(xd, n=n, p=p, freqs=freqs, fs=fs, measure=meas, flags=DIRECT, bands=([0, 8], [8, 32]), **d)
            assert torch.equal(gb, wb), meas
    want, S = eng.sliding_ffdtf_spectra(xd, rec, st, n, p, freqs, fs, flags=DIRECT)[:2]
    got, Sg = eng.sliding_ensemble(xd, n=n, p=p, freqs=freqs, fs=fs, spectra=True, flags=DIRECT, **b)
    assert torch.equal(got, want) and torch.equal(torch.view_as_real(Sg), torch.view_as_real(S))


def test_batch_invariance_direct_form():
    """A group computed alone, inside a batch of groups with different trial counts, and with odd chunk sizes: same bits."""
    m, p, n, E, hop, L = SHAPES[1]
    eng = default_engine()
    x, onsets, offsets = workload(m, p, n, 70, hop, L)
    xd = eng.to_device(x[None])
    groups = [onsets[:40], onsets[40:47], onsets[47:70]]
    zeros = [np.zeros(len(g), dtype=np.int64) for g in groups]
    W = len(offsets)
    for meas in ("ffdtf", "ddtf", "gpdc"):
        kw = dict(n=n, p=p, freqs=FREQS, fs=FS, measure=meas)
        batch = eng.sliding_ensemble(xd, **kw, **describe(eng, groups, zeros, offsets))
        for c in (1, 5, W + 3):
            assert torch.equal(eng.sliding_ensemble(xd, chunk=c, **kw, **describe(eng, groups, zeros, offsets)), batch), (meas, c)
        for gi, g in enumerate(groups):
            alone = eng.sliding_ensemble(xd, **kw, **one_group(eng, g, offsets))
            assert torch.equal(alone, batch[gi * W:(gi + 1) * W]), (meas, gi)
    # the shared form chunked: hop blocks are summed per chunk in the same order, windows assembled the same way
    d = describe(eng, groups, zeros, offsets)
    full = eng.sliding_ensemble(xd, n=n, p=p, freqs=FREQS, fs=FS, grid=(hop, W), **d)
    for c in (1, 5, W + 3):
        assert torch.equal(eng.sliding_ensemble(xd, n=n, p=p, freqs=FREQS, fs=FS, grid=(hop, W), chunk=c, **d), full), c


def test_onsets_and_cut_epochs_agree_and_ragged_recordings():
    m, p, n, E, hop, L = SHAPES[1]
    x, onsets, offsets = workload(m, p, n, E, hop, L)
    pre = 30
    epochs = np.stack([x[:, s - pre:s - pre + L] for s in onsets], axis=2)          # the reference's (m, L, trials)
    for meas in ("ffdtf", "ddtf", "gpdc"):
        a = sliding_ensemble(x, onsets, n, p, FREQS, FS, pre=pre, post=L - pre, hop=hop, measure=meas, share_overlap=False)
        b = sliding_ensemble_epochs(epochs, n, hop, p, FREQS, FS, measure=meas, share_overlap=False)
        assert a.shape == (len(offsets), m, m, len(FREQS)) and np.array_equal(a, b), meas
        s = sliding_ensemble(x, onsets, n, p, FREQS, FS, pre=pre, post=L - pre, hop=hop, measure=meas)
        assert rel(s, a) < 1e-10
    # two recordings with different numbers of onsets
    x2 = np.stack([x, _signal(1, m, x.shape[1], 99)[0]])
    ons = [onsets[:25], onsets[5:40:2]]
    both = sliding_ensemble(x2, ons, n, p, FREQS, FS, pre=0, post=L, hop=hop, share_overlap=False)
    assert both.shape == (2, len(offsets), m, m, len(FREQS))
    for r in range(2):
        assert np.array_equal(both[r], sliding_ensemble(x2[r], ons[r], n, p, FREQS, FS, pre=0, post=L, hop=hop, share_overlap=False))
    cut = sliding_ensemble_epochs([np.stack([x2[r][:, s:s + L] for s in ons[r]], axis=2) for r in range(2)], n, hop, p, FREQS,
                                  FS, share_overlap=False)
    assert np.array_equal(cut, both)
    with pytest.raises(ValueError, match="onset array"):
        sliding_ensemble(x2, ons[:1], n, p, FREQS, FS, pre=0, post=L, hop=hop)


def test_failures():
    """A group in which one channel is zero in every trial is a singular fit the solver must report; descriptions that
    would read out of bounds never reach a kernel."""
    m, p, n, E, hop, L = SHAPES[1]
    eng = default_engine()
    x, onsets, offsets = workload(m, p, n, E, hop, L)
    x2 = np.stack([x, x, x])
    x2[1, 2] = 0.0                                                          # group 1: channel 2 is zero in every trial
    xd = eng.to_device(x2)
    W = len(offsets)
    starts = [onsets[:20], onsets[:15], onsets[10:40]]
    recs = [np.full(len(s), r, dtype=np.int64) for r, s in enumerate(starts)]
    d = describe(eng, starts, recs, offsets)
    bad_items = list(range(W, 2 * W))
    for meas in ("ffdtf", "ddtf", "gpdc"):
        for grid in (None, (hop, W)):
            kw = dict(n=n, p=p, freqs=FREQS, fs=FS, measure=meas, grid=grid, **d)
            with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
                eng.sliding_ensemble(xd, **kw)
            assert isinstance(ei.value, SingularMatrixError)
            assert list(ei.value.items) == bad_items and set(ei.value.groups) == {1}
            assert list(ei.value.offsets) == list(offsets) and "group 1, window at offset 0" in str(ei.value.args[1])
            nan = eng.sliding_ensemble(xd, check="nan", **kw)
            out, bad = eng.sliding_ensemble(xd, check="mask", **kw)
            assert bad.is_cuda and bad.cpu().tolist() == [W <= i < 2 * W for i in range(3 * W)]
            assert bool(torch.isnan(nan[W:2 * W]).all()) and bool(torch.isfinite(nan[:W]).all())
            assert bool(torch.isfinite(nan[2 * W:]).all())
            for gi in (0, 2):                                               # the other groups are untouched
                alone = eng.sliding_ensemble(xd, n=n, p=p, freqs=FREQS, fs=FS, measure=meas, grid=grid,
                                             **describe(eng, [starts[gi]], [recs[gi]], offsets))
                assert torch.equal(alone, nan[gi * W:(gi + 1) * W]) and torch.equal(alone, out[gi * W:(gi + 1) * W])
    # refused before any launch
    T = x.shape[1]
    kw = dict(n=n, p=p, freqs=FREQS, fs=FS)
    with pytest.raises(ValueError, match="must lie in"):
        eng.sliding_ensemble(xd, **kw, **one_group(eng, np.r_[onsets[:5], T - L + 1], offsets))
    with pytest.raises(ValueError, match="must lie in"):
        eng.sliding_ensemble(xd, **kw, **one_group(eng, np.r_[-1, onsets[:5]], offsets))
    with pytest.raises(ValueError, match="must lie in"):
        sliding_ensemble(x, np.r_[onsets[:5], T - 10], n, p, FREQS, FS, pre=0, post=L, hop=hop)
    with pytest.raises(ValueError, match="is empty"):
        eng.sliding_ensemble(xd, **kw, **describe(eng, [onsets[:5], onsets[:0], onsets[5:9]], [np.zeros(5), np.zeros(0), np.zeros(4)], offsets))
    with pytest.raises(ValueError, match="integer model order"):
        eng.sliding_ensemble(xd, n=n, p=None, freqs=FREQS, fs=FS, **one_group(eng, onsets, offsets))
    with pytest.raises(ValueError, match="contradicts"):
        dd = one_group(eng, onsets, offsets)
        dd["item_offset"] = dd["item_offset"].flip(0).contiguous()
        eng.sliding_ensemble(xd, grid=(hop, W), **kw, **dd)
    # the empty batch: correctly shaped empties
    e = torch.zeros(0, dtype=torch.int64, device=eng.device)
    dd = dict(one_group(eng, onsets, offsets), item_group=e, item_offset=e)
    assert tuple(eng.sliding_ensemble(xd, **kw, **dd).shape) == (0, m, m, len(FREQS))
    assert tuple(eng.sliding_ensemble(xd, bands=([0, 4], [4, 8]), measure="gpdc", **kw, **dd).shape) == (0, m, m, 2)
    assert tuple(eng.lagcov_ensemble(xd, n=n, p=p, **dd).shape) == (0, p + 1, 16, 16)
    assert _lib.FLAG_DIRECT_LAGCOV == DIRECT
