"""Block (multivariate) Granger causality per sliding window on the MI355X (`Engine.sliding_block_granger` /
`block_granger`, `sliding.sliding_block_granger`, `mtmvar.block_granger_causality`, `escan_batch.run(block_granger=True)`):
the new kernels against the NumPy restatement of the textbook definition on the GPU's own fit, end to end against the
restatement on the oracle's fit, the identities the definition satisfies (non-negativity, swap, block scaling), the
invariants of the fused call (bands, chunks, the stage on its own, grids), the failure modes, a generator whose direction
of influence is known, and the ESCan driver.  All @pytest.mark.gpu."""
import functools
import json

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O
from tests import block_gc_restated as G
from tests.scale_shapes import EPS, normal_matrix_cond

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd import mtmvar as M
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import regular_grid, sliding_block_granger, window_items
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad
    from tests.test_gpu_escan_batch import _reader, tree  # noqa: F401  (the fixture of the ESCan test, reused)

FS = 100.0
# m, split, p, F, n, recordings, windows
SHAPES = [(3, 1, 1, 16, 400, 2, 4), (5, 2, 3, 30, 400, 2, 4), (8, 4, 2, 16, 400, 2, 4), (17, 16, 2, 16, 500, 2, 4),
          (19, 7, 4, 16, 500, 2, 4), (33, 17, 4, 16, 800, 2, 4), (64, 32, 8, 32, 1000, 1, 2), (64, 63, 2, 16, 600, 2, 4)]
IDS = ["x".join(str(v) for v in s[:5]) for s in SHAPES]


def _signal(n_rec, m, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rec, m, T))
    x[..., 1:] += 0.5 * x[..., :-1]
    x[:, 1:] += 0.3 * x[:, :-1]
    return x


def _freqs(F):
    return np.linspace(1.0, 45.0, F)


@functools.lru_cache(maxsize=None)
def _input(shape):
    m, split, p, F, n, n_rec, n_win = shape
    T = n + (n // 2) * (n_win - 1)
    if m >= 33:
        x = np.stack([synthetic_var_dyad(40 + r, m=m, p=4, T=T, burn=300) for r in range(n_rec)])
    else:
        x = _signal(n_rec, m, T, 100 + m)
    return x, (n // 2) * np.arange(n_win)


def _run(x, pos, shape, split=None, **kw):
    m, split0, p, F, n, n_rec, n_win = shape
    eng = default_engine()
    xd = eng.to_device(x)
    rec, st = window_items(x.shape[0], pos, eng.device)
    return eng.sliding_block_granger(xd, rec, st, n, p, _freqs(F), FS, split=split0 if split is None else split, **kw)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The GPU's outputs and fit of one shape, and per window the restatement on that fit with the bound of item 1."""
    m, split, p, F, n, n_rec, n_win = shape
    x, pos = _input(shape)
    spectral, time, ar, V, infos = _run(x, pos, shape, return_ar=True)
    assert not any(bool(i.any()) for i in infos)
    spectral, time = spectral.cpu().numpy(), time.cpu().numpy()
    ar, V = ar.cpu().numpy()[:, :m, :m], V.cpu().numpy()[:, :m, :m]
    want, tol = [], []
    for it in range(len(spectral)):
        d = G.definition(ar[it], V[it], split, _freqs(F), FS)
        e = np.abs(d - G.inversion_free(ar[it], V[it], split, _freqs(F), FS)).max()
        want.append(d)
        tol.append(max(1e-10, 100.0 * e) * (1.0 + np.abs(d).max()))
    for a in (spectral, time):
        a.setflags(write=False)
    return dict(spectral=spectral, time=time, ar=ar, V=V, want=np.stack(want), tol=np.asarray(tol))


def _windows(shape):
    m, split, p, F, n, n_rec, n_win = shape
    x, pos = _input(shape)
    return [x[r, :, s:s + n] for r in range(n_rec) for s in pos]


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """Per window, the restatement on the oracle's fit and the bound of item 2 for the time-domain values: 1e-7 (1 + |F|)
    up to 19 channels, n_dst * 1e2 * cond * eps * (1 + |F|) from 33 (cond of the full window's normal matrix; a principal
    sub-block of a positive definite matrix is no worse conditioned than the whole)."""
    m, split, p, F, n, n_rec, n_win = shape
    out = []
    for xw in _windows(shape):
        ar, V = O.ar_coeff(xw, p)
        t = G.time_domain(O.lag_covariances(xw, p), V, split, p)
        if m <= 19:
            out.append((G.definition(ar, V, split, _freqs(F), FS), t, 1e-7 * (1.0 + np.abs(t)), None))
        else:
            cond = normal_matrix_cond(O, xw, p)
            out.append((None, t, np.array([m - split, split, m, m]) * 1e2 * cond * EPS * (1.0 + np.abs(t)), cond))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_spectral_arithmetic_against_the_definition_on_the_gpus_own_fit(shape):
    c = _case(shape)
    assert c["spectral"].shape == c["want"].shape
    for it, (got, want, tol) in enumerate(zip(c["spectral"], c["want"], c["tol"])):
        err = np.abs(got - want).max()
        print(f"{shape[:5]} window {it}: |gpu - definition| = {err:.2e}, bound {tol:.2e}, max|f| = {np.abs(want).max():.3f}")
        assert err <= tol, (it, err, tol)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_end_to_end_against_the_restatement_on_the_oracles_fit(shape):
    m = shape[0]
    c = _case(shape)
    for it, (f, t, tbound, cond) in enumerate(_oracle(shape)):
        err = np.abs(c["time"][it] - t)
        print(f"{shape[:5]} window {it}: time err {err}, bound {tbound}" + (f", cond {cond:.2e}" if cond else ""))
        assert (err <= tbound).all()
        if m <= 19:
            ef = np.abs(c["spectral"][it] - f) / (1.0 + np.abs(f))
            print(f"{shape[:5]} window {it}: spectral {ef.max():.2e} (bound 1e-7)")
            assert ef.max() <= 1e-7


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_properties(shape):
    c = _case(shape)
    assert np.isfinite(c["spectral"]).all() and np.isfinite(c["time"]).all()
    assert (c["spectral"] >= -c["tol"][:, None, None]).all()
    for it, (_, _, tbound, _) in enumerate(_oracle(shape)):
        assert (c["time"][it, :3] >= -tbound[:3]).all()
    total = np.abs(c["time"][:, 3] - c["time"][:, :3].sum(axis=1)).max()
    print(f"{shape[:5]}: |total - sum of the three| = {total:.2e} (bound 1e-12)")
    assert total <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_swapping_the_blocks_swaps_the_directions(shape):
    m, split = shape[0], shape[1]
    c = _case(shape)
    x, pos = _input(shape)
    xs = np.concatenate([x[:, split:], x[:, :split]], axis=1)
    spectral, time = (a.cpu().numpy() for a in _run(xs, pos, shape, split=m - split))
    tol = c["tol"]
    err_f = np.abs(spectral[:, ::-1] - c["spectral"]).max(axis=(1, 2))
    err_t = np.abs(time[:, [1, 0, 2, 3]] - c["time"]).max(axis=1)
    print(f"{shape[:5]}: swap spectral {err_f.max():.2e}, time {err_t.max():.2e}, bound {tol.min():.2e}")
    assert (err_f <= tol).all()
    assert (err_t <= tol).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_block_scaling_leaves_every_output_unchanged(shape):
    """Block A times 2^-17, block B times 2^9: the log-determinants cancel, they do not overflow."""
    split = shape[1]
    c = _case(shape)
    x, pos = _input(shape)
    xs = x.copy()
    xs[:, :split] *= 2.0 ** -17
    xs[:, split:] *= 2.0 ** 9
    spectral, time = (a.cpu().numpy() for a in _run(xs, pos, shape))
    err_f = np.abs(spectral - c["spectral"]).max(axis=(1, 2))
    err_t = np.abs(time - c["time"]).max(axis=1)
    print(f"{shape[:5]}: block scaling spectral {err_f.max():.2e}, time {err_t.max():.2e}, bound {c['tol'].min():.2e}")
    assert (err_f <= c["tol"]).all()
    assert (err_t <= c["tol"]).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bands_chunks_stage_and_repeats_are_bit_identical(shape):
    m, split, p, F, n, n_rec, n_win = shape
    eng = default_engine()
    c = _case(shape)
    x, pos = _input(shape)
    full = torch.as_tensor(c["spectral"].copy(), device=eng.device)
    lo, hi = [0, 3, 5, F - 4], [3, 5, F - 4, F]
    red, t_b = _run(x, pos, shape, bands=(lo, hi))
    assert tuple(red.shape) == (len(full), 2, 4)
    assert torch.equal(red, eng.band_sums(full, lo, hi))
    assert np.array_equal(t_b.cpu().numpy(), c["time"])
    for kw in (dict(chunk=1), dict(), dict(chunk=3)):
        s2, t2 = _run(x, pos, shape, **kw)
        assert np.array_equal(s2.cpu().numpy(), c["spectral"]) and np.array_equal(t2.cpu().numpy(), c["time"]), kw
    red1, _ = _run(x, pos, shape, bands=(lo, hi), chunk=1)
    assert torch.equal(red1, red)
    _, _, ar, V, _ = _run(x, pos, shape, return_ar=True)
    stage = eng.block_granger(ar, V, m, split, _freqs(F), FS)
    assert np.array_equal(stage.cpu().numpy(), c["spectral"])
    out = eng.empty(len(full), 2, F)
    s3, _ = _run(x, pos, shape, out=out)
    assert s3 is out and torch.equal(out, full)


@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[7]], ids=[IDS[4], IDS[7]])
def test_the_restricted_fits_follow_the_form_of_k2_the_flags_select(shape):
    """HMV_FLAG_YW_TILED / _ONE_LAUNCH reach the two restricted K2 runs as they reach the full fit: the time-domain values
    and spectral values of either LDL^T form stay within the oracle bounds of item 2, at a 16-channel and a 64-channel
    restricted block."""
    from hyperscanning_signal_analysis_amd import _lib
    c = _case(shape)
    x, pos = _input(shape)
    for flag in (_lib.FLAG_YW_ONE_LAUNCH, _lib.FLAG_YW_TILED):
        spectral, time = (a.cpu().numpy() for a in _run(x, pos, shape, flags=flag))
        for it, (f, t, tbound, _) in enumerate(_oracle(shape)):
            err = np.abs(time[it] - t)
            print(f"{shape[:5]} flags {flag} window {it}: time err {err.max():.2e}, bound {tbound.min():.2e}")
            assert (err <= tbound).all()
            if f is not None:                                      # (item 2 has a spectral bound up to 19 channels)
                assert (np.abs(spectral[it] - f) <= 1e-7 * (1.0 + np.abs(f))).all()
        assert np.abs(time[:, 3] - time[:, :3].sum(axis=1)).max() <= 1e-12


def test_grids_and_wrappers():
    """The hop = n // 2 form (shared-overlap K1) and the even-windows form against the oracle bound of item 2."""
    m, split, p, n, F = 6, 2, 3, 400, 16
    x = _signal(2, m, 1200, 7)
    freqs = _freqs(F)
    for kw, pos in ((dict(hop=n // 2), np.arange(0, 1200 - n + 1, n // 2)), (dict(), None)):
        spectral, time = sliding_block_granger(x, n, 3, p, freqs, FS, split=split, **kw)
        if pos is None:
            pos, _ = O.window_positions(1200, 3, n)
        else:
            assert regular_grid(pos, n, p) is not None
        assert spectral.shape == (2, len(pos), 2, F) and time.shape == (2, len(pos), 4)
        for r in range(2):
            for w, s in enumerate(pos):
                xw = x[r, :, s:s + n]
                ar, V = O.ar_coeff(xw, p)
                f = G.definition(ar, V, split, freqs, FS)
                t = G.time_domain(O.lag_covariances(xw, p), V, split, p)
                assert (np.abs(spectral[r, w] - f) <= 1e-7 * (1.0 + np.abs(f))).all()
                assert (np.abs(time[r, w] - t) <= 1e-7 * (1.0 + np.abs(t))).all()
    # one recording, and the single-window form in the reference's signature style
    s1, t1 = sliding_block_granger(x[0], n, 3, p, freqs, FS, split=split, hop=n // 2)
    assert s1.shape == (len(np.arange(0, 1200 - n + 1, n // 2)), 2, F)
    sw, tw = M.block_granger_causality(x[0, :, :n], freqs, FS, split, optimal_model_order=p)
    assert sw.shape == (2, F) and tw.shape == (4,)
    assert np.abs(sw - s1[0]).max() <= 1e-9 * (1.0 + np.abs(sw).max()) and np.abs(tw - t1[0]).max() <= 1e-9
    sa, ta = M.block_granger_causality(x[0, :, :n], freqs, FS, split, max_model_order=5)
    assert sa.shape == (2, F) and np.isfinite(sa).all() and np.isfinite(ta).all()


def test_a_window_with_a_dead_channel_fails_alone():
    eng = default_engine()
    m, split, p, n, F = 6, 3, 3, 300, 16
    x = _signal(1, m, 4 * n, 21)
    bad = x.copy()
    bad[0, 4, 2 * n:3 * n] = 0.0                                   # window 2: an all-zero channel
    pos = np.arange(4) * n
    rec, st = window_items(1, pos, eng.device)
    freqs = _freqs(F)
    xd, bd = eng.to_device(x), eng.to_device(bad)
    good_f, good_t = eng.sliding_block_granger(xd, rec, st, n, p, freqs, FS, split=split)
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
        eng.sliding_block_granger(bd, rec, st, n, p, freqs, FS, split=split)
    assert list(ei.value.items) == [2] and "item 2" in str(ei.value.args[1])
    nan_f, nan_t = eng.sliding_block_granger(bd, rec, st, n, p, freqs, FS, split=split, check="nan")
    assert torch.isnan(nan_f[2]).all() and torch.isnan(nan_t[2]).all()
    keep = [0, 1, 3]
    assert torch.equal(nan_f[keep], good_f[keep]) and torch.equal(nan_t[keep], good_t[keep])
    _, _, mask = eng.sliding_block_granger(bd, rec, st, n, p, freqs, FS, split=split, check="mask")
    assert mask.is_cuda and mask.cpu().tolist() == [False, False, True, False]
    red, _ = eng.sliding_block_granger(bd, rec, st, n, p, freqs, FS, split=split, check="nan", bands=([0, 8], [8, 16]))
    assert torch.isnan(red[2]).all() and torch.isfinite(red[keep]).all()
    e = torch.zeros(0, dtype=torch.int64, device=eng.device)
    s0, t0 = eng.sliding_block_granger(xd, e, e, n, p, freqs, FS, split=split)
    assert tuple(s0.shape) == (0, 2, F) and tuple(t0.shape) == (0, 4)
    with pytest.raises(ValueError, match="automatic model order"):
        eng.sliding_block_granger(xd, rec, st, n, None, freqs, FS, split=split)
    with pytest.raises(ValueError, match="split"):
        eng.sliding_block_granger(xd, rec, st, n, p, freqs, FS, split=m)


def _driven_pair(seed, T=1000, burn=200):
    """Two independent 4-channel participants, every channel x_t = 0.5 x_{t-1} - 0.3 x_{t-2} + e_t; channel 0 of A enters
    channel 0 of B at lag 1 with weight 0.5."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((8, T + burn))
    x = np.zeros((8, T + burn))
    for t in range(2, T + burn):
        x[:, t] = 0.5 * x[:, t - 1] - 0.3 * x[:, t - 2] + e[:, t]
        x[4, t] += 0.5 * x[0, t - 1]
    return x[:, burn:]


def test_the_driving_participant_is_found():
    x = np.stack([_driven_pair(s) for s in range(6)])
    spectral, time = sliding_block_granger(x, 1000, 1, 2, _freqs(16), FS, split=4)
    assert spectral.shape == (6, 1, 2, 16)
    for s in range(6):
        ab, ba = spectral[s, 0, 0].sum(), spectral[s, 0, 1].sum()
        print(f"seed {s}: sum f_AB = {ab:.4f}, sum f_BA = {ba:.4f}, F_AB = {time[s, 0, 0]:.4f}, F_BA = {time[s, 0, 1]:.4f}")
        assert ab >= 4.0 * ba and time[s, 0, 0] > time[s, 0, 1]


def test_escan_block_granger(tree, tmp_path):  # noqa: F811
    freqs = np.arange(1.0, 33.0, 1.0)
    kw = dict(window_s=2.0, overlap=0.5, model_order=3, freqs=freqs, low_cutoff_hz=1.0, high_cutoff_hz=45.0, reader=_reader,
              verbose=False)
    base = EB.run(tree, tmp_path / "plain", **kw)
    gc = EB.run(tree, tmp_path / "gc", block_granger=True, **kw)
    assert base["done"] == gc["done"] == ["W_003", "W_010"]
    found = EB.discover_dyads(tree)
    lo, hi = hd.band_bins(freqs)
    for dy in base["done"]:
        z0 = np.load(tmp_path / "plain" / f"{dy}_ffdtf.npz", allow_pickle=False)
        z1 = np.load(tmp_path / "gc" / f"{dy}_ffdtf.npz", allow_pickle=False)
        m0, m1 = json.loads(str(z0["meta"])), json.loads(str(z1["meta"]))
        assert "block_granger" not in m0 and m1["block_granger"] is True
        assert set(z1.files) - set(z0.files) == {f"{s['task']}/{s['event']}/{k}" for s in m0["segments"]
                                                  for k in ("block_gc_bands", "block_gc_time")}
        for seg in m1["segments"]:
            key = f"{seg['task']}/{seg['event']}"
            assert np.array_equal(z1[f"{key}/ffdtf_bands"], z0[f"{key}/ffdtf_bands"], equal_nan=True)
            recs = {r: _reader(found[dy][seg["task"]][r]) for r in ("ch", "cg")}
            block, names, fs = EB.segment_block(recs["ch"], recs["cg"], seg["start_s"], seg["duration_s"], 1.0, 45.0)
            split = sum(1 for nm in names if nm.endswith("_ch"))
            want_f, want_t = sliding_block_granger(block, seg["window"], None, 3, freqs, fs, split=split,
                                                   hop=seg["window"] // 2, bands=(lo, hi), check="nan")
            assert z1[f"{key}/block_gc_bands"].shape == (seg["windows"], 2, len(lo))
            assert z1[f"{key}/block_gc_time"].shape == (seg["windows"], 4)
            assert np.array_equal(z1[f"{key}/block_gc_bands"], want_f, equal_nan=True)
            assert np.array_equal(z1[f"{key}/block_gc_time"], want_t, equal_nan=True)
            assert np.isfinite(want_f).all() and (want_f > -1e-9).all()
