"""Phase synchrony on the GPU (csrc/phase_sync.hip through `Engine.phase_sync`, `Engine.analytic_signal`,
`sliding.sliding_phase_sync` and `escan_batch.run(phase_sync=...)`): the kernel against the NumPy restatement to the derived
bound of tests/phase_sync_restated.py, exact symmetry, bits that do not depend on the batch, nothing written outside the
outputs, `info`, the analytic signal against an extended-precision restatement, and the composition end to end."""
import json

import numpy as np
import pytest
import torch

from tests import phase_sync_restated as PR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd.eeg_io import band_response
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions, sliding_phase_sync, window_items, window_positions

T1 = 1400
N_CASES = (1, 3, 4, 5, 63, 64, 65, 130, 1000)
KEYS = ("coherency", "mag", "lagged")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def z64():
    """(3, 64, T1) complex128: independent noise in mixed amplitudes plus one pi/2-lagged pair (channels 0 and 1)."""
    rng = np.random.default_rng(2024)
    z = rng.standard_normal((3, 64, T1)) + 1j * rng.standard_normal((3, 64, T1))
    ph = 2.0 * np.pi * 0.04 * np.arange(T1) + 0.05 * np.cumsum(rng.standard_normal((3, T1)), axis=-1)
    z[:, 0] += 6.0 * np.exp(1j * ph)
    z[:, 1] += 6.0 * np.exp(1j * (ph - np.pi / 2.0))
    z *= (10.0 ** rng.uniform(-6.0, 1.5, 64))[None, :, None]
    return z


def items_for(n):
    """Odd starts, one window ending exactly at T1, recording 1 used twice."""
    return [(0, 1), (1, min(37, T1 - n)), (2, T1 - n), (1, min(333, T1 - n)), (0, min(399, T1 - n))]


def run(z, items, n, mode, coherency=True, want=("mag", "lagged")):
    eng = default_engine()
    zd = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z)).to(eng.device)
    rec = torch.tensor([r for r, _ in items], dtype=torch.int64, device=eng.device)
    start = torch.tensor([s for _, s in items], dtype=torch.int64, device=eng.device)
    res = eng.phase_sync(zd, rec, start, n, mode, want=want, coherency=coherency)
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("m", (1, 2, 5, 16, 17, 33, 48, 64))
def test_kernel_against_the_restatement(z64, m):
    """A NumPy-made z isolates the kernel from the FFT.  worst |gpu - restated| / gram_bound <= 1 for coherency, mag and
    lagged, ciPLV restricted to the pairs with den >= 0.01.  For the windows of 63 samples and more the restatement has
    every off-diagonal |Re R| < 0.9 (asserted), so there the restriction drops nothing; windows of 1 .. 5 samples of noise
    cannot promise that (at n = 1 every |R| is 1 and Re R is the cosine of a random angle), so for them the share of pairs
    the restriction keeps is asserted instead (more than half), and coherency and mag are compared on every pair."""
    z = z64[:, :m]
    worst = {k: 0.0 for k in KEYS}
    off = ~np.eye(m, dtype=bool)
    for n in N_CASES:
        items = items_for(n)
        for mode in (PR.UNIT, PR.RAW):
            got = run(z, items, n, mode)
            assert not got["info"].any()
            for it, (r, s) in enumerate(items):
                want, bound = PR.measures_restated(z[r], s, n, mode), PR.gram_bound(z[r], s, n, mode)
                assert want["info"] == 0
                keep = np.ones((m, m), dtype=bool)
                if mode == PR.UNIT:
                    keep = off & (bound["den"] >= 0.01)
                    if n >= 63:
                        assert (np.abs(want["coherency"][0][off]) < 0.9).all()
                        assert keep[off].all()
                    elif m > 1:
                        assert keep[off].mean() > 0.5, (n, keep[off].mean())
                    assert not got["lagged"][it][~off].any()                 # the diagonal of ciPLV is exactly 0
                for k in KEYS:
                    err = np.abs(got[k][it] - want[k])
                    sel = np.broadcast_to(keep if k == "lagged" else np.ones((m, m), dtype=bool), err.shape)
                    assert np.isfinite(got[k][it]).all() and (bound[k][sel] > 0).all(), (k, n, mode)
                    ratio = float((err[sel] / bound[k][sel]).max()) if sel.any() else 0.0
                    worst[k] = max(worst[k], ratio)
                    assert ratio <= 1.0, (k, m, n, mode, it, ratio)
    print(f"m={m}: worst |gpu - restated| / bound = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("m,n", ((33, 130), (64, 67), (5, 3)))
def test_exact_structure(z64, m, n):
    z = z64[:, :m].copy()
    z[2, m - 1, :] = 0.0                                          # a channel without a sample (recording 2 only)
    items = items_for(n)
    for mode in (PR.UNIT, PR.RAW):
        got = run(z, items, n, mode)
        for it, (r, s) in enumerate(items):
            mag, lag, (re, im) = got["mag"][it], got["lagged"][it], got["coherency"][it]
            dead = r == 2
            if dead and mode == PR.RAW:
                assert got["info"][it] == 2
                live = np.arange(m) < m - 1
                assert np.isnan(mag[~live]).all() and np.isnan(mag[:, ~live]).all() and np.isnan(re[~live]).all()
                mag, lag, re, im = (a[np.ix_(live, live)] for a in (mag, lag, re, im))
            else:
                assert got["info"][it] == 0
            k = mag.shape[0]
            assert same_bits(mag, mag.T) and same_bits(lag, lag.T) and same_bits(re, re.T)
            assert np.array_equal(im, -im.T) and not im.diagonal().any()
            iu = np.triu_indices(k, 1)
            assert np.array_equal(bits(im)[iu], bits(-im.T)[iu])              # off the diagonal: bit for bit
            d = np.ones(k)
            if dead and mode == PR.UNIT:
                d[-1] = 0.0                                       # PLV of a channel without a sample: 0, info 0
                assert not mag[-1].any() and not mag[:, -1].any() and not lag[-1].any()
            assert np.array_equal(mag.diagonal(), d) and not lag.diagonal().any()
            assert (mag >= 0).all() and (mag <= 1 + 8 * PR.EPS).all() and (lag >= 0).all() and (lag <= 1 + 8 * PR.EPS).all()
    # UNIT: a power of two on a channel changes no bit
    base = run(z, items, n, PR.UNIT)
    zs = z.copy()
    zs[:, 0] *= 2.0 ** 7
    zs[:, m // 2] *= 2.0 ** -9
    scaled = run(zs, items, n, PR.UNIT)
    for k in KEYS + ("info",):
        assert np.array_equal(base[k].view(np.int64 if k != "info" else np.int32), scaled[k].view(np.int64 if k != "info" else np.int32))


def test_bits_do_not_depend_on_the_batch(z64):
    eng = default_engine()
    m, n = 17, 65
    z = z64[:, :m]
    rng = np.random.default_rng(3)
    items = [(int(r), int(s)) for r, s in zip(rng.integers(0, 3, 37), rng.integers(0, T1 - n + 1, 37))]
    items[5] = (2, T1 - n)
    for mode in (PR.UNIT, PR.RAW):
        full = run(z, items, n, mode)
        again = run(z, items, n, mode)
        for k in KEYS:
            assert same_bits(full[k], again[k])                                # run to run
        for it in (0, 5, 36):
            alone = run(z, [items[it]], n, mode)
            for k in KEYS:
                assert same_bits(alone[k][0], full[k][it]), (k, it)
        perm = rng.permutation(37)
        shuffled = run(z, [items[i] for i in perm], n, mode)
        for k in KEYS:
            assert same_bits(shuffled[k], full[k][perm]), k
        # a strided view: ld > T, a padded recording stride, NaN everywhere outside the view
        big = torch.full((3, m + 2, T1 + 11), float("nan"), dtype=torch.complex128, device=eng.device)
        view = big[:, 1:m + 1, 5:5 + T1]
        view.copy_(torch.from_numpy(np.ascontiguousarray(z)))
        assert view.stride(1) == T1 + 11 and view.stride(0) == (m + 2) * (T1 + 11) and not view.is_contiguous()
        strided = run(view, items, n, mode)
        assert not strided["info"].any()
        for k in KEYS:
            assert same_bits(strided[k], full[k]), k
        # five channels of a 64-channel recording, read in place, against the same five alone (both NT = 1)
        zd = torch.from_numpy(np.ascontiguousarray(z64)).to(eng.device)
        inside, alone5 = run(zd[:, :5], items, n, mode), run(z64[:, :5], items, n, mode)
        assert zd[:, :5].stride(0) == 64 * T1
        for k in KEYS:
            assert same_bits(inside[k], alone5[k]), k
        # ... and the same pairs inside a wider call (another NT) keep their bits too
        for k in KEYS:
            assert same_bits(full[k][..., :5, :5], inside[k]), k


def test_nothing_is_written_outside_the_outputs(z64):
    eng = default_engine()
    m, n, G = 33, 64, 512
    items = items_for(n)
    k = len(items)
    zd = torch.from_numpy(np.ascontiguousarray(z64[:, :m])).to(eng.device)
    rec = torch.tensor([r for r, _ in items], dtype=torch.int64, device=eng.device)
    start = torch.tensor([s for _, s in items], dtype=torch.int64, device=eng.device)
    for mode in (PR.UNIT, PR.RAW):
        sizes = {"coherency": 2 * k * m * m, "mag": k * m * m, "lagged": k * m * m}
        bufs = {q: torch.full((G + sz + G,), float("nan"), dtype=torch.float64, device=eng.device) for q, sz in sizes.items()}
        info = torch.full((G + k + G,), -77, dtype=torch.int32, device=eng.device)
        with torch.cuda.device(eng.device):
            rc = eng.lib.hmv_phase_sync_c128(zd.data_ptr(), zd.stride(0), zd.stride(1), T1, 3, m, rec.data_ptr(), start.data_ptr(),
                                             k, n, mode, bufs["coherency"].data_ptr() + 8 * G, bufs["mag"].data_ptr() + 8 * G,
                                             bufs["lagged"].data_ptr() + 8 * G, info.data_ptr() + 4 * G, eng.stream())
        assert rc == 0
        ref = run(zd, items, n, mode)
        for q, sz in sizes.items():
            b = bufs[q].cpu().numpy()
            assert np.isnan(b[:G]).all() and np.isnan(b[G + sz:]).all(), q
            assert same_bits(b[G:G + sz], ref[q].reshape(-1)), q
        i = info.cpu().numpy()
        assert (i[:G] == -77).all() and (i[G + k:] == -77).all() and not i[G:G + k].any()


def test_info_non_finite_and_zero_power(z64):
    m, n = 17, 130
    z = z64[:, :m].copy()
    items = [(1, s) for s in range(0, T1 - n + 1, 97)] + [(0, 300), (2, 300)]
    clean = {mode: run(z, items, n, mode) for mode in (PR.UNIT, PR.RAW)}
    for bad in (np.nan, np.inf, complex(1.0, -np.inf)):
        zb = z.copy()
        zb[1, 9, 400] = bad
        hit = np.array([r == 1 and s <= 400 < s + n for r, s in items])
        assert 0 < hit.sum() < len(items)
        for mode in (PR.UNIT, PR.RAW):
            got = run(zb, items, n, mode)
            assert np.array_equal(got["info"], hit.astype(np.int32))
            for k in KEYS:
                assert np.isnan(got[k][hit]).all() and same_bits(got[k][~hit], clean[mode][k][~hit]), (k, bad)
    # a channel of zero power in some windows only
    zz = z.copy()
    zz[1, 4, 380:520] = 0.0
    dead = np.array([r == 1 and s >= 380 and s + n <= 520 for r, s in items])
    assert dead.sum() == 1
    u, r = run(zz, items, n, PR.UNIT), run(zz, items, n, PR.RAW)
    assert not u["info"].any() and np.array_equal(r["info"], 2 * dead.astype(np.int32))
    it = int(np.nonzero(dead)[0][0])
    assert not u["mag"][it][4].any() and not u["mag"][it][:, 4].any() and np.isfinite(u["mag"]).all()
    live = np.arange(m) != 4
    for k in ("mag", "lagged"):
        assert np.isnan(r[k][it][4]).all() and np.isnan(r[k][it][:, 4]).all() and np.isfinite(r[k][it][np.ix_(live, live)]).all()
        assert np.isfinite(r[k][~dead]).all()
    assert np.isnan(r["coherency"][it][:, 4]).all() and np.isnan(r["coherency"][it][:, :, 4]).all()
    want = PR.measures_restated(zz[1], items[it][1], n, PR.RAW)
    assert want["info"] == 2 and np.allclose(r["mag"][it][np.ix_(live, live)], want["mag"][np.ix_(live, live)], rtol=1e-12)


@pytest.mark.parametrize("T", (997, 1000, 4096, 30011))
def test_analytic_signal_against_extended_precision(T):
    """Per row, the relative L2 error of `Engine.analytic_signal` against the np.longdouble restatement is at most 4 x the
    error of the float64 NumPy restatement against the same (the factor allows rocFFT's different radix plan at the same
    log2 T growth).  Both printed.  A recording alone has the bits it has in a batch of three."""
    eng = default_engine()
    rng = np.random.default_rng(T)
    x = 50e-6 * rng.standard_normal((3, 4, T))
    resp = np.stack([band_response(T, 250.0, 8.0, 12.0), band_response(T, 250.0)])
    xd, rd = eng.to_device(x), eng.to_device(resp)
    z = eng.analytic_signal(xd, rd)
    assert z.shape == (3, 2, 4, T) and z.dtype == torch.complex128
    zn = z.cpu().numpy()
    for b in range(2):
        exact = PR.analytic_restated(x, resp[b], np.longdouble)
        f64 = PR.analytic_restated(x, resp[b], np.float64)
        norm = np.sqrt((np.abs(exact) ** 2).sum(-1))
        e_gpu = (np.sqrt((np.abs(zn[:, b] - exact) ** 2).sum(-1)) / norm).astype(np.float64)
        e_np = (np.sqrt((np.abs(f64 - exact) ** 2).sum(-1)) / norm).astype(np.float64)
        print(f"T={T} band {b}: relative L2 error gpu {e_gpu.max():.3g} (worst row ratio {float((e_gpu / e_np).max()):.3g}), "
              f"numpy float64 {e_np.max():.3g}")
        assert (e_gpu <= 4.0 * e_np).all(), (T, b, e_gpu, e_np)
    for k in range(3):
        assert same_bits(torch.view_as_real(eng.analytic_signal(xd[k], rd)).cpu().numpy(), torch.view_as_real(z[k]).cpu().numpy())
    one = eng.analytic_signal(xd[1], rd[0])
    assert one.shape == (4, T) and same_bits(torch.view_as_real(one).cpu().numpy(), torch.view_as_real(z[1, 0]).cpu().numpy())


@pytest.fixture(scope="module")
def dyads():
    return np.stack([PR.planted_dyad(0)[0], PR.planted_dyad(1)[0]])


@pytest.mark.parametrize("hop", (None, 500))
def test_public_call_is_the_composition(dyads, hop):
    """`sliding.sliding_phase_sync` equals, bit for bit, `Engine.phase_sync` on `Engine.analytic_signal`'s own output: two
    bands, the four measures, windows by count and by hop, one slab and several."""
    eng = default_engine()
    bands, measures = ((8.0, 12.0), (13.0, 30.0)), ("plv", "ciplv", "coh", "imcoh")
    n_rec, m, T = dyads.shape
    W = 2500
    pos = hop_positions(T, W, hop) if hop else window_positions(T, 6, W)[0]
    xd = eng.to_device(dyads)
    resp = torch.stack([eng.to_device(band_response(T, PR.FS, lo, hi)) for lo, hi in bands])
    z = eng.analytic_signal(xd, resp)
    rec, start = window_items(n_rec, pos, eng.device)
    want = {}
    for b in range(2):
        u = eng.phase_sync(z[:, b], rec, start, W, _lib.PHASE_UNIT)
        r = eng.phase_sync(z[:, b], rec, start, W, _lib.PHASE_RAW)
        for q, t in (("plv", u["mag"]), ("ciplv", u["lagged"]), ("coh", r["mag"]), ("imcoh", r["lagged"])):
            want.setdefault(q, []).append(t.view(n_rec, len(pos), m, m).cpu().numpy())
    want = {q: np.stack(v, axis=2) for q, v in want.items()}
    unit = 16 * m * T
    for ws in (8 << 30, 4 * unit, 3 * unit, 1):
        got = sliding_phase_sync(dyads, W, 6, PR.FS, bands, hop=hop, measures=measures, max_workspace_bytes=ws)
        assert sorted(got) == sorted(measures)
        for q in measures:
            assert got[q].shape == (n_rec, len(pos), 2, m, m) and same_bits(got[q], want[q]), (q, ws)
    single = sliding_phase_sync(dyads[1], W, 6, PR.FS, bands, hop=hop, measures=("ciplv",))
    assert sorted(single) == ["ciplv"] and same_bits(single["ciplv"], want["ciplv"][1])
    if hop:                                                         # the planted couplings, through the public call
        idx = [int(np.nonzero(np.asarray(pos) == s)[0][0]) for s in PR.STARTS]
        worst = max(PR.check_planted(want["plv"][0, i, 0], want["ciplv"][0, i, 0]) for i in idx)
        print(f"largest PLV outside the planted pairs: {worst:.3f}")


def test_check_names_the_window_or_returns_nans(dyads):
    x = dyads[:, :, :6000].copy()
    x[1, 3, 100] = np.nan                                           # the transform spreads it over recording 1
    with pytest.raises(ValueError, match=r"recording 1, window at sample 0 \(item 3\), band 0 .*info = 1"):
        sliding_phase_sync(x, 2500, 3, PR.FS, ((8.0, 12.0), (13.0, 30.0)), measures=("plv", "coh"))
    got = sliding_phase_sync(x, 2500, 3, PR.FS, ((8.0, 12.0), (13.0, 30.0)), measures=("plv", "coh"), check="nan")
    assert sorted(got) == ["coh", "info", "plv"] and got["info"].shape == (2, 3, 2)
    assert not got["info"][0].any() and (got["info"][1] == 1).all()
    assert np.isnan(got["plv"][1]).all() and np.isfinite(got["plv"][0]).all() and np.isfinite(got["coh"][0]).all()
    x[1, 3, 100] = 0.0
    x[0, 2, :] = 0.0                                                # zero power: PLV has nothing to refuse, coherence does
    assert np.isfinite(sliding_phase_sync(x, 2500, 3, PR.FS, ((8.0, 12.0),), measures=("plv", "ciplv"))["plv"]).all()
    with pytest.raises(ValueError, match=r"recording 0, window at sample 0 \(item 0\), band 0 .*info = 2"):
        sliding_phase_sync(x, 2500, 3, PR.FS, ((8.0, 12.0),), measures=("imcoh",))


from tests.test_gpu_escan_batch import _reader, tree  # noqa: E402,F401  (the small synthetic tree and its reader)


def test_escan_batch_phase_sync(tree, tmp_path):
    freqs = np.arange(1.0, 33.0, 1.0)
    kw = dict(window_s=2.0, overlap=0.5, model_order=3, freqs=freqs, low_cutoff_hz=1.0, high_cutoff_hz=45.0, reader=_reader,
              verbose=False, tasks=("talk",))
    res = EB.run(tree, tmp_path / "with", phase_sync=("plv", "ciplv"), **kw)
    base = EB.run(tree, tmp_path / "without", phase_sync=None, **kw)
    assert res["done"] == base["done"] == ["W_003", "W_010"]
    found = EB.discover_dyads(tree)
    for dy in res["done"]:
        z, z0 = np.load(tmp_path / "with" / f"{dy}_ffdtf.npz"), np.load(tmp_path / "without" / f"{dy}_ffdtf.npz")
        meta, meta0 = json.loads(str(z["meta"])), json.loads(str(z0["meta"]))
        assert meta["phase_sync"] == ["plv", "ciplv"] and "phase_sync" not in meta0
        assert not any("phase_" in k for k in z0.files)
        new = sorted(set(z.files) - set(z0.files))
        assert new == sorted(f"{s['task']}/{s['event']}/phase_{q}" for s in meta["segments"] for q in ("plv", "ciplv"))
        assert set(z0.files) <= set(z.files)
        for k in z0.files:
            if k != "meta":
                assert np.array_equal(z[k], z0[k], equal_nan=z[k].dtype.kind == "f"), k
        for seg in meta["segments"]:
            key = f"{seg['task']}/{seg['event']}"
            recs = {r: _reader(found[dy][seg["task"]][r]) for r in ("ch", "cg")}
            block, names, fs = EB.segment_block(recs["ch"], recs["cg"], seg["start_s"], seg["duration_s"], 1.0, 45.0)
            direct = sliding_phase_sync(block, seg["window"], 0, fs, hd.DEFAULT_BANDS, hop=seg["window"] // 2,
                                        measures=("plv", "ciplv"))
            for q in ("plv", "ciplv"):
                assert z[f"{key}/phase_{q}"].shape == (seg["windows"], len(hd.DEFAULT_BANDS), 16, 16)
                assert same_bits(z[f"{key}/phase_{q}"], direct[q]), (key, q)
