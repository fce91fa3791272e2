"""The phase-lag family on the GPU (csrc/phase_lag.hip through `Engine.phase_lag`, `Engine.sliding_phase_lag`,
`sliding.sliding_phase_lag` and `escan_batch.run(phase_lag=...)`): PLI bit-equal to the NumPy restatement, wpli and dwpli to
the derived bound of tests/phase_lag_restated.py, exact structure, bits that depend on the pair's samples only, nothing
written outside the outputs, `info`, and the composition end to end."""
import json

import numpy as np
import pytest
import torch

from tests import phase_lag_restated as LR
from tests import phase_sync_restated as PR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd.eeg_io import band_response
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions, sliding_phase_lag, window_items, window_positions

T1 = 1400
KEYS = LR.MEASURES


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def z64():
    """(3, 64, T1) complex128: the z of tests/test_gpu_phase_sync.py."""
    return LR.z64_recipe(T1)


@pytest.fixture(scope="module")
def restated(z64):
    """(n, item) -> the restatement and its bound on all 64 channels, made once: a cell's values depend on its two channels
    only, so the first m rows and columns serve every m."""
    out = {}
    for n in LR.N_CASES:
        for it, (r, s) in enumerate(LR.items_for(n, T1)):
            out[n, it] = (LR.measures_restated(z64[r], s, n), LR.lag_bound(z64[r], s, n), LR.sign_margin(z64[r], s, n))
    return out


def run(z, items, n, want=KEYS, split=0):
    eng = default_engine()
    zd = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z)).to(eng.device)
    rec = torch.tensor([r for r, _ in items], dtype=torch.int64, device=eng.device)
    start = torch.tensor([s for _, s in items], dtype=torch.int64, device=eng.device)
    res = eng.phase_lag(zd, rec, start, n, want=want, split=split)
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("m", (1, 2, 5, 16, 17, 33, 48, 64))
def test_kernel_against_the_restatement(z64, restated, m):
    """A NumPy-made z isolates the kernel from the FFT.  The input's sign margin is 0 (a condition on the input, asserted),
    so PLI is bit-equal; wpli and dwpli lie within `lag_bound` on every off-diagonal pair (worst ratio printed; on the
    MI355X 0.034 for wpli and 0.049 for dwpli at 64 channels), NaN exactly where the restatement has NaN (dwpli at n = 1)."""
    z = z64[:, :m]
    worst = {"wpli": 0.0, "dwpli": 0.0}
    off = ~np.eye(m, dtype=bool)
    for n in LR.N_CASES:
        items = LR.items_for(n, T1)
        got = run(z, items, n)
        assert not got["info"].any()
        for it in range(len(items)):
            want, bound, doubt = restated[n, it]
            assert doubt == 0 and want["info"] == 0
            assert same_bits(got["pli"][it], np.ascontiguousarray(want["pli"][:m, :m])), (m, n, it)
            for k in ("wpli", "dwpli"):
                g, w, b = got[k][it], want[k][:m, :m], bound[k][:m, :m]
                assert not g.diagonal().any()
                assert np.array_equal(np.isnan(g), np.isnan(w)), (k, m, n, it)
                if n == 1:
                    assert k == "wpli" or np.isnan(g[off]).all()
                sel = off & np.isfinite(w)
                if sel.any():
                    assert (b[sel] > 0).all()
                    ratio = float((np.abs(g - w)[sel] / b[sel]).max())
                    worst[k] = max(worst[k], ratio)
                    assert ratio <= 1.0, (k, m, n, it, ratio)
    print(f"m={m}: pli bit-equal; worst |gpu - restated| / lag_bound = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("m,n", ((33, 130), (64, 67), (5, 3)))
def test_exact_structure(z64, m, n):
    z = z64[:, :m]
    items = LR.items_for(n, T1)
    base = run(z, items, n)
    assert not base["info"].any()
    off = ~np.eye(m, dtype=bool)
    for k in KEYS:
        for it in range(len(items)):
            a = base[k][it]
            assert same_bits(a, a.T) and not a.diagonal().any() and np.isfinite(a).all(), (k, it)
        if k != "dwpli":
            assert (base[k] >= 0.0).all() and (base[k] <= 1.0).all(), k                  # no slack
    assert (base["dwpli"][:, off] <= 1.0).all()
    one = run(z, LR.items_for(1, T1), 1)
    assert np.isnan(one["dwpli"][:, off]).all() and not one["dwpli"][:, ~off].any()
    assert (one["wpli"][:, off] == 1.0).all() and (one["pli"][:, off] == 1.0).all() and not one["info"].any()
    zs = z.copy()                                                   # a power of two on two channels changes no bit
    zs[:, 0] *= 2.0 ** 7
    zs[:, m // 2] *= 2.0 ** -9
    scaled = run(zs, items, n)
    for k in KEYS:
        assert same_bits(base[k], scaled[k]), k
    assert np.array_equal(base["info"], scaled["info"])


def test_bits_depend_on_the_pairs_samples_only(z64):
    eng = default_engine()
    n = 65
    rng = np.random.default_rng(3)
    items = [(int(r), int(s)) for r, s in zip(rng.integers(0, 3, 23), rng.integers(0, T1 - n + 1, 23))]
    items[5] = (2, T1 - n)
    full = run(z64, items, n)
    again = run(z64, items, n)
    for k in KEYS:
        assert same_bits(full[k], again[k])                                    # run to run
    for it in (0, 5, 22):                                                      # a batch against its items one by one
        alone = run(z64, [items[it]], n)
        for k in KEYS:
            assert same_bits(alone[k][0], full[k][it]), (k, it)
    perm = rng.permutation(23)
    shuffled = run(z64, [items[i] for i in perm], n)
    for k in KEYS:
        assert same_bits(shuffled[k], full[k][perm]), k
    # m = 64 against the same channels as an m = 17 call (another NT, other threads), read in place and alone
    zd = torch.from_numpy(np.ascontiguousarray(z64)).to(eng.device)
    inside, alone17 = run(zd[:, :17], items, n), run(z64[:, :17], items, n)
    assert zd[:, :17].stride(0) == 64 * T1
    for k in KEYS:
        assert same_bits(inside[k], alone17[k]) and same_bits(full[k][:, :17, :17], inside[k]), k
    # one output alone has the bits it has among the three
    for k in KEYS:
        only = run(z64, items, n, want=(k,))
        assert sorted(only) == sorted((k, "info")) and same_bits(only[k], full[k]), k
    # split: the cross cells keep the bits of the split = 0 call, the other off-diagonal cells are NaN, the diagonal 0
    for split in (1, 16, 17, 32, 63):
        got = run(z64, items, n, split=split)
        done = LR.computed_pairs(64, split)
        off = ~np.eye(64, dtype=bool)
        assert not got["info"].any()
        for k in KEYS:
            assert same_bits(got[k][:, done], full[k][:, done]), (k, split)
            assert np.isnan(got[k][:, off & ~done]).all() and not got[k][:, ~off].any(), (k, split)
    for m, split in ((17, 16), (5, 2), (48, 31)):
        got = run(z64[:, :m], items, n, split=split)
        done = LR.computed_pairs(m, split)
        for k in KEYS:
            assert same_bits(got[k][:, done], full[k][:, :m, :m][:, done]), (k, m, split)
            assert np.isnan(got[k][:, ~np.eye(m, dtype=bool) & ~done]).all(), (k, m, split)


def test_nothing_is_written_outside_the_outputs(z64):
    eng = default_engine()
    m, n, G = 33, 64, 512
    items = LR.items_for(n, T1)
    k = len(items)
    zd = torch.from_numpy(np.ascontiguousarray(z64[:, :m])).to(eng.device)
    rec = torch.tensor([r for r, _ in items], dtype=torch.int64, device=eng.device)
    start = torch.tensor([s for _, s in items], dtype=torch.int64, device=eng.device)
    ref = run(zd, items, n)
    sz = k * m * m
    for absent in (None,) + KEYS:                                   # all three, then each one NULL in turn
        bufs = {q: torch.full((G + sz + G,), -7.5, dtype=torch.float64, device=eng.device) for q in KEYS}
        info = torch.full((G + k + G,), -77, dtype=torch.int32, device=eng.device)
        ptr = {q: (0 if q == absent else bufs[q].data_ptr() + 8 * G) for q in KEYS}
        with torch.cuda.device(eng.device):
            rc = eng.lib.hmv_phase_lag_c128(zd.data_ptr(), zd.stride(0), zd.stride(1), T1, 3, m, 0, rec.data_ptr(),
                                            start.data_ptr(), k, n, ptr["pli"] or None, ptr["wpli"] or None,
                                            ptr["dwpli"] or None, info.data_ptr() + 4 * G, eng.stream())
        assert rc == 0
        for q in KEYS:
            b = bufs[q].cpu().numpy()
            assert (b[:G] == -7.5).all() and (b[G + sz:] == -7.5).all(), (q, absent)
            if q == absent:
                assert (b == -7.5).all(), q                          # a NULL output's neighbour in memory is not touched
            else:
                assert same_bits(b[G:G + sz], ref[q].reshape(-1)), (q, absent)
        i = info.cpu().numpy()
        assert (i[:G] == -77).all() and (i[G + k:] == -77).all() and not i[G:G + k].any()


def test_info_non_finite_flat_and_duplicated(z64):
    m, n = 17, 130
    z = z64[:, :m].copy()
    items = [(1, s) for s in range(0, T1 - n + 1, 97)] + [(0, 300), (2, 300)]
    clean = run(z, items, n)
    assert not clean["info"].any()
    for bad in (np.nan, np.inf, complex(1.0, -np.inf)):
        zb = z.copy()
        zb[1, 9, 400] = bad
        hit = np.array([r == 1 and s <= 400 < s + n for r, s in items])
        assert 0 < hit.sum() < len(items)
        for split in (0, 5, 12):                                     # channel 9 on either side of the split
            got = run(zb, items, n, split=split)
            assert np.array_equal(got["info"], hit.astype(np.int32))
            ref = clean if split == 0 else run(z, items, n, split=split)
            for k in KEYS:
                assert np.isnan(got[k][hit]).all() and same_bits(got[k][~hit], ref[k][~hit]), (k, bad, split)
    # a zeroed channel in one window, a duplicated (and power-of-two scaled) channel in recording 2
    zz = z.copy()
    zz[1, 4, 380:520] = 0.0
    zz[2, 11] = -0.25 * zz[2, 3]
    flat = np.array([r == 1 and s >= 380 and s + n <= 520 for r, s in items])
    dup = np.array([r == 2 for r, _ in items])
    assert flat.sum() == 1 and dup.sum() == 1
    got = run(zz, items, n)
    assert np.array_equal(got["info"], 2 * (flat | dup).astype(np.int32))
    cells = np.zeros((len(items), m, m), dtype=bool)
    cells[flat, 4, :] = cells[flat, :, 4] = True
    cells[dup, 3, 11] = cells[dup, 11, 3] = True
    cells[:, np.arange(m), np.arange(m)] = False
    assert not got["pli"][cells].any() and np.isnan(got["wpli"][cells]).all() and np.isnan(got["dwpli"][cells]).all()
    touched = np.zeros_like(cells)                                   # cells whose samples changed
    partly = np.array([r == 1 and s < 520 and s + n > 380 for r, s in items])     # channel 4 zeroed in part of the window
    assert partly.sum() == 3 and not got["info"][partly & ~flat].any()
    touched[partly, 4, :] = touched[partly, :, 4] = True
    touched[dup, 11, :] = touched[dup, :, 11] = True
    for k in KEYS:
        assert np.isfinite(got[k][~cells]).all() and same_bits(got[k][~touched], clean[k][~touched]), k
    it = int(np.nonzero(dup)[0][0])
    want = LR.measures_restated(zz[2], items[it][1], n)
    assert want["info"] == 2 and same_bits(got["pli"][it], want["pli"])
    # with a split that leaves the duplicated pair on one side, the item is clean
    assert run(zz, items, n, split=12)["info"][it] == 0 and run(zz, items, n, split=4)["info"][it] == 2


@pytest.fixture(scope="module")
def dyads():
    return np.stack([PR.planted_dyad(0)[0], PR.planted_dyad(1)[0]])


@pytest.mark.parametrize("hop", (None, 500))
def test_public_call_is_the_composition(dyads, hop):
    """`sliding.sliding_phase_lag` equals, bit for bit, `Engine.phase_lag` on `Engine.analytic_signal`'s own output: two
    bands, the three measures, windows by count and by hop, one slab and several, with and without a split; the driver fed
    with both families gives each the bits of its own call."""
    eng = default_engine()
    bands = ((8.0, 12.0), (13.0, 30.0))
    n_rec, m, T = dyads.shape
    W = 2500
    pos = hop_positions(T, W, hop) if hop else window_positions(T, 6, W)[0]
    xd = eng.to_device(dyads)
    resp = torch.stack([eng.to_device(band_response(T, PR.FS, lo, hi)) for lo, hi in bands])
    z = eng.analytic_signal(xd, resp)
    rec, start = window_items(n_rec, pos, eng.device)
    for split in (0, 4):
        want = {}
        for b in range(2):
            r = eng.phase_lag(z[:, b], rec, start, W, want=KEYS, split=split)
            for q in KEYS:
                want.setdefault(q, []).append(r[q].view(n_rec, len(pos), m, m).cpu().numpy())
        want = {q: np.stack(v, axis=2) for q, v in want.items()}
        unit = 16 * m * T
        for ws in (8 << 30, 3 * unit, 1):
            got = sliding_phase_lag(dyads, W, 6, PR.FS, bands, hop=hop, measures=KEYS, split=split, max_workspace_bytes=ws)
            assert sorted(got) == sorted(KEYS)
            for q in KEYS:
                assert got[q].shape == (n_rec, len(pos), 2, m, m) and same_bits(got[q], want[q]), (q, ws, split)
    single = sliding_phase_lag(dyads[1], W, 6, PR.FS, bands, hop=hop, split=4)
    assert sorted(single) == ["wpli"] and same_bits(single["wpli"], want["wpli"][1])
    # the combined driver: one analytic signal for both families, each with the bits of its own call
    sync_q, lag_q = ("plv", "imcoh"), ("pli", "wpli", "dwpli")
    for ws in (8 << 30, 3 * 16 * m * T):
        both = eng.sliding_phase("both", xd, rec, start, W, PR.FS, bands, sync=sync_q, lag=lag_q, split=4, max_workspace_bytes=ws)
        s_alone = eng.sliding_phase_sync(xd, rec, start, W, PR.FS, bands, measures=sync_q)
        l_alone = eng.sliding_phase_lag(xd, rec, start, W, PR.FS, bands, measures=lag_q, split=4)
        for got, alone, qs in ((both[0], s_alone, sync_q), (both[1], l_alone, lag_q)):
            assert sorted(got) == sorted(qs + ("info",))
            for q in qs:
                assert same_bits(got[q].cpu().numpy(), alone[q].cpu().numpy()), q
            assert np.array_equal(got["info"].cpu().numpy(), alone["info"].cpu().numpy())
    if hop:                                                         # the planted couplings, through the public call
        idx = [int(np.nonzero(np.asarray(pos) == s)[0][0]) for s in PR.STARTS]
        full = sliding_phase_lag(dyads[0], W, 6, PR.FS, (PR.BAND,), hop=hop, measures=KEYS)
        for q in KEYS:
            assert (full[q][idx, 0, 0, 5] > 0.95).all(), q
        med = [float(np.median(full[q][idx, 0, 2, 6])) for q in ("pli", "wpli")]
        print(f"planted dyad through the public call: (2, 6) median pli {med[0]:.3f} wpli {med[1]:.3f}")
        assert med[0] < 0.25 and med[1] < 0.40


def test_check_names_the_window_or_returns_nans(dyads):
    x = dyads[:, :, :6000].copy()
    x[1, 3, 100] = np.nan                                           # the transform spreads it over recording 1
    bands = ((8.0, 12.0), (13.0, 30.0))
    with pytest.raises(ValueError, match=r"sliding_phase_lag: recording 1, window at sample 0 \(item 3\), band 0 .*info = 1"):
        sliding_phase_lag(x, 2500, 3, PR.FS, bands, measures=("pli", "wpli"))
    got = sliding_phase_lag(x, 2500, 3, PR.FS, bands, measures=("pli", "wpli"), check="nan")
    assert sorted(got) == ["info", "pli", "wpli"] and got["info"].shape == (2, 3, 2)
    assert not got["info"][0].any() and (got["info"][1] == 1).all()
    assert np.isnan(got["wpli"][1]).all() and np.isfinite(got["wpli"][0]).all() and np.isfinite(got["pli"][0]).all()
    x[1, 3, 100] = 0.0
    x[0, 2, :] = 0.0                                                # a flat channel: its analytic signal is zero
    with pytest.raises(ValueError, match=r"sliding_phase_lag: recording 0, window at sample 0 \(item 0\), band 0 .*info = 2"):
        sliding_phase_lag(x, 2500, 3, PR.FS, bands)
    got = sliding_phase_lag(x, 2500, 3, PR.FS, bands, measures=("pli", "wpli"), check="nan")
    assert (got["info"][0] == 2).all() and not got["info"][1].any()
    live = np.arange(8) != 2
    assert not got["pli"][0][..., 2, :].any() and np.isnan(got["wpli"][0][..., 2, live]).all()
    assert np.isnan(got["wpli"][0][..., live, 2]).all() and not got["wpli"][0][..., 2, 2].any()
    assert np.isfinite(got["wpli"][0][..., live, :][..., live]).all() and np.isfinite(got["wpli"][1]).all()

from tests.test_gpu_escan_batch import _reader, tree  # noqa: E402,F401  (the small synthetic tree and its reader)


def test_escan_batch_phase_lag(tree, tmp_path):
    freqs = np.arange(1.0, 33.0, 1.0)
    kw = dict(window_s=2.0, overlap=0.5, model_order=3, freqs=freqs, low_cutoff_hz=1.0, high_cutoff_hz=45.0, reader=_reader,
              verbose=False, tasks=("talk",))
    res = EB.run(tree, tmp_path / "with", phase_lag=("pli", "wpli"), **kw)
    base = EB.run(tree, tmp_path / "without", **kw)
    both = EB.run(tree, tmp_path / "both", phase_lag=("wpli",), phase_sync=("plv",), **kw)
    sync = EB.run(tree, tmp_path / "sync", phase_sync=("plv",), **kw)
    assert res["done"] == base["done"] == both["done"] == sync["done"] == ["W_003", "W_010"]
    found = EB.discover_dyads(tree)
    for dy in res["done"]:
        z, z0 = np.load(tmp_path / "with" / f"{dy}_ffdtf.npz"), np.load(tmp_path / "without" / f"{dy}_ffdtf.npz")
        zb, zs = np.load(tmp_path / "both" / f"{dy}_ffdtf.npz"), np.load(tmp_path / "sync" / f"{dy}_ffdtf.npz")
        meta, meta0, metab = (json.loads(str(f["meta"])) for f in (z, z0, zb))
        assert meta["phase_lag"] == ["pli", "wpli"] and "phase_lag" not in meta0 and "phase_sync" not in meta
        assert metab["phase_lag"] == ["wpli"] and metab["phase_sync"] == ["plv"]
        assert not any("phase_" in k for k in z0.files)
        new = sorted(set(z.files) - set(z0.files))
        assert new == sorted(f"{s['task']}/{s['event']}/phase_{q}" for s in meta["segments"] for q in ("pli", "wpli"))
        assert set(z0.files) <= set(z.files)
        for k in z0.files:                                          # what was written before is written as before
            if k != "meta":
                assert np.array_equal(z[k], z0[k], equal_nan=z[k].dtype.kind == "f"), k
        for seg in meta["segments"]:
            key = f"{seg['task']}/{seg['event']}"
            recs = {r: _reader(found[dy][seg["task"]][r]) for r in ("ch", "cg")}
            block, names, fs = EB.segment_block(recs["ch"], recs["cg"], seg["start_s"], seg["duration_s"], 1.0, 45.0)
            direct = sliding_phase_lag(block, seg["window"], 0, fs, hd.DEFAULT_BANDS, hop=seg["window"] // 2,
                                       measures=("pli", "wpli"))
            for q in ("pli", "wpli"):
                assert z[f"{key}/phase_{q}"].shape == (seg["windows"], len(hd.DEFAULT_BANDS), 16, 16)
                assert same_bits(z[f"{key}/phase_{q}"], direct[q]), (key, q)
            # both families in one run: each dataset has the bits of the run that asked for it alone
            assert same_bits(zb[f"{key}/phase_wpli"], z[f"{key}/phase_wpli"])
            assert same_bits(zb[f"{key}/phase_plv"], zs[f"{key}/phase_plv"])
