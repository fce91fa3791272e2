"""FIR decimation on the GPU (csrc/decimate.hip through `Engine.decimate`): parity with SciPy's two decimators to the
derived bound of tests/decimate_restated.py, tile seams, bit-identity across batch / strides / segments, nothing written
outside the output, the reach of a NaN, and the regime it exists for end to end (`sliding_ffdtf`, `escan_batch.run`)."""
import json

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O
from tests import decimate_restated as DR
from tests import scale_shapes as SS

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd.eeg_io import decimation_taps
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import decimate, hop_positions, regular_grid, sliding_ffdtf, window_items
    from hyperscanning_signal_analysis_amd.synthetic import band_limited_dyad

EPS = np.finfo(np.float64).eps


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def dec(x, q, design="decimate", **kw):
    eng = default_engine()
    return eng.decimate(eng.to_device(x), q, design, **kw).cpu().numpy()


@pytest.mark.parametrize("q", (2, 3, 4, 5, 8, 13, 32))
def test_parity_with_scipy(q):
    """`scipy.signal.decimate(ftype='fir', zero_phase=True)` and `resample_poly(x, 1, q)` at physical-unit amplitude.  Two
    summations of the same n_taps products in different orders differ per output by at most
    2 n_taps 2^-52 sum_j |h_j| |x_{kq+H-j}| (decimate_restated.rounding_bound), computed here from the inputs."""
    from scipy.signal import decimate as sp_decimate
    from scipy.signal import resample_poly
    rng = np.random.default_rng(7 + q)
    worst = 0.0
    for T in (1, 7, 39, 40, 41, 1000, 1003):
        x = 50e-6 * rng.standard_normal((2, 3, T))
        for design, want in (("decimate", sp_decimate(x, q, ftype="fir", zero_phase=True, axis=-1)),
                             ("resample_poly", resample_poly(x, 1, q, axis=-1))):
            got = dec(x, q, design)
            assert got.shape == want.shape == (2, 3, -(-T // q))
            r = DR.worst_ratio(got, want, DR.rounding_bound(x, q, decimation_taps(q, design)))
            worst = max(worst, r)
            assert r <= 1.0, (design, T, q, r)
    print(f"q={q}: worst |gpu - scipy| / bound = {worst:.3g}")


@pytest.mark.parametrize("T,q", ((20011, 2), (20011, 5), (30011, 16), (26003, 32)))
def test_tile_seams(T, q):
    """One row over more than three output tiles and a ragged last one (1024, 1024, 512 and 256 outputs per workgroup at
    these factors), against the restatement to the same bound; a second, 2-D call checks the (m, T) form."""
    h = decimation_taps(q)
    tile = _lib.load().hmv_decimate_tile(q, len(h))
    T_out = -(-T // q)
    assert tile in (256, 512, 1024) and T_out > 3 * tile and T_out % tile != 0
    x = 50e-6 * np.random.default_rng(T + q).standard_normal((1, T))
    got = dec(x, q)
    assert got.shape == (1, T_out)
    r = DR.worst_ratio(got, DR.decimate_restated(x, q, h), DR.rounding_bound(x, q, h))
    print(f"T={T} q={q} tile={tile}: worst |gpu - restated| / bound = {r:.3g}")
    assert r <= 1.0


@pytest.mark.parametrize("q", (3, 4))
def test_bit_identity_across_batch_strides_and_segments(q):
    eng = default_engine()
    rng = np.random.default_rng(40 + q)
    n_rec, m, T = 3, 5, 2731
    x = rng.standard_normal((n_rec, m, T))
    full = dec(x, q)
    # a row alone, and a single recording as (m, T), have the bits they have inside the batch
    assert np.array_equal(bits(dec(x[1:2, 3:4], q)), bits(full[1:2, 3:4]))
    assert np.array_equal(bits(dec(x[2], q)), bits(full[2]))
    # ld > T and a padded recording stride
    big = torch.full((n_rec, m + 2, T + 37), float("nan"), dtype=torch.float64, device=eng.device)
    view = big[:, 1:m + 1, 5:5 + T]
    view.copy_(eng.to_device(x))
    assert view.stride() == ((m + 2) * (T + 37), T + 37, 1)
    assert np.array_equal(bits(eng.decimate(view, q).cpu().numpy()), bits(full))
    # a segment [a, b) with a a multiple of q equals the slice of the full decimation wherever the taps stay inside it
    H = (len(decimation_taps(q)) - 1) // 2
    a, b = 4 * q, T - 3
    seg = eng.decimate(eng.to_device(x)[..., a:b], q).cpu().numpy()
    k = np.arange(seg.shape[-1])
    inside = (k * q - H >= 0) & (a + k * q + H <= b - 1)
    assert inside.sum() > 100 and not inside[0] and not inside[-1]
    assert np.array_equal(bits(seg[..., inside]), bits(full[..., a // q + k[inside]]))
    # the other design and explicit taps go the same way
    h = decimation_taps(q, "resample_poly")
    assert np.array_equal(bits(dec(x, q, "resample_poly")), bits(dec(x, q, h)))
    assert not np.array_equal(dec(x, q, "resample_poly"), full)


def test_nothing_is_written_outside_the_output():
    eng = default_engine()
    q, G = 4, 19
    n_rec, m, T = 2, 3, 4099                                     # 1025 outputs: one full tile and one output more
    T_out = -(-T // q)
    x = np.random.default_rng(3).standard_normal((n_rec, m, T))
    sentinel = -7.25
    big = torch.full((n_rec + 1, m + 1, G + T_out + G), sentinel, dtype=torch.float64, device=eng.device)
    out = big[:n_rec, :m, G:G + T_out]
    res = eng.decimate(eng.to_device(x), q, out=out)
    assert res.data_ptr() == out.data_ptr()
    host = big.cpu().numpy()
    assert np.array_equal(bits(host[:n_rec, :m, G:G + T_out]), bits(dec(x, q)))
    host[:n_rec, :m, G:G + T_out] = sentinel
    assert (host == sentinel).all()
    with pytest.raises(ValueError, match="out must be"):
        eng.decimate(eng.to_device(x), q, out=big[:n_rec, :m, :T_out - 1])


@pytest.mark.parametrize("q,s", ((4, 0), (4, 1501), (4, 2999), (5, 1234), (2, 777)))
def test_nan_reach(q, s):
    """One NaN at sample s: exactly the outputs with |k q - s| <= H are NaN, every other output keeps its bits."""
    T = 3000
    x = np.random.default_rng(q + s).standard_normal((2, 2, T))
    clean = dec(x, q)
    x[1, 0, s] = np.nan
    dirty = dec(x, q)
    H = (len(decimation_taps(q)) - 1) // 2
    k = np.arange(clean.shape[-1])
    hit = np.zeros(clean.shape, dtype=bool)
    hit[1, 0] = np.abs(k * q - s) <= H
    assert hit.sum() >= H // q
    assert np.array_equal(np.isnan(dirty), hit)
    assert np.array_equal(bits(dirty[~hit]), bits(clean[~hit]))


def test_end_to_end_on_low_passed_recordings():
    """The regime this exists for: a 30 Hz low-passed recording at 500 Hz, order 8.  At the full rate the normal equations
    of a 2 s window are beyond cond 1e13; decimated by 4 they are below 1e7, and the ffDTF of the device-decimated
    recording agrees with the oracle on SciPy's decimation to the suite's contract 1e2 cond eps."""
    from scipy.signal import decimate as sp_decimate
    p, q, W = 8, 4, 250
    x = band_limited_dyad(3, 8, 8000, 500.0, 30.0, 8)
    y, fs = decimate(x, 500.0, q)
    assert fs == 125.0 and y.shape == (8, 2000) and isinstance(y, np.ndarray)
    y_ref = sp_decimate(x, q, ftype="fir", zero_phase=True, axis=-1)
    h = decimation_taps(q)
    assert DR.worst_ratio(y, y_ref, DR.rounding_bound(x, q, h)) <= 1.0
    cond_full = SS.normal_matrix_cond(O, x[:, :4 * W], p)
    conds = [SS.normal_matrix_cond(O, y_ref[:, s:s + W], p) for s in range(0, 2000, W)]
    print(f"cond of the normal equations: full rate {cond_full:.3g}, decimated {min(conds):.3g} .. {max(conds):.3g}")
    assert cond_full > 1e13 and max(conds) < 1e7
    freqs = np.arange(1.0, 33.0)
    got = sliding_ffdtf(y, W, 8, p, freqs, fs)
    want = O.sliding_ffdtf(y_ref, W, 8, p, freqs, fs)
    assert got.shape == want.shape == (8, 8, 8, 32)
    for w in range(8):
        err = np.abs(got[w] - want[w]).max() / np.abs(want[w]).max()
        print(f"window {w}: cond {conds[w]:.3g}, rel err {err:.3g}, tolerance {1e2 * conds[w] * EPS:.3g}")
        assert err <= 1e2 * conds[w] * EPS, (w, err, conds[w])


# ---- escan_batch.run(decimate=4): a one-dyad tree with an injected reader, as tests/test_gpu_escan_batch.py builds one
FS = 256.0
CHANS = ["Fp1", "Fp2", "F3", "M1", "C3", "C4", "M2", "O1", "O2", "Pz"]          # two mastoids to be dropped: 8 + 8 channels


def _write(path, seed, dur_s, events):
    rng = np.random.default_rng(seed)
    n = int(dur_s * FS)
    t = np.arange(n) / FS - 2.0
    x = rng.standard_normal((n, len(CHANS)))
    x[1:] += 0.6 * x[:-1]
    x[:, 1:] += 0.3 * x[:, :-1]
    ev = [{"name": nm, "start_s": 100.0 + st, "start_rel_s": st, "duration_s": du} for nm, st, du in events]
    attrs = {"sampling_freq": FS, "task_events_structure": json.dumps(ev)}
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, data=x, time=t, channels=np.asarray(CHANS), attrs=json.dumps(attrs))


def _reader(path):
    with np.load(path, allow_pickle=False) as z:
        return {"data_tc": z["data"], "time": z["time"], "channels": [str(c) for c in z["channels"]],
                "attrs": json.loads(str(z["attrs"]))}


def test_escan_batch_decimate(tmp_path):
    root = tmp_path / "tree"
    for r, (code, role) in enumerate((("ch", "child"), ("cg", "caregiver"))):
        _write(root / "EEG" / "W_003" / role / f"W_003_EEG_{code}_talk.nc", 50 + r, 20.0, [("talk_1", 0.5, 9.3), ("talk_2", 10.0, 7.0)])
    q, order = 4, 3
    freqs = np.arange(1.0, 33.0) * 0.9                           # 32 points below the new Nyquist rate of 32 Hz
    kw = dict(window_s=2.0, overlap=0.5, model_order=order, freqs=freqs, low_cutoff_hz=1.0, high_cutoff_hz=20.0,
              reader=_reader, verbose=False)
    res = EB.run(root, tmp_path / "dec", decimate=q, **kw)
    assert res["done"] == ["W_003"] and not res["failed"]
    z = np.load(tmp_path / "dec" / "W_003_ffdtf.npz", allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    assert meta["decimate"] == q and meta["decimate_design"] == "decimate" and meta["fs"] == FS / q
    assert [s["event"] for s in meta["segments"]] == ["talk_1", "talk_2"] and not meta["failed_segments"]
    eng = default_engine()
    recs = {r: _reader(root / "EEG" / "W_003" / role / f"W_003_EEG_{r}_talk.nc") for r, role in (("ch", "child"), ("cg", "caregiver"))}
    lo, hi = hd.band_bins(freqs)
    W = 128
    for seg in meta["segments"]:
        key = f"{seg['task']}/{seg['event']}"
        block, names, fs = EB.segment_block(recs["ch"], recs["cg"], seg["start_s"], seg["duration_s"], 1.0, 20.0)
        assert fs == FS and block.shape[0] == 16
        T_dec = -(-block.shape[1] // q)
        assert seg["fs"] == FS / q and seg["samples"] == T_dec and seg["window"] == W
        starts = z[f"{key}/starts"]
        assert starts.tolist() == list(range(0, 64 * len(starts), 64)) and len(starts) == (T_dec - W) // 64 + 1 == seg["windows"]
        assert 0 <= T_dec - (starts[-1] + W) < 64
        # the manual route: Engine.decimate, then the band-summed ffDTF of the same positions
        xd = eng.decimate(eng.to_device(block[None]), q)
        pos = hop_positions(T_dec, W, 64)
        rec_i, st_i = window_items(1, pos, eng.device)
        manual, bad = eng.sliding_ffdtf(xd, rec_i, st_i, W, order, freqs, FS / q, check="mask", grid=regular_grid(pos, W, order),
                                        bands=(lo, hi))
        assert not bool(bad.any())
        got = z[f"{key}/ffdtf_bands"]
        assert got.shape == (len(starts), 16, 16, len(lo)) and np.isfinite(got).all()
        assert np.array_equal(bits(got), bits(manual.cpu().numpy()))
    assert set(z.files) == {"channels", "freqs", "bands", "meta"} | {f"talk/{e}/{k}" for e in ("talk_1", "talk_2")
                                                                      for k in ("ffdtf_bands", "starts")}
    # the checks of the arguments are raised, not logged per segment or per dyad
    with pytest.raises(ValueError, match="Nyquist"):
        EB.run(root, tmp_path / "bad1", decimate=q, **dict(kw, freqs=np.arange(1.0, 40.0)))
    with pytest.raises(ValueError, match="rank"):
        EB.run(root, tmp_path / "bad2", decimate=q, **dict(kw, model_order=8))
    # decimate=None: the file of a run without the argument, array by array and key by key
    EB.run(root, tmp_path / "none", decimate=None, **kw)
    EB.run(root, tmp_path / "plain", **kw)
    a = np.load(tmp_path / "none" / "W_003_ffdtf.npz", allow_pickle=False)
    b = np.load(tmp_path / "plain" / "W_003_ffdtf.npz", allow_pickle=False)
    assert a.files == b.files
    for name in a.files:
        if name == "meta":
            ma, mb = json.loads(str(a[name])), json.loads(str(b[name]))
            ma.pop("created"), mb.pop("created")
            assert ma == mb and "decimate" not in ma and "fs" not in ma
        else:
            assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape
            assert a[name].tobytes() == b[name].tobytes(), name
