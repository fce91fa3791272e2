"""K2's pivoted fallback on the GPU (csrc/yw_lu.hip; HMV_FLAG_YW_PIVOTED, HMV_TUNE_YW_FORM = 5, Engine(pivoted_yw=True)).

Windows that the recursion and the unpivoted LDL^T refuse are solved by a dense LU with partial pivoting, as the
reference's `np.linalg.solve` does.  Where the conditioning leaves an answer, the LU is held to the project's contract,
1e2 cond eps against the oracle.  Where it does not (cond >~ 1e15: two valid LU row orders differ by O(1) in the
coefficients), it is held to what an LU promises: the normwise backward error eta = ||B - G X||_F / (||G||_F ||X||_F +
||B||_F) on the real channels, on the system built from the GPU's own R, with
  * eta_gpu <= N eps, the textbook bound, and
  * eta_gpu <= c eta_numpy with c = 4 x 0.992 = 3.97: 0.992 is the largest eta_restated / eta_numpy that the NumPy
    restatement of the kernel (tests/yw_lu_restated.py, printed by tests/test_yw_pivoted_cpu.py) reaches over these same
    windows -- the restatement and the kernel differ only in the order of accumulation inside a step, so the ratio
    measures exactly that; over the 48 windows it printed 0.35 .. 0.99 (eta_numpy 0.12 .. 0.38 eps).
All @pytest.mark.gpu."""
import functools
import json

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O
from tests import yw_lu_restated as Y

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    from hyperscanning_signal_analysis_amd import sliding
    from hyperscanning_signal_analysis_amd.engine import Engine, SingularMatrixError, default_engine
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

EPS = Y.EPS
C_RATIO = 4.0 * 0.992
POWERS = (-20, -12, 12, 20)


@functools.lru_cache(maxsize=None)
def pivoted_engine():
    return Engine(pivoted_yw=True)


class lu_alone:
    """`with lu_alone(eng):` -- HMV_TUNE_YW_FORM = 5 for the block, the default behind it."""
    def __init__(self, eng):
        self.lib = eng.lib

    def __enter__(self):
        assert self.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 5) == 0

    def __exit__(self, *exc):
        assert self.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 0) == 0


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _items(eng, W):
    return (torch.arange(W, dtype=torch.int64, device=eng.device), torch.zeros(W, dtype=torch.int64, device=eng.device))


def _lagcov(eng, batch, p):
    rec, st = _items(eng, batch.shape[0])
    return eng.lagcov(eng.to_device(batch), rec, st, batch.shape[2], p)


# ------------------------------------------------------------------------------ 1. the LU alone, well conditioned
def _ordinary(m, p, n, W=6):
    rng = np.random.default_rng(100 * m + p)
    x = rng.standard_normal((W, m, n))
    x[:, :, 1:] += 0.6 * x[:, :, :-1]
    return x


@pytest.mark.parametrize("m,p,n", [(4, 3, 200), (16, 1, 200), (19, 6, 700), (33, 5, 900), (48, 4, 900), (64, 2, 700),
                                   (64, 8, 1500), (17, 20, 1500), (5, 32, 800)])
def test_lu_alone_on_well_conditioned_windows(m, p, n):
    eng = default_engine()
    x = _ordinary(m, p, n)
    R = _lagcov(eng, x, p)
    with lu_alone(eng):
        ar, V, _, info, route = eng.yw_solve(R, m, return_route=True)
        ar1, V1, _, info1 = eng.yw_solve(R[2:3].contiguous(), m)
        torch.cuda.synchronize()
    assert not bool(info.any()) and bool((route == 2).all()) and int(info1[0]) == 0
    assert torch.equal(ar1[0], ar[2]) and torch.equal(V1[0], V[2])          # alone = inside the batch
    mp = eng.pad(m)
    if mp > m:                                                              # the padding: no coefficients, identity in V
        assert not bool(ar[:, m:].any()) and not bool(ar[:, :, m:].any())
        assert torch.equal(V[:, m:, m:], torch.eye(mp - m, dtype=torch.float64, device=V.device).expand(len(x), -1, -1))
    ar, V = ar.cpu().numpy(), V.cpu().numpy()
    for w in range(len(x)):
        want_ar, want_V = O.ar_coeff(x[w], p)
        tol = 1e2 * np.linalg.cond(O.count_corr(x[w], p)[0]) * EPS
        ea, ev = rel(ar[w, :m, :m], want_ar), rel(V[w, :m, :m], want_V)
        print(f"m={m} p={p} window {w}: ar {ea:.2e}  V {ev:.2e}  tol {tol:.2e}")
        assert ea < tol and ev < tol, (w, ea, ev, tol)


# ------------------------------------------------------------------------------------------- 2. the g6 batch
def test_g6_batch_option_off_and_on(golden):
    g = golden("g6_errors.npz")
    eng = default_engine()
    m, n = g["nc0_x"].shape
    p = g["nc0_ar"].shape[2]
    ordinary = synthetic_var_dyad(43, m=m, p=min(p, 4), T=n, burn=300)
    batch = np.stack([g["nc0_x"], ordinary, g["nc1_x"], g["nc2_x"], g["xs"], g["xz"]])
    R = _lagcov(eng, batch, p)
    a0, v0, _, i0, r0 = eng.yw_solve(R, m, return_route=True)
    # option off: today's results -- the routes and infos the existing guard test states, the legacy walk's bits
    assert r0.tolist()[:3] == [0, 0, 1] and i0.tolist()[:3] == [0, 0, 0]
    assert int(i0[4]) != 0 and int(i0[5]) != 0                              # xs and the dead channel are refused
    assert set(r0.tolist()) <= {0, 1}
    assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 4) == 0
    try:
        a4, v4, _, i4 = eng.yw_solve(R, m)
        torch.cuda.synchronize()
    finally:
        assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 0) == 0
    assert torch.equal(i4, i0) and torch.equal(a4[:3], a0[:3]) and torch.equal(v4[:3], v0[:3])
    assert rel(a0[0, :m, :m].cpu().numpy(), g["nc0_ar"]) < 1e2 * float(g["nc0_cond"]) * EPS
    # option on
    a1, v1, _, i1, r1 = eng.yw_solve(R, m, flags=_lib.FLAG_YW_PIVOTED, return_route=True)
    for w, route in ((0, 0), (1, 0), (2, 1)):
        assert int(r1[w]) == route and int(i1[w]) == 0
        assert torch.equal(a1[w], a0[w]) and torch.equal(v1[w], v0[w]), w
    assert int(i1[4]) == 0 and int(r1[4]) == 2                              # xs: solved by the LU
    assert bool(torch.isfinite(a1[4]).all()) and bool(torch.isfinite(v1[4]).all())
    assert int(i1[3]) == 0                                                  # nc2
    if int(r1[3]) == 2:
        assert int(i0[3]) != 0
        assert rel(a1[3, :m, :m].cpu().numpy(), g["nc2_ar"]) < 1e2 * float(g["nc2_cond"]) * EPS
    else:
        assert torch.equal(a1[3], a0[3])
    assert int(i1[5]) == 3 and int(r1[5]) == 2                              # dead channel 2: column 2 is exactly zero
    # and through the Python layer
    ap, vp, _, ip, rp = pivoted_engine().yw_solve(R, m, return_route=True)
    assert torch.equal(ip, i1) and torch.equal(rp, r1) and torch.equal(ap[:5], a1[:5]) and torch.equal(vp[:5], v1[:5])


# --------------------------------------------------------------- 3. backward error where parity does not exist
@pytest.mark.parametrize("m,p,n", Y.COLLINEAR_SHAPES)
def test_backward_error_on_collinear_windows(m, p, n):
    eng = default_engine()
    batch = Y.collinear_batch(m, n)
    R = _lagcov(eng, batch, p)
    ar, V, _, info, route = eng.yw_solve(R, m, flags=_lib.FLAG_YW_PIVOTED, return_route=True)
    assert not bool(info.any()), info.tolist()
    print(f"m={m} p={p}: routes {route.tolist()}")
    assert bool((route == 2).any())                                         # otherwise nothing below tests the LU
    mp = eng.pad(m)
    N = mp * p
    idx = Y.real_index(m, p)
    Rh, arh, Vh = R.cpu().numpy(), ar.cpu().numpy(), V.cpu().numpy()
    for w in range(len(batch)):
        G, B = Y.build_system(Rh[w])
        X = arh[w].transpose(2, 1, 0).reshape(N, mp)                        # X[k MP + j][i] = ar[i][j][k]
        eg = Y.eta(G, B, X, idx)
        en = Y.eta(G, B, np.linalg.solve(G, B), idx)
        print(f"  window {w} route {int(route[w])}: eta_gpu {eg / EPS:.3f} eps  eta_numpy {en / EPS:.3f} eps  ratio {eg / en:.3f}")
        assert eg <= N * EPS, (w, eg / EPS)
        assert eg <= C_RATIO * en, (w, eg / EPS, en / EPS)
        Xl, Bl = X.astype(np.longdouble), B.astype(np.longdouble)
        want = (Rh[w, 0].astype(np.longdouble) - Xl.T @ Bl).astype(np.float64)
        bound = N * EPS * (np.abs(Rh[w, 0]) + np.abs(X).T @ np.abs(B))
        assert (np.abs(Vh[w] - want) <= bound).all(), (w, float((np.abs(Vh[w] - want) / bound).max()))


# ---------------------------------------------------------------------------------------------------- 4. scale
@pytest.mark.parametrize("kind,m,p,n", [("collinear", 19, 3, 200), ("ordinary", 33, 5, 900), ("collinear", 64, 2, 300)])
def test_scale(kind, m, p, n):
    """samples * 2^k: under the LU alone the same ar bits and V * 4^k bit for bit; in fallback mode the same routes."""
    eng = default_engine()
    batch = Y.collinear_batch(m, n)[::2] if kind == "collinear" else _ordinary(m, p, n, W=3)
    xd = eng.to_device(batch)
    rec, st = _items(eng, batch.shape[0])

    def both(k):
        R = eng.lagcov(xd * 2.0 ** k, rec, st, n, p)
        with lu_alone(eng):
            ar, V, _, info = eng.yw_solve(R, m)
            torch.cuda.synchronize()
        _, _, _, info_f, route = eng.yw_solve(R, m, flags=_lib.FLAG_YW_PIVOTED, return_route=True)
        return ar, V, info, info_f, route
    ar0, V0, info0, inf0, route0 = both(0)
    assert not bool(info0.any()) and not bool(inf0.any())
    if kind == "collinear":
        assert bool((route0 == 2).any())
    for k in POWERS:
        ar, V, info, info_f, route = both(k)
        assert not bool(info.any()) and not bool(info_f.any()), k
        assert torch.equal(ar, ar0), k
        assert torch.equal(V[:, :m, :m], V0[:, :m, :m] * 4.0 ** k), k
        assert torch.equal(route, route0), (k, route.tolist(), route0.tolist())


# ---------------------------------------------------------------------------------------------- 5. fused calls
M5, N5, P5, HOP5, NW5, BAD5 = 19, 200, 3, 100, 7, 3
FREQS5 = np.linspace(1.0, 60.0, 32)
FS5 = 128.0


@functools.lru_cache(maxsize=None)
def _fused_case():
    """One recording, 7 half-overlapping windows; inside window 3 the last three channels are exact sums of others (an
    xs-style window: its normal equations are singular up to rounding), its neighbours share only half of it."""
    x = synthetic_var_dyad(77, m=M5, p=2, T=HOP5 * (NW5 + 1), burn=300)
    s = slice(BAD5 * HOP5, BAD5 * HOP5 + N5)
    x[16, s] = x[0, s] + x[1, s]
    x[17, s] = x[2, s] - x[3, s]
    x[18, s] = x[4, s] + x[5, s]
    eng = default_engine()
    xd = eng.to_device(x[None])
    pos = HOP5 * np.arange(NW5)
    rec, st = sliding.window_items(1, pos, eng.device)
    return x, xd, rec, st, sliding.regular_grid(pos, N5, P5)


def _good():
    return [w for w in range(NW5) if w != BAD5]


@pytest.mark.parametrize("direct", [False, True], ids=["grid", "direct"])
@pytest.mark.parametrize("chunk", [None, 2])
def test_fused_ffdtf(direct, chunk):
    x, xd, rec, st, grid = _fused_case()
    assert grid == (HOP5, 0, NW5)
    eng, pe = default_engine(), pivoted_engine()
    flags = _lib.FLAG_DIRECT_LAGCOV if direct else 0
    kw = dict(grid=grid, flags=flags, chunk=chunk)
    with pytest.raises(SingularMatrixError) as e:
        eng.sliding_ffdtf(xd, rec, st, N5, P5, FREQS5, FS5, **kw)
    assert e.value.items.tolist() == [BAD5] and f"item {BAD5}" in e.value.args[1]
    base = eng.sliding_ffdtf(xd, rec, st, N5, P5, FREQS5, FS5, check=False, **kw)
    got = pe.sliding_ffdtf(xd, rec, st, N5, P5, FREQS5, FS5, **kw)               # check=True: nothing is refused
    assert torch.equal(got[_good()], base[_good()])
    bad = got[BAD5]
    assert bool(torch.isfinite(bad).all()) and float((bad.sum(dim=(1, 2)) - 1.0).abs().max()) < 1e-12
    # the staged route from the same K1: lagcov -> yw_solve(PIVOTED) -> transfer -> normalise
    R = eng.lagcov(xd, rec, st, N5, P5) if direct else eng.lagcov_regular(xd[0], 0, HOP5, NW5, N5, P5)
    ar, V, _, info, route = eng.yw_solve(R, M5, flags=_lib.FLAG_YW_PIVOTED, return_route=True)
    assert not bool(info.any()) and int(route[BAD5]) == 2 and not bool((route[_good()] == 2).any())
    t = eng.transfer(ar, M5, eng.twiddles(FREQS5, FS5, P5), want_P=True)
    staged = eng.normalise(t["P"], t["rowsum"], M5)[0]
    assert np.allclose(bad.cpu().numpy(), staged[BAD5].cpu().numpy(), rtol=1e-7, atol=1e-12)
    # the flag alone, on the default engine, is the same call
    assert torch.equal(eng.sliding_ffdtf(xd, rec, st, N5, P5, FREQS5, FS5, grid=grid, chunk=chunk,
                                         flags=flags | _lib.FLAG_YW_PIVOTED), got)


@pytest.mark.parametrize("measure", ["ddtf", "gpdc", "block_granger"])
def test_fused_other_measures_accept_the_engine(measure):
    x, xd, rec, st, grid = _fused_case()
    eng, pe = default_engine(), pivoted_engine()

    def run(e):
        if measure == "block_granger":
            return e.sliding_block_granger(xd, rec, st, N5, P5, FREQS5, FS5, split=9, grid=grid, check="mask", chunk=2)
        fn = e.sliding_ddtf if measure == "ddtf" else e.sliding_gpdc
        return fn(xd, rec, st, N5, P5, FREQS5, FS5, grid=grid, check="mask", chunk=2)
    base, got = run(eng), run(pe)
    assert bool(base[-1][BAD5]) and not bool(base[-1][_good()].any())           # the default refuses the bad window
    assert not bool(got[-1][_good()].any())
    for a, b in zip(base[:-1], got[:-1]):
        assert torch.equal(a[_good()], b[_good()])
    if not bool(got[-1][BAD5]):           # solved: finite; otherwise (a V that is not positive definite) it is reported
        for b in got[:-1]:
            assert bool(torch.isfinite(b[BAD5]).all())


def test_yw_routes_reports_the_one_window():
    x, xd, rec, st, grid = _fused_case()
    r = sliding.yw_routes(x, N5, NW5, P5, hop=HOP5)
    assert r["route"].shape == (NW5,) and r["route"].dtype == np.int8 and r["info"].shape == (NW5,)
    assert r["route"][BAD5] == 2 and not (np.delete(r["route"], BAD5) == 2).any() and not r["info"].any()
    r3 = sliding.yw_routes(np.stack([x, x[::-1].copy()]), N5, NW5, P5, hop=HOP5)
    assert r3["route"].shape == (2, NW5) and np.array_equal(r3["route"][0], r["route"])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_pivoted_engine_refuses_what_an_lu_cannot_give():
    x, xd, rec, st, grid = _fused_case()
    eng, pe = default_engine(), pivoted_engine()
    assert pe.pivoted_yw and not eng.pivoted_yw
    for fn in (pe.sliding_ffdtf, pe.sliding_ddtf, pe.sliding_gpdc):
        with pytest.raises(ValueError, match="automatic model order"):
            fn(xd, rec, st, N5, None, FREQS5, FS5, max_model_order=4)
    with pytest.raises(ValueError, match="automatic model order"):
        eng.sliding_ffdtf(xd, rec, st, N5, None, FREQS5, FS5, max_model_order=4, flags=_lib.FLAG_YW_PIVOTED)
    R = eng.lagcov(xd, rec, st, N5, P5)
    with pytest.raises(ValueError, match="want_logdet"):
        pe.yw_solve(R, M5, want_logdet=True)
    with pytest.raises(ValueError, match="want_logdet"):
        eng.yw_solve(R, M5, want_logdet=True, flags=_lib.FLAG_YW_PIVOTED)
    with pytest.raises(ValueError, match="automatic model order"):
        pe.yw_solve_auto(R, M5, N5)


FS6 = 128.0
CHANS6 = ["Fp1", "Fp2", "F3", "F4", "C3", "C4", "O1", "O2"]


def _write(path, seed, dur_s, events):
    rng = np.random.default_rng(seed)
    n = int(dur_s * FS6)
    t = np.arange(n) / FS6 - 2.0
    x = rng.standard_normal((n, len(CHANS6)))
    x[1:] += 0.6 * x[:-1]
    x[:, 1:] += 0.3 * x[:, :-1]
    ev = [{"name": nm, "start_s": 100.0 + st, "start_rel_s": st, "duration_s": du} for nm, st, du in events]
    attrs = {"sampling_freq": FS6, "task_events_structure": json.dumps(ev)}
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, data=x, time=t, channels=np.asarray(CHANS6), attrs=json.dumps(attrs))


def _reader(path):
    with np.load(path, allow_pickle=False) as z:
        return {"data_tc": z["data"], "time": z["time"], "channels": [str(c) for c in z["channels"]],
                "attrs": json.loads(str(z["attrs"]))}


def test_escan_batch_with_the_fallback(tmp_path):
    root = tmp_path / "tree"
    for r, (code, role) in enumerate((("ch", "child"), ("cg", "caregiver"))):
        _write(root / "EEG" / "W_003" / role / f"W_003_EEG_{code}_passive_movies.nc", r, 30.0,
               [("Peppa", 1.0, 11.0), ("Brave", 14.0, 9.5)])
    freqs = np.arange(1.0, 33.0, 1.0)
    res = EB.run(root, tmp_path / "out", window_s=2.0, overlap=0.5, model_order=3, freqs=freqs, low_cutoff_hz=1.0,
                 high_cutoff_hz=45.0, reader=_reader, verbose=False, pivoted_fallback=True, measures=("ffdtf", "gpdc"))
    assert res["done"] == ["W_003"] and not res["failed"]
    z = np.load(tmp_path / "out" / "W_003_ffdtf.npz", allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    assert not meta["failed_segments"] and [s["event"] for s in meta["segments"]] == ["Peppa", "Brave"]
    for seg in meta["segments"]:
        routes = seg["yw_routes"]
        assert sorted(routes) == ["ldlt", "lu", "recursion"] and sum(routes.values()) == seg["windows"] > 0
        assert seg["singular_windows"] == 0
        assert np.isfinite(z[f"{seg['task']}/{seg['event']}/ffdtf_bands"]).all()
    # without the option the meta carries no such entry
    res = EB.run(root, tmp_path / "out2", window_s=2.0, overlap=0.5, model_order=3, freqs=freqs, low_cutoff_hz=1.0,
                 high_cutoff_hz=45.0, reader=_reader, verbose=False)
    meta2 = json.loads(str(np.load(tmp_path / "out2" / "W_003_ffdtf.npz", allow_pickle=False)["meta"]))
    assert all("yw_routes" not in s for s in meta2["segments"])
