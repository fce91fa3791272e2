"""The C driver behind the twelve fused `hmv_sliding_*` entries is a plan and four stages; what the one 260-line function
gave before that, pinned bit for bit in tests/golden/sliding_driver_bits.json (recorded on the MI355X from the commit
before the change, by `hashes` below).  The block Granger entries are pinned by tests/test_gpu_block_routes.py and the K3
split is compared bit for bit by tests/test_gpu_k3_split.py; here is every other entry and every branch the plan takes.

What can go wrong is host code, not a kernel shape, so the inputs are that module's: three seeded recordings of three
half-overlapping windows, at the two smallest shapes (m, p, F, n) that differ in padding and take K3's in-kernel band form
(F % 32 == 0).  Groups of calls (one entry of the golden file each):

  6x3x32x256, 19x2x32x400   ffDTF, dDTF, GPDC and ffDTF + spectra at a fixed order -- full and bands, one chunk and chunks
                            of two (the last of one window), item tables and a declared grid, every flag, return_ar,
                            overlap=False --, the same four at the automatic order (max_model_order=6, return_orders), the
                            half-batch split (16 windows in one chunk, FLAG_YW_TILED, overlap), and the singular fixture window
                            (g6_errors.npz xs, repeated to the window length) among the items with check="mask"
  k1_forms                  `sliding_ensemble` without and with a grid (direct and shared K1), the split K1 through
                            `ensemble_significance`, `sliding_pairs` without and with R_base, `sliding_mix`, each on the
                            tables of its own GPU tests
  shape_rule                64 channels, p = 2, F = 16, HMV_TUNE_YW_FORM = 1, 128 and 127 windows in one chunk: the two sides
                            of the rule that picks the LDL^T launch chain (tests/test_gpu_k3_split.py's Batch)

Hashed are defined values only: outputs, infos, the [:m, :m] corner of ar / V, every leaf of returned dicts, NaN positions
included (every NaN is hashed as the same NaN); of a call with a failed window the mask, info_yw and the good windows.  The
inputs are hashed too.  All @pytest.mark.gpu."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_block_gc_significance import FS, D, W, _bands, _freqs, _input
from tests.test_gpu_block_routes import _flat, _sha

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import window_items

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sliding_driver_bits.json")
SHAPES = [(6, 3, 32, 256), (19, 2, 32, 400)]            # (m, p, F, n)
GROUPS = ["x".join(str(v) for v in s) for s in SHAPES] + ["k1_forms", "shape_rule"]
FLAGS = ("DIRECT_LAGCOV", "YW_ONE_LAUNCH", "YW_TILED", "YW_PIVOTED", "UNFUSED_NORM")
PMAX = 6
N = D * W
SINGULAR = 2 * W                                        # the first window of the third recording


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name), allow_pickle=False)


def _windows(shape):
    """Every call of one (m, p, F, n) shape: ({input name: host array}, {case: {name: host array}})."""
    m, p, F, n = shape
    xh, pos = _input((m, 1, p, F, n))
    eng = default_engine()
    x = eng.to_device(xh)
    rec, st = window_items(D, pos, eng.device)
    f, bands, grid = _freqs(F), _bands(F), (n // 2, 0, W)
    out = {}
    fixed = {"ffdtf": eng.sliding_ffdtf, "ddtf": eng.sliding_ddtf, "gpdc": eng.sliding_gpdc}

    for name, fn in fixed.items():
        def run(order=p, **kw):
            return _flat(fn(x, rec, st, n, order, f, FS, **kw), m)
        for tag, kw in (("full", {}), ("bands", dict(bands=bands))):
            out[f"{name}/{tag}"] = run(**kw)
            out[f"{name}/{tag}/chunk2"] = run(chunk=2, **kw)
            out[f"{name}/{tag}/grid"] = run(grid=grid, **kw)
            out[f"{name}/{tag}/flags0"] = run(flags=0, **kw)
            for flag in FLAGS:
                out[f"{name}/{tag}/{flag}"] = run(flags=getattr(_lib, "FLAG_" + flag), **kw)
            out[f"{name}/{tag}/return_ar"] = run(return_ar=True, **kw)
            out[f"{name}/{tag}/no_overlap"] = run(overlap=False, **kw)
            out[f"{name}/{tag}/auto"] = run(None, max_model_order=PMAX, return_orders=True, **kw)
        out[f"{name}/auto/chunk2_grid_return_ar"] = run(None, max_model_order=PMAX, return_orders=True, chunk=2, grid=grid,
                                                       return_ar=True)

    def run_s(order=p, **kw):
        return _flat(eng.sliding_ffdtf_spectra(x, rec, st, n, order, f, FS, **kw), m)
    out["spectra/full"] = run_s()
    out["spectra/chunk2"] = run_s(chunk=2)
    out["spectra/grid"] = run_s(grid=grid)
    out["spectra/flags0"] = run_s(flags=0)
    for flag in FLAGS:
        out[f"spectra/{flag}"] = run_s(flags=getattr(_lib, "FLAG_" + flag))
    out["spectra/auto"] = run_s(None, max_model_order=PMAX, return_orders=True)
    out["spectra/auto/chunk2_grid"] = run_s(None, max_model_order=PMAX, return_orders=True, chunk=2, grid=grid)

    # ---- the half-batch split of the tiled K2: 16 windows in one chunk on two streams
    k = np.arange(16)
    rec16 = torch.as_tensor(k % D).to(eng.device)
    st16 = torch.as_tensor((k // D) * (n // 4)).to(eng.device)
    out["ffdtf/half_batch_split"] = _flat(eng.sliding_ffdtf(x, rec16, st16, n, p, f, FS, flags=_lib.FLAG_YW_TILED, overlap=True,
                                                            return_ar=True), m)

    # ---- a singular window among the items: the mask, info_yw, and the windows that are good
    xs = _golden("g6_errors.npz")["xs"]
    xh_s = xh.copy()
    xh_s[2, :4, :n] = np.tile(xs, (1, 2))[:, :n]
    x_s = eng.to_device(xh_s)
    for name, fn in fixed.items():
        res, bad, ar, V, infos = fn(x_s, rec, st, n, p, f, FS, check="mask", return_ar=True)
        info_yw = infos if isinstance(infos, torch.Tensor) else infos[0]
        good = ~bad
        named = {"bad": bad, "info_yw": info_yw, "out": res[good], "ar": ar[good][:, :m, :m], "V": V[good][:, :m, :m]}
        if not isinstance(infos, torch.Tensor):
            named["info_tf"] = infos[1].view(N, F)[good]
        out[f"{name}/singular_mask"] = {key: v.cpu().numpy() for key, v in named.items()}
    torch.cuda.synchronize()
    return {"x": xh, "x_singular": xh_s}, out


def _k1_forms():
    """The entries whose K1 is not the single-trial one, each on the tables of its own tests' smallest fused shape."""
    from tests import test_gpu_ensemble as TE
    from tests import test_gpu_ensemble_contrast as TC
    from tests import test_gpu_ensemble_significance as TS
    from tests import test_gpu_pseudo_dyads as TP
    from hyperscanning_signal_analysis_amd.sliding import hop_positions
    eng = default_engine()
    out, inputs = {}, {}
    f, bands = _freqs(32), _bands(32)

    # ---- sliding_ensemble: one group, without a grid (direct K1) and with one (shared K1)
    m, p, n, E, hop, L = TE.SHAPES[0]
    xh, onsets, offsets = TE.workload(m, p, n, E, hop, L)
    inputs["ensemble"] = xh
    xd = eng.to_device(xh[None])
    d = TE.one_group(eng, onsets, offsets)
    for gname, grid in (("direct", None), ("shared", (hop, len(offsets)))):
        for measure in ("ffdtf", "ddtf", "gpdc"):
            for tag, kw in (("full", {}), ("bands", dict(bands=bands)), ("chunk2_return_ar", dict(chunk=2, return_ar=True))):
                out[f"ensemble/{gname}/{measure}/{tag}"] = _flat(
                    eng.sliding_ensemble(xd, n=n, p=p, freqs=f, fs=FS, measure=measure, grid=grid, **d, **kw), m)
        out[f"ensemble/{gname}/spectra"] = _flat(eng.sliding_ensemble(xd, n=n, p=p, freqs=f, fs=FS, spectra=True, grid=grid, **d), m)

    # ---- the split K1 (hmv_sliding_ensemble_split_f64) through ensemble_significance
    n, hop, p, split, S = 60, 30, 3, 3, 3
    groups = TS.stat_groups(seed=43, counts=(5, 7, 4))
    m, L = groups[0].shape[:2]
    counts = [g.shape[2] for g in groups]
    offsets = hop_positions(L, n, hop)
    G, Wn = len(groups), len(offsets)
    xh = np.concatenate([np.moveaxis(e, 2, 0) for e in groups], axis=0)
    inputs["ensemble_split"] = xh
    xd = eng.to_device(xh)
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
    d = dict(trial_rec=i64(np.arange(sum(counts))), trial_start=i64(np.zeros(sum(counts))),
             group_ptr=i64(np.concatenate([[0], np.cumsum(counts)])), item_group=i64(np.repeat(np.arange(G), Wn)),
             item_offset=i64(np.tile(offsets, G)))
    for measure in ("ffdtf", "gpdc"):
        for chunk in (None, Wn):
            out[f"ensemble_split/{measure}/chunk{chunk}"] = _flat(eng.ensemble_significance(
                xd, n=n, p=p, freqs=f, fs=FS, bands=bands, measure=measure, n_surrogates=S, seed=3, split=split, chunk=chunk,
                grid=(hop, Wn), **d), m)

    # ---- sliding_pairs, without and with R_base (tests/test_gpu_pseudo_dyads.py::test_fused_bits)
    m, split, n, p, T = 6, 2, 128, 3, 500
    xh = TP.coloured(np.random.default_rng(100 * m + 32), (3, m, T))
    inputs["pairs"] = xh
    x = eng.to_device(xh)
    starts = (0, 100, 201, T - n)
    rec_a = TP.i64(eng, [a for a, b in TP.PAIRS3 for _ in starts])
    rec_b = TP.i64(eng, [b for a, b in TP.PAIRS3 for _ in starts])
    st = TP.i64(eng, [s for _ in TP.PAIRS3 for s in starts])
    k = TP.i64(eng, np.tile(np.arange(4), 9))
    base = eng.lagcov(x, TP.i64(eng, np.repeat(np.arange(3), 4)), TP.i64(eng, np.tile(starts, 3)), n, p)
    based = dict(R_base=base, base_a=rec_a * 4 + k, base_b=rec_b * 4 + k, chunk=5)
    for measure in ("ffdtf", "ddtf", "gpdc"):
        for bname, kw in (("plain", {}), ("R_base", based)):
            out[f"pairs/{bname}/{measure}/bands"] = _flat(
                eng.sliding_pairs(x, rec_a, rec_b, st, n, p, f, 128.0, measure=measure, split=split, bands=bands, **kw), m)
            out[f"pairs/{bname}/{measure}/return_ar"] = _flat(
                eng.sliding_pairs(x, rec_a, rec_b, st, n, p, f, 128.0, measure=measure, split=split, return_ar=True, **kw), m)

    # ---- sliding_mix (tests/test_gpu_ensemble_contrast.py::test_bits_do_not_depend_on_the_batch)
    m, p, n, E, Wn, rows = 20, 4, 80, 6, 3, 17
    rng = np.random.default_rng(3)
    xh = np.stack([TC.coloured(rng, (m, n + 40)) for _ in range(E)])
    Wt = rng.uniform(0.0, 1.0, (rows, E))
    inputs["mix"], inputs["mix_weights"] = xh, Wt
    Rt = eng.lagcov_trials(eng.to_device(xh), TC._i64(eng, np.arange(E)), TC._i64(eng, np.zeros(E)), TC._i64(eng, [0, 20, 40]), n, p)
    Wd, sd = eng.to_device(Wt), eng.to_device(1.0 / Wt.sum(axis=1))
    for measure in ("ffdtf", "ddtf", "gpdc"):
        for tag, kw in (("bands_return_ar", dict(bands=bands, return_ar=True)), ("full_chunk4", dict(chunk=4))):
            out[f"mix/{measure}/{tag}"] = _flat(eng.sliding_mix(Rt, Wd, sd, n, f, 100.0, m=m, measure=measure, **kw), m)
    out["mix/spectra"] = _flat(eng.sliding_mix(Rt, Wd, sd, n, f, 100.0, m=m, spectra=True), m)
    torch.cuda.synchronize()
    return inputs, out


def _shape_rule():
    """HMV_TUNE_YW_FORM = 1 at 64 channels: 128 windows in one chunk take the LDL^T launch chain, 127 the one launch."""
    from tests.test_gpu_k3_split import OFF, Batch
    eng = default_engine()
    out, inputs = {}, {}
    for items in (128, 127):
        b = Batch(eng, _golden, 64, items=items)
        inputs[f"x{items}"] = b.x.cpu().numpy()
        assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 1) == 0
        try:
            res, info_yw, info_tf, _, _ = b.run(16, OFF)
        finally:
            assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 0) == 0
        out[f"windows{items}"] = {"out": res.cpu().numpy(), "info_yw": info_yw.cpu().numpy(), "info_tf": info_tf.cpu().numpy()}
    return inputs, out


@functools.lru_cache(maxsize=None)
def outputs(group):
    """Every call of one group, once: ({input name: host array}, {case: {name: host array}})."""
    if group == "k1_forms":
        return _k1_forms()
    if group == "shape_rule":
        return _shape_rule()
    return _windows(SHAPES[GROUPS.index(group)])


def hashes(group):
    """What tests/golden/sliding_driver_bits.json holds for one group: SHA-256 of the inputs and of every array of every call."""
    inputs, out = outputs(group)
    return {"input": {k: _sha(v) for k, v in inputs.items()},
            "cases": {case: {k: _sha(v) for k, v in arrays.items()} for case, arrays in out.items()}}


@pytest.mark.parametrize("group", GROUPS)
def test_every_call_returns_what_it_returned_before(group):
    """Shapes and None-ness of the returned tuples, independent of the golden file."""
    _, out = outputs(group)
    shapes = lambda case: {k: v.shape for k, v in out[case].items()}  # noqa: E731
    if group == "shape_rule":
        for items in (128, 127):
            assert shapes(f"windows{items}") == {"out": (items, 64, 64, 16), "info_yw": (items,), "info_tf": (items, 16)}
            bad = np.flatnonzero(out[f"windows{items}"]["info_yw"])
            assert bad.tolist() == [3, 38]                 # the two singular windows of the batch, and nothing else
        return
    if group == "k1_forms":
        m, p, L, n, hop = 3, 1, 120, 24, 6
        Wn = (L - n) // hop + 1
        for g in ("direct", "shared"):
            assert shapes(f"ensemble/{g}/ffdtf/full") == {"": (Wn, m, m, 32)}
            assert shapes(f"ensemble/{g}/gpdc/bands") == {"": (Wn, m, m, 2)}
            assert shapes(f"ensemble/{g}/ddtf/chunk2_return_ar") == {
                "0": (Wn, m, m, 32), "1": (Wn, m, m, p), "2": (Wn, m, m), "3.0": (Wn,), "3.1": (Wn * 32,)}
            assert shapes(f"ensemble/{g}/gpdc/chunk2_return_ar") == {"0": (Wn, m, m, 32), "1": (Wn, m, m, p), "2": (Wn, m, m), "3": (Wn,)}
            assert shapes(f"ensemble/{g}/spectra") == {"0": (Wn, m, m, 32), "1": (Wn, m, m, 32)}
            assert out[f"ensemble/{g}/spectra"]["1"].dtype == np.complex128
        assert shapes("ensemble_split/ffdtf/chunkNone")["p"] == (9, 6, 6, 2)
        assert shapes("pairs/R_base/ddtf/return_ar") == {"0": (36, 6, 6, 32), "1": (36, 6, 6, 3), "2": (36, 6, 6), "3.0": (36,),
                                                        "3.1": (36 * 32,)}
        assert shapes("pairs/plain/ffdtf/bands") == {"": (36, 6, 6, 2)}
        assert shapes("mix/gpdc/bands_return_ar") == {"0": (51, 20, 20, 2), "1": (51, 20, 20, 4), "2": (51, 20, 20), "3": (51,)}
        assert shapes("mix/ffdtf/full_chunk4") == {"": (51, 20, 20, 32)}
        assert shapes("mix/spectra") == {"0": (51, 20, 20, 32), "1": (51, 20, 20, 32)}
        return
    m, p, F, n = SHAPES[GROUPS.index(group)]
    model = {"1": (N, m, m, p), "2": (N, m, m)}
    for name in ("ffdtf", "ddtf", "gpdc"):
        infos = {"3": (N,)} if name == "gpdc" else {"3.0": (N,), "3.1": (N * F,)}
        assert shapes(f"{name}/full") == shapes(f"{name}/full/chunk2") == shapes(f"{name}/full/grid") == {"": (N, m, m, F)}
        assert shapes(f"{name}/bands") == shapes(f"{name}/bands/YW_TILED") == {"": (N, m, m, 2)}
        assert shapes(f"{name}/full/return_ar") == {"0": (N, m, m, F), **model, **infos}
        assert shapes(f"{name}/bands/return_ar") == {"0": (N, m, m, 2), **model, **infos}
        assert shapes(f"{name}/full/auto") == {"0": (N, m, m, F), "1": (N,), "2": (N, PMAX)}
        assert shapes(f"{name}/auto/chunk2_grid_return_ar") == {
            "0": (N, m, m, F), "1": (N, m, m, PMAX), "2": (N, m, m), **infos, "4": (N,), "5": (N, PMAX)}
        got = out[f"{name}/singular_mask"]
        assert got["bad"].shape == (N,) and bool(got["bad"][SINGULAR]) and int(got["info_yw"][SINGULAR]) != 0
        assert got["out"].shape == (N - int(got["bad"].sum()), m, m, F) and not np.isnan(got["out"]).any()
    assert shapes("spectra/full") == shapes("spectra/YW_PIVOTED") == {"0": (N, m, m, F), "1": (N, m, m, F)}
    assert out["spectra/full"]["1"].dtype == np.complex128
    assert shapes("spectra/auto") == {"0": (N, m, m, F), "1": (N, m, m, F), "2": (N,), "3": (N, PMAX)}
    assert shapes("ffdtf/half_batch_split") == {"0": (16, m, m, F), "1": (16, m, m, p), "2": (16, m, m), "3.0": (16,), "3.1": (16 * F,)}
    orders = out["ffdtf/full/auto"]["1"]
    assert orders.dtype == np.int32 and (orders >= 1).all() and (orders <= PMAX).all()


@pytest.mark.parametrize("group", GROUPS)
def test_pinned_bits(group):
    """Every array of every call above, bit for bit what the driver gave as one function.  The inputs are hashed too, so
    that a mismatch says which side moved."""
    with open(GOLDEN) as fh:
        want = json.load(fh)[group]
    got = hashes(group)
    assert got["input"] == want["input"], "the generators no longer reproduce the recorded inputs"
    assert sorted(got["cases"]) == sorted(want["cases"])
    moved = [f"{case}:{k}" for case in want["cases"] for k in sorted(set(want["cases"][case]) | set(got["cases"][case]))
             if got["cases"][case].get(k) != want["cases"][case].get(k)]
    assert not moved, f"bits moved: {moved}"
