"""The block Granger entries are routes of `Engine._sliding_call` and their significance tests run on the shared loops of
significance.py: what the two hand-written drivers and the two copied loops gave before that, pinned bit for bit in
tests/golden/block_routes_bits.json (recorded on the MI355X from the commit before the change, by `hashes` below).

What can go wrong here is a Python path, not a kernel shape, so the shapes are the two smallest of
tests/test_gpu_block_gc_significance.py that differ in padding, with that module's seeded inputs: three recordings of three
half-overlapping windows.  Hashed are defined values only: outputs, infos, the [:m, :m] corner of ar / V and every leaf of
the returned dicts, NaN positions included (every NaN is hashed as the same NaN).  All @pytest.mark.gpu."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_block_gc_significance import FS, SHAPES as ALL_SHAPES, D, W, _bands, _freqs, _input

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import window_items

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_routes_bits.json")
SHAPES = [ALL_SHAPES[1], ALL_SHAPES[2]]            # (m, split, p, F, n) = (6, 2, 3, 8, 256), (19, 7, 2, 8, 400)
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
VALUES = (("time",), ("bands",), ("time", "bands"))
S, SEED = 5, 11


def _flat(res, m, prefix=""):
    """A call's result -- tensor, None, tuple or dict, nested -- as {name: host array}; (items, MP, MP, ...) arrays of the
    padded layouts (ar, V) cut to their [:m, :m] corner."""
    if res is None:
        return {prefix + "none": np.zeros(0)}
    if isinstance(res, torch.Tensor):
        mp = 16 * ((m + 15) // 16)
        if res.dim() >= 3 and tuple(res.shape[1:3]) == (mp, mp):
            res = res[:, :m, :m]
        return {prefix.rstrip("."): res.cpu().numpy()}
    named = res.items() if isinstance(res, dict) else enumerate(res)
    out = {}
    for k, v in named:
        out.update(_flat(v, m, f"{prefix}{k}."))
    return out


@functools.lru_cache(maxsize=None)
def outputs(shape):
    """Every call of this module on one shape, once: (x on the host, {case: {name: host array}})."""
    m, split, p, F, n = shape
    xh, pos = _input(shape)
    eng = default_engine()
    x = eng.to_device(xh)
    rec, st = window_items(D, pos, eng.device)
    wst = torch.as_tensor(np.asarray(pos, dtype=np.int64)).to(eng.device)
    N = D * W
    f, bands = _freqs(F), _bands(F)
    none = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    out = {}

    def keep(name, res):
        out[name] = _flat(res, m)

    def keep_refusal(name, call):
        with pytest.raises(ValueError) as ei:
            call()
        out[name] = {"error": np.frombuffer(str(ei.value).encode(), dtype=np.uint8)}

    # ---- sliding_block_granger
    def one(**kw):
        return eng.sliding_block_granger(x, rec, st, n, p, f, FS, split=split, **kw)
    keep("one/full", one())
    keep("one/bands", one(bands=bands))
    keep_refusal("one/empty_bands", lambda: one(bands=none))     # the full array, then `band_sums`, which takes no empty set
    keep("one/grid", one(grid=(n // 2, 0, W)))
    keep("one/grid_bands_mask", one(grid=(n // 2, 0, W), bands=bands, check="mask"))
    keep("one/chunk2", one(chunk=2))
    keep("one/chunk2_bands", one(chunk=2, bands=bands))
    keep("one/return_ar", one(return_ar=True))
    keep("one/return_ar_mask_bands", one(return_ar=True, check="mask", bands=bands))
    keep("one/nan", one(check="nan"))
    keep("one/unchecked", one(check=False))
    given = eng.empty(N, 2, 2)
    keep("one/out_bands", (one(bands=bands, out=given), given))

    # ---- sliding_block_granger_pairs: A of recording d with B of recording d + 1
    pi = torch.as_tensor([1, 2, 0], device=eng.device)
    rec_b = pi[rec].contiguous()
    base_a = torch.arange(N, dtype=torch.int64, device=eng.device)
    base_b = (rec_b * W + base_a % W).contiguous()

    def pairs(b=rec_b, freqs=f, **kw):
        return eng.sliding_block_granger_pairs(x, rec, b, st, n, p, freqs, FS, split=split, **kw)
    keep("pairs/both", pairs())
    keep("pairs/spectral", pairs(want=("spectral",)))
    keep("pairs/time", pairs(want=("time",), freqs=None))
    keep("pairs/spectral_return_ar_mask", pairs(want=("spectral",), return_ar=True, check="mask"))
    keep("pairs/time_return_ar_mask", pairs(want=("time",), freqs=None, return_ar=True, check="mask"))
    keep("pairs/bands", pairs(bands=bands))
    keep_refusal("pairs/empty_bands", lambda: pairs(bands=none))
    keep("pairs/return_red", pairs(return_red=True, return_ar=True, check="mask"))
    observed = pairs(b=rec, return_red=True)
    keep("pairs/observed_return_red", observed)
    base = dict(R_base=eng.lagcov(x, rec, st, n, p), base_a=base_a, base_b=base_b)
    keep("pairs/R_base", pairs(**base))
    keep("pairs/R_base_bands_return_ar", pairs(bands=bands, return_ar=True, **base))
    keep("pairs/red_base", pairs(red_base=observed[2], **base))
    keep("pairs/red_base_time_mask", pairs(want=("time",), freqs=None, red_base=observed[2], return_red=True, check="mask", **base))
    keep("pairs/chunk2", pairs(chunk=2))
    keep("pairs/chunk2_red_base_bands", pairs(chunk=2, bands=bands, red_base=observed[2], **base))
    keep("pairs/nan", pairs(check="nan"))

    # ---- the surrogate tests: default chunk, and a chunk that splits a surrogate (N = 9 windows)
    for null in ("shift", "phase"):
        for values in VALUES:
            for chunk in (None, 2):
                keep(f"surrogate/{null}/{'+'.join(values)}/chunk{chunk}", eng.block_granger_significance(
                    x, rec, st, n, p, f, FS, bands, split=split, null=null, n_surrogates=S, seed=SEED, values=values, chunk=chunk))
        keep(f"surrogate/{null}/nan", eng.block_granger_significance(
            x, rec, st, n, p, f, FS, bands, split=split, null=null, n_surrogates=S, seed=SEED, check="nan"))
        for chunk in (None, 2):
            keep(f"measure/{null}/chunk{chunk}", eng.sliding_significance(
                x, rec, st, n, p, f, FS, bands, measure="ffdtf", null=null, n_surrogates=S, seed=SEED, split=split, chunk=chunk))

    # ---- the pseudo-dyad tests: exhaustive and seeded, whole surrogates and blocks smaller than D * W
    for name, draw in (("exhaustive", {}), ("seeded", dict(n_surrogates=4, seed=5))):
        for values in VALUES:
            for chunk in (None, 4):
                keep(f"pseudo/{name}/{'+'.join(values)}/chunk{chunk}", eng.block_granger_pseudo_dyad_significance(
                    x, wst, n, p, f, FS, bands, split=split, values=values, chunk=chunk, **draw))
        keep(f"pseudo/{name}/nan", eng.block_granger_pseudo_dyad_significance(x, wst, n, p, f, FS, bands, split=split,
                                                                              check="nan", **draw))
        for chunk in (None, 4):
            keep(f"pseudo_measure/{name}/chunk{chunk}", eng.pseudo_dyad_significance(
                x, wst, n, p, f, FS, bands, measure="gpdc", split=split, chunk=chunk, **draw))
    torch.cuda.synchronize()
    return xh, out


def _sha(a):
    a = np.ascontiguousarray(a).copy()
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan                     # one NaN: where it is counts, its payload does not
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def hashes(shape):
    """What tests/golden/block_routes_bits.json holds for one shape: SHA-256 of the input and of every array of every call."""
    xh, out = outputs(shape)
    return {"input": _sha(xh), "cases": {case: {k: _sha(v) for k, v in arrays.items()} for case, arrays in out.items()}}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_call_returns_what_it_returned_before(shape):
    """Shapes and None-ness of the tuples, independent of the golden file: (spectral, time[, (red, info_red)][, bad][, ar, V,
    (info_yw, info_red, info_gc)])."""
    m, split, p, F, n = shape
    _, out = outputs(shape)
    N = D * W
    assert {k: v.shape for k, v in out["one/return_ar_mask_bands"].items()} == {
        "0": (N, 2, 2), "1": (N, 4), "2": (N,), "3": (N, m, m, p), "4": (N, m, m), "5.0": (N,), "5.1": (N, 2), "5.2": (N * F,)}
    assert {k: v.shape for k, v in out["pairs/return_red"].items()} == {
        "0": (N, 2, F), "1": (N, 4), "2.0": (N, 2), "2.1": (N, 2), "3": (N,), "4": (N, m, m, p), "5": (N, m, m), "6.0": (N,),
        "6.1": (N, 2), "6.2": (N * F,)}
    assert sorted(out["pairs/time_return_ar_mask"]) == ["0.none", "1", "2", "3", "4", "5.0", "5.1", "5.2.none"]
    assert sorted(out["pairs/spectral_return_ar_mask"]) == ["0", "1.none", "2", "3", "4", "5.0", "5.1.none", "5.2"]
    for case in ("one/empty_bands", "pairs/empty_bands"):      # the detour of an empty band set ends in `band_sums`' refusal
        assert out[case]["error"].tobytes().startswith(b"hmv_band_sums_f64: ")
    a, b = out["one/out_bands"]["0.0"], out["one/out_bands"]["1"]          # what comes back is the tensor that was given
    assert np.array_equal(a, b) and np.array_equal(a, out["one/bands"]["0"])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pinned_bits(shape):
    """Every array of every call above, bit for bit what the two separate drivers and the two copied loops gave.  The input
    is hashed too, so that a mismatch says which side moved."""
    with open(GOLDEN) as fh:
        want = json.load(fh)["x".join(str(v) for v in shape)]
    got = hashes(shape)
    assert got["input"] == want["input"], "numpy's generator no longer reproduces the recorded input"
    assert sorted(got["cases"]) == sorted(want["cases"])
    moved = [f"{case}:{k}" for case in want["cases"] for k in sorted(set(want["cases"][case]) | set(got["cases"][case]))
             if got["cases"][case].get(k) != want["cases"][case].get(k)]
    assert not moved, f"bits moved: {moved}"
