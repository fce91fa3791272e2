"""The phase family's Python lives in phase.py and its C entries share their checks: what every public call of the family
returned before that, pinned bit for bit in tests/golden/phase_family_bits.json (recorded on the MI355X from the commit
before the move, where the combined call was still `Engine._sliding_phase`, by `hashes` below:
HYPERMVAR_RECORD_PHASE_BITS=1 makes the test write the file instead of reading it).

What can go wrong is host code, so the shapes are the smallest that reach every path: m = 5 (one tile, padding) and m = 33
with split 17 (three tiles, a split inside a tile); T = 700 and n = 130 (neither a multiple of 64 nor of 4); 2 recordings (3
dyads) of 3 windows, the last ending at T; 2 bands; slabs of one recording and one band and a single slab; a strided z that
is read in place and a z that needs the contiguous copy.  SHA-256 of the raw bytes of every returned array.
All @pytest.mark.gpu."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.sliding import window_items

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_family_bits.json")
SHAPES = ((5, 2), (33, 17))                            # (m, split)
IDS = [f"{m}x{s}" for m, s in SHAPES]
T, N, FS, D = 700, 130, 250.0, 3
STARTS = (0, 285, T - N)
BANDS = ((8.0, 12.0), (13.0, 30.0))
SYNC, LAG = ("plv", "ciplv", "coh", "imcoh"), ("pli", "wpli", "dwpli")
SLABS = {"slabs": 1, "one_slab": 8 << 30}              # max_workspace_bytes: one recording and one band at a time / all


def _flat(res, prefix=""):
    """A call's result -- tensor, None, tuple or dict, nested -- as {name: host array}."""
    if res is None:
        return {prefix + "none": np.zeros(0)}
    if isinstance(res, torch.Tensor):
        return {prefix.rstrip("."): res.cpu().numpy()}
    out = {}
    for k, v in (res.items() if isinstance(res, dict) else enumerate(res)):
        out.update(_flat(v, f"{prefix}{k}."))
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def hashes(shape):
    """What tests/golden/phase_family_bits.json holds for one shape: {"input": .., "cases": {case: {array: SHA-256}}}."""
    m, split = shape
    rng = np.random.default_rng(1000 + m)
    xh = rng.standard_normal((D, m, T))
    xh[:, split:] += 0.5 * np.roll(xh[:, :m - split], 3, axis=-1)            # some coupling across the split
    shift_h = rng.integers(0, T, size=2 * len(STARTS))
    eng = default_engine()
    x3 = eng.to_device(xh)
    x = x3[:2]
    rec, st = window_items(2, STARTS, eng.device)
    wst = torch.as_tensor(np.asarray(STARTS, dtype=np.int64)).to(eng.device)
    resp = torch.stack([eng.band_response(T, FS, lo, hi) for lo, hi in BANDS])
    z = eng.analytic_signal(x, resp)                                         # (2, 2, m, T)
    view = z[:, 1]                                                           # strided: read in place
    turned = z[:, 0].transpose(1, 2).contiguous().transpose(1, 2)            # time is not the unit stride: copied
    assert not view.is_contiguous() and view.stride(2) == 1 and turned.stride(2) == m
    out = {}

    def keep(name, res):
        out[name] = {k: _sha(v) for k, v in _flat(res).items()}

    keep("phase_sync/unit_view", eng.phase_sync(view, rec, st, N, _lib.PHASE_UNIT, coherency=True))
    keep("phase_sync/raw_turned", eng.phase_sync(turned, rec, st, N, _lib.PHASE_RAW, coherency=True))
    shift = torch.as_tensor(shift_h.astype(np.int64)).to(eng.device)
    keep("phase_sync_pairs/unit_view", eng.phase_sync_pairs(view, rec, 1 - rec, st, N, _lib.PHASE_UNIT, split=split,
                                                            shift_b=shift))
    keep("phase_sync_pairs/raw_turned", eng.phase_sync_pairs(turned, rec, rec, st, N, _lib.PHASE_RAW, split=split,
                                                             shift_b=shift, cols=(1, -1)))
    keep("phase_lag/all_view", eng.phase_lag(view, rec, st, N, want=LAG))
    keep("phase_lag/split_turned", eng.phase_lag(turned, rec, st, N, want=LAG, split=split))
    for name, ws in SLABS.items():
        kw = dict(max_workspace_bytes=ws)
        keep(f"sliding_phase_sync/{name}", eng.sliding_phase_sync(x, rec, st, N, FS, BANDS, measures=SYNC, **kw))
        keep(f"sliding_phase_lag/{name}", eng.sliding_phase_lag(x, rec, st, N, FS, BANDS, measures=LAG, split=split, **kw))
        keep(f"sliding_phase/{name}", eng.sliding_phase("both", x, rec, st, N, FS, BANDS, sync=("plv", "imcoh"), lag=LAG,
                                                        split=split, check="nan", **kw))
        # chunk = 4 items: three surrogate blocks per slab of 3 rows, nine for the single slab of 12
        keep(f"phase_sync_significance/{name}",
             eng.phase_sync_significance(x, rec, st, N, FS, BANDS, measures=("plv", "coh"), n_surrogates=3, seed=5, split=split,
                                         chunk=4, full=True, **kw))
    keep("phase_sync_pseudo_dyad_significance",
         eng.phase_sync_pseudo_dyad_significance(x3, wst, N, FS, BANDS, measures=("ciplv", "imcoh"), split=split, n_surrogates=2,
                                                 seed=7))
    return {"input": _sha(xh), "cases": out}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pinned_bits(shape):
    """Every array of every call above, bit for bit what the commit before the move gave.  The input is hashed too, so that
    a mismatch says which side moved."""
    got, key = hashes(shape), "x".join(str(v) for v in shape)
    if os.environ.get("HYPERMVAR_RECORD_PHASE_BITS"):
        recorded = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        recorded[key] = got
        with open(GOLDEN, "w") as fh:
            json.dump(recorded, fh, indent=1, sort_keys=True)
            fh.write("\n")
    with open(GOLDEN) as fh:
        want = json.load(fh)[key]
    assert got["input"] == want["input"], "numpy's generator no longer reproduces the recorded input"
    assert sorted(got["cases"]) == sorted(want["cases"])
    moved = [f"{case}:{k}" for case in want["cases"] for k in sorted(set(want["cases"][case]) | set(got["cases"][case]))
             if got["cases"][case].get(k) != want["cases"][case].get(k)]
    assert not moved, f"bits moved: {moved}"
    assert len(got["cases"]) == 15 and all(len(v) >= 2 for v in got["cases"].values())
