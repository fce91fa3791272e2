"""Every host-side launcher that picks a kernel instantiation by the padded channel count, at each of the four padded
sizes, through the unfused `Engine` methods: what they returned before the hand-written `switch (m_pad)` blocks became
`hmv::for_nt`, pinned bit for bit in tests/golden/dispatch_sizes_bits.json (recorded on the MI355X from the commit before
that change by `hashes` below: HYPERMVAR_RECORD_DISPATCH_BITS=1 makes the test write the file instead of reading it).

What can go wrong is host code -- a wrong tile count, a wrong block size, a swapped bool -- so the shapes are the smallest
at which that shows: m = 3, 17, 33, 49 (padded to 16, 32, 48, 64), p = 3, n = 96, 5 windows over 2 recordings of T = 400
samples, F = 6 frequencies, whiteness over 4 lags.  Window 4 is nearly collinear (channel 1 = channel 0 + 1e-9 noise inside
that window only), so that the pivoted LU has a window to take at every size; at m = 33 and 49 the window is also shorter
than the m p regressors, so every Gram matrix there is singular, and at m = 33 the guard's LDL^T re-solve gets windows too.

Routes on the commit the file was recorded from (`return_route`: 0 recursion, 1 LDL^T, 2 LU; they are part of the file):
    m = 3, 17   flags 0 and forms 3, 4: 0 0 0 0 0 (window 4 stays with the recursion); FLAG_YW_PIVOTED: 0 0 0 0 2
    m = 33      flags 0 and form 4: 0 0 0 1 0, form 3: 0 1 0 1 0 (the guard's LDL^T); FLAG_YW_PIVOTED: 2 2 2 1 2, behind the
                tiled and the one-launch LDL^T 2 1 2 1 2; with want_logdet 0 0 0 0 0
    m = 49      flags 0: 0 0 0 0 0; FLAG_YW_PIVOTED: 2 2 2 2 2
    every m     FLAG_YW_TILED and FLAG_YW_ONE_LAUNCH alone: 1 1 1 1 1; form 5: 2 2 2 2 2
so the route word of window 4 is 2 wherever the fallback is on (asserted below), and the LDL^T behind the recursion's guard
solves a window at m = 33 only: at the other sizes its launch finds no window flagged and only has to be the right one.
SHA-256 of the raw bytes of every returned array; the input is hashed too.  All @pytest.mark.gpu."""
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_sizes_bits.json")
SIZES = (3, 17, 33, 49)
P, N, T, F, FS, MAX_LAG = 3, 96, 400, 6, 250.0, 4
REC = (0, 0, 0, 1, 1)
START = (0, 150, T - N, 0, 200)
COLLINEAR = 4                                           # the window (recording 1, samples 200 .. 295) with channel 1 ~ channel 0


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
def hashes(m):
    """What tests/golden/dispatch_sizes_bits.json holds for one m: {"input", "routes": {case: [route per window]},
    "cases": {case: {array: SHA-256}}}."""
    rng = np.random.default_rng(2000 + m)
    xh = rng.standard_normal((2, m, T))
    xh[:, :, 1:] += 0.5 * xh[:, :, :-1]                                      # some autocorrelation for the fit to find
    s0 = START[COLLINEAR]
    xh[REC[COLLINEAR], 1, s0:s0 + N] = xh[REC[COLLINEAR], 0, s0:s0 + N] + 1e-9 * rng.standard_normal(N)
    eng = default_engine()
    x = eng.to_device(xh)
    rec = torch.as_tensor(np.asarray(REC, dtype=np.int64)).to(eng.device)
    st = torch.as_tensor(np.asarray(START, dtype=np.int64)).to(eng.device)
    freqs = np.linspace(4.0, 40.0, F)
    out, routes = {}, {}

    def keep(name, res):
        out[name] = {k: _sha(v) for k, v in _flat(res).items()}

    def solve(name, flags, logdet):
        res = eng.yw_solve(R, m, want_logdet=logdet, flags=flags, return_route=True)
        keep(name, res)
        routes[name] = res[4].cpu().tolist()
        return res

    R = eng.lagcov(x, rec, st, N, P)
    keep("lagcov", R)
    forms = {"default": 0, "tiled": _lib.FLAG_YW_TILED, "one_launch": _lib.FLAG_YW_ONE_LAUNCH}
    for name, flags in forms.items():
        for logdet in (False, True):
            solve(f"yw_solve/{name}" + ("/logdet" if logdet else ""), flags, logdet)
    for name, flags in forms.items():                   # (an LU gives no criterion curve: no logdet with the fallback)
        solve(f"yw_solve/{name}/pivoted", flags | _lib.FLAG_YW_PIVOTED, False)
    ar, V = solve("yw_solve/fit", _lib.FLAG_YW_PIVOTED, False)[:2]           # a finite model of every window for K3 on
    try:
        for form in (3, 4, 5):
            assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, form) == 0
            solve(f"yw_solve/form{form}", 0, False)
            if form != 5:                               # form 5 is the LU alone
                solve(f"yw_solve/form{form}/logdet", 0, True)
        for form in (4, 0):
            assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, form) == 0
            keep(f"yw_solve_auto/form{form}", eng.yw_solve_auto(R, m, N, "AIC"))
    finally:
        assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 0) == 0
    tw = eng.twiddles(freqs, FS, P)
    tf = eng.transfer(ar, m, tw, want_P=True, want_H=True, want_A=True)
    keep("transfer", tf)
    keep("transfer/no_A", eng.transfer(ar, m, tw, want_P=True, want_H=True))     # 64 channels: the hand-scheduled body
    keep("complex_inverse", eng.complex_inverse(tf["A"], m))
    keep("spectra", eng.spectra(tf["H"], V, m))
    E = eng.residuals(x, rec, st, N, ar)
    keep("residuals", E)
    n_res = N - P
    i64 = dict(dtype=torch.int64, device=eng.device)
    C = eng.lagcov(E, torch.arange(len(REC), **i64), torch.zeros(len(REC), **i64), n_res, MAX_LAG)
    keep("whiteness", eng.whiteness(C, m, n_res, 1.96 / np.sqrt(n_res)))
    kw = dict(return_ar=True, check=False, flags=_lib.FLAG_YW_PIVOTED)
    keep("sliding_ffdtf", eng.sliding_ffdtf(x, rec, st, N, P, freqs, FS, **kw))
    keep("sliding_ffdtf/unfused_norm", eng.sliding_ffdtf(x, rec, st, N, P, freqs, FS, return_ar=True, check=False,
                                                         flags=_lib.FLAG_YW_PIVOTED | _lib.FLAG_UNFUSED_NORM))
    keep("sliding_ddtf", eng.sliding_ddtf(x, rec, st, N, P, freqs, FS, **kw))
    keep("sliding_ffdtf_spectra", eng.sliding_ffdtf_spectra(x, rec, st, N, P, freqs, FS, check=False,
                                                            flags=_lib.FLAG_YW_PIVOTED))
    torch.cuda.synchronize()
    return {"input": _sha(xh), "routes": routes, "cases": out}


@pytest.mark.parametrize("m", SIZES)
def test_pinned_bits(m):
    """Every array of every call above, bit for bit what the commit before the change gave, and the routes of the
    docstring.  The input is hashed too, so that a mismatch says which side moved."""
    got, key = hashes(m), str(m)
    if os.environ.get("HYPERMVAR_RECORD_DISPATCH_BITS"):
        recorded = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        recorded[key] = got
        with open(GOLDEN, "w") as fh:
            json.dump(recorded, fh, indent=1, sort_keys=True)
            fh.write("\n")
    with open(GOLDEN) as fh:
        want = json.load(fh)[key]
    print(m, "routes", got["routes"])
    assert got["input"] == want["input"], "numpy's generator no longer reproduces the recorded input"
    assert got["routes"] == want["routes"]
    assert all(r[COLLINEAR] == 2 for name, r in got["routes"].items() if name.endswith("pivoted") or name.endswith("form5"))
    assert sorted(got["cases"]) == sorted(want["cases"])
    moved = [f"{case}:{k}" for case in want["cases"] for k in sorted(set(want["cases"][case]) | set(got["cases"][case]))
             if got["cases"][case].get(k) != want["cases"][case].get(k)]
    assert not moved, f"bits moved: {moved}"
    assert len(got["cases"]) == 28 and all(len(v) >= 1 for v in got["cases"].values())
