#!/usr/bin/env python3
"""K2's default form alone (64 channels, p = 8) at several batch sizes, timed with HIP events: one JSON line.
For an A/B of two builds on one box run it once per build with HYPERMVAR_LIB naming the library, alternating.
    python tools/dbg/k2_sizes.py [--form N] [--reps N] [--once] [sizes ...]      (default sizes 128 599 4792)
--once: one untimed launch per size and nothing else (for a counter run, which serialises the kernels)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from hyperscanning_signal_analysis_amd import _lib                                     # noqa: E402
from hyperscanning_signal_analysis_amd.engine import Engine                            # noqa: E402
from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("sizes", type=int, nargs="*", default=[128, 599, 4792])
ap.add_argument("--form", type=int, default=0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--once", action="store_true")
a = ap.parse_args()
m, p, n, hop = 64, 8, 1000, 13          # K2's time does not depend on the overlap of its windows: a short recording
nmax = max(a.sizes)
eng = Engine()
x = synthetic_var_dyad(0, m=m, p=p, T=n + hop * nmax, fs=500.0)
xd = eng.to_device(x[None])
rec = torch.zeros(nmax, dtype=torch.int64, device=eng.device)
st = hop * torch.arange(nmax, dtype=torch.int64, device=eng.device)
R = eng.lagcov(xd, rec, st, n, p)
mp = eng.pad(m)
ws = torch.zeros(nmax * int(eng.lib.hmv_yw_workspace_doubles(m, p)), dtype=torch.float64, device=eng.device)
ar, V, info = eng.empty(nmax, mp, mp, p), eng.empty(nmax, mp, mp), eng.empty(nmax, dtype=torch.int32)
assert eng.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, a.form) == 0
res = {"lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)), "form": a.form}
for nw in a.sizes:
    def run():
        rc = eng.lib.hmv_yw_solve_f64(R.data_ptr(), nw, m, p, ws.data_ptr(), ar.data_ptr(), V.data_ptr(), 0, info.data_ptr(),
                                      0, eng.stream())
        assert rc == 0
    run()
    torch.cuda.synchronize()
    if a.once:
        continue
    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    res[f"ms_{nw}"] = round(e0.elapsed_time(e1) / a.reps, 4)
    res[f"bad_{nw}"] = int((info[:nw] != 0).sum())
print(json.dumps(res))
