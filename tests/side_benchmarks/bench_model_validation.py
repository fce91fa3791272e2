"""Side measurement of the model-validation path (`Engine.residuals`, K1 over the residuals, `Engine.whiteness`,
`Engine.model_validation`) on one MI355X, at two shapes:
  northstar   599 windows x 64 channels x 1000 samples (one dyad, 50 % overlap), p = 8, h = 20
  config4     10 000 windows x 4 channels x 160 samples, p = 5, h = 12
In one process, timed with device events around the stages: the fit alone (K1 + K2), the three stages of the validation
one by one and the one-call form, and for scale the existing `sliding_ffdtf` band call on the same windows.  A warm-up
call, then the median of --reps runs.

    python tests/side_benchmarks/bench_model_validation.py --out profiles/model_validation_bench.json
    python tests/side_benchmarks/bench_model_validation.py --resources --out profiles/model_validation_bench.json   (no GPU)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"northstar": dict(m=64, n=1000, hop=500, T=300_000, n_rec=1, p=8, h=20, F=256, fs=500.0),
          "config4": dict(m=4, n=160, hop=160, T=160 * 2000, n_rec=5, p=5, h=12, F=32, fs=8.0)}


def event_timed(call, reps):
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions, regular_grid, window_items
    from hyperscanning_signal_analysis_amd.synthetic import northstar_freqs, synthetic_var_dyad

    eng = Engine()
    res = {"reps": args.reps, "shapes": {}, "milliseconds": {}, "ratios": {}}
    for name, sh in SHAPES.items():
        m, n, hop, T, n_rec, p, h, F, fs = (sh[k] for k in ("m", "n", "hop", "T", "n_rec", "p", "h", "F", "fs"))
        if name == "northstar":
            x = np.stack([synthetic_var_dyad(d, m=m, p=p, T=T, fs=fs) for d in range(n_rec)])
            freqs = northstar_freqs(F)
            lo, hi = hd.band_bins(freqs)
        else:                                        # many short windows: coloured noise is enough to time them
            x = np.random.default_rng(5).standard_normal((n_rec, m, T))
            x[..., 1:] += 0.5 * x[..., :-1]
            x[:, 1:] += 0.3 * x[:, :-1]
            freqs = np.linspace(fs / (2 * F), fs / 2, F)
            lo, hi = np.array([0, F // 2]), np.array([F // 2, F])
        xd = eng.to_device(x)
        pos = hop_positions(T, n, hop)
        rec, st = window_items(n_rec, pos, eng.device)
        items = int(rec.numel())
        fd = eng.to_device(freqs)
        grid = regular_grid(pos, n, p) if n_rec == 1 else None
        N = n - p
        thr = 1.96 / float(np.sqrt(N))
        ar = eng.yw_solve(eng.lagcov(xd, rec, st, n, p), m)[0]
        E = eng.residuals(xd, rec, st, n, ar, validate=False)
        idx = torch.arange(items, dtype=torch.int64, device=eng.device)
        zero = torch.zeros_like(idx)
        C = eng.lagcov(E, idx, zero, N, h)
        ms = {
            "fit (K1 + K2)": event_timed(lambda: eng.yw_solve(eng.lagcov(xd, rec, st, n, p), m), args.reps),
            "validation/residuals": event_timed(lambda: eng.residuals(xd, rec, st, n, ar, validate=False), args.reps),
            "validation/lagcov of residuals": event_timed(lambda: eng.lagcov(E, idx, zero, N, h), args.reps),
            "validation/whiteness": event_timed(lambda: eng.whiteness(C, m, N, thr), args.reps),
            "validation/one call": event_timed(lambda: eng.model_validation(xd, rec, st, n, ar, h, validate=False), args.reps),
            "sliding_ffdtf bands": event_timed(lambda: eng.sliding_ffdtf(xd, rec, st, n, p, fd, fs, bands=(lo, hi), check=False,
                                                                         grid=grid, validate=False), args.reps),
        }
        res["shapes"][name] = dict(sh, windows=items)
        res["milliseconds"][name] = ms
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res["ratios"][name] = {"validation / sliding_ffdtf bands": med["validation/one call"] / med["sliding_ffdtf bands"],
                               "validation / fit": med["validation/one call"] / med["fit (K1 + K2)"]}
        for k, v in med.items():
            print(f"{name:10s} {k:34s} {v:10.3f} ms", flush=True)
    return res


def resources(res):
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in txt.splitlines():
        if "resid_" in line or "whiteness_kernel" in line:
            name, vals = line[:70].strip(), line[70:].split()
            rows[name] = {"vgpr": int(vals[0]), "sgpr": int(vals[2]), "vgpr_spill": int(vals[3]), "sgpr_spill": int(vals[4]),
                          "scratch_bytes": int(vals[5]), "lds_bytes": int(vals[6])}
    res["kernel_resources"] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="add tools/kernel_resources.py's figures to --out (no GPU)")
    args = ap.parse_args()
    if args.resources:
        res = resources(json.load(open(args.out)) if args.out and os.path.exists(args.out) else {})
    else:
        res = run(args)
        if args.out and os.path.exists(args.out):                     # keep what a --resources run recorded
            old = json.load(open(args.out))
            if "kernel_resources" in old:
                res["kernel_resources"] = old["kernel_resources"]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("ratios",) if k in res}))


if __name__ == "__main__":
    main()
