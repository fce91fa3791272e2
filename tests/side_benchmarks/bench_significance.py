"""Side measurement of the surrogate significance test (`Engine.sliding_significance`) at the north-star shape: one
recording of 64 ch x 300 000 samples at 500 Hz, 599 windows of 1000 samples (hop 500), p = 8, F = 256, DEFAULT_BANDS,
S = 100 surrogates.  Runs ffDTF under both nulls and dDTF / GPDC under the shift null; reports surrogate windows/s
(S x 599 over synchronised wall time, draws and uploads included) beside the plain band rate of the same measure,
measured in the same process.

    python tests/side_benchmarks/bench_significance.py --out result.json
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tests/side_benchmarks/bench_significance.py --surrogates 10
    python tests/side_benchmarks/bench_significance.py --merge-stats DIR/.../run_kernel_stats.csv --out result.json

The last form (no GPU) adds the per-kernel times of the profiled run."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

M_CH, N_WIN, WIN, P, F, FS, T = 64, 599, 1000, 8, 256, 500.0, 300_000
CASES = (("ffdtf", "shift"), ("ffdtf", "phase"), ("ddtf", "shift"), ("gpdc", "shift"))


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import regular_grid, window_items, window_positions
    from hyperscanning_signal_analysis_amd.synthetic import northstar_freqs, synthetic_var_dyad

    eng = Engine()
    x = synthetic_var_dyad(0, m=M_CH, p=P, T=T, fs=FS)
    xd = eng.to_device(x[None])
    pos, w = window_positions(T, N_WIN, WIN)
    rec, st = window_items(1, pos, eng.device)
    grid = regular_grid(pos, w, P)
    freqs = northstar_freqs(F)
    fd = eng.to_device(freqs)
    lo, hi = hd.band_bins(freqs)
    S = int(args.surrogates)
    plain = {"ffdtf": eng.sliding_ffdtf, "ddtf": eng.sliding_ddtf, "gpdc": eng.sliding_gpdc}
    res = {"shape": {"channels": M_CH, "windows": N_WIN, "window": WIN, "hop": int(grid[0]), "p": P, "F": F,
                     "bands": len(lo), "surrogates": S},
           "plain_band_windows_per_s": {}, "surrogate_windows_per_s": {}, "seconds": {}, "ratio_to_plain": {},
           "block_items": {}}
    cases = [c for c in CASES if args.cases is None or f"{c[0]}_{c[1]}" in args.cases.split(",")]
    for meas in sorted({c[0] for c in cases}):
        fn = plain[meas]
        fn(xd, rec, st, w, P, fd, FS, grid=grid, check=False, bands=(lo, hi))
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn(xd, rec, st, w, P, fd, FS, grid=grid, check=False, bands=(lo, hi))
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res["plain_band_windows_per_s"][meas] = N_WIN / float(np.median(ts))
        print(f"plain {meas:6s} {np.median(ts) * 1e3:9.2f} ms  {res['plain_band_windows_per_s'][meas]:10,.0f} windows/s",
              flush=True)
    for meas, null in cases:
        key = f"{meas}_{null}"

        def sig(n_s):
            return eng.sliding_significance(xd, rec, st, w, P, fd, FS, (lo, hi), measure=meas, null=null, n_surrogates=n_s,
                                            seed=1, check=True, grid=grid)
        sig(2)                                  # warm-up: code objects, FFT plans, the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = sig(S)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert int(r["n_valid"].min()) == S
        res["seconds"][key] = dt
        res["surrogate_windows_per_s"][key] = S * N_WIN / dt
        res["ratio_to_plain"][key] = res["surrogate_windows_per_s"][key] / res["plain_band_windows_per_s"][meas]
        res["block_items"][key] = eng.significance_chunk(meas, null, N_WIN, M_CH, WIN, P, F, len(lo))
        print(f"{key:12s} {dt:8.2f} s  {res['surrogate_windows_per_s'][key]:10,.0f} surrogate windows/s  "
              f"({res['ratio_to_plain'][key]:.3f} x plain)", flush=True)
        del r
    return res


def merge_stats(path, res):
    """rocprofv3 --stats kernel table -> per-kernel ms per call, the surrogate kernels and rocFFT's listed apart."""
    table, new = {}, {}
    for r in csv.DictReader(open(path)):
        row = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) * 1e-6, "total_ms": float(r["TotalDurationNs"]) * 1e-6}
        table[r["Name"][:120]] = row
        if any(k in r["Name"] for k in ("surrogate_", "null_")):
            new[r["Name"].split("(")[0].replace("void ", "")] = row
    res["kernel_stats_one_profiled_run"] = table
    res["new_kernels"] = new
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--surrogates", type=int, default=100)
    ap.add_argument("--cases", default=None, help="comma list of measure_null, default: all four")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None, help="kernel_stats.csv of a rocprofv3 run: merged into --out (no GPU)")
    args = ap.parse_args()
    if args.merge_stats:
        res = merge_stats(args.merge_stats, json.load(open(args.out)))
    else:
        res = run(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k in ("surrogate_windows_per_s", "ratio_to_plain", "new_kernels")}))


if __name__ == "__main__":
    main()
