"""Side measurement of the sliding-window dDTF / GPDC entries at the north-star shape (599 windows of 64 ch x 1000
samples, hop 500, p = 8, F = 256, one MI355X): windows/s of ffDTF, dDTF (full and band sums), GPDC (full and band sums)
and of the chain of batched calls `measures()` of bench_connectivity.py uses for dDTF (K1 -> K2 -> K3 with H and A ->
K4 -> K5 -> inverse of S -> partial coherence -> ffDTF x |kappa|), on the same box in the same process.

    python tests/side_benchmarks/bench_sliding_conn.py --out result.json [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tests/side_benchmarks/bench_sliding_conn.py --reps 1 --no-chain
    python tests/side_benchmarks/bench_sliding_conn.py --merge-stats DIR/.../run_kernel_stats.csv --out result.json

The last form (no GPU) adds the per-kernel times of the profiled run and the achieved TFLOP/s or GB/s of the new
kernels against the MI355X's peaks.  The chain has no chunking of its own; it runs here in batches of 150 windows."""
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
PEAK_F64_TFLOPS = 78.6            # MI355X spec, vector = matrix f64 (bench.py)
PEAK_HBM_GBS = 8000.0             # MI355X spec, HBM3E


def accounting():
    """flop and HBM bytes per window of the new kernels at the shape above (MP = m = 64, D = 2p + 1 = 17)."""
    m, p, D = M_CH, P, 2 * P + 1
    plane = m * m * F * 8
    return {
        "ddtf_factor_kernel": {"flop": 2 * m ** 3 / 3 + 2 * p * m ** 3, "bytes": (p + 1) * m * m * 8 * 2,
                               "note": "chol(V), L^-1, B_k = -L^-1 ar_k"},
        "ddtf_gram_kernel": {"flop": 2 * (p + 1) ** 2 * m ** 3, "bytes": D * m * m * 8,
                             "note": "G_d = sum B_k^T B_l on v_mfma_f64_16x16x4_f64; B re-read from L2"},
        "ddtf_apply_kernel": {"flop": F * (m * (m + 1) // 2) * D * 7, "bytes": 2 * plane,
                              "note": "Horner over D terms per pair i <= j and frequency; reads ffDTF, writes dDTF"},
        "gpdc_sliding_kernel": {"flop": F * m * m * (4 * p + 6), "bytes": plane,
                                "note": "A(f) built on chip, written once as GPDC"},
    }


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
    out_full = eng.empty(N_WIN, M_CH, M_CH, F)

    def chain(sl):
        R = eng.lagcov(xd, rec[sl], st[sl], w, P)
        ar, V, _, _ = eng.yw_solve(R, M_CH)
        t = eng.transfer(ar, M_CH, eng.twiddles(freqs, FS, P), want_P=True, want_H=True, want_A=True)
        ff = eng.normalise(t["P"], t["rowsum"], M_CH)[0]
        S = eng.spectra(t["H"], V, M_CH)
        kappa, _ = eng.partial_coherence(S, M_CH)
        return ff * kappa.abs()

    cases = {
        "ffdtf": lambda: eng.sliding_ffdtf(xd, rec, st, w, P, fd, FS, out=out_full, grid=grid, check=False),
        "ddtf": lambda: eng.sliding_ddtf(xd, rec, st, w, P, fd, FS, out=out_full, grid=grid, check=False),
        "ddtf_bands": lambda: eng.sliding_ddtf(xd, rec, st, w, P, fd, FS, grid=grid, check=False, bands=(lo, hi)),
        "gpdc": lambda: eng.sliding_gpdc(xd, rec, st, w, P, fd, FS, out=out_full, grid=grid, check=False),
        "gpdc_bands": lambda: eng.sliding_gpdc(xd, rec, st, w, P, fd, FS, grid=grid, check=False, bands=(lo, hi)),
    }
    if not args.no_chain:
        cases["chain_ddtf"] = lambda: [chain(slice(a, min(a + 150, N_WIN))) for a in range(0, N_WIN, 150)]
    res = {"shape": {"channels": M_CH, "windows": N_WIN, "window": WIN, "hop": int(grid[0]), "p": P, "F": F,
                     "bands": len(lo)}, "reps": args.reps, "seconds": {}, "windows_per_s": {}}
    for name, fn in cases.items():
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            if name == "chain_ddtf":
                torch.cuda.empty_cache()
        res["seconds"][name] = ts
        res["windows_per_s"][name] = N_WIN / float(np.median(ts))
        print(f"{name:11s} {np.median(ts) * 1e3:9.2f} ms  {res['windows_per_s'][name]:10,.0f} windows/s", flush=True)
    if "chain_ddtf" in res["windows_per_s"]:
        res["ddtf_speedup_vs_chain"] = res["windows_per_s"]["ddtf"] / res["windows_per_s"]["chain_ddtf"]
    return res


def merge_stats(path, res):
    """rocprofv3 --stats kernel table -> per-kernel ms per call; achieved rates of the new kernels."""
    rows = list(csv.DictReader(open(path)))
    acc = accounting()
    table, rates = {}, {}
    for r in rows:
        name = r["Name"].split("(")[0].replace("void ", "").split("<")[0].split("::")[-1]
        calls, avg_ns = int(r["Calls"]), float(r["AverageNs"])
        table[r["Name"][:120]] = {"calls": calls, "avg_ms": avg_ns * 1e-6, "total_ms": float(r["TotalDurationNs"]) * 1e-6}
        if name in acc:
            a = acc[name]
            s = avg_ns * 1e-9
            rates[name] = {"avg_ms": avg_ns * 1e-6, "tflops": a["flop"] * N_WIN / s / 1e12,
                           "frac_of_f64_peak": a["flop"] * N_WIN / s / 1e12 / PEAK_F64_TFLOPS,
                           "gbs": a["bytes"] * N_WIN / s / 1e9, "frac_of_hbm_peak": a["bytes"] * N_WIN / s / 1e9 / PEAK_HBM_GBS,
                           "note": a["note"]}
    res["kernel_stats_one_profiled_run"] = table
    res["new_kernels_achieved"] = rates
    res["peaks"] = {"f64_tflops": PEAK_F64_TFLOPS, "hbm_gbs": PEAK_HBM_GBS}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--merge-stats", default=None, help="kernel_stats.csv of a rocprofv3 run: merged into --out (no GPU)")
    args = ap.parse_args()
    if args.merge_stats:
        res = json.load(open(args.out))
        res = merge_stats(args.merge_stats, res)
    else:
        res = run(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k in ("windows_per_s", "ddtf_speedup_vs_chain", "new_kernels_achieved")}))


if __name__ == "__main__":
    main()
