"""Side measurement of sliding-window block Granger causality at the north-star shape (599 windows of 64 ch x 1000
samples, hop 500, split 32, p = 8, F = 256, one MI355X): windows/s of `Engine.sliding_block_granger`, full and with 5
bands, beside `sliding_ffdtf` timed in the same process -- the expectation to record against is "about one
`sliding_ffdtf` call" -- and the register / LDS table of the new kernels from tools/kernel_resources.py.

    python tests/side_benchmarks/bench_block_gc.py --out profiles/block_gc_bench.json [--reps 5]
    python tests/side_benchmarks/bench_block_gc.py --resources-only --out profiles/block_gc_bench.json      (no GPU)

The per-kernel times of one profiled run are kept beside it in profiles/block_gc_kernel_times.json: this script does not
write that file."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

M_CH, SPLIT, N_WIN, WIN, P, F, FS, T = 64, 32, 599, 1000, 8, 256, 500.0, 300_000


def kernel_resources():
    """tools/kernel_resources.py on the built library, the rows of block_gc.hip (and the factor kernel it shares)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        if "bgc_" in line or "ddtf_factor_kernel" in line:
            sig, *cols = line.rsplit(None, 7)                       # the demangled signature, then seven numbers
            name = sig.split("(")[0].split("::")[-1]
            vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in cols)
            rows[name] = {"vgpr": vgpr, "agpr": agpr, "sgpr": sgpr, "vgpr_spill": vspill, "sgpr_spill": sspill,
                          "scratch_bytes": scratch, "static_lds_bytes": lds}
    if "bgc_freq_kernel" in rows:
        ns = max(SPLIT, M_CH - SPLIT)
        slab = ns * (ns | 1) * 16
        wpb = max(1, min(4, 65536 // slab))
        rows["bgc_freq_kernel"]["dynamic_lds_bytes_at_this_shape"] = wpb * slab
        rows["bgc_freq_kernel"]["waves_per_workgroup_at_this_shape"] = wpb
    return rows


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
    cases = {
        "ffdtf": lambda: eng.sliding_ffdtf(xd, rec, st, w, P, fd, FS, out=out_full, grid=grid, check=False),
        "block_gc": lambda: eng.sliding_block_granger(xd, rec, st, w, P, fd, FS, split=SPLIT, grid=grid, check=False),
        "block_gc_bands": lambda: eng.sliding_block_granger(xd, rec, st, w, P, fd, FS, split=SPLIT, grid=grid, check=False,
                                                            bands=(lo, hi)),
    }
    res = {"shape": {"channels": M_CH, "split": SPLIT, "windows": N_WIN, "window": WIN, "hop": int(grid[0]), "p": P, "F": F,
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
        res["seconds"][name] = ts
        res["windows_per_s"][name] = N_WIN / float(np.median(ts))
        print(f"{name:15s} {np.median(ts) * 1e3:9.2f} ms  {res['windows_per_s'][name]:10,.0f} windows/s", flush=True)
    res["block_gc_time_over_ffdtf_time"] = float(np.median(res["seconds"]["block_gc"]) / np.median(res["seconds"]["ffdtf"]))
    prop = torch.cuda.get_device_properties(0)
    res["measured_on"] = {"name": torch.cuda.get_device_name(0), "gfx_arch": prop.gcnArchName.split(":")[0],
                          "compute_units": prop.multi_processor_count}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources-only", action="store_true", help="the kernel table alone: no GPU, no timing")
    args = ap.parse_args()
    res = {"status": "not yet measured: kernel resources only"} if args.resources_only else run(args)
    res["expectation"] = "about one sliding_ffdtf call; no rate is promised and none is a pass criterion"
    res["kernel_resources"] = kernel_resources()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "seconds"}))


if __name__ == "__main__":
    main()
