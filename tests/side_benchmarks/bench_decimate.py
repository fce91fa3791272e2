"""Side measurement of the FIR decimation kernel (csrc/decimate.hip, `Engine.decimate`) on one MI355X.  Nothing is asserted.

  * copy ratio: kernel time for 2 recordings x 64 channels x 300 000 samples at q = 4 (81 taps) against `x.clone()` of the
    same tensor in the same process -- a plain copy reads the 8 T bytes per row the kernel must read and writes 8 T, the
    kernel writes 8 T / q; both timed with device events around --batch back-to-back launches, median of --reps;
  * host comparison: `scipy.signal.decimate(x, 4, ftype='fir', zero_phase=True)` on the same array on the host;
  * the ill-conditioned story at the north-star shape (64 channels, 599 windows): `band_limited_dyad` low-passed at 45 Hz and
    30 Hz -- `yw_routes` counts, failed windows and band windows/s at 500 Hz with 1000-sample windows and p = 8, pivoted
    fallback off and on (as bench_ill_conditioned.py), and after `Engine.decimate(q=4)` with 250-sample windows and p = 2
    (the same 16 ms of lags), the decimation inside the timed region.  Both use the same 256 frequencies below 62.5 Hz;
  * the register / LDS / scratch table of the new kernel from tools/kernel_resources.py.

    python tests/side_benchmarks/bench_decimate.py --out profiles/decimate_bench.json [--reps 5] [--batch 50] [--kernel-only]
    python tests/side_benchmarks/bench_decimate.py --resources --out profiles/decimate_bench.json   (no GPU)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N_REC, M_CH, T, Q = 2, 64, 300_000, 4
N_WIN, WIN, P, F, FS = 599, 1000, 8, 256, 500.0
CUTOFFS = (45.0, 30.0)


def kernel_resources():
    """tools/kernel_resources.py on the built library: the rows of decimate.hip."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        if "decimate_kernel" in line:
            sig, *cols = line.rsplit(None, 7)                       # the demangled signature, then seven numbers
            name = sig.split("(")[0].split("::")[-1]
            vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in cols)
            rows[name] = {"vgpr": vgpr, "agpr": agpr, "sgpr": sgpr, "vgpr_spill": vspill, "sgpr_spill": sspill,
                          "scratch_bytes": scratch, "static_lds_bytes": lds}
    return rows


def run(args):
    import torch
    from scipy.signal import decimate as sp_decimate
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine, route_counts
    from hyperscanning_signal_analysis_amd.sliding import regular_grid, window_items, window_positions
    from hyperscanning_signal_analysis_amd.synthetic import band_limited_dyad

    off, on = Engine(pivoted_yw=False), Engine(pivoted_yw=True)
    lib = off.lib

    def event_ms(fn):
        """ms per call: device events around args.batch back-to-back launches, median of args.reps"""
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / args.batch)
        return float(np.median(ts))

    def wall_s(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    # ---- the kernel against a copy of its input
    xh = np.random.default_rng(0).standard_normal((N_REC, M_CH, T))
    xd = off.to_device(xh)
    T_out = -(-T // Q)
    y = off.empty(N_REC, M_CH, T_out)
    n_taps = 20 * Q + 1
    dec_ms = event_ms(lambda: off.decimate(xd, Q, out=y))
    clone_ms = event_ms(lambda: xd.clone())
    rows = N_REC * M_CH
    res = {"copy_ratio": {
        "shape": {"recordings": N_REC, "channels": M_CH, "samples": T, "q": Q, "taps": n_taps,
                  "outputs_per_workgroup": int(lib.hmv_decimate_tile(Q, n_taps))},
        "reps": args.reps, "launches_per_rep": args.batch,
        "decimate_ms": dec_ms, "clone_ms": clone_ms, "decimate_over_clone": dec_ms / clone_ms,
        "decimate_bytes": 8 * rows * (T + T_out), "clone_bytes": 16 * rows * T,
        "decimate_GB_per_s": 8 * rows * (T + T_out) / dec_ms / 1e6, "clone_GB_per_s": 16 * rows * T / clone_ms / 1e6,
        "decimate_GFMA_per_s": rows * T_out * n_taps / dec_ms / 1e6}}
    print(f"copy ratio: {res['copy_ratio']}", flush=True)
    ts = []
    for _ in range(max(1, min(args.reps, 3))):
        t0 = time.perf_counter()
        yh = sp_decimate(xh, Q, ftype="fir", zero_phase=True, axis=-1)
        ts.append(time.perf_counter() - t0)
    res["host_scipy"] = {"call": "scipy.signal.decimate(x, 4, ftype='fir', zero_phase=True, axis=-1)", "ms": float(np.median(ts)) * 1e3,
                         "over_kernel": float(np.median(ts)) * 1e3 / dec_ms,
                         "max_abs_diff_to_device": float(np.abs(yh - y.cpu().numpy()).max())}
    print(f"host: {res['host_scipy']}", flush=True)
    del xd, y
    prop = torch.cuda.get_device_properties(0)
    res["measured_on"] = {"name": torch.cuda.get_device_name(0), "gfx_arch": prop.gcnArchName.split(":")[0],
                          "compute_units": prop.multi_processor_count}
    if args.kernel_only:
        return res

    # ---- the ill-conditioned story
    freqs = 0.24 * np.arange(1, F + 1)                                # 256 points up to 61.44 Hz: below fs / (2 q) = 62.5 Hz
    fd = off.to_device(freqs)
    lo, hi = hd.band_bins(freqs)
    pos, w = window_positions(T, N_WIN, WIN)
    rec, st = window_items(1, pos, off.device)
    grid = regular_grid(pos, w, P)
    Wd, Pd = WIN // Q, P // Q
    pos_d, wd = window_positions(T_out, N_WIN, Wd)
    rec_d, st_d = window_items(1, pos_d, off.device)
    grid_d = regular_grid(pos_d, wd, Pd)
    res["ill_conditioned"] = {"shape": {"channels": M_CH, "windows": N_WIN, "F": F, "bands": len(lo),
                                        "full_rate": {"fs": FS, "window": WIN, "hop": int(grid[0]), "p": P},
                                        "decimated": {"q": Q, "fs": FS / Q, "window": Wd, "hop": int(grid_d[0]), "p": Pd}}}

    def bands(eng, x1):
        return eng.sliding_ffdtf(x1, rec, st, w, P, fd, FS, grid=grid, bands=(lo, hi), check="mask")

    def bands_decimated(eng, x1):
        return eng.sliding_ffdtf(eng.decimate(x1, Q), rec_d, st_d, wd, Pd, fd, FS / Q, grid=grid_d, bands=(lo, hi), check="mask")

    for fc in CUTOFFS:
        x1 = off.to_device(band_limited_dyad(0, M_CH, T, fs=FS, high_cutoff_hz=fc, p=P)[None])
        row = {}
        route, info = on.window_routes(x1, rec, st, w, P)
        row["full_rate"] = {"yw_routes": route_counts(route), "lu_info_nonzero": int((info != 0).sum())}
        route, info = on.window_routes(on.decimate(x1, Q), rec_d, st_d, wd, Pd)
        row["decimated"] = {"yw_routes": route_counts(route), "lu_info_nonzero": int((info != 0).sum())}
        for leg, fn in (("full_rate", bands), ("decimated", bands_decimated)):
            for name, eng in (("off", off), ("on", on)):
                out, bad = fn(eng, x1)
                row[leg][f"failed_windows_{name}"] = int(bad.sum())
                row[leg][f"band_windows_per_s_{name}"] = N_WIN / wall_s(lambda eng=eng, fn=fn: fn(eng, x1))
        res["ill_conditioned"][f"{fc:g}Hz"] = row
        print(f"low-pass {fc:g} Hz: {row}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back launches between the two device events")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="the copy ratio and the host comparison alone")
    ap.add_argument("--resources", action="store_true", help="the kernel table alone: no GPU, no timing")
    args = ap.parse_args()
    res = {"status": "not yet measured: kernel resources only"} if args.resources else run(args)
    res["expectation"] = ("the kernel is bound by the 8 T bytes per row it reads: its time is compared with a plain copy of its "
                          "input; no rate is promised and none is a pass criterion")
    res["kernel_resources"] = kernel_resources()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
