"""Side measurement of K2's pivoted fallback (csrc/yw_lu.hip, `Engine(pivoted_yw=True)`) at the north-star shape (599
windows of 64 ch x 1000 samples, hop 500, p = 8, F = 256, 5 bands, one MI355X):

  * band-limited recordings (`synthetic.band_limited_dyad`, low-pass 45 Hz and 30 Hz at fs = 500): how many windows each K2
    solver takes (`Engine.window_routes`), how many windows fail with the option off and on, band-sum windows/s of
    `sliding_ffdtf` off and on;
  * the well-conditioned benchmark recording: windows/s with the option on against off in the same process -- the extra
    cost should be one launch of workgroups that read one int; it is reported, not asserted;
  * the LU kernel alone (HMV_TUNE_YW_FORM = 5): time of a batch of one window per compute unit, i.e. the time one
    workgroup needs for one window, and of the whole 599-window batch;
  * the register / LDS / scratch table of the new kernels from tools/kernel_resources.py.

    python tests/side_benchmarks/bench_ill_conditioned.py --out profiles/ill_conditioned_bench.json [--reps 5]
    python tests/side_benchmarks/bench_ill_conditioned.py --resources --out profiles/ill_conditioned_bench.json   (no GPU)
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

M_CH, N_WIN, WIN, P, F, FS, T = 64, 599, 1000, 8, 256, 500.0, 300_000
CUTOFFS = (45.0, 30.0)


def kernel_resources():
    """tools/kernel_resources.py on the built library: the rows of yw_lu.hip."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        if "yw_lu_kernel" in line or "yw_route_" in line:
            sig, *cols = line.rsplit(None, 7)                       # the demangled signature, then seven numbers
            name = sig.split("(")[0].split("::")[-1]
            vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in cols)
            rows[name] = {"vgpr": vgpr, "agpr": agpr, "sgpr": sgpr, "vgpr_spill": vspill, "sgpr_spill": sspill,
                          "scratch_bytes": scratch, "static_lds_bytes": lds}
    return rows


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine, route_counts
    from hyperscanning_signal_analysis_amd.sliding import regular_grid, window_items, window_positions
    from hyperscanning_signal_analysis_amd.synthetic import band_limited_dyad, northstar_freqs, synthetic_var_dyad

    off, on = Engine(pivoted_yw=False), Engine(pivoted_yw=True)
    pos, w = window_positions(T, N_WIN, WIN)
    rec, st = window_items(1, pos, off.device)
    grid = regular_grid(pos, w, P)
    freqs = northstar_freqs(F)
    fd = off.to_device(freqs)
    lo, hi = hd.band_bins(freqs)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    def bands(eng, xd):
        return eng.sliding_ffdtf(xd, rec, st, w, P, fd, FS, grid=grid, bands=(lo, hi), check="mask")

    res = {"shape": {"channels": M_CH, "windows": N_WIN, "window": WIN, "hop": int(grid[0]), "p": P, "F": F, "bands": len(lo)},
           "reps": args.reps, "band_limited": {}}
    for fc in CUTOFFS:
        xd = off.to_device(band_limited_dyad(0, M_CH, T, fs=FS, high_cutoff_hz=fc, p=P)[None])
        route, info = on.window_routes(xd, rec, st, w, P)
        row = {"routes": route_counts(route), "lu_info_nonzero": int((info != 0).sum())}
        for name, eng in (("off", off), ("on", on)):
            out, bad = bands(eng, xd)
            row[f"failed_windows_{name}"] = int(bad.sum())
            row[f"nonfinite_windows_{name}"] = int((~torch.isfinite(out).all(dim=(1, 2, 3)) & ~bad).sum())
            sec = timed(lambda eng=eng, xd=xd: bands(eng, xd))
            row[f"band_windows_per_s_{name}"] = N_WIN / sec
        res["band_limited"][f"{fc:g}Hz"] = row
        print(f"low-pass {fc:g} Hz: {row}", flush=True)

    xd = off.to_device(synthetic_var_dyad(0, m=M_CH, p=P, T=T, fs=FS)[None])
    route, _ = on.window_routes(xd, rec, st, w, P)
    well = {"routes": route_counts(route)}
    for name, eng in (("off", off), ("on", on)):
        well[f"band_windows_per_s_{name}"] = N_WIN / timed(lambda eng=eng: bands(eng, xd))
    well["on_over_off"] = well["band_windows_per_s_on"] / well["band_windows_per_s_off"]
    res["well_conditioned"] = well
    print(f"well conditioned: {well}", flush=True)

    # the LU kernel alone
    R = off.lagcov(xd, rec, st, w, P)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lu = {}
    assert off.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 5) == 0
    try:
        for name, n in (("one_window_per_cu", min(cus, N_WIN)), ("all_windows", N_WIN)):
            Rn = R[:n].contiguous()
            sec = timed(lambda Rn=Rn: off.yw_solve(Rn, M_CH))
            lu[name] = {"windows": n, "ms": sec * 1e3, "ms_per_window_of_the_batch": sec * 1e3 / n}
    finally:
        assert off.lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 0) == 0
    sec = timed(lambda: off.yw_solve(R, M_CH))
    lu["default_solver_all_windows_ms"] = sec * 1e3
    res["lu_kernel"] = lu
    print(f"LU alone: {lu}", flush=True)
    prop = torch.cuda.get_device_properties(0)
    res["measured_on"] = {"name": torch.cuda.get_device_name(0), "gfx_arch": prop.gcnArchName.split(":")[0],
                          "compute_units": prop.multi_processor_count}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="the kernel table alone: no GPU, no timing")
    args = ap.parse_args()
    res = {"status": "not yet measured: kernel resources only"} if args.resources else run(args)
    res["expectation"] = ("with the option on, a well-conditioned batch pays one launch of workgroups that read one int; "
                          "no rate is promised and none is a pass criterion")
    res["kernel_resources"] = kernel_resources()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
