"""Side measurement of the per-window automatic model order (`p=None`, hmv_sliding_auto_f64) on one MI355X, at two shapes:

  (a) 599 windows x 64 channels x 1000 samples, hop 500, F = 256, pmax = 8, AIC, on the 64-channel mixed-order
      recording (`synthetic.mixed_order_recording`) made long enough for 599 windows;
  (b) the reference's own shape: 4 channels, n = 160, hop 80, F = 30, pmax = 20, AIC, 10 000 windows.

For each shape and each measure (ffDTF full, ffDTF bands, dDTF, GPDC) windows/s of
  (i)   the one-call route: `sliding_<measure>(..., p=None)`;
  (ii)  the two-pass route, built only from calls that exist without the feature: `Engine.lagcov` +
        `yw_solve(want_logdet=True)` at pmax, download of the log determinants, arg-min of the criterion on the host, one
        `sliding_<measure>(..., p=q)` call per order group (each group's windows are no regular grid any more);
  (iii) the fixed-order call at p = pmax on the same windows (what the selection costs: (i) / (iii)),
median of --reps repetitions in one process, warm-up excluded.

    python tests/side_benchmarks/bench_auto_order.py --out result.json [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tests/side_benchmarks/bench_auto_order.py --reps 1
    python tests/side_benchmarks/bench_auto_order.py --merge-stats DIR/.../run_kernel_stats.csv --out result.json
    python tests/side_benchmarks/bench_auto_order.py --resources --out result.json      (no GPU: registers, LDS, occupancy)

(--only-auto profiles the one-call route alone.)"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {
    "a_64ch": dict(m=64, n=1000, hop=500, F=256, pmax=8, windows=599, orders=[1, 2, 4, 6], fs=500.0),
    "b_4ch": dict(m=4, n=160, hop=80, F=30, pmax=20, windows=10_000, orders=[1, 2, 3, 5, 8, 12], fs=100.0),
}
CRIT = "AIC"


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions, regular_grid, window_items
    from hyperscanning_signal_analysis_amd.synthetic import mixed_order_recording, northstar_freqs

    eng = Engine()
    res = {"crit": CRIT, "reps": args.reps, "shapes": {}}
    for tag, sh in SHAPES.items():
        m, n, hop, F, pmax, W = sh["m"], sh["n"], sh["hop"], sh["F"], sh["pmax"], sh["windows"]
        T = (W - 1) * hop + n
        seg = -(-T // len(sh["orders"]))
        x = mixed_order_recording(100, m, sh["orders"], seg)[:, :T]
        xd = eng.to_device(x[None])
        pos = hop_positions(T, n, hop)
        assert len(pos) == W
        rec, st = window_items(1, pos, eng.device)
        grid = regular_grid(pos, n, pmax)
        freqs = northstar_freqs(F) if F == 256 else np.linspace(1.0, 45.0, F)
        fd = eng.to_device(freqs)
        lo, hi = hd.band_bins(freqs)
        pen = 2.0 * np.arange(1, pmax + 1) * m * m / n

        def two_pass(fn, **kw):
            R = eng.lagcov_regular(xd[0], int(pos[0]), hop, W, n, pmax) if grid else eng.lagcov(xd, rec, st, n, pmax)
            _, _, logdet, info = eng.yw_solve(R, m, want_logdet=True)
            crit = logdet.cpu().numpy() + pen                    # the host round trip of the two-pass route
            orders = 1 + np.argmin(crit, axis=1)
            outs = {}
            for q in np.unique(orders):
                sel = torch.as_tensor(np.nonzero(orders == q)[0], device=eng.device)
                outs[int(q)] = fn(xd, rec[sel], st[sel], n, int(q), fd, sh["fs"], check=False, **kw)
            return orders, outs

        measures = {
            "ffdtf": (eng.sliding_ffdtf, {}),
            "ffdtf_bands": (eng.sliding_ffdtf, dict(bands=(lo, hi))),
            "ddtf": (eng.sliding_ddtf, {}),
            "gpdc": (eng.sliding_gpdc, {}),
        }
        out = {"shape": dict(sh, bands=len(lo)), "seconds": {}, "windows_per_s": {}, "ratios": {}}
        orders_auto = None
        for name, (fn, kw) in measures.items():
            routes = {"auto": lambda: fn(xd, rec, st, n, None, fd, sh["fs"], max_model_order=pmax, crit_type=CRIT, grid=grid,
                                         check=False, return_orders=True, **kw)}
            if not args.only_auto:
                routes["two_pass"] = lambda: two_pass(fn, **kw)
                routes["fixed_pmax"] = lambda: fn(xd, rec, st, n, pmax, fd, sh["fs"], grid=grid, check=False, **kw)
            for route, call in routes.items():
                r = call()
                torch.cuda.synchronize()
                if route == "auto":
                    orders_auto = r[1].cpu().numpy()
                elif route == "two_pass":
                    assert np.array_equal(r[0], orders_auto), "the two routes disagree on the orders"
                del r
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                key = f"{name}/{route}"
                out["seconds"][key] = ts
                out["windows_per_s"][key] = W / float(np.median(ts))
                print(f"{tag:7s} {key:24s} {np.median(ts) * 1e3:9.2f} ms  {out['windows_per_s'][key]:12,.0f} windows/s", flush=True)
            if not args.only_auto:
                wps = out["windows_per_s"]
                out["ratios"][name] = {"auto_over_two_pass": wps[f"{name}/auto"] / wps[f"{name}/two_pass"],
                                       "auto_over_fixed_pmax": wps[f"{name}/auto"] / wps[f"{name}/fixed_pmax"]}
        out["orders_picked"] = np.bincount(orders_auto, minlength=pmax + 1).tolist()
        res["shapes"][tag] = out
        del xd
        torch.cuda.empty_cache()
    return res


def merge_stats(path, res):
    """rocprofv3 --stats kernel table of ONE profiled run (--reps 1) -> calls, average and total ms per kernel."""
    table = {}
    for r in csv.DictReader(open(path)):
        table[r["Name"][:120]] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) * 1e-6,
                                  "total_ms": float(r["TotalDurationNs"]) * 1e-6}
    res["kernel_stats_one_profiled_run"] = table
    return res


def resources(res):
    """Registers, LDS and the workgroups per CU they allow, of the selecting kernel and of the fixed-order recursion."""
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in txt.splitlines():
        if "yw_auto_kernel" in line or "yw_lwr_kernel" in line:
            name, vals = line[:70].strip(), line[70:].split()
            vgpr, lds = int(vals[0]), int(vals[6])
            # 512 VGPRs per SIMD lane, 4 waves per workgroup on 4 SIMDs; 160 KB of LDS per CU
            rows[name] = {"vgpr": vgpr, "sgpr": int(vals[2]), "vgpr_spill": int(vals[3]), "sgpr_spill": int(vals[4]),
                          "scratch_bytes": int(vals[5]), "lds_bytes": lds,
                          "workgroups_per_cu": min(512 // max(vgpr, 1), (160 * 1024) // max(lds, 1))}
    res["kernel_resources"] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-auto", action="store_true", help="the one-call route alone")
    ap.add_argument("--merge-stats", default=None, help="kernel_stats.csv of a rocprofv3 run: merged into --out (no GPU)")
    ap.add_argument("--resources", action="store_true", help="add tools/kernel_resources.py's figures to --out (no GPU)")
    args = ap.parse_args()
    if args.merge_stats or args.resources:
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        if args.merge_stats:
            res = merge_stats(args.merge_stats, res)
        if args.resources:
            res = resources(res)
    else:
        res = run(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({t: {"windows_per_s": s["windows_per_s"], "ratios": s["ratios"]} for t, s in res.get("shapes", {}).items()}))


if __name__ == "__main__":
    main()
