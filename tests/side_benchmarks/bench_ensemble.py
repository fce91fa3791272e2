"""Side measurement of the event-locked ensemble path (`Engine.sliding_ensemble` / `lagcov_ensemble`) on one MI355X.

Shapes (one recording per group, the group's onsets drawn at random inside it; epochs may overlap):
  A     64 channels, fs 500, 8 groups x 100 trials, 1000-sample epochs, n = 100, hop = 20 (k = 5), p = 8, F = 256: 46 windows
        per group
  A_h5  the same with hop = 5  (hop <= p: the direct form by rule)
  A_h10 the same with hop = 10 (k = 10)
  B     19 channels, fs 250, 32 groups x 60 trials, 400-sample epochs, n = 80, hop = 16 (k = 5), p = 6, F = 64

Routes:
  (i)   the new call, `Engine.sliding_ensemble`, for the ffDTF bands, dDTF and GPDC: with the declared grid (the library
        picks the K1 form) and with `FLAG_DIRECT_LAGCOV`;
  (ii)  K1 alone: `Engine.lagcov_ensemble` (direct, and shared where the rule allows it) against the covariances as the
        library makes them without it -- `Engine.lagcov` on trials x windows single-trial items, group by group, and
        `Engine.trial_mean` per window.  Every later stage is the same code on both routes, so this is where they differ;
  (iii) the host loop over windows through `mtmvar.full_freq_dtf` on (m, n, trials) input, timed on --host-windows windows
        and EXTRAPOLATED to the shape's item count (labelled so in the output).
One process, a warm-up call, the median of --reps synchronised wall times.  The K1 figure in TFLOP/s counts the direct form's
2 MP^2 (p+1) n E flops per item for both forms (the shared form does 1/k of them: its figure is an effective rate).

    python tests/side_benchmarks/bench_ensemble.py --out profiles/ensemble_bench.json [--reps 5] [--shapes A,B]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tests/side_benchmarks/bench_ensemble.py --reps 1 --k1-only --plumbing
    python tests/side_benchmarks/bench_ensemble.py --merge-trace DIR/.../run_kernel_trace.csv --out profiles/ensemble_bench.json
    python tests/side_benchmarks/bench_ensemble.py --resources --out profiles/ensemble_bench.json     (no GPU)"""
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
    "A": dict(m=64, fs=500.0, groups=8, trials=100, L=1000, n=100, hop=20, p=8, F=256, T=60_000),
    "A_h5": dict(m=64, fs=500.0, groups=8, trials=100, L=1000, n=100, hop=5, p=8, F=256, T=60_000),
    "A_h10": dict(m=64, fs=500.0, groups=8, trials=100, L=1000, n=100, hop=10, p=8, F=256, T=60_000),
    "B": dict(m=19, fs=250.0, groups=32, trials=60, L=400, n=80, hop=16, p=6, F=64, T=30_000),
}


def timed(call, reps, sync):
    call()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import _lib, mtmvar as M
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions
    from hyperscanning_signal_analysis_amd.synthetic import northstar_freqs

    eng = Engine()
    sync = torch.cuda.synchronize
    res = {"reps": args.reps, "shapes": {}}
    for tag in args.shapes.split(","):
        sh = SHAPES[tag]
        m, G, E, L, n, hop, p, F, T = (sh[k] for k in ("m", "groups", "trials", "L", "n", "hop", "p", "F", "T"))
        mp = eng.pad(m)
        rng = np.random.default_rng(5)
        x = rng.standard_normal((G, m, T))
        x[..., 1:] += 0.5 * x[..., :-1]
        x[:, 1:] += 0.3 * x[:, :-1]
        xd = eng.to_device(x)
        offsets = hop_positions(L, n, hop)
        W = len(offsets)
        onsets = [np.sort(rng.choice(np.arange(0, T - L + 1), E, replace=False)) for _ in range(G)]
        i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
        d = dict(trial_rec=i64(np.repeat(np.arange(G), E)), trial_start=i64(np.concatenate(onsets)),
                 group_ptr=i64(np.arange(G + 1) * E), item_group=i64(np.repeat(np.arange(G), W)),
                 item_offset=i64(np.tile(offsets, G)))
        items = G * W
        grid = (hop, W)
        shared = int(eng.lib.hmv_lagcov_ensemble_workspace_doubles(items, m, n, p, hop, W)) > 0
        freqs = northstar_freqs(F) if F == 256 else np.linspace(1.0, 45.0, F)
        fd = eng.to_device(freqs)
        lo, hi = hd.band_bins(freqs)
        out = {"shape": dict(sh, windows_per_group=W, items=items, k=n / hop, shared_form_by_rule=shared), "seconds": {},
               "items_per_s": {}}

        def record(key, ts, count=items):
            out["seconds"][key] = ts
            out["items_per_s"][key] = count / float(np.median(ts))
            print(f"{tag:6s} {key:34s} {np.median(ts) * 1e3:10.3f} ms  {out['items_per_s'][key]:12,.0f} items/s", flush=True)

        # (ii) K1 alone
        record("k1/ensemble_direct", timed(lambda: eng.lagcov_ensemble(xd, n=n, p=p, validate=False, **d), args.reps, sync))
        if shared:
            record("k1/ensemble_shared", timed(lambda: eng.lagcov_ensemble(xd, n=n, p=p, grid=grid, validate=False, **d),
                                               args.reps, sync))
        # without the feature: single-trial items window-major, trial-minor, one group at a time, then the mean per window
        per_group = []
        for g in range(G):
            st = (onsets[g][None, :] + offsets[:, None]).reshape(-1)
            per_group.append((i64(np.full(W * E, g)), i64(st)))

        def plumbing():
            outR = eng.empty(items, p + 1, mp, mp)
            for g, (rec, st) in enumerate(per_group):
                R = eng.lagcov(xd, rec, st, n, p)
                for w in range(W):
                    outR[g * W + w] = eng.trial_mean(R[w * E:(w + 1) * E], m)[0]
            return outR
        if not args.k1_only or args.plumbing:
            record("k1/single_trial_items_and_mean", timed(plumbing, max(1, min(args.reps, 3)), sync))
            a = eng.lagcov_ensemble(xd, n=n, p=p, validate=False, **d)
            b = plumbing()
            out["k1_routes_max_rel_diff"] = float((a - b).abs().max() / a.abs().max())
            del a, b
        flops = 2.0 * mp * mp * (p + 1) * n * E * items
        out["k1_tflops"] = {k.split("/")[1]: flops / float(np.median(v)) / 1e12 for k, v in out["seconds"].items()
                            if k.startswith("k1/")}
        lag_groups = (p + 3) // 3
        chunks = -(-n // 64)
        out["k1_bytes"] = {
            # per item and lag group every trial's chunk is staged once (96 columns, of which min(n, 96) hold samples)
            "direct_read": float(items * lag_groups * E * m * min(n + p, 96 * chunks) * 8),
            "direct_write": float(items * (p + 1) * mp * mp * 8),
            "single_trial_write_and_reread": float(2 * items * E * (p + 1) * mp * mp * 8),
        }
        if not args.k1_only:
            # (i) the fused call
            for meas, kw in (("ffdtf_bands", dict(measure="ffdtf", bands=(lo, hi))), ("ddtf", dict(measure="ddtf")),
                             ("gpdc", dict(measure="gpdc"))):
                for form, fkw in (("rule", dict(grid=grid)), ("direct", dict(grid=grid, flags=_lib.FLAG_DIRECT_LAGCOV))):
                    if form == "direct" and not shared:
                        continue
                    call = lambda: eng.sliding_ensemble(xd, n=n, p=p, freqs=fd, fs=sh["fs"], check=False, validate=False,  # noqa: E731
                                                        **kw, **fkw, **d)
                    record(f"fused/{meas}/{form}", timed(call, args.reps, sync))
            # (iii) the host loop, a few windows, extrapolated
            hw = min(args.host_windows, W)
            stacks = [np.stack([x[0][:, s + off:s + off + n] for s in onsets[0]], axis=2) for off in offsets[:hw]]
            ts = timed(lambda: [M.full_freq_dtf(s, freqs, sh["fs"], optimal_model_order=p) for s in stacks], 2, sync)
            record("host_loop/ffdtf (EXTRAPOLATED from %d windows)" % hw, ts, count=hw)
        res["shapes"][tag] = out
        del xd
        torch.cuda.empty_cache()
    return res


def merge_trace(path, res):
    """rocprofv3 kernel trace of ONE profiled run -> calls, mean and total ms of the K1 kernels per launch shape (the
    launch grid tells the benchmark shapes apart: threads in x, lag groups or lags in y)."""
    table = {}
    for r in csv.DictReader(open(path)):
        if any(s in r["Kernel_Name"] for s in ("lagcov", "lagens", "lagcomb", "trial_mean")):
            key = "%s [grid %s x %s]" % (r["Kernel_Name"].split("(")[0][:80], r["Grid_Size_X"], r["Grid_Size_Y"])
            t = table.setdefault(key, {"calls": 0, "total_ms": 0.0})
            t["calls"] += 1
            t["total_ms"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
    for t in table.values():
        t["mean_ms"] = t["total_ms"] / t["calls"]
    res["k1_kernel_times_one_profiled_run"] = table
    return res


def resources(res):
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in txt.splitlines():
        if any(s in line for s in ("lagcov_ens_kernel", "lagens_", "lagcov_kernel", "lagcomb_kernel")):
            name, vals = line[:70].strip(), line[70:].split()
            rows[name] = {"vgpr": int(vals[0]), "sgpr": int(vals[2]), "vgpr_spill": int(vals[3]), "sgpr_spill": int(vals[4]),
                          "scratch_bytes": int(vals[5]), "lds_bytes": int(vals[6])}
    res["kernel_resources"] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--host-windows", type=int, default=3)
    ap.add_argument("--k1-only", action="store_true", help="K1 of the new call alone (for a profiled run)")
    ap.add_argument("--plumbing", action="store_true", help="with --k1-only: the single-trial route too")
    ap.add_argument("--merge-trace", default=None, help="kernel_trace.csv of a rocprofv3 run: merged into --out (no GPU)")
    ap.add_argument("--resources", action="store_true", help="add tools/kernel_resources.py's figures to --out (no GPU)")
    args = ap.parse_args()
    if args.merge_trace or args.resources:
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        if args.merge_trace:
            res = merge_trace(args.merge_trace, res)
        if args.resources:
            res = resources(res)
    else:
        res = run(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({t: {"items_per_s": s["items_per_s"], "k1_tflops": s["k1_tflops"]} for t, s in res.get("shapes", {}).items()}))


if __name__ == "__main__":
    main()
