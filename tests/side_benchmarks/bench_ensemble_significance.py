"""Side measurement of the trial-shuffle significance path (`Engine.ensemble_significance`, `lagcov_ensemble_split`) on one
MI355X, at the shapes A and B of bench_ensemble.py (A: 64 channels = 32 + 32, 8 groups x 100 trials, n = 100, hop 20, p = 8,
F = 256, 368 items;  B: 19 channels = 10 + 9, 32 groups x 60 trials, n = 80, hop 16, p = 6, F = 64).

One block of --block surrogates is laid out as `ensemble_significance` lays it out (surrogate-major: block * G groups, block *
items items, one permutation per surrogate and group) and timed three ways for K1 alone,
  (i)   `lagcov_ensemble_split` with R_base   (within-participant blocks copied, their accumulators skipped)
  (ii)  `lagcov_ensemble_split` without R_base (every element computed)
  (iii) `lagcov_ensemble` with FLAG_DIRECT_LAGCOV on the same items (table A only: the kernel the split kernel derives from)
and through the fused call for the band values of the three measures: the split entry with R_base beside
`sliding_ensemble(flags=FLAG_DIRECT_LAGCOV)` on the same items, and `ensemble_significance` end to end (observed call and
base included) in surrogate items per second.  One process, a warm-up call, the median of --reps synchronised wall times.

    python tests/side_benchmarks/bench_ensemble_significance.py --out profiles/ensemble_significance_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tests/side_benchmarks/bench_ensemble_significance.py --reps 1 --k1-only
    python tests/side_benchmarks/bench_ensemble_significance.py --merge-trace DIR/.../run_kernel_trace.csv --out profiles/ensemble_significance_bench.json
    python tests/side_benchmarks/bench_ensemble_significance.py --resources --out profiles/ensemble_significance_bench.json   (no GPU)"""
import argparse
import csv
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ensemble import SHAPES, timed  # noqa: E402

SPLIT = {"A": 32, "B": 10}


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import _lib, surrogates as sg
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions
    from hyperscanning_signal_analysis_amd.synthetic import northstar_freqs

    eng = Engine()
    sync = torch.cuda.synchronize
    res = {"reps": args.reps, "block": args.block, "shapes": {}}
    for tag in args.shapes.split(","):
        sh = SHAPES[tag]
        m, G, E, L, n, hop, p, F, T = (sh[k] for k in ("m", "groups", "trials", "L", "n", "hop", "p", "F", "T"))
        split, Sb = SPLIT[tag], args.block
        rng = np.random.default_rng(5)
        x = rng.standard_normal((G, m, T))
        x[..., 1:] += 0.5 * x[..., :-1]
        x[:, 1:] += 0.3 * x[:, :-1]
        xd = eng.to_device(x)
        offsets = hop_positions(L, n, hop)
        W = len(offsets)
        N = G * W
        onsets = np.concatenate([np.sort(rng.choice(np.arange(0, T - L + 1), E, replace=False)) for _ in range(G)])
        rec = np.repeat(np.arange(G), E)
        i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
        one = dict(trial_rec=i64(rec), trial_start=i64(onsets), group_ptr=i64(np.arange(G + 1) * E),
                   item_group=i64(np.repeat(np.arange(G), W)), item_offset=i64(np.tile(offsets, G)))
        perms = sg.trial_permutations(np.random.default_rng(1), Sb, [E] * G)
        src = np.stack([np.concatenate([g * E + perms[s][g] for g in range(G)]) for s in range(Sb)]).reshape(-1)
        blk = dict(trial_rec=i64(np.tile(rec, Sb)), trial_start=i64(np.tile(onsets, Sb)), group_ptr=i64(np.arange(Sb * G + 1) * E),
                   item_group=i64(np.repeat(np.arange(Sb * G), W)), item_offset=i64(np.tile(offsets, Sb * G)))
        tb = dict(trial_rec_b=i64(rec[src % (G * E)]), trial_start_b=i64(onsets[src % (G * E)]))
        item_base = i64(np.tile(np.arange(N), Sb))
        items = Sb * N
        freqs = northstar_freqs(F) if F == 256 else np.linspace(1.0, 45.0, F)
        fd = eng.to_device(freqs)
        lo, hi = hd.band_bins(freqs)
        out = {"shape": dict(sh, split=split, windows_per_group=W, items=N, block_items=items), "seconds": {}, "items_per_s": {}}

        def record(key, ts, count=items):
            out["seconds"][key] = ts
            out["items_per_s"][key] = count / float(np.median(ts))
            print(f"{tag:3s} {key:40s} {np.median(ts) * 1e3:10.3f} ms  {out['items_per_s'][key]:12,.0f} items/s", flush=True)

        R_base = eng.lagcov_ensemble(xd, n=n, p=p, validate=False, **one)
        kw = dict(n=n, p=p, split=split, validate=False, **blk, **tb)
        record("k1/split_with_base", timed(lambda: eng.lagcov_ensemble_split(xd, R_base=R_base, item_base=item_base, **kw),
                                           args.reps, sync))
        record("k1/split_without_base", timed(lambda: eng.lagcov_ensemble_split(xd, **kw), args.reps, sync))
        record("k1/ensemble_direct", timed(lambda: eng.lagcov_ensemble(xd, n=n, p=p, flags=_lib.FLAG_DIRECT_LAGCOV,
                                                                       validate=False, **blk), args.reps, sync))
        med = {k: float(np.median(v)) for k, v in out["seconds"].items()}
        out["k1_ratios"] = {"with_base / without_base": med["k1/split_with_base"] / med["k1/split_without_base"],
                            "with_base / ensemble_direct": med["k1/split_with_base"] / med["k1/ensemble_direct"],
                            "without_base / ensemble_direct": med["k1/split_without_base"] / med["k1/ensemble_direct"]}
        a = eng.lagcov_ensemble_split(xd, R_base=R_base, item_base=item_base, **kw)
        b = eng.lagcov_ensemble_split(xd, **kw)
        out["with_vs_without_base_max_rel_diff"] = float((a - b).abs().max() / b.abs().max())
        del a, b
        if not args.k1_only:
            shuffle = (tb["trial_rec_b"], tb["trial_start_b"], split, R_base, item_base)
            for meas in ("ffdtf", "ddtf", "gpdc"):
                rt = eng._ensemble_route(meas, n, p, blk["trial_rec"], blk["trial_start"], blk["group_ptr"], shuffle=shuffle)
                record(f"fused/{meas}_bands/split_with_base",
                       timed(lambda: eng._sliding_call(rt, xd, (blk["item_group"], blk["item_offset"]), fd, sh["fs"],
                                                       bands=(lo, hi), check="mask", validate=False), args.reps, sync))
                record(f"fused/{meas}_bands/ensemble_direct",
                       timed(lambda: eng.sliding_ensemble(xd, n=n, p=p, freqs=fd, fs=sh["fs"], measure=meas, bands=(lo, hi),
                                                          check="mask", validate=False, flags=_lib.FLAG_DIRECT_LAGCOV, **blk),
                             args.reps, sync))
                record(f"significance/{meas}_bands/end_to_end_S{2 * Sb}",
                       timed(lambda: eng.ensemble_significance(xd, n=n, p=p, freqs=fd, fs=sh["fs"], bands=(lo, hi), measure=meas,
                                                               n_surrogates=2 * Sb, seed=1, split=split, check="nan",
                                                               grid=(hop, W), **one), max(1, min(args.reps, 3)), sync),
                       count=2 * Sb * N)
        res["shapes"][tag] = out
        del xd, R_base
        torch.cuda.empty_cache()
    return res


def merge_trace(path, res):
    """rocprofv3 kernel trace of ONE profiled run (--reps 1 --k1-only) -> calls, mean and total ms of the K1 kernels per
    launch shape (items in x, lag groups in y)."""
    table = {}
    for r in csv.DictReader(open(path)):
        if "lagcov_ens" in r["Kernel_Name"]:
            key = "%s [grid %s x %s]" % (r["Kernel_Name"].split("(")[0][:80], r["Grid_Size_X"], r["Grid_Size_Y"])
            t = table.setdefault(key, {"calls": 0, "total_ms": 0.0, "each_ms": []})
            t["calls"] += 1
            ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
            t["total_ms"] += ms
            t["each_ms"].append(round(ms, 4))
    for t in table.values():
        t["mean_ms"] = t["total_ms"] / t["calls"]
    res["k1_kernel_times_one_profiled_run"] = table
    return res


def resources(res):
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in txt.splitlines():
        if "lagcov_ens" in line:
            name, vals = line[:70].strip(), line[70:].split()
            rows[name] = {"vgpr": int(vals[0]), "sgpr": int(vals[2]), "vgpr_spill": int(vals[3]), "sgpr_spill": int(vals[4]),
                          "scratch_bytes": int(vals[5]), "lds_bytes": int(vals[6])}
    res["kernel_resources"] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=8, help="surrogates per timed block")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--k1-only", action="store_true", help="the three K1 runs alone (for a profiled run)")
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
    print(json.dumps({t: {"items_per_s": s["items_per_s"], "k1_ratios": s["k1_ratios"]} for t, s in res.get("shapes", {}).items()}))


if __name__ == "__main__":
    main()
