"""Side measurement of the pseudo-dyad path (`Engine.lagcov_pairs`, `Engine.sliding_pairs`, `Engine.pseudo_dyad_significance`)
on one MI355X: 16 dyads of 64 = 32 + 32 channels x 30 000 samples, 1000-sample windows every 500 (59 windows), p = 8,
F = 256, five bands, exhaustive partners (15 partner sets, 14 160 surrogate windows).

A block of --block partner sets (--block x 944 items) is laid out as `pseudo_dyad_significance` lays one surrogate out
(dyad-major, window-minor) and timed
  (a) for K1 alone: `lagcov_pairs` with R_base (both within-participant blocks copied), `lagcov_pairs` without R_base, and
      `lagcov` on the pseudo recordings written out (--block x 16 recordings built with torch.cat, the build not timed);
  (b) through the fused call for the band values of the three measures: `sliding_pairs` with R_base beside
      `sliding_<measure>` with bands on the written-out recordings -- the route a user has without the pair entry -- in
      its direct form and with the shared-overlap grid the front-ends declare for it;
  (c) `pseudo_dyad_significance` end to end (observed call, base and statistics included) in surrogate windows per second.
One process, a warm-up call, the median of --reps synchronised wall times.

    python tests/side_benchmarks/bench_pseudo_dyads.py --out profiles/pseudo_dyads_bench.json
    python tests/side_benchmarks/bench_pseudo_dyads.py --resources --out profiles/pseudo_dyads_bench.json   (no GPU)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ensemble import timed  # noqa: E402

SHAPE = dict(D=16, m=64, split=32, T=30_000, n=1000, hop=500, p=8, F=256, fs=500.0)


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import _lib, surrogates as sg
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions, regular_grid
    from hyperscanning_signal_analysis_amd.synthetic import northstar_freqs

    eng = Engine()
    sync = torch.cuda.synchronize
    D, m, split, T, n, hop, p, F, fs = (SHAPE[k] for k in ("D", "m", "split", "T", "n", "hop", "p", "F", "fs"))
    rng = np.random.default_rng(5)
    x = rng.standard_normal((D, m, T))
    x[..., 1:] += 0.5 * x[..., :-1]
    x[:, 1:] += 0.3 * x[:, :-1]
    xd = eng.to_device(x)
    pos = hop_positions(T, n, hop)
    W = len(pos)
    N = D * W
    partners = sg.partner_derangements(None, None, D)
    Sb = min(args.block, len(partners))
    items = Sb * N
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
    dy = np.repeat(np.arange(D), W)
    rec_a = i64(np.tile(dy, Sb))
    rec_b = i64(np.concatenate([partners[s][dy] for s in range(Sb)]))
    st = i64(np.tile(pos, Sb * D))
    base_a = i64(np.tile(np.arange(N), Sb))
    base_b = i64(np.concatenate([partners[s][dy] * W + np.tile(np.arange(W), D) for s in range(Sb)]))
    R_base = eng.lagcov(xd, i64(dy), i64(np.tile(pos, D)), n, p)
    # the pseudo recordings written out: recording s * D + d = [A of d ; B of partners[s][d]]
    mat = torch.stack([torch.cat([xd[d, :split], xd[int(partners[s][d]), split:]], dim=0) for s in range(Sb) for d in range(D)])
    rec_m = i64(np.repeat(np.arange(Sb * D), W))
    freqs = northstar_freqs(F)
    fd = eng.to_device(freqs)
    lo, hi = hd.band_bins(freqs)
    grid = regular_grid(pos, n, p)
    res = {"reps": args.reps, "block": Sb, "shape": dict(SHAPE, windows=W, items_per_partner_set=N, block_items=items,
                                                         partner_sets=len(partners), surrogate_windows=len(partners) * N,
                                                         bands=len(lo)),
           "seconds": {}, "windows_per_s": {}}

    def record(key, ts, count=items):
        res["seconds"][key] = ts
        res["windows_per_s"][key] = count / float(np.median(ts))
        print(f"{key:46s} {np.median(ts) * 1e3:10.3f} ms  {res['windows_per_s'][key]:12,.0f} windows/s", flush=True)

    kw = dict(n=n, p=p, split=split, validate=False)
    record("k1/pairs_with_base", timed(lambda: eng.lagcov_pairs(xd, rec_a, rec_b, st, R_base=R_base, base_a=base_a,
                                                                base_b=base_b, **kw), args.reps, sync))
    record("k1/pairs_without_base", timed(lambda: eng.lagcov_pairs(xd, rec_a, rec_b, st, **kw), args.reps, sync))
    record("k1/lagcov_materialised", timed(lambda: eng.lagcov(mat, rec_m, st, n, p), args.reps, sync))
    med = {k: float(np.median(v)) for k, v in res["seconds"].items()}
    res["k1_ratios"] = {"with_base / without_base": med["k1/pairs_with_base"] / med["k1/pairs_without_base"],
                        "with_base / materialised": med["k1/pairs_with_base"] / med["k1/lagcov_materialised"],
                        "without_base / materialised": med["k1/pairs_without_base"] / med["k1/lagcov_materialised"]}
    a = eng.lagcov_pairs(xd, rec_a, rec_b, st, R_base=R_base, base_a=base_a, base_b=base_b, **kw)
    res["with_base_equals_materialised"] = bool(torch.equal(a, eng.lagcov(mat, rec_m, st, n, p)))
    del a
    if not args.k1_only:
        run_m = {"ffdtf": eng.sliding_ffdtf, "ddtf": eng.sliding_ddtf, "gpdc": eng.sliding_gpdc}
        for meas in ("ffdtf", "ddtf", "gpdc"):
            record(f"fused/{meas}_bands/pairs_with_base",
                   timed(lambda: eng.sliding_pairs(xd, rec_a, rec_b, st, n, p, fd, fs, measure=meas, split=split, bands=(lo, hi),
                                                   R_base=R_base, base_a=base_a, base_b=base_b, check="mask", validate=False),
                         args.reps, sync))
            record(f"fused/{meas}_bands/materialised_direct",
                   timed(lambda: run_m[meas](mat, rec_m, st, n, p, fd, fs, bands=(lo, hi), check="mask", validate=False,
                                             flags=_lib.FLAG_DIRECT_LAGCOV), args.reps, sync))
            record(f"fused/{meas}_bands/materialised_shared_overlap",
                   timed(lambda: run_m[meas](mat, rec_m, st, n, p, fd, fs, bands=(lo, hi), check="mask", validate=False,
                                             grid=grid), args.reps, sync))
            record(f"significance/{meas}_bands/end_to_end",
                   timed(lambda: eng.pseudo_dyad_significance(xd, i64(pos), n, p, fd, fs, (lo, hi), measure=meas, split=split,
                                                              check="nan"), max(1, min(args.reps, 3)), sync),
                   count=len(partners) * N)
        w = res["windows_per_s"]
        res["fused_ratios"] = {meas: {"pairs / materialised_direct": w[f"fused/{meas}_bands/pairs_with_base"] /
                                      w[f"fused/{meas}_bands/materialised_direct"],
                                      "pairs / materialised_shared_overlap": w[f"fused/{meas}_bands/pairs_with_base"] /
                                      w[f"fused/{meas}_bands/materialised_shared_overlap"]}
                               for meas in ("ffdtf", "ddtf", "gpdc")}
    return res


def resources(res):
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in txt.splitlines():
        if "lagcov_pairs" in line or ("lagcov_kernel<" in line and ", 3>" in line):
            name, vals = line[:70].strip(), line[70:].split()
            rows[name] = {"vgpr": int(vals[0]), "sgpr": int(vals[2]), "vgpr_spill": int(vals[3]), "sgpr_spill": int(vals[4]),
                          "scratch_bytes": int(vals[5]), "lds_bytes": int(vals[6])}
    res["kernel_resources"] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=3, help="partner sets per timed block")
    ap.add_argument("--out", default=None)
    ap.add_argument("--k1-only", action="store_true", help="the three K1 runs alone")
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
    print(json.dumps({k: res[k] for k in ("windows_per_s", "k1_ratios", "fused_ratios") if k in res}))


if __name__ == "__main__":
    main()
