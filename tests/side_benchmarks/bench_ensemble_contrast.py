"""Side measurement of the condition-contrast path (`Engine.lagcov_mix`, `Engine.sliding_mix`) on one MI355X, at shape A of
bench_ensemble.py: 64 channels, 8 groups x (50 + 50) trials, n = 100, hop 20 (46 windows per group), p = 8, F = 256; S = 100
relabellings, i.e. 200 mix rows per group.

  (a) the mix kernel alone on one group's per-trial stack (trials x windows x 9 tiles of 64 x 64) with the 200 label rows: the
      bytes it moves (the stack once per tile of 16 rows, the output once) per second, beside a plain device-to-device copy
      of the stack timed in the same run (bytes read + bytes written per second, like the kernel's figure);
  (b) the surrogate stage of all groups two ways: `lagcov_trials` once per group + `sliding_mix` over the 2 S label rows, and
      the route the package had before -- `sliding_ensemble` on relabelled trial tables, 2 S groups of 50 trials per group of
      the data, which runs K1 over every trial S times (shared-overlap form, the rule's choice at this shape);
  (c) both in surrogate items (mix row x window) per second;
  (d) the kernel's resources (`--resources`, no GPU).
One process, a warm-up call, the median of --reps synchronised wall times.

    python tests/side_benchmarks/bench_ensemble_contrast.py --out profiles/ensemble_contrast_bench.json
    python tests/side_benchmarks/bench_ensemble_contrast.py --resources --out profiles/ensemble_contrast_bench.json   (no GPU)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ensemble import SHAPES, timed  # noqa: E402


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import distributed as hd, surrogates as sg
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import hop_positions
    from hyperscanning_signal_analysis_amd.synthetic import northstar_freqs

    eng = Engine()
    sync = torch.cuda.synchronize
    sh = SHAPES["A"]
    m, G, E, L, n, hop, p, F, T = (sh[k] for k in ("m", "groups", "trials", "L", "n", "hop", "p", "F", "T"))
    G = min(G, args.groups)
    EA, S = E // 2, args.surrogates
    rng = np.random.default_rng(5)
    x = rng.standard_normal((G, m, T))
    x[..., 1:] += 0.5 * x[..., :-1]
    x[:, 1:] += 0.3 * x[:, :-1]
    xd = eng.to_device(x)
    offsets = hop_positions(L, n, hop)
    W = len(offsets)
    onsets = np.stack([np.sort(rng.choice(np.arange(0, T - L + 1), E, replace=False)) for _ in range(G)])
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(eng.device)  # noqa: E731
    off_d = i64(offsets)
    draws = sg.label_draws(np.random.default_rng(1), S, [EA] * G, [E - EA] * G)
    freqs = northstar_freqs(F)
    fd = eng.to_device(freqs)
    lo, hi = hd.band_bins(freqs)
    items = G * 2 * S * W
    res = {"reps": args.reps, "shape": dict(sh, groups=G, trials_a=EA, trials_b=E - EA, surrogates=S, windows_per_group=W,
                                            mix_rows_per_group=2 * S, surrogate_items=items), "seconds": {}}

    def labels(g):
        Wh = np.zeros((2 * S, E))
        for s in range(S):
            Wh[2 * s, draws[s][g]] = 1.0
            Wh[2 * s + 1] = 1.0 - Wh[2 * s]
        return eng.to_device(Wh), eng.to_device(np.tile([1.0 / EA, 1.0 / (E - EA)], S))

    # (a) the kernel alone, one group
    rec0, st0 = i64(np.zeros(E)), i64(onsets[0])
    Rt = eng.lagcov_trials(xd, rec0, st0, off_d, n, p, grid=(hop, W), validate=False)
    Wd, sc = labels(0)
    stack_bytes = Rt.numel() * 8
    passes = -(-2 * S // 16)
    moved = passes * stack_bytes + 2 * S * W * Rt[0, 0].numel() * 8
    t_mix = timed(lambda: eng.lagcov_mix(Rt, Wd, sc, m=m), args.reps, sync)
    dst = torch.empty_like(Rt)
    t_copy = timed(lambda: dst.copy_(Rt), args.reps, sync)
    del dst
    res["seconds"]["mix_kernel_one_group"] = t_mix
    res["seconds"]["d2d_copy_of_the_stack"] = t_copy
    res["mix_kernel"] = {
        "stack_bytes": stack_bytes, "passes_over_the_stack": passes, "bytes_moved": moved,
        "GBps_read_plus_written": moved / float(np.median(t_mix)) / 1e9,
        "stack_GBps_read": passes * stack_bytes / float(np.median(t_mix)) / 1e9,
        "d2d_copy_GBps_read_plus_written": 2 * stack_bytes / float(np.median(t_copy)) / 1e9}
    res["mix_kernel"]["fraction_of_copy"] = res["mix_kernel"]["GBps_read_plus_written"] / res["mix_kernel"]["d2d_copy_GBps_read_plus_written"]
    print(json.dumps(res["mix_kernel"]), flush=True)
    del Rt
    torch.cuda.empty_cache()
    if args.kernel_only:
        return res

    # (b), (c) the surrogate stage of every group, both routes
    tables = []
    for g in range(G):
        src = np.concatenate([np.concatenate([draws[s][g], np.setdiff1d(np.arange(E), draws[s][g])]) for s in range(S)])
        tables.append(dict(trial_rec=i64(np.full(2 * S * (E // 2), g)), trial_start=i64(onsets[g][src]),
                           group_ptr=i64(np.arange(2 * S + 1) * (E // 2)),
                           item_group=i64(np.repeat(np.arange(2 * S), W)), item_offset=i64(np.tile(offsets, 2 * S))))
    mixes = [labels(g) for g in range(G)]
    trials = [(i64(np.full(E, g)), i64(onsets[g])) for g in range(G)]
    assert EA == E - EA, "the relabelled tables above assume equal condition sizes"
    res["items_per_s"], res["ratio_relabel_over_mix"], res["routes_max_abs_diff"] = {}, {}, {}
    for meas in args.measures.split(","):
        def mix_route(keep=None):
            for g in range(G):
                Rg = eng.lagcov_trials(xd, trials[g][0], trials[g][1], off_d, n, p, grid=(hop, W), validate=False)
                v, _ = eng.sliding_mix(Rg, mixes[g][0], mixes[g][1], n, fd, sh["fs"], m=m, measure=meas, bands=(lo, hi),
                                       check="mask", validate=False)
                if keep is not None and g == 0:
                    keep.append(v)

        def relabel_route(keep=None):
            for g in range(G):
                v, _ = eng.sliding_ensemble(xd, n=n, p=p, freqs=fd, fs=sh["fs"], measure=meas, bands=(lo, hi), check="mask",
                                            validate=False, grid=(hop, W), **tables[g])
                if keep is not None and g == 0:
                    keep.append(v)
        a, b = [], []
        mix_route(a)
        relabel_route(b)
        res["routes_max_abs_diff"][meas] = float((a[0] - b[0]).abs().max())
        del a, b
        for key, fn in (("mix", mix_route), ("relabel", relabel_route)):
            ts = timed(fn, args.reps, sync)
            res["seconds"][f"surrogate_stage/{meas}_bands/{key}"] = ts
            res["items_per_s"][f"{meas}_bands/{key}"] = items / float(np.median(ts))
            print(f"{meas:6s} {key:8s} {np.median(ts) * 1e3:10.1f} ms  {items / np.median(ts):12,.0f} surrogate items/s", flush=True)
        res["ratio_relabel_over_mix"][meas] = (float(np.median(res["seconds"][f"surrogate_stage/{meas}_bands/relabel"]))
                                               / float(np.median(res["seconds"][f"surrogate_stage/{meas}_bands/mix"])))
    return res


def resources(res):
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in txt.splitlines():
        if "lagcov_mix" in line:
            name, vals = line[:70].strip(), line[70:].split()
            rows[name] = {"vgpr": int(vals[0]), "sgpr": int(vals[2]), "vgpr_spill": int(vals[3]), "sgpr_spill": int(vals[4]),
                          "scratch_bytes": int(vals[5]), "lds_bytes": int(vals[6])}
    res["kernel_resources"] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--surrogates", type=int, default=100)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--measures", default="ffdtf,gpdc")
    ap.add_argument("--kernel-only", action="store_true", help="part (a) alone")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="add tools/kernel_resources.py's figures to --out (no GPU)")
    args = ap.parse_args()
    if args.resources:
        res = resources(json.load(open(args.out)) if args.out and os.path.exists(args.out) else {})
    else:
        res = run(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("mix_kernel", "items_per_s", "ratio_relabel_over_mix", "kernel_resources") if k in res}))


if __name__ == "__main__":
    main()
