"""Side measurement of the significance tests of block Granger causality at the north-star shape (599 windows of 64 ch x
1000 samples, hop 500, split 32, p = 8, F = 256, 5 bands, S = 20, one MI355X): surrogate windows/s of
`Engine.block_granger_significance` under the shift null with values=("time",) and ("time", "bands"), and of the pseudo-dyad
test with D = 4 dyads (150 windows each) with and without `red_base`, beside the rate of a plain `sliding_block_granger` call
in the same process.  There is no number to meet; the expectation to record against is that a time-only surrogate costs a
small fraction of a full call, because it skips the per-frequency kernel.

    python tests/side_benchmarks/bench_block_gc_significance.py --out profiles/block_gc_significance_bench.json [--reps 3]
    python tests/side_benchmarks/bench_block_gc_significance.py --resources-only --out ...                       (no GPU)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.side_benchmarks.bench_block_gc import kernel_resources  # noqa: E402

M_CH, SPLIT, N_WIN, WIN, HOP, P, F, FS, T, S = 64, 32, 599, 1000, 500, 8, 256, 500.0, 300_000, 20
DYADS, W_DYAD = 4, 150


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import window_items, window_positions
    from hyperscanning_signal_analysis_amd.synthetic import northstar_freqs, synthetic_var_dyad

    eng = Engine()
    x = np.stack([synthetic_var_dyad(d, m=M_CH, p=P, T=T, fs=FS) for d in range(DYADS)])
    xd = eng.to_device(x)
    pos, w = window_positions(T, N_WIN, WIN)
    rec, st = window_items(1, pos, eng.device)
    freqs = northstar_freqs(F)
    fd = eng.to_device(freqs)
    bands = hd.band_bins(freqs)
    i64 = dict(dtype=torch.int64, device=eng.device)
    dy = torch.arange(DYADS, **i64).repeat_interleave(W_DYAD)
    dstart = torch.as_tensor(np.asarray(pos[:W_DYAD], dtype=np.int64)).to(eng.device)
    starts = dstart.repeat(DYADS)
    N = DYADS * W_DYAD

    def surrogates(values):
        return lambda: eng.block_granger_significance(xd[:1], rec, st, w, P, fd, FS, bands, split=SPLIT, null="shift",
                                                      n_surrogates=S, seed=1, values=values)

    # the pseudo-dyad surrogates alone, as the driver calls them: one derangement, with the bases of an observed run
    _, _, red = eng.sliding_block_granger_pairs(xd, dy, dy, starts, w, P, None, FS, split=SPLIT, want=("time",), return_red=True)
    R_base = eng.lagcov(xd, dy, starts, w, P)
    rec_b = ((dy + 1) % DYADS).contiguous()
    base_a = torch.arange(N, **i64)
    base_b = (rec_b * W_DYAD + base_a % W_DYAD).contiguous()

    def pairs(want, with_red, with_R=True):
        kw = dict(R_base=R_base, base_a=base_a, base_b=base_b) if with_R else {}
        return lambda: eng.sliding_block_granger_pairs(xd, dy, rec_b, starts, w, P, fd, FS, split=SPLIT, want=want,
                                                       bands=bands if "spectral" in want else None,
                                                       red_base=red if with_red else None, check="mask", validate=False, **kw)

    # name -> (call, surrogate windows per call)
    cases = {
        "block_gc_plain": (lambda: eng.sliding_block_granger(xd[:1], rec, st, w, P, fd, FS, split=SPLIT, bands=bands,
                                                             check=False), N_WIN),
        "shift_time": (surrogates(("time",)), S * N_WIN),
        "shift_time_bands": (surrogates(("time", "bands")), S * N_WIN),
        "pseudo_dyad_test_time": (lambda: eng.block_granger_pseudo_dyad_significance(
            xd, dstart, w, P, fd, FS, bands, split=SPLIT, values=("time",)), (DYADS - 1) * N),
        "pseudo_dyad_test_time_bands": (lambda: eng.block_granger_pseudo_dyad_significance(
            xd, dstart, w, P, fd, FS, bands, split=SPLIT), (DYADS - 1) * N),
        "pairs_time_red_base": (pairs(("time",), True), N),
        "pairs_time_R_base_only": (pairs(("time",), False), N),
        "pairs_time_no_base": (pairs(("time",), False, False), N),
        "pairs_both_red_base": (pairs(("spectral", "time"), True), N),
        "pairs_both_R_base_only": (pairs(("spectral", "time"), False), N),
    }
    res = {"shape": {"channels": M_CH, "split": SPLIT, "windows": N_WIN, "window": WIN, "hop": HOP, "p": P, "F": F,
                     "bands": len(bands[0]), "surrogates": S, "dyads": DYADS, "windows_per_dyad": W_DYAD},
           "reps": args.reps, "seconds": {}, "surrogate_windows_per_s": {}}
    for name, (fn, windows) in cases.items():
        ts = timed(fn, args.reps)
        res["seconds"][name] = ts
        res["surrogate_windows_per_s"][name] = windows / float(np.median(ts))
        print(f"{name:30s} {np.median(ts) * 1e3:9.2f} ms  {res['surrogate_windows_per_s'][name]:10,.0f} windows/s", flush=True)
    res["note"] = ("the shift and pseudo-dyad rows time the whole test (observed run, surrogate generation, accumulation) over "
                   "its surrogate windows; the pairs rows time one surrogate call of the pseudo-dyad test; block_gc_plain is one "
                   "sliding_block_granger call with bands, its windows per second")
    prop = torch.cuda.get_device_properties(0)
    res["measured_on"] = {"name": torch.cuda.get_device_name(0), "gfx_arch": prop.gcnArchName.split(":")[0],
                          "compute_units": prop.multi_processor_count}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources-only", action="store_true", help="the kernel table alone: no GPU, no timing")
    args = ap.parse_args()
    res = {"status": "not yet measured: kernel resources only"} if args.resources_only else run(args)
    res["expectation"] = ("a time-only surrogate costs a small fraction of a full call (it skips the per-frequency kernel); no "
                          "rate is promised and none is a pass criterion")
    res["kernel_resources"] = kernel_resources()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "seconds"}))


if __name__ == "__main__":
    main()
