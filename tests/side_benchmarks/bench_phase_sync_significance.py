"""Side measurement of the null tests of phase synchrony (csrc/phase_sync.hip's pairs form, `Engine.phase_sync_pairs`,
`Engine.phase_sync_significance`) on one MI355X.  Nothing is asserted.

North-star shape of bench_phase_sync.py: one dyad of 64 channels x 300 000 samples at 500 Hz, 599 windows of 1000 samples
every 500, `distributed.DEFAULT_BANDS` (5 bands), PLV + ciPLV, split 32.  One process; device events after a warm-up, the
median of --reps with the smallest and the largest beside it:

  (a) `phase_gram_kernel<4>` (the full form), UNIT, over the 2995 band windows of the resident z;
  (b) the pairs form over the same items with shift 0;
  (c) the pairs form with a random shift per item;
  (d) the written-out route for one surrogate: roll participant B's z by the surrogate's shift, then (a);
  (e) the whole shift test (`Engine.phase_sync_significance`, S = 100, check="nan") in surrogate band windows per second;
  and (a), (b) on the 16-channel instance (the first 16 channels read in place, split 8).

    python tests/side_benchmarks/bench_phase_sync_significance.py --out profiles/phase_sync_significance_bench.json [--reps 7]
    python tests/side_benchmarks/bench_phase_sync_significance.py --resources --out profiles/phase_sync_significance_bench.json
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

M_CH, T, FS, SPLIT = 64, 300_000, 500.0, 32
N_WIN, WIN, S = 599, 1000, 100


def kernel_resources():
    """tools/kernel_resources.py on the built library: the rows of phase_sync.hip, both forms."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        if "phase_gram_kernel" in line:
            sig, *cols = line.rsplit(None, 7)                       # the demangled signature, then seven numbers
            name = sig.split("(")[0].split("::")[-1]
            vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in cols)
            rows[name] = {"vgpr": vgpr, "agpr": agpr, "sgpr": sgpr, "vgpr_spill": vspill, "sgpr_spill": sspill,
                          "scratch_bytes": scratch, "static_lds_bytes": lds,
                          "workgroups_per_cu": min(512 // max(vgpr, 1), 163840 // lds, 8)}
    return rows


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.eeg_io import resolve_bands_hz
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import window_items, window_positions

    eng = Engine()

    def event_ms(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return {"ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

    bands = hd.DEFAULT_BANDS
    nb = len(bands)
    xd = eng.to_device(np.random.default_rng(0).standard_normal((1, M_CH, T)))
    pos, w = window_positions(T, N_WIN, WIN)
    rec, st = window_items(1, pos, eng.device)
    resp = torch.stack([eng.band_response(T, FS, lo, hi) for lo, hi in resolve_bands_hz(bands, FS)])
    res = {"shape": {"channels": M_CH, "split": SPLIT, "samples": T, "fs": FS, "windows": N_WIN, "window": WIN,
                     "hop": int(pos[1] - pos[0]), "bands_hz": [list(b) for b in bands], "measures": ["plv", "ciplv"],
                     "surrogates": S}, "reps": args.reps}

    z = eng.analytic_signal(xd, resp)[0]                              # (nb, m, T): the bands as recordings
    bb = torch.arange(nb, dtype=torch.int64, device=eng.device)
    rec_z = (rec[:, None] * nb + bb[None, :]).reshape(-1)
    st_z = st[:, None].expand(-1, nb).reshape(-1).contiguous()
    items = int(rec_z.numel())
    shift = torch.as_tensor(np.random.default_rng(1).integers(WIN, T - WIN, items, endpoint=True)).to(eng.device)
    res["items"] = items
    for name, zz, split in (("64_channels", z, SPLIT), ("16_channels", z[:, :16], 8)):
        m = int(zz.shape[1])
        vals = eng.empty(items, m, m, 2)
        out = {"a_full_form_unit": event_ms(lambda: eng._phase_sync(zz, rec_z, st_z, w, _lib.PHASE_UNIT, True, True, False)),
               "b_pairs_shift_0": event_ms(lambda: eng._phase_sync_pairs(zz, rec_z, rec_z, st_z, w, _lib.PHASE_UNIT, split, None,
                                                                        vals, (0, 1)))}
        if m == M_CH:
            out["c_pairs_random_shifts"] = event_ms(lambda: eng._phase_sync_pairs(zz, rec_z, rec_z, st_z, w, _lib.PHASE_UNIT, split,
                                                                                 shift, vals, (0, 1)))
            zs = z.clone()
            d = int(shift[0])

            def written_out():
                zs[:, split:] = torch.roll(z[:, split:], -d, dims=-1)
                eng._phase_sync(zs, rec_z, st_z, w, _lib.PHASE_UNIT, True, True, False)
            out["d_written_out_one_surrogate"] = event_ms(written_out)
            del zs
        res[name] = out
        del vals
        print(f"{name}: {out}", flush=True)
    del z

    def whole():
        eng.phase_sync_significance(xd, rec, st, w, FS, bands, measures=("plv", "ciplv"), n_surrogates=S, seed=0, split=SPLIT,
                                    check="nan")
    whole()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        whole()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    s = float(np.median(ts))
    res["e_whole_shift_test"] = {"s": s, "min_s": float(min(ts)), "max_s": float(max(ts)),
                                 "surrogate_band_windows_per_s": S * items / s}
    print(f"whole test: {res['e_whole_shift_test']}", flush=True)
    prop = torch.cuda.get_device_properties(0)
    res["measured_on"] = {"name": torch.cuda.get_device_name(0), "gfx_arch": prop.gcnArchName.split(":")[0],
                          "compute_units": prop.multi_processor_count}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="the kernel table alone: no GPU, no timing")
    args = ap.parse_args()
    res = {"status": "not yet measured: kernel resources only"} if args.resources else run(args)
    res["expectation"] = ("(c) reads what (d) reads, issues 4 of its 10 tiles of MFMAs and makes no extra pass over z, so (c) "
                          "should not be slower than (d); whether (b) beats (a) is reported, not promised")
    res["kernel_resources"] = kernel_resources()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
