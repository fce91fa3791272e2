"""Side measurement of the sliding-window phase-lag family (csrc/phase_lag.hip, `Engine.sliding_phase_lag`) on one MI355X.
Nothing is asserted.

North-star shape: one dyad of 64 channels x 300 000 samples at 500 Hz, 599 windows of 1000 samples every 500,
`distributed.DEFAULT_BANDS` (5 bands).  One process, device events after a warm-up, median of --reps:

  * `phase_lag_kernel<4>` alone on the resident z (5 x 599 items): wpli only and all three outputs, at split = 0 (2016 pairs)
    and split = 32 (1024 pairs), in ms and in pair-samples per second;
  * the whole call (`Engine.sliding_phase_lag`, check="nan"), and `Engine.sliding_phase_sync(("plv", "ciplv"))` in the same
    process for scale;
  * the combined driver (both families off one analytic signal) against the sum of the two separate calls;
  * a torch-on-device restatement of wPLI on a sample of windows -- what a user would otherwise write: it materialises the
    (m, m, n) array of every window and band;
  * the register / LDS / scratch table of the kernel from tools/kernel_resources.py.

    python tests/side_benchmarks/bench_phase_lag.py --out profiles/phase_lag_bench.json [--reps 7]
    python tests/side_benchmarks/bench_phase_lag.py --resources --out profiles/phase_lag_bench.json   (no GPU)
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

M_CH, T, FS = 64, 300_000, 500.0
N_WIN, WIN = 599, 1000
TORCH_WINDOWS = 8


def kernel_resources():
    """tools/kernel_resources.py on the built library: the rows of phase_lag.hip."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        if "phase_lag_kernel" in line:
            sig, *cols = line.rsplit(None, 7)                       # the demangled signature, then seven numbers
            name = sig.split("(")[0].split("::")[-1]
            vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in cols)
            rows[name] = {"vgpr": vgpr, "agpr": agpr, "sgpr": sgpr, "vgpr_spill": vspill, "sgpr_spill": sspill,
                          "scratch_bytes": scratch, "static_lds_bytes": lds,
                          "workgroups_per_cu": min(512 // max(vgpr, 1), 163840 // lds, 8)}
    return rows


def run(args):
    import torch
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

    bands = hd.DEFAULT_BANDS
    nb = len(bands)
    xd = eng.to_device(np.random.default_rng(0).standard_normal((1, M_CH, T)))
    pos, w = window_positions(T, N_WIN, WIN)
    rec, st = window_items(1, pos, eng.device)
    resp = torch.stack([eng.band_response(T, FS, lo, hi) for lo, hi in resolve_bands_hz(bands, FS)])
    res = {"shape": {"channels": M_CH, "samples": T, "fs": FS, "windows": N_WIN, "window": WIN, "hop": int(pos[1] - pos[0]),
                     "bands_hz": [list(b) for b in bands]}, "reps": args.reps}

    # ---- the kernel alone, on the resident z of all bands
    z = eng.analytic_signal(xd, resp)[0]                              # (nb, m, T): the bands as recordings
    bb = torch.arange(nb, dtype=torch.int64, device=eng.device)
    rec_z = (rec[:, None] * nb + bb[None, :]).reshape(-1)
    st_z = st[:, None].expand(-1, nb).reshape(-1)
    items = int(rec_z.numel())
    res["kernel"] = {"items": items, "z_bytes_read_by_windows": items * 16 * M_CH * WIN}
    for split, pairs in ((0, M_CH * (M_CH - 1) // 2), (32, 32 * 32)):
        for name, want in (("wpli", ("wpli",)), ("all_three", ("pli", "wpli", "dwpli"))):
            ms = event_ms(lambda want=want, split=split: eng._phase_lag(z, rec_z, st_z, w, want, split))
            res["kernel"][f"split{split}_{name}"] = {"ms": ms, "pairs": pairs,
                                                     "G_pair_samples_per_s": items * pairs * WIN / ms / 1e6}
    print(f"kernel: {res['kernel']}", flush=True)

    # ---- what a user would otherwise write: torch on the device, a sample of windows of one band
    def torch_wpli():
        out = []
        for s in pos[:TORCH_WINDOWS]:
            zw = z[2, :, int(s):int(s) + WIN]
            xx = (zw[:, None, :] * zw[None, :, :].conj()).imag        # (m, m, n): 33 MB per window
            out.append(xx.sum(-1).abs() / xx.abs().sum(-1))
        return torch.stack(out)
    t_ms = event_ms(torch_wpli)
    got = eng._phase_lag(z[2:3], rec[:TORCH_WINDOWS], st[:TORCH_WINDOWS], w, ("wpli",), 0)["wpli"]
    ref = torch_wpli()
    off = ~torch.eye(M_CH, dtype=torch.bool, device=eng.device)
    res["torch_on_device_wpli"] = {"windows": TORCH_WINDOWS, "ms_per_band_window": t_ms / TORCH_WINDOWS,
                                   "ms_for_the_shape_extrapolated": t_ms / TORCH_WINDOWS * items,
                                   "temporary_bytes_per_window": 8 * M_CH * M_CH * WIN,
                                   "max_abs_diff_to_kernel": float((got - ref)[:, off].abs().max())}
    del z, got, ref
    print(f"torch: {res['torch_on_device_wpli']}", flush=True)

    # ---- the whole calls
    lag = wall_s(lambda: eng.sliding_phase_lag(xd, rec, st, w, FS, bands, measures=("wpli",), check="nan"))
    lag3 = wall_s(lambda: eng.sliding_phase_lag(xd, rec, st, w, FS, bands, measures=("pli", "wpli", "dwpli"), check="nan"))
    lag32 = wall_s(lambda: eng.sliding_phase_lag(xd, rec, st, w, FS, bands, measures=("wpli",), split=32, check="nan"))
    sync = wall_s(lambda: eng.sliding_phase_sync(xd, rec, st, w, FS, bands, measures=("plv", "ciplv"), check="nan"))
    both = wall_s(lambda: eng.sliding_phase("bench", xd, rec, st, w, FS, bands, sync=("plv", "ciplv"), lag=("wpli",),
                                            check="nan"))
    res["whole_call"] = {"sliding_phase_lag_wpli_ms": lag * 1e3, "sliding_phase_lag_all_three_ms": lag3 * 1e3,
                         "sliding_phase_lag_wpli_split32_ms": lag32 * 1e3, "band_windows_per_s_wpli": N_WIN * nb / lag,
                         "sliding_phase_sync_plv_ciplv_ms": sync * 1e3,
                         "combined_plv_ciplv_wpli_ms": both * 1e3, "sum_of_the_separate_calls_ms": (lag + sync) * 1e3}
    print(f"whole call: {res['whole_call']}", flush=True)
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
    res = {"status": "not yet measured on the GPU: kernel resources only"} if args.resources else run(args)
    res["expectation"] = ("2016 pairs x 1000 samples x 2995 items = 6.0e9 pair-samples of about twelve VALU instructions each "
                          "(six of them float64); no rate is promised and none is a pass criterion")
    res["kernel_resources"] = kernel_resources()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
