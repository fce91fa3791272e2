"""Side measurement of sliding-window phase synchrony (csrc/phase_sync.hip, `Engine.sliding_phase_sync`) on one MI355X.
Nothing is asserted.

North-star shape: one dyad of 64 channels x 300 000 samples at 500 Hz, 599 windows of 1000 samples every 500,
`distributed.DEFAULT_BANDS` (5 bands), PLV + ciPLV.  Device events after a warm-up, median of --reps:

  * the analytic signal: the forward FFT of the recording, and multiply + inverse FFT per band;
  * `phase_gram_kernel<4>` alone on the resident z (5 x 599 items), UNIT and RAW mode: ms and TFLOP/s, counted as the 8 m^2 n
    flops of the full Hermitian product per item (the kernel issues 10 / 16 of them: one triangle of tiles), beside K1's
    rate on the same MFMA form (profiles/r03_kernel_stats.csv: lagcov_kernel<4, 3> on 600 hop blocks of 500 samples, 9 lags,
    22.1 GFLOP);
  * the whole call (`Engine.sliding_phase_sync`, check="nan") in band windows/s, beside a `sliding_ffdtf` band call
    (p = 8, 256 frequencies, 5 bands) in the same process;
  * the NumPy restatement (tests/phase_sync_restated.py) on the host for a handful of windows of the same z;
  * the register / LDS / scratch table of the kernel from tools/kernel_resources.py.

    python tests/side_benchmarks/bench_phase_sync.py --out profiles/phase_sync_bench.json [--reps 7]
    python tests/side_benchmarks/bench_phase_sync.py --resources --out profiles/phase_sync_bench.json   (no GPU)
"""
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

M_CH, T, FS = 64, 300_000, 500.0
N_WIN, WIN, P, F = 599, 1000, 8, 256
K1_GFLOP = 600 * 500 * 9 * 2 * 64 * 64 / 1e9


def kernel_resources():
    """tools/kernel_resources.py on the built library: the rows of phase_sync.hip."""
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


def k1_reference():
    """K1's recorded time at the north-star shape (the same v_mfma_f64_4x4x4_4b_f64 form)."""
    path = os.path.join(ROOT, "profiles", "r03_kernel_stats.csv")
    try:
        with open(path) as f:
            for row in csv.reader(f):
                if row and row[0].startswith("void hmv::lagcov_kernel<4, 3>"):
                    ms = float(row[3]) / 1e6
                    return {"source": "profiles/r03_kernel_stats.csv", "kernel": "lagcov_kernel<4, 3>", "ms": ms,
                            "GFLOP": K1_GFLOP, "TFLOP_per_s": K1_GFLOP / ms}
    except OSError:
        pass
    return None


def run(args):
    import torch
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd import distributed as hd
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import regular_grid, window_items, window_positions
    from tests import phase_sync_restated as PR

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
    from hyperscanning_signal_analysis_amd.eeg_io import resolve_bands_hz
    resp = torch.stack([eng.band_response(T, FS, lo, hi) for lo, hi in resolve_bands_hz(bands, FS)])
    res = {"shape": {"channels": M_CH, "samples": T, "fs": FS, "windows": N_WIN, "window": WIN, "hop": int(pos[1] - pos[0]),
                     "bands_hz": [list(b) for b in bands], "measures": ["plv", "ciplv"]}, "reps": args.reps}

    # ---- the analytic signal
    X = torch.fft.fft(xd[0], dim=-1)
    z1 = torch.empty(M_CH, T, dtype=torch.complex128, device=eng.device)
    fft_ms = event_ms(lambda: torch.fft.fft(xd[0], dim=-1))
    band_ms = [event_ms(lambda b=b: torch.fft.ifft(X * resp[b], dim=-1, out=z1)) for b in range(nb)]
    del X, z1
    res["analytic_signal"] = {"forward_fft_ms": fft_ms, "multiply_inverse_ms_per_band": band_ms,
                              "all_bands_ms": fft_ms + float(np.sum(band_ms)), "z_bytes_per_band": 16 * M_CH * T}
    print(f"analytic signal: {res['analytic_signal']}", flush=True)

    # ---- the kernel alone, on the resident z of all bands
    z = eng.analytic_signal(xd, resp)[0]                              # (nb, m, T): the bands as recordings
    bb = torch.arange(nb, dtype=torch.int64, device=eng.device)
    rec_z = (rec[:, None] * nb + bb[None, :]).reshape(-1)
    st_z = st[:, None].expand(-1, nb).reshape(-1)
    items = int(rec_z.numel())
    gflop = items * 8.0 * M_CH * M_CH * WIN / 1e9
    res["kernel"] = {"items": items, "GFLOP_full_hermitian": gflop, "GFLOP_issued": gflop * 10.0 / 16.0,
                     "z_bytes_read_by_windows": items * 16 * M_CH * WIN, "k1_reference": k1_reference()}
    for name, mode in (("unit", _lib.PHASE_UNIT), ("raw", _lib.PHASE_RAW)):
        ms = event_ms(lambda mode=mode: eng._phase_sync(z, rec_z, st_z, w, mode, True, True, False))
        res["kernel"][name] = {"ms": ms, "TFLOP_per_s_full_hermitian": gflop / ms, "TFLOP_per_s_issued": gflop * 0.625 / ms,
                               "read_GB_per_s": items * 16 * M_CH * WIN / ms / 1e6}
    print(f"kernel: {res['kernel']}", flush=True)

    # ---- the restatement on the host, a handful of windows
    zh = z[2].cpu().numpy()
    t0 = time.perf_counter()
    hw = [PR.measures_restated(zh, int(s), WIN, PR.UNIT) for s in pos[:4]]
    host_ms = (time.perf_counter() - t0) * 1e3 / 4
    got = eng._phase_sync(z[2:3], rec[:4], st[:4], w, _lib.PHASE_UNIT, True, True, False)
    res["host_restatement"] = {"windows": 4, "ms_per_band_window": host_ms,
                               "max_abs_diff_plv": float(max(np.abs(h["mag"] - g).max() for h, g in zip(hw, got["mag"].cpu().numpy()))),
                               "max_abs_diff_ciplv": float(max(np.abs(h["lagged"] - g).max()
                                                               for h, g in zip(hw, got["lagged"].cpu().numpy())))}
    del z
    print(f"host: {res['host_restatement']}", flush=True)

    # ---- the whole call, beside a sliding_ffdtf band call
    s = wall_s(lambda: eng.sliding_phase_sync(xd, rec, st, w, FS, bands, measures=("plv", "ciplv"), check="nan"))
    res["whole_call"] = {"ms": s * 1e3, "band_windows_per_s": N_WIN * nb / s, "windows_per_s": N_WIN / s}
    s4 = wall_s(lambda: eng.sliding_phase_sync(xd, rec, st, w, FS, bands, measures=("plv", "ciplv", "coh", "imcoh"), check="nan"))
    res["whole_call_four_measures"] = {"ms": s4 * 1e3, "band_windows_per_s": N_WIN * nb / s4}
    freqs = 0.5 * np.arange(1, F + 1)
    fd = eng.to_device(freqs)
    lo, hi = hd.band_bins(freqs)
    grid = regular_grid(pos, w, P)
    sf = wall_s(lambda: eng.sliding_ffdtf(xd, rec, st, w, P, fd, FS, grid=grid, bands=(lo, hi), check="mask"))
    res["sliding_ffdtf_bands"] = {"p": P, "F": F, "bands": len(lo), "ms": sf * 1e3, "band_windows_per_s": N_WIN * len(lo) / sf,
                                  "windows_per_s": N_WIN / sf}
    print(f"whole call: {res['whole_call']}; ffdtf: {res['sliding_ffdtf_bands']}", flush=True)
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
    res["expectation"] = ("by flop count the Gram stage is 33 MFLOP per 64-channel window and band, 98 GFLOP for the shape, against "
                          "about 3 GB of window reads; no rate is promised and none is a pass criterion")
    res["kernel_resources"] = kernel_resources()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
