"""ESCan batch front-end: exported per-task EEG NetCDF files of many dyads -> sliding-window ffDTF (and multitaper
PSD) per dyad x task segment on the MI355X.  BASELINE.json config 5 / SURVEY.md section 8(f) row 2.

What it mirrors of the reference (nothing here is on the GPU hot path; it FEEDS it):
  * file layout written by `export_passive_and_talk_data` (/root/reference/src/export.py:467-609):
        <root>/EEG/<DYAD>/<child|caregiver>/<DYAD>_EEG_<ch|cg>_<task>.nc      (variable `signals`, dims (time, channel))
    with attrs `sampling_freq`, `task_events_structure` (a list of {name, start_s, start_rel_s, duration_s}, possibly
    JSON-encoded: /root/reference/src/export.py:246-288, 328-340; decoding as /root/reference/src/ncdf.py:5-19, 88-91);
  * segmenting a task file by its events like `load_eeg_nc` + `trim_to_event_window`
    (/root/reference/src/io_utils.py:113-118, 130-150: `start_rel_s`, inclusive `start <= t <= start + duration`) and the
    region logic of `_build_task_regions_from_xarray` (/root/reference/src/ncdf.py:93-111);
  * preprocessing with the semantics of `load_eeg_signals` (/root/reference/src/mne_bridge.py:113-223: zero-phase
    Butterworth-4 high / low pass and the 50 Hz notch on the WHOLE file, then the cut, M1/M2 dropped, per-channel z-score),
    child block stacked on caregiver block as in BASELINE config 2;
  * windows by the reference's `_create_windows` rule (src/eeg_alpha_ibi_ffdtf.py:451-518) with
    n_windows = 2 T / W - 1 (2 s windows, 50 % overlap when T is a multiple of the hop);
  * per dyad output file + batch bookkeeping of the reference's drivers: results saved immediately per dyad
    (src/eeg_alpha_ibi_ffdtf.py:637-658), `[SKIP]` for missing inputs (:674-684), failed dyads collected and appended to
    a log file (/root/reference/scripts/export_dyade_to_ncdf_by_task_batch.py:93-116).  Skip-if-exists is an addition.

The NetCDF reader is injectable (`reader=`): xarray / netCDF4 are not installed in the build image, so the default
reader imports them lazily and the tests inject a NumPy reader over a synthetic tree.

Multi-GPU: dyads are sharded over ranks (`world`, `rank`), no collective; every rank writes its own dyad files.
"""
from __future__ import annotations

import json
import re
import time
from pathlib import Path

import numpy as np

from . import distributed as hdist
from .eeg_io import filter_eeg
from .engine import default_engine
from .sliding import hop_positions, regular_grid, validation_p_values, window_items

__all__ = ["discover_dyads", "decode_events", "segment_block", "prepare_dyad", "run", "run_pseudo_dyads", "savez_fast",
           "xarray_reader", "resolve_decimate", "decimated_segment", "DecimateConfigError"]

ROLES = (("ch", "child"), ("cg", "caregiver"))
MEASURES = ("ffdtf", "ddtf", "gpdc")          # what run(measures=...) can compute per window; ffDTF always
_FILE_RE = re.compile(r"^(?P<dyad>.+)_EEG_(?P<role>ch|cg)_(?P<task>.+)$")


def xarray_reader(path):
    """Default reader: {data_tc (time, channel), time, channels, attrs} of one exported file (needs xarray + netCDF4)."""
    try:
        import xarray as xr
    except ImportError as e:  # pragma: no cover
        raise ImportError("reading the reference's .nc files needs xarray + netCDF4; pass reader= otherwise") from e
    da = xr.load_dataarray(str(path))
    return {"data_tc": da.transpose("time", "channel").values, "time": da.coords["time"].values,
            "channels": [str(c) for c in da.coords["channel"].values], "attrs": dict(da.attrs)}


def discover_dyads(root, tasks=None):
    """{dyad: {task: {"ch": path, "cg": path}}} for every <root>/EEG/<dyad>/<child|caregiver>/*_EEG_<ch|cg>_<task>.nc."""
    base = Path(root) / "EEG"
    found = {}
    if not base.is_dir():
        raise FileNotFoundError(f"EEG folder not found: {base}")
    for p in sorted(base.rglob("*.nc")):
        m = _FILE_RE.match(p.stem)
        if m is None:
            continue
        if tasks is not None and m.group("task") not in tasks:
            continue
        found.setdefault(m.group("dyad"), {}).setdefault(m.group("task"), {})[m.group("role")] = p
    return found


def decode_events(attrs):
    """task_events_structure -> [(name, start_rel_s, duration_s)]; accepts the list or its JSON string (ncdf.py:95-97)."""
    ev = attrs.get("task_events_structure", [])
    if isinstance(ev, (str, bytes)):
        ev = json.loads(ev) if str(ev).strip() else []
    out = []
    for k, e in enumerate(ev or []):
        if not isinstance(e, dict):
            continue
        start = e.get("start_rel_s", e.get("start_s", 0.0))
        out.append((str(e.get("name", f"event_{k + 1}")), float(start), float(e.get("duration_s", 0.0))))
    return out


def _filtered(rec, low_cutoff_hz, high_cutoff_hz):
    """Whole-file filtering + mastoid drop with load_eeg_signals' semantics, WITHOUT its trim and z-score."""
    fs = float(rec["attrs"].get("sampling_freq", rec["attrs"].get("sampling_frequency_Hz", 128.0)))
    x = filter_eeg(rec["data_tc"], fs, low_cutoff_hz, high_cutoff_hz)
    names = [str(c) for c in rec["channels"]]
    keep = [k for k, c in enumerate(names) if c not in ("M1", "M2")]
    return x[:, keep], [names[k] for k in keep], np.asarray(rec["time"], dtype=np.float64), fs


def segment_block(child, caregiver, start_s, duration_s, low_cutoff_hz=None, high_cutoff_hz=None, channel_subset=None):
    """(block (2 n_ch, T) z-scored, names, fs) of one event: both members filtered over their whole file, cut to
    start <= t <= start + duration (io_utils.py:148-150), z-scored per channel inside the segment, stacked child
    first on their common length."""
    parts, names, fss = [], [], []
    for role, rec in (("ch", child), ("cg", caregiver)):
        x, ch, t, fs = _filtered(rec, low_cutoff_hz, high_cutoff_hz)
        if channel_subset is not None:
            idx = [ch.index(c) for c in channel_subset if c in ch]
            if not idx:
                raise ValueError(f"None of the requested channels {channel_subset} found. Available: {ch}")
            x, ch = x[:, idx], [ch[k] for k in idx]
        mask = (t >= start_s) & (t <= start_s + duration_s)
        seg = np.ascontiguousarray(x[mask].T)
        sd = np.std(seg, axis=1, keepdims=True)
        sd[sd == 0] = 1.0
        parts.append((seg - np.mean(seg, axis=1, keepdims=True)) / sd)
        names += [f"{c}_{role}" for c in ch]
        fss.append(fs)
    if fss[0] != fss[1]:
        raise ValueError(f"sampling rates differ: {fss[0]} vs {fss[1]}")
    T = min(p.shape[1] for p in parts)
    return np.vstack([p[:, :T] for p in parts]), names, fss[0]


def prepare_dyad(dyad, files_by_task, reader, low_cutoff_hz=None, high_cutoff_hz=None, channel_subset=None, say=None):
    """Host part of one dyad: every task file is read and filtered ONCE (both members), then cut into its events, z-scored
    per segment and stacked child on caregiver.  Returns {"segments": [{task, event, start_s, duration_s, block, names, fs}],
    "notes": [printed lines], "host_s": seconds}.  Pure NumPy / SciPy: runs in a worker thread beside the GPU work of the
    previous dyad (filtfilt releases the GIL)."""
    t0 = time.perf_counter()
    segs, notes = [], []
    for task, files in sorted(files_by_task.items()):
        if "ch" not in files or "cg" not in files:
            notes.append(f"[SKIP] {dyad} {task}: missing {'child' if 'ch' not in files else 'caregiver'} file")
            continue
        recs = {r: reader(files[r]) for r in ("ch", "cg")}
        filt = {}
        for r in ("ch", "cg"):
            x, ch, t, fs = _filtered(recs[r], low_cutoff_hz, high_cutoff_hz)         # whole file, once
            if channel_subset is not None:
                idx = [ch.index(c) for c in channel_subset if c in ch]
                if not idx:
                    raise ValueError(f"None of the requested channels {channel_subset} found. Available: {ch}")
                x, ch = x[:, idx], [ch[k] for k in idx]
            filt[r] = (x, ch, t, fs)
        if filt["ch"][3] != filt["cg"][3]:
            raise ValueError(f"sampling rates differ: {filt['ch'][3]} vs {filt['cg'][3]}")
        for name, start, dur in decode_events(recs["ch"]["attrs"]):
            parts, names = [], []
            for r in ("ch", "cg"):
                x, ch, t, fs = filt[r]
                mask = (t >= start) & (t <= start + dur)
                seg = np.ascontiguousarray(x[mask].T)
                sd = np.std(seg, axis=1, keepdims=True)
                sd[sd == 0] = 1.0
                parts.append((seg - np.mean(seg, axis=1, keepdims=True)) / sd)
                names += [f"{c}_{r}" for c in ch]
            T = min(q.shape[1] for q in parts)
            segs.append({"task": task, "event": name, "start_s": start, "duration_s": dur, "fs": filt["ch"][3],
                         "block": np.vstack([q[:, :T] for q in parts]), "names": names})
    return {"segments": segs, "notes": notes, "host_s": time.perf_counter() - t0}


def savez_fast(path, compresslevel=0, **arrays):
    """np.savez / np.savez_compressed with a choice of deflate level (same .npz container, np.load reads it).  float64
    connectivity values do not compress -- 5 % at NumPy's fixed level 6 (88.8 of 94.2 MB for the band sums of one
    full-size dyad) for 3.9 s of a host core, more than the dyad's preprocessing and 100x its GPU time; level 1 is hardly
    faster (3.4 s).  0 = stored (default), 1..9 = deflate."""
    import zipfile
    method = zipfile.ZIP_STORED if int(compresslevel) <= 0 else zipfile.ZIP_DEFLATED
    kw = {} if method == zipfile.ZIP_STORED else {"compresslevel": int(compresslevel)}
    with zipfile.ZipFile(path, mode="w", compression=method, allowZip64=True, **kw) as zf:
        for key, val in arrays.items():
            with zf.open(key + ".npy", mode="w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


def resolve_pivoted_fallback(pivoted_fallback, engine_setting: bool, auto: bool):
    """`run(pivoted_fallback=...)` against the engine's own setting -> (on?, the `flags` keyword of the engine calls).  None
    takes the engine's; False cannot switch off what the engine ORs into every call.  Needs no GPU."""
    from . import _lib
    if pivoted_fallback is not None and not isinstance(pivoted_fallback, bool):
        raise ValueError(f"pivoted_fallback must be True, False or None, got {pivoted_fallback!r}")
    if pivoted_fallback is False and engine_setting:
        raise ValueError("escan_batch.run(pivoted_fallback=False): the engine was made with pivoted_yw (or "
                         "HYPERMVAR_YW_PIVOTED is set) and adds the fallback to every call; pass an engine without it")
    pivoted = bool(engine_setting) if pivoted_fallback is None else pivoted_fallback
    if pivoted and auto:
        raise ValueError("escan_batch.run(pivoted_fallback=True): the automatic model order (model_order=None) is not "
                         "available with the pivoted Yule-Walker fallback (an LU gives no criterion curve); pass an integer "
                         "model_order")
    return pivoted, ({"flags": _lib.FLAG_YW_PIVOTED} if pivoted else {})


class DecimateConfigError(ValueError):
    """`run(decimate=q)` cannot work at this rate, window and order: raised out of the batch, not logged per segment."""


def resolve_decimate(decimate, design="decimate"):
    """`run(decimate=..., decimate_design=...)` -> None, or (q, the design's name for the meta entry).  Needs no GPU."""
    if decimate is None:
        return None
    from . import _lib
    from .eeg_io import decimation_taps
    if isinstance(decimate, bool) or not isinstance(decimate, (int, np.integer)):
        raise DecimateConfigError(f"decimate must be None or an integer in 2..{_lib.MAX_DECIMATE}, got {decimate!r}")
    try:
        decimation_taps(int(decimate), design)        # the factor's range and the design, as the engine will see them
    except ValueError as e:
        raise DecimateConfigError(f"escan_batch.run(decimate={decimate!r}): {e}") from None
    return int(decimate), design if isinstance(design, str) else "taps"


def decimated_segment(q, fs, window_s, m, order, freqs=None):
    """What `run(decimate=q)` does to a segment recorded at `fs` with m channels -> (fs / q, window length in decimated
    samples).  Refuses, before anything is computed, a requested frequency that is not below the new Nyquist rate and a
    window with no more samples than the m * order unknowns of one row of the model.  Needs no GPU."""
    fs_new = float(fs) / int(q)
    W = int(round(window_s * fs_new))
    if freqs is not None and np.size(freqs) and float(np.max(freqs)) >= fs_new / 2.0:
        raise DecimateConfigError(
            f"escan_batch.run(decimate={q}): the requested frequencies reach {float(np.max(freqs)):g} Hz, which is not below "
            f"the Nyquist rate {fs_new / 2.0:g} Hz of the decimated recording ({fs:g} Hz / (2 * {q}))")
    if W <= int(m) * int(order):
        raise DecimateConfigError(
            f"escan_batch.run(decimate={q}): a {window_s:g} s window has {W} samples at {fs_new:g} Hz, no more than the "
            f"{m} channels x order {order} = {int(m) * int(order)} unknowns of one row of the model: the normal equations "
            f"would be rank-deficient (the rank trap of decimating without lowering the order).  Use a lower model order "
            f"(order {max(1, int(order) // int(q))} at {fs_new:g} Hz spans the time of order {order} at {fs:g} Hz), "
            f"a longer window or fewer channels")
    return fs_new, W


def run(root, out_dir, tasks=None, window_s=2.0, overlap=0.5, model_order=8, freqs=None, bands=hdist.DEFAULT_BANDS,
        low_cutoff_hz=None, high_cutoff_hz=None, channel_subset=None, with_psd=False, psd_fmin=1.0, psd_fmax=30.0,
        psd_bandwidth=2.0, save_full=False, skip_existing=True, reader=None, engine=None, world=1, rank=0,
        verbose=True, prefetch=2, timing=None, save_workers=4, compresslevel=0, measures=("ffdtf",), significance=None,
        max_model_order=20, crit_type="AIC", validation_lags=None, block_granger=False, pivoted_fallback=None,
        decimate=None, decimate_design="decimate", phase_sync=None):
    """Process every dyad under <root>/EEG.  Per dyad one `<out_dir>/<dyad>_ffdtf.npz` with, per segment `<task>/<event>`:
        <seg>/ffdtf_bands   (windows, n, n, n_bands)   band-integrated ffDTF of every window
        <seg>/ffdtf         (windows, n, n, F)         only with save_full=True (8.4 MB per window at 64 channels)
        <seg>/starts        (windows,)                 first sample of every window inside the segment
        <seg>/psd, <seg>/psd_freqs                     multitaper PSD of the segment block (with_psd=True)
        <seg>/ddtf_bands, <seg>/gpdc_bands (and <seg>/ddtf, <seg>/gpdc with save_full=True)
                                                       with measures=(..., "ddtf", "gpdc"): dDTF / GPDC of the same windows
        <seg>/<measure>_bands_p, _p_fwe, _null_mean, _null_std   (windows, n, n, n_bands)
        <seg>/<measure>_bands_n_valid                           (windows,)
                                                       with significance=dict(null=..., n_surrogates=..., seed=...,
                                                       min_shift=None): the surrogate test of every computed measure
                                                       (`Engine.sliding_significance`; split = the child's channel count,
                                                       the same seed for every segment)
        <seg>/orders        (windows,) int32           only with model_order=None: the order `mvar_criterion(window,
                                                       max_model_order, crit_type)` (mtmvar.py:551-601) picks for every
                                                       window, selected on the device inside the same call (0: failed
                                                       window); meta then says "model_order": "auto" and carries
                                                       `max_model_order` and `crit_type`.  Every measure of a window uses
                                                       that window's order.  Not offered together with `significance`.
        <seg>/whiteness_q, <seg>/whiteness_p   (windows, 3)   only with validation_lags=h (an integer): Box-Pierce, Li-McLeod and
                                                       Hosking portmanteau statistics of every window's residuals over h
                                                       lags and their chi-square tails (`Engine.model_validation`; the
                                                       segment's own windows and order -- `model_order`, or the per-window
                                                       automatic one), NaN for a singular window
        <seg>/block_gc_bands (windows, 2, n_bands), <seg>/block_gc_time (windows, 4)
                                                       only with block_granger=True: band-summed spectral block Granger
                                                       causality child -> caregiver (index 0) and caregiver -> child
                                                       (index 1) and the time-domain values (`Engine.sliding_block_granger`;
                                                       split = the child's channel count); meta then says
                                                       "block_granger": true.  Needs an integer model_order.
        <seg>/phase_<measure>   (windows, n_bands, n, n)   only with phase_sync=(...), a tuple out of ("plv", "ciplv", "coh",
                                                       "imcoh"): band-limited phase synchrony of the MVAR leg's windows
                                                       in the bands `bands` (Hz), from the segment block after the same
                                                       filtering and decimation (`Engine.sliding_phase_sync`; the analytic
                                                       signal is circular over the segment).  NaN where a window holds a
                                                       non-finite sample or, for coh / imcoh, a channel of zero power; meta
                                                       then says "phase_sync": [...].  None (default): nothing changes.
        <seg>/acf_fraction  (windows,)                 with validation_lags: share of the residual correlations beyond
                                                       1.96 / sqrt(N)
      pivoted_fallback: windows that the Yule-Walker solvers refuse are solved by the pivoted LU, as the reference's
      `np.linalg.solve` would (`Engine(pivoted_yw=...)`); None takes the engine's setting.  Every segment's meta entry then
      carries "yw_routes": {"recursion", "ldlt", "lu"}, how many of its windows each solver took (one more K1 + K2 over the
      segment).  Needs an integer model_order.
      decimate: an integer q in 2..32 -- every segment block is decimated by q on the device right after it crosses PCIe
      (`Engine.decimate`, anti-aliased FIR; `decimate_design`: "decimate" as scipy.signal.decimate(ftype='fir',
      zero_phase=True), "resample_poly" as scipy.signal.resample_poly(x, 1, q), or a 1-D array of taps), before the MVAR and
      PSD legs.  `window_s` and `overlap` then mean seconds at the new rate fs / q, `starts` are in decimated samples, meta
      carries "decimate": q, "decimate_design" and the new "fs", and every segment entry its decimated "fs" and "samples".
      The block is not z-scored again: a low-passed signal loses only its stop-band power.  ValueError, raised out of the
      batch, if a requested frequency is not below fs / (2 q) or if the decimated window has no more samples than
      channels x model_order (the rank trap: lower the order with the rate).  None (default): nothing changes.
      plus `channels`, `freqs`, `meta` (JSON, its `measures` field lists what was computed, `significance` the test).  Returns {"done": [...], "skipped": [...], "failed": [(dyad, error)],
      "timing": {...}}.
    A window whose fit is singular is NaN-filled, not fatal (the reference would raise and lose the dyad); a segment that
    cannot be processed is logged in the dyad's meta and does not discard the dyad's other segments.
    Pipeline: reading + filtering + cutting of the next `prefetch` dyads runs in worker threads while the GPU works on the
    current one (every task file is filtered once, not once per event); per segment the block crosses PCIe once and the
    PSD runs on a second HIP stream beside the MVAR kernels.  `timing` (optional dict) receives the host / GPU split."""
    import concurrent.futures as cf

    import torch
    measures = tuple(measures)
    unknown = [m_ for m_ in measures if m_ not in MEASURES]
    if unknown or "ffdtf" not in measures or len(set(measures)) != len(measures):
        raise ValueError(f"measures must list 'ffdtf' and any of {MEASURES[1:]} once each, got {measures}")
    if significance is not None:
        from .surrogates import check_significance_dict
        significance = check_significance_dict(significance)
    if phase_sync is not None:                      # the arguments, before anything touches a device
        from .eeg_io import resolve_bands_hz, resolve_phase_measures
        phase_sync = resolve_phase_measures(phase_sync)
        resolve_bands_hz(bands, float("inf"))       # not empty, pairs, lo < hi; the edges against fs / 2 per segment
    auto = model_order is None
    if block_granger and auto:
        raise ValueError("escan_batch.run(block_granger=True): the automatic model order (model_order=None) is not "
                         "available for block Granger causality; pass an integer model_order")
    if auto:
        from .engine import auto_order_args, no_auto_order
        pmax, _ = auto_order_args(max_model_order, crit_type, 1 << 62)     # (the window length is checked per segment)
        if significance is not None:
            no_auto_order(None, "escan_batch.run(significance=...)")
    order = None if auto else int(model_order)
    order_kw = dict(max_model_order=pmax, crit_type=crit_type) if auto else {}
    eng = engine or default_engine()
    pivoted, yw_kw = resolve_pivoted_fallback(pivoted_fallback, eng.pivoted_yw, auto)
    dec = resolve_decimate(decimate, decimate_design)
    reader = reader or xarray_reader
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    say = print if verbose else (lambda *a, **k: None)
    tree = discover_dyads(root, tasks)
    dyads = sorted(tree)
    mine = [dyads[k] for k in hdist.shard_dyads(len(dyads), world, rank)]
    say(f"[INFO] {len(dyads)} dyads under {root}; rank {rank}/{world} takes {len(mine)}")
    done, skipped, failed = [], [], []
    todo = []
    for dyad in mine:
        if skip_existing and (out_dir / f"{dyad}_ffdtf.npz").exists():
            say(f"[SKIP] {dyad}: {dyad}_ffdtf.npz exists")
            skipped.append(dyad)
        else:
            todo.append(dyad)
    tm = {"wall_s": 0.0, "host_prepare_s": 0.0, "wait_for_host_s": 0.0, "gpu_s": 0.0, "save_s": 0.0, "dyads": []}
    t_all = time.perf_counter()
    psd_stream = torch.cuda.Stream(eng.device) if with_psd else None
    # two pools: the writes (3 - 4 s of zlib per full-size dyad when compressed) must not take the workers that prepare the
    # next dyads, or the GPU waits for its input behind somebody's output
    pool = cf.ThreadPoolExecutor(max_workers=max(1, int(prefetch)))
    save_pool = cf.ThreadPoolExecutor(max_workers=max(1, int(save_workers)))
    futures, saves = {}, []

    def submit(k):
        if k < len(todo) and k not in futures:
            futures[k] = pool.submit(prepare_dyad, todo[k], tree[todo[k]], reader, low_cutoff_hz, high_cutoff_hz, channel_subset)

    for k in range(min(len(todo), max(1, int(prefetch)))):
        submit(k)
    try:
        for k, dyad in enumerate(todo):
            target = out_dir / f"{dyad}_ffdtf.npz"
            try:
                tw = time.perf_counter()
                prep = futures.pop(k).result()
                wait_s = time.perf_counter() - tw
                submit(k + max(1, int(prefetch)))
                for line in prep["notes"]:
                    say(line)
                result, meta = {}, {"dyad": dyad, "segments": [], "failed_segments": [],
                                    "model_order": "auto" if auto else order,
                                    "window_s": window_s, "overlap": overlap, "measures": list(measures),
                                    "created": time.strftime("%Y-%m-%dT%H:%M:%S")}
                if auto:
                    meta["max_model_order"], meta["crit_type"] = pmax, crit_type
                if significance is not None:
                    meta["significance"] = dict(significance)
                if block_granger:
                    meta["block_granger"] = True
                if dec is not None:
                    meta["decimate"], meta["decimate_design"] = dec
                if phase_sync is not None:
                    meta["phase_sync"] = list(phase_sync)
                names_out, freqs_out = None, None
                tg = time.perf_counter()
                pending = []                                       # device results of this dyad, fetched after the last launch
                for seg in prep["segments"]:
                    key = f"{seg['task']}/{seg['event']}"
                    try:
                        block, fs = seg["block"], seg["fs"]
                        T = block.shape[1]
                        if dec is None:
                            W = int(round(window_s * fs))
                        else:
                            fs, W = decimated_segment(dec[0], fs, window_s, block.shape[0], pmax if auto else order, freqs)
                            T = -(-T // dec[0])
                        hop = max(1, int(round(W * (1.0 - overlap))))
                        if T < W:
                            say(f"[SKIP] {dyad} {key}: {T} samples < one window ({W})")
                            continue
                        pos = hop_positions(T, W, hop)            # fixed hop; the tail shorter than one hop is dropped
                        f = np.asarray(freqs if freqs is not None else np.arange(0.5, min(fs / 2.0, 128.0) + 1e-9, 0.5))
                        xd = eng.to_device(block[None])
                        if dec is not None:
                            xd = eng.decimate(xd, dec[0], decimate_design)
                        rec_i, st_i = window_items(1, pos, eng.device)
                        psd_dev = None
                        if with_psd:                               # second stream, same resident block
                            from .psd import compute_psd_multitaper_device
                            psd_stream.wait_stream(torch.cuda.current_stream(eng.device))
                            with torch.cuda.stream(psd_stream):
                                pf, psd_dev = compute_psd_multitaper_device(xd[0], fs, psd_fmin, psd_fmax, psd_bandwidth, engine=eng)
                            xd.record_stream(psd_stream)
                        lo, hi = hdist.band_bins(f, bands)
                        grid_w = regular_grid(pos, W, pmax if auto else order)
                        extra = {}                                 # dDTF / GPDC of the same windows, NaN-filled alike
                        if dec is not None:
                            extra["_decimated"] = (fs, T)
                        if save_full:
                            r = eng.sliding_ffdtf(xd, rec_i, st_i, W, order, f, fs, check="mask", grid=grid_w,
                                                  return_orders=auto, **order_kw, **yw_kw)
                            ff, bad = r[0], r[1]
                            bsum = eng.band_sums(ff, lo, hi)
                            ff.masked_fill_(bad.view(-1, 1, 1, 1), float("nan"))
                        else:          # the reduced product straight from K3's row workers: the full array is never written
                            ff = None
                            r = eng.sliding_ffdtf(xd, rec_i, st_i, W, order, f, fs, check="mask", grid=grid_w, bands=(lo, hi),
                                                  return_orders=auto, **order_kw, **yw_kw)
                            bsum, bad = r[0], r[1]
                        if auto:
                            extra["orders"] = r[2]
                        bsum.masked_fill_(bad.view(-1, 1, 1, 1), float("nan"))
                        for meas in (m_ for m_ in measures if m_ != "ffdtf"):
                            run_m = eng.sliding_ddtf if meas == "ddtf" else eng.sliding_gpdc
                            if save_full:
                                full_m, bad_m = run_m(xd, rec_i, st_i, W, order, f, fs, check="mask", grid=grid_w, **order_kw, **yw_kw)
                                red_m = eng.band_sums(full_m, lo, hi)
                                full_m.masked_fill_(bad_m.view(-1, 1, 1, 1), float("nan"))
                                extra[meas] = full_m
                            else:
                                red_m, bad_m = run_m(xd, rec_i, st_i, W, order, f, fs, check="mask", grid=grid_w,
                                                     bands=(lo, hi), **order_kw, **yw_kw)
                            red_m.masked_fill_(bad_m.view(-1, 1, 1, 1), float("nan"))
                            extra[f"{meas}_bands"] = red_m
                        if validation_lags is not None:          # K1 + K2 once more, then residuals and whiteness
                            fit_p = pmax if auto else order
                            R_v = eng.lagcov(xd, rec_i, st_i, W, fit_p)
                            if auto:
                                ar_v, _, ord_v, _, info_v = eng.yw_solve_auto(R_v, block.shape[0], W, crit_type)
                            else:
                                ar_v, _, _, info_v = eng.yw_solve(R_v, block.shape[0], **yw_kw)
                                ord_v = torch.full_like(info_v, fit_p)
                            val = eng.model_validation(xd, rec_i, st_i, W, ar_v, validation_lags, validate=False)
                            bad_v = (info_v != 0) | (val["info"] != 0)
                            extra["whiteness_q"] = val["q"].masked_fill(bad_v.view(-1, 1), float("nan"))
                            extra["acf_fraction"] = (val["acf_count"].to(torch.float64)
                                                     / float(int(validation_lags) * block.shape[0] ** 2)
                                                     ).masked_fill(bad_v, float("nan"))
                            extra["_whiteness_orders"] = ord_v
                        if block_granger:                        # the child block comes first (segment_block)
                            gc_f, gc_t, gc_bad = eng.sliding_block_granger(
                                xd, rec_i, st_i, W, order, f, fs, bands=(lo, hi), check="mask", grid=grid_w,
                                split=sum(1 for nm in seg["names"] if nm.endswith("_ch")), **yw_kw)
                            extra["block_gc_bands"] = gc_f.masked_fill_(gc_bad.view(-1, 1, 1), float("nan"))
                            extra["block_gc_time"] = gc_t.masked_fill_(gc_bad.view(-1, 1), float("nan"))
                        if phase_sync is not None:               # no model: the same windows, the bands in Hz
                            ps = eng.sliding_phase_sync(xd, rec_i, st_i, W, fs, bands, measures=phase_sync, check="nan")
                            for q_ in phase_sync:
                                extra[f"phase_{q_}"] = ps[q_]
                        if significance is not None:             # the child block comes first (segment_block)
                            split = sum(1 for nm in seg["names"] if nm.endswith("_ch"))
                            for meas in measures:
                                sig = eng.sliding_significance(xd, rec_i, st_i, W, order, f, fs, (lo, hi),
                                                               measure=meas, null=significance["null"],
                                                               n_surrogates=significance["n_surrogates"],
                                                               seed=significance["seed"], split=split,
                                                               min_shift=significance["min_shift"], check="nan", grid=grid_w)
                                for k_ in ("p", "p_fwe", "null_mean", "null_std", "n_valid"):
                                    extra[f"{meas}_bands_{k_}"] = sig[k_]
                        if pivoted:                              # which solver took each window: K1 + K2 once more
                            extra["_yw_routes"] = eng.window_routes(xd, rec_i, st_i, W, order)[0]
                        pending.append((seg, key, pos, W, f, bsum, ff if save_full else None, bad, psd_dev, pf if with_psd else None,
                                        extra))
                    except DecimateConfigError:                    # the batch's own arguments: nothing to log per segment
                        raise
                    except Exception as e:                         # one bad segment does not discard the dyad
                        meta["failed_segments"].append({"segment": key, "error": f"{type(e).__name__}: {e}"})
                        say(f"Failed segment: {dyad} {key} -> {e}")
                if psd_stream is not None:
                    torch.cuda.current_stream(eng.device).wait_stream(psd_stream)
                for seg, key, pos, W, f, bsum, ff, bad, psd_dev, pf, extra in pending:
                    result[f"{key}/ffdtf_bands"] = bsum.cpu().numpy()
                    if ff is not None:
                        result[f"{key}/ffdtf"] = ff.cpu().numpy()
                    ord_v = extra.pop("_whiteness_orders", None)
                    routes = extra.pop("_yw_routes", None)
                    decimated = extra.pop("_decimated", None)
                    for name, arr in extra.items():
                        result[f"{key}/{name}"] = arr.cpu().numpy()
                    if ord_v is not None:
                        q_v = result[f"{key}/whiteness_q"]
                        _, result[f"{key}/whiteness_p"], _ = validation_p_values(
                            q_v, np.zeros((len(q_v), 1)), ord_v.cpu().numpy(), seg["block"].shape[0], int(validation_lags),
                            np.isnan(q_v[:, 0]))
                    result[f"{key}/starts"] = np.asarray(pos)
                    if psd_dev is not None:
                        result[f"{key}/psd"], result[f"{key}/psd_freqs"] = psd_dev.cpu().numpy(), pf
                    n_bad = int(bad.sum().item())
                    T = seg["block"].shape[1]
                    meta["segments"].append({"task": seg["task"], "event": seg["event"], "start_s": seg["start_s"],
                                             "duration_s": seg["duration_s"], "fs": seg["fs"], "samples": int(T),
                                             "windows": int(len(pos)), "window": int(W), "singular_windows": n_bad})
                    if routes is not None:
                        from .engine import route_counts
                        meta["segments"][-1]["yw_routes"] = route_counts(routes)
                    if decimated is not None:
                        meta["fs"], T = decimated
                        meta["segments"][-1].update(fs=meta["fs"], samples=int(T))
                    names_out, freqs_out = seg["names"], f
                    say(f"[OK] {dyad} {key}: {seg['block'].shape[0]} ch x {T} samples, {len(pos)} windows"
                        + (f", {n_bad} singular" if n_bad else ""))
                torch.cuda.synchronize(eng.device)
                gpu_s = time.perf_counter() - tg
                if not meta["segments"]:
                    say(f"[SKIP] {dyad}: no complete child + caregiver segment")
                    skipped.append(dyad)
                    continue
                # the write goes to a worker pool of its own (stored by default; deflate -- compresslevel > 0 -- costs 3 - 4 s of
                # a core per full-size dyad, zlib outside the GIL): the GPU and the next dyad's host work do not wait for it
                def _save(target=target, names_out=names_out, freqs_out=freqs_out, meta=meta, result=result):
                    t0 = time.perf_counter()
                    tmp = target.with_suffix(".tmp.npz")
                    savez_fast(tmp, compresslevel, channels=np.asarray(names_out), freqs=freqs_out,
                               bands=np.asarray(bands, dtype=np.float64), meta=np.asarray(json.dumps(meta)), **result)
                    tmp.replace(target)                       # a file that exists is complete (skip-if-exists relies on it)
                    return time.perf_counter() - t0
                saves.append((dyad, target, save_pool.submit(_save)))
                save_s = 0.0
                done.append(dyad)
                tm["host_prepare_s"] += prep["host_s"]; tm["wait_for_host_s"] += wait_s
                tm["gpu_s"] += gpu_s; tm["save_s"] += save_s
                tm["dyads"].append({"dyad": dyad, "host_prepare_s": prep["host_s"], "waited_for_host_s": wait_s,
                                    "gpu_s": gpu_s, "save_s": save_s, "segments": len(meta["segments"])})
            except DecimateConfigError:
                raise
            except Exception as e:                  # one bad dyad does not stop the batch (export_..._batch.py:93-99)
                failed.append((dyad, f"{type(e).__name__}: {e}"))
                say(f"Failed: {dyad} -> {e}")
                submit(k + max(1, int(prefetch)))
        for dyad, target, fut in saves:                   # every file on disk before the call returns
            try:
                tm["save_s"] += fut.result()
                say(f"[SAVED] {target}")
            except Exception as e:
                done.remove(dyad)
                failed.append((dyad, f"{type(e).__name__}: {e}"))
                say(f"Failed: {dyad} -> {e}")
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
        save_pool.shutdown(wait=True)
    tm["wall_s"] = time.perf_counter() - t_all
    tm["gpu_busy_fraction_of_wall"] = tm["gpu_s"] / tm["wall_s"] if tm["wall_s"] > 0 else 0.0
    if timing is not None:
        timing.update(tm)
    say(f"Finished. Success: {len(done)}, Skipped: {len(skipped)}, Failed: {len(failed)}")
    with open(out_dir / ("batch.log" if world == 1 else f"batch_rank{rank}.log"), "a", encoding="utf-8") as log:
        log.write(f"Finished. Success: {len(done)}, Skipped: {len(skipped)}, Failed: {len(failed)}\n")
        if failed:
            log.write("Failed dyads:\n")
            for dyad, err in failed:
                log.write(f"  - {dyad}: {err}\n")
    return {"done": done, "skipped": skipped, "failed": failed, "timing": tm}


def _event_block(files, reader, event, low_cutoff_hz, high_cutoff_hz, channel_subset):
    """Host part of one dyad of `run_pseudo_dyads`: the named event of the task, through `segment_block`.  Returns
    (block, names, fs), or the reason there is none."""
    if "ch" not in files or "cg" not in files:
        return f"missing {'child' if 'ch' not in files else 'caregiver'} file"
    child, caregiver = reader(files["ch"]), reader(files["cg"])
    for name, start, dur in decode_events(child["attrs"]):
        if name == event:
            return segment_block(child, caregiver, start, dur, low_cutoff_hz, high_cutoff_hz, channel_subset)
    return f"no event {event!r}"


def run_pseudo_dyads(root, out_dir, task, event, window_s=2.0, overlap=0.5, model_order=8, freqs=None,
                     bands=hdist.DEFAULT_BANDS, low_cutoff_hz=None, high_cutoff_hz=None, channel_subset=None,
                     measures=("ffdtf",), n_surrogates=None, seed=None, min_common_fraction=0.9, reader=None, engine=None,
                     verbose=True, prefetch=2, compresslevel=0):
    """Pseudo-dyad (shuffled-partner) test of one event across every dyad under <root>/EEG: all dyads saw the same film, so
    the child of one dyad beside the caregiver of another shares the stimulus and nothing else
    (`Engine.pseudo_dyad_significance`; split = the child's channel count).  The event `event` of task `task` of every
    dyad is prepared as in `run` (`segment_block`, in a pool of `prefetch` worker threads), the segments are cropped to
    the shortest one, and windows of `window_s` seconds slide over the common length with `run`'s hop rule.  A dyad without
    both files or without the event gets a `[SKIP]` line, and so does one whose segment is shorter than
    `min_common_fraction` of the longest (it would shorten everybody's); sampling rates and channel names must agree; at
    least 2 dyads must remain.  n_surrogates=None: the exhaustive cyclic partner set, no seed; an integer: seeded draws.
    Writes `<out_dir>/pseudo_dyads_<task>_<event>.npz`:
        <measure>_bands, _p, _p_fwe, _null_mean, _null_std   (dyads, windows, n, n, n_bands)     per dyad
        <measure>_n_valid                                    (dyads, windows)
        group_<measure>_bands, _p, _p_fwe, _null_mean, _null_std  (windows, n, n, n_bands)       across dyads
        group_<measure>_n_valid                              (windows,)
        dyads, channels, freqs, starts, partners (S, dyads), meta (JSON)
    A window whose observed fit is singular has NaN statistics.  A dyad whose files cannot be read or prepared
    is reported with a `[FAILED]` line and listed under "failed", as in `run`; it is not one of the skipped.
    Returns {"path", "dyads", "skipped": [(dyad, reason)], "failed": [(dyad, error)]}."""
    import concurrent.futures as cf

    from .engine import no_auto_order
    from .surrogates import partner_count
    measures = tuple(measures)
    unknown = [m_ for m_ in measures if m_ not in MEASURES]
    if unknown or not measures or len(set(measures)) != len(measures):
        raise ValueError(f"measures must list any of {MEASURES} once each, got {measures}")
    no_auto_order(model_order, "escan_batch.run_pseudo_dyads")
    if not 0.0 < float(min_common_fraction) <= 1.0:
        raise ValueError(f"min_common_fraction must be in (0, 1], got {min_common_fraction!r}")
    partner_count(n_surrogates, seed)                                   # the surrogate count and its seed, before any file
    reader = reader or xarray_reader
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    say = print if verbose else (lambda *a, **k: None)
    tree = discover_dyads(root, [task])
    skipped, failed, blocks = [], [], {}
    with cf.ThreadPoolExecutor(max_workers=max(1, int(prefetch))) as pool:
        futures = {dyad: pool.submit(_event_block, tree[dyad].get(task, {}), reader, event, low_cutoff_hz,
                                     high_cutoff_hz, channel_subset) for dyad in sorted(tree)}
        for dyad, fut in futures.items():
            try:
                got = fut.result()
            except Exception as e:                      # one bad dyad does not stop the others; reported, as in `run`
                failed.append((dyad, f"{type(e).__name__}: {e}"))
                say(f"[FAILED] {dyad} {task}/{event}: {failed[-1][1]}")
                continue
            if isinstance(got, str):
                say(f"[SKIP] {dyad} {task}/{event}: {got}")
                skipped.append((dyad, got))
            else:
                blocks[dyad] = got
    if blocks:
        first = next(iter(blocks))
        _, names, fs = blocks[first]
        for dyad, (_, nm, f_) in blocks.items():
            if f_ != fs:
                raise ValueError(f"sampling rates differ: {first} has {fs}, {dyad} has {f_}")
            if nm != names:
                raise ValueError(f"channel names differ between {first} and {dyad}")
        longest = max(b.shape[1] for b, _, _ in blocks.values())
        for dyad in [d_ for d_, (b, _, _) in blocks.items() if b.shape[1] < float(min_common_fraction) * longest]:
            why = f"{blocks[dyad][0].shape[1]} samples < {min_common_fraction} of the longest segment ({longest})"
            say(f"[SKIP] {dyad} {task}/{event}: {why}")
            skipped.append((dyad, why))
            del blocks[dyad]
    if len(blocks) < 2:
        raise ValueError(f"the pseudo-dyad test needs at least 2 dyads with {task}/{event}, found {len(blocks)}" +
                         (f" ({len(failed)} failed: " + "; ".join(f"{d_}: {e_}" for d_, e_ in failed) + ")" if failed else ""))
    dyads = sorted(blocks)
    T = min(blocks[d_][0].shape[1] for d_ in dyads)
    x = np.stack([blocks[d_][0][:, :T] for d_ in dyads])               # cropped to the shortest segment
    split = sum(1 for nm in names if nm.endswith("_ch"))               # the child block comes first (segment_block)
    W = int(round(window_s * fs))
    hop = max(1, int(round(W * (1.0 - overlap))))
    if T < W:
        raise ValueError(f"{task}/{event}: the common length ({T} samples) is shorter than one window ({W})")
    pos = hop_positions(T, W, hop)
    f = np.asarray(freqs if freqs is not None else np.arange(0.5, min(fs / 2.0, 128.0) + 1e-9, 0.5))
    lo, hi = hdist.band_bins(f, bands)
    eng = engine or default_engine()
    import torch
    xd = eng.to_device(x)
    starts = torch.as_tensor(np.asarray(pos, dtype=np.int64)).to(eng.device)
    result, partners = {}, None
    for meas in measures:
        sig = eng.pseudo_dyad_significance(xd, starts, W, int(model_order), f, fs, (lo, hi), measure=meas, split=split,
                                           n_surrogates=n_surrogates, seed=seed, check="nan")
        for level, d_ in (("", sig), ("group_", sig["group"])):
            result[f"{level}{meas}_bands"] = d_["observed"].cpu().numpy()
            for k_ in ("p", "p_fwe", "null_mean", "null_std", "n_valid"):
                result[f"{level}{meas}_{k_}"] = d_[k_].cpu().numpy()
        partners = sig["partners"].cpu().numpy()
        say(f"[OK] {task}/{event} {meas}: {len(dyads)} dyads x {len(pos)} windows, {partners.shape[0]} partner sets")
    meta = {"task": task, "event": event, "dyads": dyads, "skipped": [list(s_) for s_ in skipped],
            "failed": [list(s_) for s_ in failed], "model_order": int(model_order),
            "window_s": window_s, "overlap": overlap, "window": W, "fs": fs, "samples": int(T), "split": int(split),
            "measures": list(measures), "n_surrogates": None if n_surrogates is None else int(n_surrogates), "seed": seed,
            "min_common_fraction": float(min_common_fraction), "created": time.strftime("%Y-%m-%dT%H:%M:%S")}
    target = out_dir / f"pseudo_dyads_{task}_{event}.npz"
    tmp = target.with_suffix(".tmp.npz")
    savez_fast(tmp, compresslevel, dyads=np.asarray(dyads), channels=np.asarray(names), freqs=f, starts=np.asarray(pos),
               partners=partners, bands=np.asarray(bands, dtype=np.float64), meta=np.asarray(json.dumps(meta)), **result)
    tmp.replace(target)
    say(f"[SAVED] {target}")
    return {"path": target, "dyads": dyads, "skipped": skipped, "failed": failed}
