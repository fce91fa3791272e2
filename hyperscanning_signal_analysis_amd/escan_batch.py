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
import typing
from pathlib import Path

import numpy as np

from . import distributed as hdist
from .eeg_io import filter_eeg
from .engine import default_engine
from .sliding import hop_positions, regular_grid, validation_p_values, window_items

__all__ = ["discover_dyads", "decode_events", "segment_block", "prepare_dyad", "run", "run_pseudo_dyads", "savez_fast",
           "xarray_reader", "resolve_decimate", "decimated_segment", "DecimateConfigError", "resolve_settings",
           "segment_geometry", "child_channels"]

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


def _member(rec, low_cutoff_hz, high_cutoff_hz, channel_subset):
    """One member's whole file -> (x (time, channel), channel names, time, fs): filtering + mastoid drop with
    load_eeg_signals' semantics, WITHOUT its trim and z-score, then the requested channels in the order asked for."""
    fs = float(rec["attrs"].get("sampling_freq", rec["attrs"].get("sampling_frequency_Hz", 128.0)))
    x = filter_eeg(rec["data_tc"], fs, low_cutoff_hz, high_cutoff_hz)
    names = [str(c) for c in rec["channels"]]
    keep = [k for k, c in enumerate(names) if c not in ("M1", "M2")]
    x, ch = x[:, keep], [names[k] for k in keep]
    if channel_subset is not None:
        idx = [ch.index(c) for c in channel_subset if c in ch]
        if not idx:
            raise ValueError(f"None of the requested channels {channel_subset} found. Available: {ch}")
        x, ch = x[:, idx], [ch[k] for k in idx]
    return x, ch, np.asarray(rec["time"], dtype=np.float64), fs


def _members(child, caregiver, low_cutoff_hz, high_cutoff_hz, channel_subset):
    """`_member` of the child and of the caregiver, in that order; their sampling rates must agree."""
    members = [_member(rec, low_cutoff_hz, high_cutoff_hz, channel_subset) for rec in (child, caregiver)]
    if members[0][3] != members[1][3]:
        raise ValueError(f"sampling rates differ: {members[0][3]} vs {members[1][3]}")
    return members


def _cut_event(members, start_s, duration_s):
    """One event out of both members' filtered files (`_members`) -> (block, names): each cut to
    start <= t <= start + duration (io_utils.py:148-150) and z-scored per channel inside the segment, the child stacked on the
    caregiver on their common length."""
    parts, names = [], []
    for (role, _), (x, ch, t, fs) in zip(ROLES, members):
        mask = (t >= start_s) & (t <= start_s + duration_s)
        seg = np.ascontiguousarray(x[mask].T)
        sd = np.std(seg, axis=1, keepdims=True)
        sd[sd == 0] = 1.0
        parts.append((seg - np.mean(seg, axis=1, keepdims=True)) / sd)
        names += [f"{c}_{role}" for c in ch]
    T = min(p.shape[1] for p in parts)
    return np.vstack([p[:, :T] for p in parts]), names


def child_channels(names):
    """How many of a block's channels are the child's: the `split` of the block measures (the child block comes first)."""
    return sum(1 for nm in names if nm.endswith("_ch"))


def segment_block(child, caregiver, start_s, duration_s, low_cutoff_hz=None, high_cutoff_hz=None, channel_subset=None):
    """(block (2 n_ch, T) z-scored, names, fs) of one event: both members filtered over their whole file, cut to the
    event, z-scored per channel inside the segment, stacked child first on their common length."""
    members = _members(child, caregiver, low_cutoff_hz, high_cutoff_hz, channel_subset)
    block, names = _cut_event(members, start_s, duration_s)
    return block, names, members[0][3]


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
        child, caregiver = reader(files["ch"]), reader(files["cg"])
        members = _members(child, caregiver, low_cutoff_hz, high_cutoff_hz, channel_subset)         # whole files, once
        for name, start, dur in decode_events(child["attrs"]):
            block, names = _cut_event(members, start, dur)
            segs.append({"task": task, "event": name, "start_s": start, "duration_s": dur, "fs": members[0][3],
                         "block": block, "names": names})
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


class _Settings(typing.NamedTuple):
    """What `run`'s keyword arguments come to (`resolve_settings`); `run_pseudo_dyads` fills the fields that
    `segment_geometry` reads."""
    window_s: float
    overlap: float
    freqs: object                       # None: 0.5 Hz steps up to the Nyquist rate of every segment
    bands: tuple
    measures: tuple
    order: int | None                   # None: the automatic order of every window
    fit_order: int                      # lags of a fit: the order, or max_model_order of the automatic order
    crit_type: str = "AIC"
    order_kw: dict = {}                 # max_model_order and crit_type of the engine calls, with the automatic order only
    significance: dict | None = None
    phase_sync: tuple | None = None
    validation_lags: int | None = None
    block_granger: bool = False
    pivoted: bool = False
    yw_kw: dict = {}                    # the `flags` keyword of the engine calls, with the pivoted fallback only
    decimate: tuple | None = None       # (q, the design's name for the meta entry)
    decimate_design: object = "decimate"
    psd: tuple | None = None            # (fmin, fmax, bandwidth)
    save_full: bool = False
    phase_lag: tuple | None = None


def resolve_settings(engine=None, *, window_s=2.0, overlap=0.5, model_order=8, freqs=None, bands=hdist.DEFAULT_BANDS,
                     with_psd=False, psd_fmin=1.0, psd_fmax=30.0, psd_bandwidth=2.0, save_full=False, measures=("ffdtf",),
                     significance=None, max_model_order=20, crit_type="AIC", validation_lags=None, block_granger=False,
                     pivoted_fallback=None, decimate=None, decimate_design="decimate", phase_sync=None,
                     phase_lag=None):
    """`run`'s keyword arguments (same names, same defaults) -> (`_Settings`, the engine).  What needs no engine is refused
    first: the measures, the significance dict, the phase measures and bands, then the automatic order where it is not
    offered.  Only then the engine is made (engine=None: `default_engine()`), the pivoted fallback is resolved against its
    setting, and the decimation last.  Nothing is created or read."""
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
    if phase_lag is not None:                       # a family of its own names ("pli", "wpli", "dwpli")
        from .eeg_io import resolve_bands_hz, resolve_phase_lag_measures
        phase_lag = resolve_phase_lag_measures(phase_lag)
        resolve_bands_hz(bands, float("inf"))
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
    return _Settings(window_s, overlap, freqs, bands, measures, order, pmax if auto else order, crit_type, order_kw,
                     significance, phase_sync, validation_lags, bool(block_granger), pivoted, yw_kw, dec, decimate_design,
                     (psd_fmin, psd_fmax, psd_bandwidth) if with_psd else None, bool(save_full), phase_lag), eng


class _Geometry(typing.NamedTuple):
    """Where the windows of one segment lie (`segment_geometry`).  A segment shorter than one window has fs, T and W only."""
    fs: float                           # after the decimation, if any; so is T
    T: int
    W: int
    hop: int | None = None
    pos: np.ndarray | None = None       # first sample of every window; None: T < W
    freqs: np.ndarray | None = None
    lo: np.ndarray | None = None        # `band_bins` of the bands on `freqs`
    hi: np.ndarray | None = None
    grid: tuple | None = None           # `regular_grid`: what K1 may share between overlapping windows


def segment_geometry(cfg, fs, T, m):
    """Host arithmetic of one segment of m channels and T samples recorded at fs -> `_Geometry`: the window of
    `cfg.window_s` seconds and its hop at the (decimated) rate, the fixed-hop starts (the tail shorter than one hop is dropped),
    the frequency grid and the bands' bins on it.  `DecimateConfigError` as `decimated_segment` raises it."""
    if cfg.decimate is None:
        W = int(round(cfg.window_s * fs))
    else:
        fs, W = decimated_segment(cfg.decimate[0], fs, cfg.window_s, m, cfg.fit_order, cfg.freqs)
        T = -(-T // cfg.decimate[0])
    if T < W:
        return _Geometry(fs, T, W)
    hop = max(1, int(round(W * (1.0 - cfg.overlap))))
    pos = hop_positions(T, W, hop)
    f = np.asarray(cfg.freqs if cfg.freqs is not None else np.arange(0.5, min(fs / 2.0, 128.0) + 1e-9, 0.5))
    lo, hi = hdist.band_bins(f, cfg.bands)
    return _Geometry(fs, T, W, hop, pos, f, lo, hi, regular_grid(pos, W, cfg.fit_order))


class _Segment(typing.NamedTuple):
    """One launched segment (`_launch_segment`): device tensors, nothing fetched yet."""
    seg: dict                           # `prepare_dyad`'s entry
    key: str                            # <task>/<event>
    geo: _Geometry
    arrays: dict                        # saved as <key>/<name>, in this order; nothing else is in here
    bad: object                         # failed-window mask of the ffDTF call
    whiteness_orders: object = None     # the order every window was validated at
    routes: object = None               # which solver took every window
    decimated: tuple | None = None      # (fs, T) after the decimation
    psd: object = None
    psd_freqs: object = None


def _measure(eng, meas, xd, items, cfg, geo, **kw):
    """One measure of every window -> (band sums, the full array or None, failed-window mask, what else the call returned),
    failed windows NaN-filled.  save_full: the full array, then its band sums; else the reduced product straight from the
    measure's kernels, and the full array is never written."""
    call = getattr(eng, f"sliding_{meas}")
    kw.update(check="mask", grid=geo.grid, **cfg.order_kw, **cfg.yw_kw)
    if cfg.save_full:
        full, bad, *more = call(xd, *items, geo.W, cfg.order, geo.freqs, geo.fs, **kw)
        red = eng.band_sums(full, geo.lo, geo.hi)
        full.masked_fill_(bad.view(-1, 1, 1, 1), float("nan"))
    else:
        full = None
        red, bad, *more = call(xd, *items, geo.W, cfg.order, geo.freqs, geo.fs, bands=(geo.lo, geo.hi), **kw)
    red.masked_fill_(bad.view(-1, 1, 1, 1), float("nan"))
    return red, full, bad, more


def _launch_segment(eng, cfg, seg, key, geo, psd_stream):
    """Device work of one segment, nothing fetched: the block crosses PCIe once, the PSD goes to its own stream beside the
    MVAR kernels, every option adds its engine calls.  Returns the `_Segment`."""
    import torch
    m, W, f, fs = seg["block"].shape[0], geo.W, geo.freqs, geo.fs
    auto = cfg.order is None
    xd = eng.to_device(seg["block"][None])
    if cfg.decimate is not None:
        xd = eng.decimate(xd, cfg.decimate[0], cfg.decimate_design)
    items = window_items(1, geo.pos, eng.device)
    psd = pf = None
    if cfg.psd is not None:                             # second stream, same resident block
        from .psd import compute_psd_multitaper_device
        psd_stream.wait_stream(torch.cuda.current_stream(eng.device))
        with torch.cuda.stream(psd_stream):
            pf, psd = compute_psd_multitaper_device(xd[0], fs, *cfg.psd, engine=eng)
        xd.record_stream(psd_stream)
    arrays = {}
    arrays["ffdtf_bands"], full, bad, more = _measure(eng, "ffdtf", xd, items, cfg, geo, return_orders=auto)
    if full is not None:
        arrays["ffdtf"] = full
    if auto:
        arrays["orders"] = more[0]
    for meas in (m_ for m_ in cfg.measures if m_ != "ffdtf"):      # dDTF / GPDC of the same windows, NaN-filled alike
        red, full, _, _ = _measure(eng, meas, xd, items, cfg, geo)
        if full is not None:
            arrays[meas] = full
        arrays[f"{meas}_bands"] = red
    ord_v = None
    if cfg.validation_lags is not None:                 # K1 + K2 once more, then residuals and whiteness
        R_v = eng.lagcov(xd, *items, W, cfg.fit_order)
        if auto:
            ar_v, _, ord_v, _, info_v = eng.yw_solve_auto(R_v, m, W, cfg.crit_type)
        else:
            ar_v, _, _, info_v = eng.yw_solve(R_v, m, **cfg.yw_kw)
            ord_v = torch.full_like(info_v, cfg.fit_order)
        val = eng.model_validation(xd, *items, W, ar_v, cfg.validation_lags, validate=False)
        bad_v = (info_v != 0) | (val["info"] != 0)
        arrays["whiteness_q"] = val["q"].masked_fill(bad_v.view(-1, 1), float("nan"))
        arrays["acf_fraction"] = (val["acf_count"].to(torch.float64) / float(int(cfg.validation_lags) * m ** 2)
                                  ).masked_fill(bad_v, float("nan"))
    if cfg.block_granger:
        gc_f, gc_t, gc_bad = eng.sliding_block_granger(xd, *items, W, cfg.order, f, fs, bands=(geo.lo, geo.hi), check="mask",
                                                       grid=geo.grid, split=child_channels(seg["names"]), **cfg.yw_kw)
        arrays["block_gc_bands"] = gc_f.masked_fill_(gc_bad.view(-1, 1, 1), float("nan"))
        arrays["block_gc_time"] = gc_t.masked_fill_(gc_bad.view(-1, 1), float("nan"))
    if cfg.phase_sync is not None and cfg.phase_lag is not None:      # both families off one analytic signal
        ps, pl = eng.sliding_phase("escan_batch.run", xd, *items, W, fs, cfg.bands, sync=cfg.phase_sync, lag=cfg.phase_lag,
                                   check="nan")
    else:                                               # no model: the same windows, the bands in Hz
        ps = (eng.sliding_phase_sync(xd, *items, W, fs, cfg.bands, measures=cfg.phase_sync, check="nan")
              if cfg.phase_sync is not None else None)
        pl = (eng.sliding_phase_lag(xd, *items, W, fs, cfg.bands, measures=cfg.phase_lag, check="nan")
              if cfg.phase_lag is not None else None)
    for qs_, res_ in ((cfg.phase_sync, ps), (cfg.phase_lag, pl)):
        for q_ in qs_ or ():
            arrays[f"phase_{q_}"] = res_[q_]
    if cfg.significance is not None:
        sg = cfg.significance
        for meas in cfg.measures:
            sig = eng.sliding_significance(xd, *items, W, cfg.order, f, fs, (geo.lo, geo.hi), measure=meas, null=sg["null"],
                                           n_surrogates=sg["n_surrogates"], seed=sg["seed"],
                                           split=child_channels(seg["names"]), min_shift=sg["min_shift"], check="nan",
                                           grid=geo.grid)
            for k_ in ("p", "p_fwe", "null_mean", "null_std", "n_valid"):
                arrays[f"{meas}_bands_{k_}"] = sig[k_]
    routes = eng.window_routes(xd, *items, W, cfg.order)[0] if cfg.pivoted else None       # K1 + K2 once more
    return _Segment(seg, key, geo, arrays, bad, ord_v, routes, (fs, geo.T) if cfg.decimate is not None else None, psd, pf)


def _collect_segment(s, cfg, dyad, result, meta, say):
    """Host side of one launched segment: its arrays fetched into `result`, the chi-square tails of the whiteness
    statistics, its entry in meta["segments"] and its `[OK]` line."""
    seg, key, pos = s.seg, s.key, s.geo.pos
    m, T = seg["block"].shape
    for name, arr in s.arrays.items():
        result[f"{key}/{name}"] = arr.cpu().numpy()
    if s.whiteness_orders is not None:
        q_v = result[f"{key}/whiteness_q"]
        _, result[f"{key}/whiteness_p"], _ = validation_p_values(
            q_v, np.zeros((len(q_v), 1)), s.whiteness_orders.cpu().numpy(), m, int(cfg.validation_lags), np.isnan(q_v[:, 0]))
    result[f"{key}/starts"] = np.asarray(pos)
    if s.psd is not None:
        result[f"{key}/psd"], result[f"{key}/psd_freqs"] = s.psd.cpu().numpy(), s.psd_freqs
    n_bad = int(s.bad.sum().item())
    meta["segments"].append({"task": seg["task"], "event": seg["event"], "start_s": seg["start_s"],
                             "duration_s": seg["duration_s"], "fs": seg["fs"], "samples": int(T),
                             "windows": int(len(pos)), "window": int(s.geo.W), "singular_windows": n_bad})
    if s.routes is not None:
        from .engine import route_counts
        meta["segments"][-1]["yw_routes"] = route_counts(s.routes)
    if s.decimated is not None:
        meta["fs"], T = s.decimated
        meta["segments"][-1].update(fs=meta["fs"], samples=int(T))
    say(f"[OK] {dyad} {key}: {m} ch x {T} samples, {len(pos)} windows" + (f", {n_bad} singular" if n_bad else ""))


def _process_dyad(eng, cfg, dyad, prep, psd_stream, say):
    """GPU part of one prepared dyad -> (result {member: array}, meta, channel names, freqs).  Every segment is launched
    before the first one is fetched.  A segment shorter than a window is skipped; one that cannot be processed is logged in
    meta["failed_segments"] and does not discard the others; `DecimateConfigError` leaves the batch."""
    import torch
    auto = cfg.order is None
    result, meta = {}, {"dyad": dyad, "segments": [], "failed_segments": [], "model_order": "auto" if auto else cfg.order,
                        "window_s": cfg.window_s, "overlap": cfg.overlap, "measures": list(cfg.measures),
                        "created": time.strftime("%Y-%m-%dT%H:%M:%S")}
    if auto:
        meta["max_model_order"], meta["crit_type"] = cfg.fit_order, cfg.crit_type
    if cfg.significance is not None:
        meta["significance"] = dict(cfg.significance)
    if cfg.block_granger:
        meta["block_granger"] = True
    if cfg.decimate is not None:
        meta["decimate"], meta["decimate_design"] = cfg.decimate
    if cfg.phase_sync is not None:
        meta["phase_sync"] = list(cfg.phase_sync)
    if cfg.phase_lag is not None:
        meta["phase_lag"] = list(cfg.phase_lag)
    pending = []
    for seg in prep["segments"]:
        key = f"{seg['task']}/{seg['event']}"
        try:
            geo = segment_geometry(cfg, seg["fs"], seg["block"].shape[1], seg["block"].shape[0])
            if geo.pos is None:
                say(f"[SKIP] {dyad} {key}: {geo.T} samples < one window ({geo.W})")
                continue
            pending.append(_launch_segment(eng, cfg, seg, key, geo, psd_stream))
        except DecimateConfigError:                    # the batch's own arguments: nothing to log per segment
            raise
        except Exception as e:                         # one bad segment does not discard the dyad
            meta["failed_segments"].append({"segment": key, "error": f"{type(e).__name__}: {e}"})
            say(f"Failed segment: {dyad} {key} -> {e}")
    if psd_stream is not None:
        torch.cuda.current_stream(eng.device).wait_stream(psd_stream)
    names, freqs = None, None
    for s in pending:
        _collect_segment(s, cfg, dyad, result, meta, say)
        names, freqs = s.seg["names"], s.geo.freqs
    return result, meta, names, freqs


def _write_dyad(target, compresslevel, names, freqs, bands, meta, result):
    """One dyad's file, complete or absent (skip-if-exists relies on it) -> seconds it took."""
    t0 = time.perf_counter()
    tmp = target.with_suffix(".tmp.npz")
    savez_fast(tmp, compresslevel, channels=np.asarray(names), freqs=freqs, bands=np.asarray(bands, dtype=np.float64),
               meta=np.asarray(json.dumps(meta)), **result)
    tmp.replace(target)
    return time.perf_counter() - t0


def run(root, out_dir, tasks=None, window_s=2.0, overlap=0.5, model_order=8, freqs=None, bands=hdist.DEFAULT_BANDS,
        low_cutoff_hz=None, high_cutoff_hz=None, channel_subset=None, with_psd=False, psd_fmin=1.0, psd_fmax=30.0,
        psd_bandwidth=2.0, save_full=False, skip_existing=True, reader=None, engine=None, world=1, rank=0,
        verbose=True, prefetch=2, timing=None, save_workers=4, compresslevel=0, measures=("ffdtf",), significance=None,
        max_model_order=20, crit_type="AIC", validation_lags=None, block_granger=False, pivoted_fallback=None,
        decimate=None, decimate_design="decimate", phase_sync=None, phase_lag=None):
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
                                                       Also with phase_lag=(...), a tuple out of ("pli", "wpli", "dwpli"):
                                                       the phase-lag index, weighted PLI and debiased squared weighted
                                                       PLI of the same windows and bands, all pairs
                                                       (`Engine.sliding_phase_lag`; zero-lag mixing cannot raise them).  NaN
                                                       where a window holds a non-finite sample or, for wpli / dwpli, a
                                                       pair of flat or duplicated channels; meta then says "phase_lag":
                                                       [...].  With both options the analytic signal is formed once.
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
    Beside the segments the file holds `channels` (the block's rows, child first), `freqs`, `bands` and `meta` (JSON: its
    `measures` field lists what was computed, `significance` the test, `segments` and `failed_segments` what became of every
    segment).
    Returns {"done": [...], "skipped": [...], "failed": [(dyad, error)], "timing": {...}}.
    A window whose fit is singular is NaN-filled, not fatal (the reference would raise and lose the dyad); a segment that
    cannot be processed is logged in the dyad's meta and does not discard the dyad's other segments.
    Pipeline: reading + filtering + cutting of the next `prefetch` dyads runs in worker threads while the GPU works on the
    current one (every task file is filtered once, not once per event); per segment the block crosses PCIe once and the
    PSD runs on a second HIP stream beside the MVAR kernels.  `timing` (optional dict) receives the host / GPU split.
    The stages: `resolve_settings` (the arguments, before anything is created), `prepare_dyad` (host, in the pool),
    `_process_dyad` (`segment_geometry`, `_launch_segment` for every segment, then `_collect_segment` for every segment) and
    `_write_dyad` (in the pool of the writes); this function keeps the pools, the prefetch, the books and the log."""
    import concurrent.futures as cf

    import torch
    cfg, eng = resolve_settings(
        engine, window_s=window_s, overlap=overlap, model_order=model_order, freqs=freqs, bands=bands, with_psd=with_psd,
        psd_fmin=psd_fmin, psd_fmax=psd_fmax, psd_bandwidth=psd_bandwidth, save_full=save_full, measures=measures,
        significance=significance, max_model_order=max_model_order, crit_type=crit_type, validation_lags=validation_lags,
        block_granger=block_granger, pivoted_fallback=pivoted_fallback, decimate=decimate, decimate_design=decimate_design,
        phase_sync=phase_sync, phase_lag=phase_lag)
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
    ahead = max(1, int(prefetch))
    pool = cf.ThreadPoolExecutor(max_workers=ahead)
    save_pool = cf.ThreadPoolExecutor(max_workers=max(1, int(save_workers)))
    futures, saves = {}, []

    def submit(k):
        if k < len(todo) and k not in futures:
            futures[k] = pool.submit(prepare_dyad, todo[k], tree[todo[k]], reader, low_cutoff_hz, high_cutoff_hz, channel_subset)

    for k in range(min(len(todo), ahead)):
        submit(k)
    try:
        for k, dyad in enumerate(todo):
            try:
                tw = time.perf_counter()
                prep = futures.pop(k).result()
                wait_s = time.perf_counter() - tw
                submit(k + ahead)
                for line in prep["notes"]:
                    say(line)
                tg = time.perf_counter()
                result, meta, names, freqs_out = _process_dyad(eng, cfg, dyad, prep, psd_stream, say)
                torch.cuda.synchronize(eng.device)
                gpu_s = time.perf_counter() - tg
                if not meta["segments"]:
                    say(f"[SKIP] {dyad}: no complete child + caregiver segment")
                    skipped.append(dyad)
                    continue
                # the write goes to a worker pool of its own (stored by default; deflate -- compresslevel > 0 -- costs 3 - 4 s of
                # a core per full-size dyad, zlib outside the GIL): the GPU and the next dyad's host work do not wait for it,
                # and its time is added to `save_s` of the batch when the file is on disk, not to the dyad's
                target = out_dir / f"{dyad}_ffdtf.npz"
                saves.append((dyad, target, save_pool.submit(_write_dyad, target, compresslevel, names, freqs_out, bands, meta,
                                                             result)))
                done.append(dyad)
                tm["host_prepare_s"] += prep["host_s"]; tm["wait_for_host_s"] += wait_s
                tm["gpu_s"] += gpu_s
                tm["dyads"].append({"dyad": dyad, "host_prepare_s": prep["host_s"], "waited_for_host_s": wait_s,
                                    "gpu_s": gpu_s, "save_s": 0.0, "segments": len(meta["segments"])})
            except DecimateConfigError:
                raise
            except Exception as e:                  # one bad dyad does not stop the batch (export_..._batch.py:93-99)
                failed.append((dyad, f"{type(e).__name__}: {e}"))
                say(f"Failed: {dyad} -> {e}")
                submit(k + ahead)
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
    split = child_channels(names)
    geo = segment_geometry(_Settings(window_s, overlap, freqs, bands, measures, int(model_order), int(model_order)),
                           fs, T, x.shape[1])
    if geo.pos is None:
        raise ValueError(f"{task}/{event}: the common length ({T} samples) is shorter than one window ({geo.W})")
    W, pos, f, lo, hi = geo.W, geo.pos, geo.freqs, geo.lo, geo.hi
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
