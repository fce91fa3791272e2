"""Batched sliding-window ffDTF: the (dyad x window) batch dimension the GPU path is built around.

`window_positions` / `create_windows` follow `EEG_IBI_FFDTF_Pipeline._create_windows`
(/root/reference/src/eeg_alpha_ibi_ffdtf.py:451-518) -- same start positions, same ValueErrors.
`sliding_ffdtf` is the batched equivalent of calling `full_freq_dtf(window, freqs, fs,
optimal_model_order=p)` (/root/reference/src/mtmvar.py:237-284) on every window of every recording.
`sliding_ddtf` / `sliding_gpdc` are `direct_dtf` (mtmvar.py:341-385) / `gen_partial_directed_coherence`
(mtmvar.py:388-468) with `optimal_model_order=p` on every window, in the same batched form.
With `p=None` every window gets the order `mvar_criterion(window, max_model_order, crit_type)` (mtmvar.py:551-601)
picks for it -- the reference's own default, `optimal_model_order=None` -- selected on the device in the same call.
`sliding_significance` adds a surrogate test (shift or phase null) to the band values of any of the three.
`sliding_pseudo_dyad_significance` tests them against shuffled partners: participant A of one dyad with participant B of another.
`decimate` is the anti-aliased integer-factor decimation to run BEFORE any of them on low-passed recordings
(`scipy.signal.decimate(..., ftype='fir', zero_phase=True)` / `resample_poly(x, 1, q)` on the device).
`sliding_phase_sync` is the band-limited phase synchrony of the same windows (PLV, ciPLV, coherence, imaginary coherence of
the analytic signal): no model, no order, no window refused for its conditioning.
`sliding_phase_lag` is the phase-lag family of the same windows (PLI, weighted PLI, debiased squared weighted PLI), the
measures zero-lag mixing cannot raise.
`sliding_fad` is `fad_decomposition` (mtmvar.py:607-757) of every channel of every window.
`sliding_ensemble` / `sliding_ensemble_epochs` are the event-locked form: the reference's functions take `signals` of shape
(channels, samples, trials) and fit ONE model to the trial-averaged covariances (`count_corr`, mtmvar.py:54-85); here a
window slides through the epoch and every position is fitted from all repetitions of the event.
`sliding_ensemble_contrast` / `sliding_ensemble_epochs_contrast` test whether such event-locked band values differ between
two conditions, by permuting the condition labels of the pooled trials.
"""
from __future__ import annotations

import numpy as np
import torch

from .distributed import DEFAULT_BANDS
from .engine import Engine, default_engine

__all__ = ["window_positions", "hop_positions", "create_windows", "sliding_ffdtf", "sliding_ffdtf_device", "window_items",
           "regular_grid", "sliding_ddtf", "sliding_ddtf_device", "sliding_gpdc", "sliding_gpdc_device", "sliding_fad",
           "sliding_significance", "ensemble_items", "sliding_ensemble", "sliding_ensemble_epochs",
           "sliding_ensemble_significance", "sliding_ensemble_epochs_significance", "sliding_pseudo_dyad_significance",
           "sliding_model_validation", "validation_p_values", "sliding_ensemble_contrast", "sliding_ensemble_epochs_contrast",
           "sliding_block_granger_significance", "sliding_block_granger_pseudo_dyad_significance", "decimate",
           "sliding_phase_sync", "sliding_phase_sync_significance", "sliding_phase_sync_pseudo_dyad_significance",
           "sliding_phase_lag"]


def decimate(x, fs, q, design="decimate", engine: Engine | None = None):
    """Decimate recordings by the integer q before fitting: x (m, T) or (n_rec, m, T), a NumPy array or a device tensor ->
    (y (.., ceil(T / q)) of the same kind, fs / q).  design="decimate": `scipy.signal.decimate(x, q, ftype='fir',
    zero_phase=True)`; "resample_poly": `scipy.signal.resample_poly(x, 1, q)`; a 1-D array: the taps themselves
    (`eeg_io.decimation_taps`).  The output is not z-scored again: a low-passed signal loses only its stop-band power.
    Afterwards window lengths are in decimated samples and the model order has to come down with the rate: a window
    needs more samples than m * p unknowns per row, or its normal equations are rank-deficient."""
    eng = engine or default_engine()
    if isinstance(x, torch.Tensor):
        return eng.decimate(x.to(device=eng.device, dtype=torch.float64), q, design), float(fs) / int(q)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim not in (2, 3):
        raise ValueError(f"decimate: x must be (m, T) or (n_rec, m, T), got shape {x.shape}")
    return eng.decimate(eng.to_device(x), q, design).cpu().numpy(), float(fs) / int(q)


def window_positions(T: int, n_windows: int = 3, window_size=None):
    """Start positions and window length of `_create_windows` (eeg_alpha_ibi_ffdtf.py:451-518): `n_windows` windows of
    `window_size` samples whose starts are spread evenly (integer-truncated) from 0 to T - window_size, so the last
    window ends exactly at T.  Same ValueError texts as the reference (pinned by tests/golden/g6_errors.npz)."""
    T, n_windows = int(T), int(n_windows)
    if window_size is None:
        window_size, rest = divmod(T, n_windows)
        if rest:
            raise ValueError(
                f"Cannot evenly divide signal of length {T} into {n_windows} "
                f"non-overlapping windows. Provide a specific window_size."
            )
    elif window_size > T:
        # (the reference tests "too short" first; a size cannot be both, so the order is immaterial)
        raise ValueError(f"window_size ({window_size}) cannot exceed signal length ({T}).")
    elif window_size * n_windows < T:          # fewer than ceil(T / n_windows) samples per window: gaps
        raise ValueError(
            f"window_size={window_size} is too short. To cover {T} samples "
            f"with {n_windows} windows without leaving gaps, the minimum "
            f"window_size is {-(-T // n_windows)}."
        )
    last_start = T - window_size
    if n_windows > 1 and last_start < n_windows - 1:
        raise ValueError(
            f"window_size={window_size} is too large to generate {n_windows} "
            f"distinct windows. Decrease window_size or n_windows."
        )
    starts = np.linspace(0, last_start, n_windows, dtype=int) if n_windows > 1 else np.zeros(1, dtype=int)
    return starts, int(window_size)


def hop_positions(T: int, window_size: int, hop: int):
    """Starts 0, hop, 2 hop, ... of every whole window of `window_size` samples inside T samples (the tail shorter than
    one hop is dropped).  This is the fixed-overlap grid of BASELINE config 2 / 5 ("2 s windows, 50 % overlap"); unlike
    `window_positions` it does not stretch the last window to the end of the recording, so it never refuses a length."""
    T, window_size, hop = int(T), int(window_size), int(hop)
    if window_size < 1 or hop < 1:
        raise ValueError("window_size and hop must be positive")
    if T < window_size:
        return np.zeros(0, dtype=int)
    return np.arange((T - window_size) // hop + 1, dtype=int) * hop


def create_windows(signals, n_windows=3, window_size=None):
    """List of `n_windows` views (channels, window_size), as the reference returns."""
    positions, w = window_positions(signals.shape[1], n_windows, window_size)
    return [signals[:, s:s + w] for s in positions]


def window_items(n_rec: int, positions, device):
    """(item_rec, item_start) int64 device tensors for `n_rec` recordings sharing the same positions."""
    pos = torch.as_tensor(np.asarray(positions, dtype=np.int64))
    item_start = pos.repeat(n_rec).to(device)
    item_rec = torch.arange(n_rec, dtype=torch.int64).repeat_interleave(len(pos)).to(device)
    return item_rec, item_start


def regular_grid(positions, window_size: int, p: int):
    """(hop, first, n_win) if the start positions are an arithmetic progression whose step divides the window into
    2..8 whole hops longer than the model order -- the case in which K1 can share the overlap between windows
    (`Engine.sliding_ffdtf(grid=...)`) -- else None."""
    pos = np.asarray(positions, dtype=np.int64)
    if len(pos) < 2:
        return None
    hop = int(pos[1] - pos[0])
    if hop <= int(p) or hop < 1 or not np.array_equal(np.diff(pos), np.full(len(pos) - 1, hop)):
        return None
    if window_size % hop != 0 or not 2 <= window_size // hop <= 8:
        return None
    return hop, int(pos[0]), len(pos)


def sliding_ffdtf_device(x: torch.Tensor, window_size: int, n_windows: int, p: int, freqs, fs: float,
                         engine: Engine | None = None, out: torch.Tensor | None = None, check: bool = True,
                         share_overlap: bool = True, max_model_order: int = 20, crit_type: str = "AIC",
                         return_orders: bool = False):
    """x: device tensor (n_rec, m, T) -> device tensor (n_rec, n_windows, m, m, F).  No host copies.
    p=None: the automatic order per window (`Engine.sliding_ffdtf`); `return_orders=True` then returns
    (ffdtf, orders (n_rec, n_windows) int32, crit (n_rec, n_windows, max_model_order))."""
    eng = engine or default_engine()
    n_rec, m, T = x.shape
    positions, w = window_positions(T, n_windows, window_size)
    if p is None:
        from .engine import auto_order_args
        auto_order_args(max_model_order, crit_type, w)
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    res = eng.sliding_ffdtf(x, item_rec, item_start, w, p, freqs, fs, out=out, check=check,
                            grid=regular_grid(positions, w, _grid_order(p, max_model_order)) if share_overlap else None,
                            **_auto_kw(p, max_model_order, crit_type, return_orders))
    return _shape_windows(res, n_rec, len(positions), m)


def _grid_order(p, max_model_order):
    return int(max_model_order) if p is None else p


def _auto_kw(p, max_model_order, crit_type, return_orders):
    """The automatic-order keywords, passed on only with p=None (an integer p takes the fixed-order call as it is)."""
    return dict(max_model_order=max_model_order, crit_type=crit_type, return_orders=return_orders) if p is None else {}


def _shape_windows(res, n_rec, n_win, m):
    """(items, m, m, last) -> (n_rec, n_windows, m, m, last); with return_orders the orders and criterion curves alike."""
    if isinstance(res, tuple):
        out, orders, crit = res
        return out.view(n_rec, n_win, m, m, -1), orders.view(n_rec, n_win), crit.view(n_rec, n_win, -1)
    return res.view(n_rec, n_win, m, m, -1)


def _to_host(res, single):
    if isinstance(res, tuple):
        return tuple((a.cpu().numpy()[0] if single else a.cpu().numpy()) for a in res)
    a = res.cpu().numpy()
    return a[0] if single else a


def sliding_ffdtf(x, window_size, n_windows, p, freqs, fs, engine: Engine | None = None, max_model_order: int = 20,
                  crit_type: str = "AIC", return_orders: bool = False):
    """NumPy in / NumPy out.  x: (m, T) or (n_rec, m, T) -> (n_windows, m, m, F) or (n_rec, n_windows, ...).
    p=None: `full_freq_dtf(window, freqs, fs, max_model_order, None, crit_type)` of every window, i.e. the automatic order;
    `return_orders=True` then returns (ffdtf, orders, crit)."""
    if p is None:
        from .engine import auto_order_args
        auto_order_args(max_model_order, crit_type, 1 << 62)         # (the window length: in sliding_ffdtf_device)
    eng = engine or default_engine()
    x = np.asarray(x, dtype=np.float64)
    single = x.ndim == 2
    xd = eng.to_device(x[None] if single else x)
    res = sliding_ffdtf_device(xd, window_size, n_windows, p, freqs, fs, eng,
                               **_auto_kw(p, max_model_order, crit_type, return_orders))
    return _to_host(res, single)


def yw_routes(x, window_size, n_windows, p, hop=None, engine: Engine | None = None):
    """How many of my windows are ill-conditioned?  K1 + K2 only, with the pivoted fallback on.  x: (m, T) or (n_rec, m, T)
    -> {"route": (n_rec, n_windows) int8, which solver took each window -- 0 the recursion, 1 the LDL^T behind its
    conditioning guard, 2 the pivoted LU (the two unpivoted solvers refused it) --, "info": (n_rec, n_windows) int32, not
    zero where even the LU met an exactly zero pivot column}, without the leading axis for a single recording.  Windows from
    `window_positions`, or every `hop` samples when `hop` is given.  An integer p is required."""
    from .engine import no_block_auto_order
    p = no_block_auto_order(p, "yw_routes")
    x = np.asarray(x, dtype=np.float64) if not isinstance(x, torch.Tensor) else x
    if x.ndim not in (2, 3):
        raise ValueError(f"yw_routes: x must be (m, T) or (n_rec, m, T), got shape {tuple(x.shape)}")
    single = x.ndim == 2
    positions, w = _positions(int(x.shape[-1]), window_size, n_windows, hop)
    eng = engine or default_engine()
    if isinstance(x, torch.Tensor):
        xd = (x[None] if single else x).to(device=eng.device, dtype=torch.float64)
    else:
        xd = eng.to_device(x[None] if single else x)
    n_rec, m, T = xd.shape
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    route, info = eng.window_routes(xd, item_rec, item_start, w, p)
    route = route.view(n_rec, len(positions)).cpu().numpy().astype(np.int8)
    info = info.view(n_rec, len(positions)).cpu().numpy()
    return {"route": route[0] if single else route, "info": info[0] if single else info}


def _positions(T: int, window_size, n_windows: int, hop):
    if hop is not None:
        if window_size is None:
            raise ValueError("hop needs a window_size")
        return hop_positions(T, window_size, hop), int(window_size)
    return window_positions(T, n_windows, window_size)


def _sliding_conn_device(measure, x, window_size, n_windows, p, freqs, fs, engine, out, check, share_overlap, hop, bands,
                         max_model_order=20, crit_type="AIC", return_orders=False):
    eng = engine or default_engine()
    n_rec, m, T = x.shape
    positions, w = _positions(T, window_size, n_windows, hop)
    if p is None:
        from .engine import auto_order_args
        auto_order_args(max_model_order, crit_type, w)
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    run = eng.sliding_ddtf if measure == "ddtf" else eng.sliding_gpdc
    res = run(x, item_rec, item_start, w, p, freqs, fs, out=out, check=check, bands=bands,
              grid=regular_grid(positions, w, _grid_order(p, max_model_order)) if share_overlap else None,
              **_auto_kw(p, max_model_order, crit_type, return_orders))
    return _shape_windows(res, n_rec, len(positions), m)


def sliding_ddtf_device(x: torch.Tensor, window_size, n_windows: int, p: int, freqs, fs: float, engine: Engine | None = None,
                        out: torch.Tensor | None = None, check=True, share_overlap: bool = True, hop=None, bands=None,
                        max_model_order: int = 20, crit_type: str = "AIC", return_orders: bool = False):
    """dDTF of every window: x device tensor (n_rec, m, T) -> device tensor (n_rec, n_windows, m, m, F), or
    (..., n_bands) with `bands=(bin_lo, bin_hi)`.  Windows from `window_positions`, or every `hop` samples
    (`hop_positions`) when `hop` is given.  check: True raises LinAlgError naming the failed window, "nan" NaN-fills it
    (`Engine.sliding_ddtf`).  p=None: the automatic order per window; `return_orders=True` then returns (out, orders
    (n_rec, n_windows), crit (n_rec, n_windows, max_model_order))."""
    return _sliding_conn_device("ddtf", x, window_size, n_windows, p, freqs, fs, engine, out, check, share_overlap, hop, bands,
                                max_model_order, crit_type, return_orders)


def sliding_gpdc_device(x: torch.Tensor, window_size, n_windows: int, p: int, freqs, fs: float, engine: Engine | None = None,
                        out: torch.Tensor | None = None, check=True, share_overlap: bool = True, hop=None, bands=None,
                        max_model_order: int = 20, crit_type: str = "AIC", return_orders: bool = False):
    """GPDC of every window, in the form of `sliding_ddtf_device` (`Engine.sliding_gpdc`)."""
    return _sliding_conn_device("gpdc", x, window_size, n_windows, p, freqs, fs, engine, out, check, share_overlap, hop, bands,
                                max_model_order, crit_type, return_orders)


def _sliding_conn_host(fn, x, window_size, n_windows, p, freqs, fs, engine, hop, bands, check, max_model_order=20,
                       crit_type="AIC", return_orders=False):
    if p is None:
        from .engine import auto_order_args
        auto_order_args(max_model_order, crit_type, 1 << 62)         # (the window length: in _sliding_conn_device)
    eng = engine or default_engine()
    x = np.asarray(x, dtype=np.float64) if not isinstance(x, torch.Tensor) else x
    single = x.ndim == 2
    if isinstance(x, torch.Tensor):
        xd = (x[None] if single else x).to(device=eng.device, dtype=torch.float64)
    else:
        xd = eng.to_device(x[None] if single else x)
    res = fn(xd, window_size, n_windows, p, freqs, fs, eng, check=check, hop=hop, bands=bands,
             **_auto_kw(p, max_model_order, crit_type, return_orders))
    return _to_host(res, single)


def sliding_ddtf(x, window_size, n_windows, p, freqs, fs, engine: Engine | None = None, hop=None, bands=None, check=True,
                 max_model_order: int = 20, crit_type: str = "AIC", return_orders: bool = False):
    """NumPy (or tensor) in / NumPy out.  x: (m, T) or (n_rec, m, T) -> (n_windows, m, m, F) or (n_rec, n_windows, ...):
    `direct_dtf(window, freqs, fs, optimal_model_order=p)` (mtmvar.py:341-385) of every window."""
    return _sliding_conn_host(sliding_ddtf_device, x, window_size, n_windows, p, freqs, fs, engine, hop, bands, check,
                              max_model_order, crit_type, return_orders)


def sliding_gpdc(x, window_size, n_windows, p, freqs, fs, engine: Engine | None = None, hop=None, bands=None, check=True,
                 max_model_order: int = 20, crit_type: str = "AIC", return_orders: bool = False):
    """NumPy (or tensor) in / NumPy out: `gen_partial_directed_coherence(window, freqs, fs, optimal_model_order=p)`
    (mtmvar.py:388-468) of every window, shaped as `sliding_ddtf`."""
    return _sliding_conn_host(sliding_gpdc_device, x, window_size, n_windows, p, freqs, fs, engine, hop, bands, check,
                              max_model_order, crit_type, return_orders)


def sliding_block_granger(x, window_size, n_windows, p, freqs, fs, *, split, hop=None, bands=None, check=True,
                          engine: Engine | None = None):
    """NumPy (or tensor) in / NumPy out: block Granger causality between the channels < split and the channels >= split of
    every window (`Engine.sliding_block_granger`).  x: (m, T) or (n_rec, m, T) -> (spectral, time) shaped
    (n_rec, n_windows, 2, F | n_bands) and (n_rec, n_windows, 4), without the leading axis for a single recording.
    Windows from `window_positions`, or every `hop` samples when `hop` is given.  An integer p is required."""
    from .engine import check_block_split, no_block_auto_order
    p = no_block_auto_order(p, "sliding_block_granger")
    x = np.asarray(x, dtype=np.float64) if not isinstance(x, torch.Tensor) else x
    single = x.ndim == 2
    split = check_block_split(split, x.shape[-2], "sliding_block_granger")
    eng = engine or default_engine()
    if isinstance(x, torch.Tensor):
        xd = (x[None] if single else x).to(device=eng.device, dtype=torch.float64)
    else:
        xd = eng.to_device(x[None] if single else x)
    n_rec, m, T = xd.shape
    positions, w = _positions(T, window_size, n_windows, hop)
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    spectral, time = eng.sliding_block_granger(xd, item_rec, item_start, w, p, freqs, fs, split=split, bands=bands,
                                               check=check, grid=regular_grid(positions, w, p))
    return _to_host((spectral.view(n_rec, len(positions), 2, -1), time.view(n_rec, len(positions), 4)), single)


def _phase_x(eng, x):
    """x (m, T) or (n_rec, m, T), array or tensor -> (x as (n_rec, m, T) float64 on the engine's device, whether it was a
    single recording): what the four phase wrappers hand to the engine."""
    single = np.ndim(x) == 2
    return _recordings_to_device(eng, x, single), single


def _sliding_phase_host(who, lag, x, window_size, n_windows, fs, bands_hz, hop, measures, split, order, check, engine,
                        max_workspace_bytes):
    """The host wrapper behind `sliding_phase_sync` (lag False: the synchrony measures) and `sliding_phase_lag` (lag True:
    the phase-lag measures, with their split): the arguments first, then x to the device, `Engine.sliding_phase` and the result
    as {measure: (n_rec, n_windows, n_bands, m, m)} on the host."""
    from .eeg_io import check_phase_lag_split, resolve_bands_hz, resolve_phase_lag_measures, resolve_phase_measures
    measures = (resolve_phase_lag_measures if lag else resolve_phase_measures)(measures)    # nothing has touched a device yet
    bands_hz = tuple(bands_hz)
    resolve_bands_hz(bands_hz, fs)
    if check is not True and check != "nan":
        raise ValueError(f"{who}: check must be True or 'nan', got {check!r}")
    x = np.asarray(x, dtype=np.float64) if not isinstance(x, torch.Tensor) else x
    if x.ndim not in (2, 3):
        raise ValueError(f"{who}: x must be (m, T) or (n_rec, m, T), got shape {tuple(x.shape)}")
    if lag:
        split = check_phase_lag_split(split, int(x.shape[-2]), who)
    positions, w = _positions(int(x.shape[-1]), window_size, n_windows, hop)
    eng = engine or default_engine()
    xd, single = _phase_x(eng, x)
    n_rec = int(xd.shape[0])
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    res = eng.sliding_phase(who, xd, item_rec, item_start, w, fs, bands_hz, sync=None if lag else measures,
                            lag=measures if lag else None, split=split, order=order, check=check,
                            max_workspace_bytes=max_workspace_bytes)[int(lag)]
    keys = measures + (("info",) if check == "nan" else ())
    out = {k: res[k].view(n_rec, len(positions), len(bands_hz), *res[k].shape[2:]).cpu().numpy() for k in keys}
    return {k: v[0] for k, v in out.items()} if single else out


def sliding_phase_sync(x, window_size, n_windows, fs, bands_hz=DEFAULT_BANDS, *, hop=None, measures=("plv",), order=4,
                       check=True, engine: Engine | None = None, max_workspace_bytes: int = 8 << 30):
    """NumPy (or tensor) in / NumPy out: band-limited phase synchrony of every window (`Engine.sliding_phase_sync`).  x: (m, T)
    or (n_rec, m, T) -> {measure: (n_rec, n_windows, n_bands, m, m)} for `measures` out of ("plv", "ciplv", "coh", "imcoh"),
    without the leading axis for a single recording; with check="nan" also "info" (n_rec, n_windows, n_bands).  `bands_hz`:
    (lo, hi) pairs in Hz (not bin ranges on a frequency grid, which is what `bands` means in this module); the analytic
    band signal is `eeg_io.band_response`'s, circular at the ends of the recording.  Windows from `window_positions`, or
    every `hop` samples when `hop` is given.  No model is fitted: there is no order and no window is refused for its
    conditioning."""
    return _sliding_phase_host("sliding_phase_sync", False, x, window_size, n_windows, fs, bands_hz, hop, measures, 0, order,
                               check, engine, max_workspace_bytes)


def sliding_phase_lag(x, window_size, n_windows, fs, bands_hz=DEFAULT_BANDS, *, hop=None, measures=("wpli",), split=0,
                      order=4, check=True, engine: Engine | None = None, max_workspace_bytes: int = 8 << 30):
    """NumPy (or tensor) in / NumPy out: the band-limited phase-lag measures of every window (`Engine.sliding_phase_lag`):
    PLI, weighted PLI and debiased squared weighted PLI, which zero-lag mixing (common reference, volume conduction) cannot
    raise.  x: (m, T) or (n_rec, m, T) -> {measure: (n_rec, n_windows, n_bands, m, m)} for `measures` out of ("pli",
    "wpli", "dwpli"), without the leading axis for a single recording; with check="nan" also "info" (n_rec, n_windows,
    n_bands).  split = 0: all pairs; 1..m-1: only the inter-brain pairs (i < split <= j), every other off-diagonal cell NaN.
    Bands, windows and `hop` as in `sliding_phase_sync`.  No model is fitted."""
    return _sliding_phase_host("sliding_phase_lag", True, x, window_size, n_windows, fs, bands_hz, hop, measures, split, order,
                               check, engine, max_workspace_bytes)


def _phase_host(v, lead=None):
    """A leaf (or dict of leaves) of a phase-synchrony test -> NumPy, per-item leaves reshaped to `lead` + their own axes."""
    if isinstance(v, dict):
        return {k: _phase_host(u, lead) for k, u in v.items()}
    a = v.cpu().numpy()
    return a if lead is None else a.reshape(lead + a.shape[1:])


def sliding_phase_sync_significance(x, window_size, n_windows, fs, bands_hz=DEFAULT_BANDS, *, measures=("plv",), n_surrogates,
                                    seed, split=None, min_shift=None, hop=None, order=4, check=True, chunk=None,
                                    engine: Engine | None = None, max_workspace_bytes: int = 8 << 30):
    """NumPy (or tensor) in / NumPy out: the shift-surrogate test of `Engine.phase_sync_significance` for the inter-brain
    cells of `sliding_phase_sync(x, window_size, n_windows, fs, bands_hz, hop=hop, measures=measures)`.  x: (m, T) or
    (n_rec, m, T); channels < split are participant A (default split = m // 2).  Returns {measure: {observed, p, p_fwe,
    null_mean, null_std (n_rec, n_windows, n_bands, m, m)}, n_valid, info (n_rec, n_windows, n_bands), tested (m, m)}, without
    the leading axis for a single recording.  The arguments are checked before the GPU is touched
    (`surrogates.phase_significance_args`)."""
    from . import surrogates as sg
    from .eeg_io import resolve_bands_hz
    single = np.ndim(x) == 2
    shape = tuple(np.shape(x))
    if len(shape) not in (2, 3):
        raise ValueError(f"sliding_phase_sync_significance: x must be (m, T) or (n_rec, m, T), got shape {shape}")
    n_rec, m, T = (1,) + shape if single else shape
    bands_hz = tuple(bands_hz)
    resolve_bands_hz(bands_hz, fs)
    positions, w = _positions(T, window_size, n_windows, hop)
    sg.phase_significance_args(measures, n_surrogates, m, T, w, split, min_shift, check)
    eng = engine or default_engine()
    xd, single = _phase_x(eng, x)
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    res = eng.phase_sync_significance(xd, item_rec, item_start, w, fs, bands_hz, measures=measures, n_surrogates=n_surrogates,
                                      seed=seed, split=split, min_shift=min_shift, order=order, check=check, chunk=chunk,
                                      max_workspace_bytes=max_workspace_bytes)
    lead = (len(positions),) if single else (n_rec, len(positions))
    return {k: _phase_host(v, None if k == "tested" else lead) for k, v in res.items()}


def sliding_phase_sync_pseudo_dyad_significance(x, window_size, n_windows, fs, bands_hz=DEFAULT_BANDS, *, measures=("plv",),
                                                split=None, n_surrogates=None, seed=None, hop=None, order=4, check=True,
                                                chunk=None, engine: Engine | None = None,
                                                max_workspace_bytes: int = 8 << 30):
    """NumPy (or tensor) in / NumPy out: the pseudo-dyad test of `Engine.phase_sync_pseudo_dyad_significance`.  x: (D, m, T),
    one recording per dyad, all time-locked to the same stimulus; windows as for `sliding_phase_sync`; partners as for
    `sliding_pseudo_dyad_significance`.  Returns {measure: {observed, p, p_fwe, null_mean, null_std (D, n_windows, n_bands, m,
    m)}, n_valid, info (D, n_windows, n_bands), tested (m, m), partners (S, D), group = {measure: {the same five (n_windows,
    n_bands, m, m)}, n_valid (n_windows, n_bands)}}.  The arguments are checked before the GPU is touched
    (`surrogates.phase_pseudo_dyad_args`)."""
    from . import surrogates as sg
    from .eeg_io import resolve_bands_hz
    shape = tuple(np.shape(x))
    if len(shape) != 3:
        raise ValueError("x must have shape (dyads, channels, samples)")
    D, m, T = shape
    sg.phase_pseudo_dyad_args(measures, D, m, n_surrogates, seed, split, check)
    bands_hz = tuple(bands_hz)
    resolve_bands_hz(bands_hz, fs)
    positions, w = _positions(T, window_size, n_windows, hop)
    eng = engine or default_engine()
    xd, _ = _phase_x(eng, x)
    item_start = torch.as_tensor(np.asarray(positions, dtype=np.int64)).to(eng.device)
    res = eng.phase_sync_pseudo_dyad_significance(xd, item_start, w, fs, bands_hz, measures=measures, split=split,
                                                  n_surrogates=n_surrogates, seed=seed, order=order, check=check, chunk=chunk,
                                                  max_workspace_bytes=max_workspace_bytes)
    return {k: _phase_host(v) for k, v in res.items()}


def sliding_significance(x, window_size, n_windows, p, freqs, fs, bands, *, measure, null, n_surrogates, seed, split=None,
                         min_shift=None, check=True, chunk=None, hop=None, share_overlap: bool = True,
                         engine: Engine | None = None):
    """NumPy (or tensor) in / NumPy out: the surrogate test of `Engine.sliding_significance` for the band values
    `sliding_<measure>(x, window_size, n_windows, p, freqs, fs, hop=hop, bands=bands)` of every window.
    x: (m, T) or (n_rec, m, T); bands = (bin_lo, bin_hi) from `distributed.band_bins`.  Returns a dict: observed, p,
    p_fwe, null_mean, null_std shaped like `sliding_ddtf` with bands -- (n_windows, m, m, n_bands) or (n_rec, n_windows,
    ...) --, n_valid (n_windows,) or (n_rec, n_windows), tested (m, m).  The arguments are checked before the GPU is
    touched (`surrogates.significance_args`)."""
    from . import surrogates as sg
    from .engine import no_auto_order
    no_auto_order(p, "sliding_significance")
    if null in sg.ENSEMBLE_NULLS:
        raise ValueError(f"null={null!r} is the test of event-locked ensembles (sliding_ensemble_significance); "
                         f"sliding_significance takes one of {sg.NULLS}")
    single = np.ndim(x) == 2
    shape = tuple(np.shape(x))
    n_rec, m, T = (1,) + shape if single else shape
    positions, w = _positions(T, window_size, n_windows, hop)
    sg.significance_args(measure, null, n_surrogates, m, T, w, split, min_shift)
    eng = engine or default_engine()
    if isinstance(x, torch.Tensor):
        xd = (x[None] if single else x).to(device=eng.device, dtype=torch.float64).contiguous()
    else:
        xd = eng.to_device(np.asarray(x, dtype=np.float64)[None] if single else np.asarray(x, dtype=np.float64))
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    grid = regular_grid(positions, w, p) if share_overlap else None
    res = eng.sliding_significance(xd, item_rec, item_start, w, p, freqs, fs, bands, measure=measure, null=null,
                                   n_surrogates=n_surrogates, seed=seed, split=split, min_shift=min_shift, check=check,
                                   chunk=chunk, grid=grid)
    nw = len(positions)
    out = {"tested": res["tested"].cpu().numpy()}
    for k, v in res.items():
        if k == "tested":
            continue
        a = v.cpu().numpy().reshape((n_rec, nw) + tuple(v.shape[1:]))
        out[k] = a[0] if single else a
    return out


def sliding_pseudo_dyad_significance(x, window_size, n_windows, p, freqs, fs, bands, *, measure, split=None, n_surrogates=None,
                                     seed=None, hop=None, check=True, chunk=None, engine: Engine | None = None):
    """NumPy (or tensor) in / NumPy out: the pseudo-dyad test of `Engine.pseudo_dyad_significance` for the band values
    `sliding_<measure>(x, window_size, n_windows, p, freqs, fs, hop=hop, bands=bands)`.  x: (D, m, T), one recording per
    dyad, all of them time-locked to the same stimulus; channels < split are participant A (default split = m // 2).
    Windows and bands as for `sliding_significance`.  n_surrogates=None: every other dyad's partner once on each side (the
    D - 1 cyclic offsets, no seed); an integer: that many seeded derangements.  Returns a dict of NumPy arrays: observed, p,
    p_fwe, null_mean, null_std (D, n_windows, m, m, n_bands), n_valid (D, n_windows), tested (m, m), partners (S, D) and
    group = {observed, p, p_fwe, null_mean, null_std (n_windows, m, m, n_bands), n_valid (n_windows,)}.  The arguments are
    checked before the GPU is touched (`surrogates.pseudo_dyad_args`)."""
    from . import surrogates as sg
    from .engine import no_auto_order
    no_auto_order(p, "sliding_pseudo_dyad_significance")
    shape = tuple(np.shape(x))
    if len(shape) != 3:
        raise ValueError("x must have shape (dyads, channels, samples)")
    D, m, T = shape
    sg.pseudo_dyad_args(measure, D, m, n_surrogates, seed, split, check)
    if bands is None or len(bands) != 2 or len(np.atleast_1d(bands[0])) < 1 or \
            len(np.atleast_1d(bands[0])) != len(np.atleast_1d(bands[1])):
        raise ValueError("sliding_pseudo_dyad_significance needs bands = (bin_lo, bin_hi) with at least one band")
    positions, w = _positions(T, window_size, n_windows, hop)
    eng = engine or default_engine()
    xd = _recordings_to_device(eng, x, False)
    item_start = torch.as_tensor(np.asarray(positions, dtype=np.int64)).to(eng.device)
    res = eng.pseudo_dyad_significance(xd, item_start, w, p, freqs, fs, bands, measure=measure, split=split,
                                       n_surrogates=n_surrogates, seed=seed, check=check, chunk=chunk)
    out = {k: v.cpu().numpy() for k, v in res.items() if k != "group"}
    out["group"] = {k: v.cpu().numpy() for k, v in res["group"].items()}
    return out


def _block_to_host(res, lead):
    """The device dict of a block Granger test -> NumPy, the per-item leaves reshaped to `lead` + their own trailing axes."""
    def host(v, lead):
        a = v.cpu().numpy()
        return a if lead is None else a.reshape(lead + a.shape[1:])
    out = {}
    for k, v in res.items():
        if k == "group":
            out[k] = {g: ({h: u.cpu().numpy() for h, u in w.items()} if isinstance(w, dict) else w.cpu().numpy())
                      for g, w in v.items()}
        elif isinstance(v, dict):
            out[k] = {h: host(u, lead) for h, u in v.items()}
        else:
            out[k] = host(v, None if k == "partners" else lead)
    return out


def sliding_block_granger_significance(x, window_size, n_windows, p, freqs, fs, bands, *, split, null, n_surrogates, seed,
                                       values=("time", "bands"), min_shift=None, check=True, chunk=None, hop=None,
                                       engine: Engine | None = None):
    """NumPy (or tensor) in / NumPy out: the surrogate test of `Engine.block_granger_significance` for the block Granger
    causality `sliding_block_granger(x, window_size, n_windows, p, freqs, fs, split=split, hop=hop, bands=bands)` of every
    window.  x: (m, T) or (n_rec, m, T).  Returns a dict, index 0 = A -> B, 1 = B -> A: time = {observed, p, p_fwe, null_mean,
    null_std (n_windows, 2)}, bands = {the same, (n_windows, 2, n_bands)}, observed_time (n_windows, 4), n_valid
    (n_windows,), each with a leading n_rec for several recordings; values=("time",) leaves `bands` out (and needs neither
    freqs nor bands), values=("bands",) leaves `time` and `observed_time` out.  The arguments are checked before the GPU is
    touched (`surrogates.block_significance_args`)."""
    from . import surrogates as sg
    from .engine import no_block_auto_order
    no_block_auto_order(p, "sliding_block_granger_significance")
    single = np.ndim(x) == 2
    shape = tuple(np.shape(x))
    n_rec, m, T = (1,) + shape if single else shape
    positions, w = _positions(T, window_size, n_windows, hop)
    sg.block_significance_args(null, n_surrogates, m, T, w, split, min_shift, values, bands, check)
    eng = engine or default_engine()
    xd = _recordings_to_device(eng, x, single)
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    res = eng.block_granger_significance(xd, item_rec, item_start, w, p, freqs, fs, bands, split=split, null=null,
                                         n_surrogates=n_surrogates, seed=seed, values=values, min_shift=min_shift,
                                         check=check, chunk=chunk)
    return _block_to_host(res, (len(positions),) if single else (n_rec, len(positions)))


def sliding_block_granger_pseudo_dyad_significance(x, window_size, n_windows, p, freqs, fs, bands, *, split, n_surrogates=None,
                                                   seed=None, values=("time", "bands"), hop=None, check=True, chunk=None,
                                                   engine: Engine | None = None):
    """NumPy (or tensor) in / NumPy out: the pseudo-dyad test of `Engine.block_granger_pseudo_dyad_significance`.  x: (D, m,
    T), one recording per dyad, all time-locked to the same stimulus; channels < split are participant A.  Windows as for
    `sliding_block_granger_significance`, partners as for `sliding_pseudo_dyad_significance`.  Returns that function's dict
    with (D, n_windows) in front, plus partners (S, D) and group = {time, bands, n_valid} with (n_windows,) in front.  The
    arguments are checked before the GPU is touched (`surrogates.block_pseudo_dyad_args`)."""
    from . import surrogates as sg
    from .engine import no_block_auto_order
    no_block_auto_order(p, "sliding_block_granger_pseudo_dyad_significance")
    shape = tuple(np.shape(x))
    if len(shape) != 3:
        raise ValueError("x must have shape (dyads, channels, samples)")
    D, m, T = shape
    sg.block_pseudo_dyad_args(D, m, n_surrogates, seed, split, values, bands, check)
    positions, w = _positions(T, window_size, n_windows, hop)
    eng = engine or default_engine()
    xd = _recordings_to_device(eng, x, False)
    item_start = torch.as_tensor(np.asarray(positions, dtype=np.int64)).to(eng.device)
    res = eng.block_granger_pseudo_dyad_significance(xd, item_start, w, p, freqs, fs, bands, split=split,
                                                     n_surrogates=n_surrogates, seed=seed, values=values, check=check,
                                                     chunk=chunk)
    return _block_to_host(res, None)


def sliding_fad(signals, fs, window_size=None, n_windows=3, hop=None, model_order=None, max_model_order=20,
                crit_type='AIC', pair_conjugates=True, imag_tol=1e-8, engine: Engine | None = None):
    """FAD decomposition of every channel of every window of one recording signals (m, T): what
    `fad_decomposition(window[ch], fs, ...)` (/root/reference/src/mtmvar.py:607-757) gives for each window of
    `_create_windows` -- starts from `window_positions(T, n_windows, window_size)`, or every `hop` samples
    (`hop_positions`, window_size required) when `hop` is given.  Returns `fad_decomposition_batch`'s dict with the
    leading series axis split into (n_windows, m).  The recording is uploaded once and the windows are read in place."""
    from .mtmvar import _fad_host, _fad_orders
    eng = engine or default_engine()
    x = np.asarray(signals, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("signals must have shape (channels, samples)")
    m, T = x.shape
    if hop is not None:
        if window_size is None:
            raise ValueError("hop needs a window_size")
        positions, w = hop_positions(T, window_size, hop), int(window_size)
    else:
        positions, w = window_positions(T, n_windows, window_size)
    order, pmax, crit = _fad_orders(model_order, max_model_order, crit_type, w)
    xd = eng.to_device(x[None])
    item_rec, item_start = window_items(1, positions, eng.device)
    d = eng.fad(xd, item_rec, item_start, w, pmax, order, crit, fs, imag_tol, pair_conjugates)
    out = _fad_host(d, model_order, pair_conjugates)
    nw = len(positions)

    def split(v):
        return v.reshape((nw, m) + v.shape[1:]) if isinstance(v, np.ndarray) else v
    out = {k: ({kk: split(vv) for kk, vv in v.items()} if isinstance(v, dict) else split(v)) for k, v in out.items()}
    return out


# ---- model validation -----------------------------------------------------------------------------------------------------
def validation_p_values(q, q_channel, orders, m: int, max_lag: int, bad=None):
    """Host side of the whiteness tests: degrees of freedom and chi-square tails of the device's statistics.
    q (..., 3), q_channel (..., m), orders (...) the model order of every window.  Returns (df, p_value (..., 3),
    p_channel (..., m)) with df = m^2 (max_lag - order); the p-values are NaN where df <= 0 or `bad`."""
    from scipy.special import chdtrc
    q, q_channel, orders = np.asarray(q, dtype=np.float64), np.asarray(q_channel, dtype=np.float64), np.asarray(orders)
    df_ch = int(max_lag) - orders.astype(np.int64)
    df = int(m) * int(m) * df_ch
    ok = df_ch > 0 if bad is None else (df_ch > 0) & ~np.asarray(bad, dtype=bool)
    safe = np.where(ok, df_ch, 1).astype(np.float64)
    p_value = np.where(ok[..., None], chdtrc(safe[..., None] * m * m, q), np.nan)
    p_channel = np.where(ok[..., None], chdtrc(safe[..., None], q_channel), np.nan)
    return df, p_value, p_channel


def sliding_model_validation(x, window_size, n_windows, p, *, max_lag, hop=None, max_model_order=20, crit_type="AIC",
                             acf_z=1.96, engine: Engine | None = None):
    """Is every window's MVAR model adequate?  NumPy (or tensor) in / NumPy out.  x: (m, T) or (n_rec, m, T); windows as
    `sliding_ddtf` (`window_positions`, or every `hop` samples).  Every window is fitted by Yule-Walker (K1 + K2) at the
    order p, or with p=None at the order `mvar_criterion(window, max_model_order, crit_type)` picks for it; then
    `Engine.model_validation` computes the residuals and their whiteness statistics over h = max_lag lags.  With p=None
    the coefficients are zero-padded to max_model_order lags, so every window has N = window_size - max_model_order
    residuals and its own order enters the degrees of freedom only.
    Returns a dict with leading shape (n_windows,) or (n_rec, n_windows):
        q, p_value (..., 3)      Box-Pierce, Li-McLeod, Hosking portmanteau statistics and their chi-square tails
        df                       m^2 (h - order)
        q_channel, p_channel (..., m)   per-channel Ljung-Box, h - order degrees of freedom
        acf_fraction             share of the h m^2 residual correlations beyond acf_z / sqrt(N) (white: about 5 %)
        s (..., h)               the per-lag terms;  orders;  resid_cov (..., m, m)
        bad                      True where the fit or the Cholesky of the residual covariance failed: every statistic NaN.
    The chi-square approximation needs N >> m^2 h: the p-values are for few channels ("Model validation")."""
    from .engine import auto_order_args
    single = np.ndim(x) == 2
    shape = tuple(np.shape(x))
    if len(shape) not in (2, 3):
        raise ValueError("x must have shape (channels, samples) or (recordings, channels, samples)")
    n_rec, m, T = (1,) + shape if single else shape
    positions, w = _positions(T, window_size, n_windows, hop)
    if p is None:
        fit_p, _ = auto_order_args(max_model_order, crit_type, w)
    else:
        fit_p = int(p)
        if not 1 <= fit_p <= 32:
            raise ValueError(f"p must be None or an integer in 1..32, got {p!r}")
    h = int(max_lag)
    if isinstance(max_lag, bool) or h != max_lag or not 1 <= h <= 32:
        raise ValueError(f"max_lag must be an integer in 1..32, got {max_lag!r}")
    if w - fit_p <= h:
        raise ValueError(f"window_size - order ({w - fit_p}) residuals must exceed max_lag ({h})")
    eng = engine or default_engine()
    xd = _recordings_to_device(eng, x, single)
    item_rec, item_start = window_items(n_rec, positions, eng.device)
    R = eng.lagcov(xd, item_rec, item_start, w, fit_p)
    if p is None:
        ar, _, orders, _, info_yw = eng.yw_solve_auto(R, m, w, crit_type)
    else:
        ar, _, _, info_yw = eng.yw_solve(R, m)
        orders = torch.full_like(info_yw, fit_p)
    res = eng.model_validation(xd, item_rec, item_start, w, ar, h, acf_z=acf_z, validate=False)
    bad = ((info_yw != 0) | (res["info"] != 0)).cpu().numpy()
    nw = len(positions)
    nan = float("nan")
    out = {k: np.where(bad.reshape((-1,) + (1,) * (res[k].dim() - 1)), nan, res[k].cpu().numpy())
           for k in ("q", "q_channel", "s", "resid_cov")}
    out["acf_fraction"] = np.where(bad, nan, res["acf_count"].cpu().numpy() / float(h * m * m))
    out["orders"] = orders.cpu().numpy()
    out["bad"] = bad
    out["df"], out["p_value"], out["p_channel"] = validation_p_values(out["q"], out["q_channel"], out["orders"], m, h, bad)
    out = {k: v.reshape((n_rec, nw) + v.shape[1:]) for k, v in out.items()}
    return {k: v[0] for k, v in out.items()} if single else out


# ---- event-locked ensembles ---------------------------------------------------------------------------------------------
def ensemble_items(onsets, pre: int, post: int, window_size: int, hop: int):
    """Trial starts and window offsets of an event-locked analysis: every epoch runs from `pre` samples before its onset to
    `post` samples after it, and windows of `window_size` samples start every `hop` samples inside it
    (`hop_positions(pre + post, window_size, hop)`).  Returns (trial_start = onsets - pre, offsets), both int64."""
    pre, post = int(pre), int(post)
    if pre < 0 or post < 0:
        raise ValueError("pre and post must be non-negative")
    on = np.asarray(onsets, dtype=np.int64)
    if on.ndim != 1:
        raise ValueError("onsets must be one-dimensional")
    return on - pre, hop_positions(pre + post, window_size, hop).astype(np.int64)


def _ensemble_index(eng, counts, offsets, window_size, share_overlap):
    """Groups of counts[g] consecutive trials, every group with the same window offsets: (group_ptr, item_group, item_offset)
    on the engine's device, items group-major, and the grid (hop, n_windows) where the offsets are regular and the overlap
    is to be shared (else None)."""
    n_groups, n_win = len(counts), len(offsets)
    dev = eng.device
    group_ptr = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
    item_group = torch.arange(n_groups, dtype=torch.int64).repeat_interleave(n_win).to(dev)
    item_offset = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).repeat(n_groups).to(dev)
    hop = int(offsets[1] - offsets[0]) if n_win > 1 else int(window_size)
    regular = n_win >= 1 and np.array_equal(np.asarray(offsets), np.arange(n_win) * hop)
    return group_ptr, item_group, item_offset, (hop, n_win) if share_overlap and regular else None


def _ensemble_run(eng, xd, trial_rec, trial_start, counts, offsets, window_size, p, freqs, fs, measure, bands, spectra, check,
                  share_overlap):
    """Groups of counts[g] consecutive trials, every group with the same window offsets -> arrays (n_groups, n_windows, ...)."""
    n_groups, n_win = len(counts), len(offsets)
    dev = eng.device
    group_ptr, item_group, item_offset, grid = _ensemble_index(eng, counts, offsets, window_size, share_overlap)
    res = eng.sliding_ensemble(xd, torch.as_tensor(trial_rec).to(dev), torch.as_tensor(trial_start).to(dev), group_ptr,
                               item_group, item_offset, int(window_size), p, freqs, fs, measure=measure, bands=bands,
                               spectra=spectra, check=check, grid=grid)
    m = xd.shape[1]
    shape = lambda a: a.view(n_groups, n_win, m, m, a.shape[-1]) if a.dim() == 4 else a.view(n_groups, n_win)  # noqa: E731
    return tuple(shape(a) for a in res) if isinstance(res, tuple) else shape(res)


def _onset_trials(x, onsets, pre, post, window_size, hop):
    """The trials of `sliding_ensemble`'s input, on the host: (single, n_rec, trial_rec, trial_start, counts, offsets)."""
    single = np.ndim(x) == 2
    on_list = [onsets] if single else list(onsets)
    n_rec = 1 if single else int(np.shape(x)[0])
    if len(on_list) != n_rec:
        raise ValueError(f"{n_rec} recording(s) need {n_rec} onset array(s), got {len(on_list)}")
    starts, offsets, counts = [], None, []
    for on in on_list:
        st, offsets = ensemble_items(on, pre, post, window_size, hop)
        starts.append(st)
        counts.append(len(st))
    if min(counts) < 1:
        raise ValueError(f"recording {int(np.argmin(counts))} has no onsets: every group needs at least one trial")
    return single, n_rec, np.repeat(np.arange(n_rec, dtype=np.int64), counts), np.concatenate(starts), counts, offsets


def _recordings_to_device(eng, x, single):
    if isinstance(x, torch.Tensor):
        return (x[None] if single else x).to(device=eng.device, dtype=torch.float64).contiguous()
    return eng.to_device(np.asarray(x, dtype=np.float64)[None] if single else np.asarray(x, dtype=np.float64))


def sliding_ensemble(x, onsets, window_size, p, freqs, fs, *, pre, post, hop, measure="ffdtf", bands=None, spectra=False,
                     check=True, share_overlap=True, engine: Engine | None = None):
    """Short-time connectivity of event-locked data.  x (m, T) with 1-D `onsets` -> (n_windows, m, m, F | n_bands); or
    x (n_rec, m, T) with a list of onset arrays, one per recording (they may differ in length) -> (n_rec, n_windows, ...).
    Window w covers the samples onset - pre + w * hop .. + window_size of every epoch; the result for it is the reference's
    `full_freq_dtf` / `direct_dtf` / `gen_partial_directed_coherence` (measure "ffdtf" / "ddtf" / "gpdc") called with
    `np.stack([x[:, s:s + window_size] for s in onsets - pre + w * hop], axis=2)` and `optimal_model_order=p`.
    bands = (bin_lo, bin_hi): band sums instead of the full arrays.  spectra=True (ffdtf): (out, S) with
    `multivariate_spectra` of the same fit.  check: True raises LinAlgError naming the failed window, "nan" NaN-fills it,
    "mask" appends the boolean mask.  share_overlap=False keeps the direct form of K1.  p=None raises ValueError: the
    reference's `mvar_criterion` does not take 3-D input, so there is no automatic order to reproduce."""
    if p is None:
        raise ValueError("sliding_ensemble needs an integer model order p (no automatic order for ensembles)")
    single, n_rec, trial_rec, trial_start, counts, offsets = _onset_trials(x, onsets, pre, post, window_size, hop)
    eng = engine or default_engine()
    xd = _recordings_to_device(eng, x, single)
    res = _ensemble_run(eng, xd, trial_rec, trial_start, counts, offsets, window_size, p, freqs, fs, measure, bands,
                        spectra, check, share_overlap)
    return _to_host(res, single)


def _epoch_groups(epochs):
    """The groups of `sliding_ensemble_epochs`'s input, checked: (single, list of (m, L, trials) arrays, counts)."""
    single = not isinstance(epochs, (list, tuple))
    groups = [np.asarray(e, dtype=np.float64) for e in ([epochs] if single else epochs)]
    if any(e.ndim != 3 for e in groups):
        raise ValueError("epochs must have shape (channels, samples, trials)")
    m, L = groups[0].shape[:2]
    if any(e.shape[:2] != (m, L) for e in groups):
        raise ValueError("all groups of epochs must share channels and samples")
    counts = [e.shape[2] for e in groups]
    if min(counts) < 1:
        raise ValueError(f"group {int(np.argmin(counts))} has no trials: every group needs at least one trial")
    return single, groups, counts


def sliding_ensemble_epochs(epochs, window_size, hop, p, freqs, fs, *, measure="ffdtf", bands=None, spectra=False,
                            check=True, share_overlap=True, engine: Engine | None = None):
    """`sliding_ensemble` for epochs that are already cut, in the reference's own layout (m, L, trials): windows of
    `window_size` samples every `hop` samples of the L-sample epoch, each fitted from all trials -> (n_windows, m, m, F |
    n_bands).  A list of such arrays (same m and L, any numbers of trials) -> (n_groups, n_windows, ...)."""
    if p is None:
        raise ValueError("sliding_ensemble_epochs needs an integer model order p (no automatic order for ensembles)")
    single, groups, counts = _epoch_groups(epochs)
    L = groups[0].shape[1]
    eng = engine or default_engine()
    # every trial becomes one recording of L samples that starts at its own sample 0
    xd = eng.to_device(np.concatenate([np.moveaxis(e, 2, 0) for e in groups], axis=0))
    n_tr = int(sum(counts))
    res = _ensemble_run(eng, xd, np.arange(n_tr, dtype=np.int64), np.zeros(n_tr, dtype=np.int64), counts,
                        hop_positions(L, window_size, hop).astype(np.int64), window_size, p, freqs, fs, measure, bands, spectra,
                        check, share_overlap)
    return _to_host(res, single)


def _ensemble_significance_args(who, p, bands, measure, n_surrogates, m, L, window_size, split, counts, check):
    """Everything about a trial-shuffle run that can be refused without a GPU."""
    from . import surrogates as sg
    if p is None:
        raise ValueError(f"{who} needs an integer model order p (no automatic order for ensembles)")
    sg.significance_args(measure, "trial", n_surrogates, m, L, window_size, split)
    if check is not True and check != "nan":
        raise ValueError(f"check must be True or 'nan', got {check!r}")
    if bands is None or len(bands) != 2 or len(np.atleast_1d(bands[0])) < 1 or \
            len(np.atleast_1d(bands[0])) != len(np.atleast_1d(bands[1])):
        raise ValueError(f"{who} needs bands = (bin_lo, bin_hi) with at least one band")
    small = [g for g, c in enumerate(counts) if c < 2]
    if small:
        raise ValueError(f"the trial shuffle needs at least 2 trials per group, group {small[0]} has {counts[small[0]]}")


def _ensemble_significance_run(eng, xd, trial_rec, trial_start, counts, offsets, window_size, p, freqs, fs, bands, measure,
                               n_surrogates, seed, split, check, chunk, share_overlap, single):
    n_groups, n_win = len(counts), len(offsets)
    dev = eng.device
    group_ptr, item_group, item_offset, grid = _ensemble_index(eng, counts, offsets, window_size, share_overlap)
    res = eng.ensemble_significance(xd, torch.as_tensor(trial_rec).to(dev), torch.as_tensor(trial_start).to(dev), group_ptr,
                                    item_group, item_offset, int(window_size), p, freqs, fs, bands, measure=measure,
                                    n_surrogates=n_surrogates, seed=seed, split=split, check=check, chunk=chunk, grid=grid)
    out = {"tested": res["tested"].cpu().numpy()}
    for k, v in res.items():
        if k != "tested":
            a = v.cpu().numpy().reshape((n_groups, n_win) + tuple(v.shape[1:]))
            out[k] = a[0] if single else a
    return out


def sliding_ensemble_significance(x, onsets, window_size, p, freqs, fs, bands, *, pre, post, hop, measure, n_surrogates, seed,
                                  split=None, check=True, chunk=None, share_overlap=True, engine: Engine | None = None):
    """Trial-shuffle test of `sliding_ensemble(x, onsets, window_size, p, freqs, fs, pre=pre, post=post, hop=hop,
    measure=measure, bands=bands)` (`Engine.ensemble_significance`): in every surrogate the epochs of the channels >=
    split (the second participant) are permuted against those of the channels < split inside each recording's group of
    trials, one permutation per surrogate and group for all windows.  Input as `sliding_ensemble`; bands = (bin_lo,
    bin_hi) is required.  Returns a dict of NumPy arrays: observed, p, p_fwe, null_mean, null_std (n_windows, m, m,
    n_bands) or (n_rec, n_windows, ...), n_valid (n_windows,) or (n_rec, n_windows), tested (m, m).  Every group needs
    at least 2 trials.  The arguments are checked before the GPU is touched."""
    single, n_rec, trial_rec, trial_start, counts, offsets = _onset_trials(x, onsets, pre, post, window_size, hop)
    m = int(np.shape(x)[-2])
    _ensemble_significance_args("sliding_ensemble_significance", p, bands, measure, n_surrogates, m, int(pre) + int(post),
                                int(window_size), split, counts, check)
    eng = engine or default_engine()
    xd = _recordings_to_device(eng, x, single)
    return _ensemble_significance_run(eng, xd, trial_rec, trial_start, counts, offsets, window_size, p, freqs, fs, bands, measure,
                                      n_surrogates, seed, split, check, chunk, share_overlap, single)


def sliding_ensemble_epochs_significance(epochs, window_size, hop, p, freqs, fs, bands, *, measure, n_surrogates, seed,
                                         split=None, check=True, chunk=None, share_overlap=True,
                                         engine: Engine | None = None):
    """`sliding_ensemble_significance` for epochs that are already cut, (m, L, trials) or a list of such groups, as
    `sliding_ensemble_epochs` takes them: trial e of the channels < split is paired with trial pi(e) of the channels >=
    split.  Returns the same dict, shaped (n_windows, ...) or (n_groups, n_windows, ...)."""
    single, groups, counts = _epoch_groups(epochs)
    m, L = groups[0].shape[:2]
    _ensemble_significance_args("sliding_ensemble_epochs_significance", p, bands, measure, n_surrogates, m, L,
                                int(window_size), split, counts, check)
    offsets = hop_positions(L, window_size, hop).astype(np.int64)
    eng = engine or default_engine()
    xd = eng.to_device(np.concatenate([np.moveaxis(e, 2, 0) for e in groups], axis=0))
    n_tr = int(sum(counts))
    return _ensemble_significance_run(eng, xd, np.arange(n_tr, dtype=np.int64), np.zeros(n_tr, dtype=np.int64), counts, offsets,
                                      window_size, p, freqs, fs, bands, measure, n_surrogates, seed, split, check, chunk,
                                      share_overlap, single)


# ---- condition contrast of event-locked ensembles --------------------------------------------------------------------------
def _contrast_args(who, p, bands, measure, n_surrogates, m, tail, split, counts_a, counts_b, check):
    """Everything about a condition contrast that can be refused without a GPU."""
    from . import surrogates as sg
    if p is None:
        raise ValueError(f"{who} needs an integer model order p (no automatic order for ensembles)")
    if len(counts_a) != len(counts_b):
        raise ValueError(f"{who}: conditions A and B must have the same number of groups, got {len(counts_a)} and {len(counts_b)}")
    sg.contrast_args(measure, n_surrogates, m, tail, split, check, bands, counts_a, counts_b)


def _contrast_run(eng, xd, rec_a, start_a, counts_a, rec_b, start_b, counts_b, offsets, window_size, p, freqs, fs, bands, measure,
                  n_surrogates, seed, tail, split, check, chunk, share_overlap, single):
    """Trial tables of the two conditions (group-major each) -> the pool of every group (A's trials, then B's), the engine's
    test, and the result as NumPy arrays shaped (n_groups, n_windows, ...), or (n_windows, ...) for a single group."""
    dev = eng.device
    pa, pb = np.concatenate([[0], np.cumsum(counts_a)]), np.concatenate([[0], np.cumsum(counts_b)])
    order = [(c, g) for g in range(len(counts_a)) for c in (0, 1)]
    pick = lambda a, b: np.concatenate([(a, b)[c][(pa, pb)[c][g]:(pa, pb)[c][g + 1]] for c, g in order])  # noqa: E731
    trial_rec, trial_start = pick(np.asarray(rec_a), np.asarray(rec_b)), pick(np.asarray(start_a), np.asarray(start_b))
    cond = np.concatenate([np.full((counts_a, counts_b)[c][g], c, dtype=np.int64) for c, g in order])
    counts = np.asarray(counts_a) + np.asarray(counts_b)
    _, _, _, grid = _ensemble_index(eng, counts, offsets, window_size, share_overlap)
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)  # noqa: E731
    res = eng.ensemble_contrast(xd, i64(trial_rec), i64(trial_start), i64(np.concatenate([[0], np.cumsum(counts)])), i64(cond),
                                i64(offsets), int(window_size), p, freqs, fs, bands, measure=measure, n_surrogates=n_surrogates,
                                seed=seed, tail=tail, split=split, check=check, chunk=chunk, grid=grid)
    out = {}
    for k, v in res.items():
        if k == "group":
            out[k] = {kk: vv.cpu().numpy() for kk, vv in v.items()}
        else:
            a = v.cpu().numpy()
            out[k] = a[0] if single and k != "tested" else a
    return out


def sliding_ensemble_contrast(x, onsets_a, onsets_b, window_size, p, freqs, fs, bands, *, pre, post, hop, measure, n_surrogates,
                              seed, tail="two-sided", split=None, check=True, chunk=None, share_overlap=True,
                              engine: Engine | None = None):
    """Label-permutation test of the difference between two conditions of event-locked connectivity
    (`Engine.ensemble_contrast`): does the band value of `sliding_ensemble(..., measure=measure, bands=bands)` differ between
    the epochs at `onsets_a` and those at `onsets_b`?  x (m, T) with two 1-D onset arrays; or x (n_rec, m, T) with two lists
    of onset arrays, one pair per recording (a dyad).  Every recording's epochs are pooled, A's first, then B's; surrogate s
    relabels the pool keeping both sizes, one relabelling per surrogate and recording for all windows.  tail: "two-sided"
    tests |A - B|, "greater" A - B, "less" B - A.  split=None tests every pair i != j, an integer the pairs with exactly one
    index < split.  Returns a dict of NumPy arrays: observed (= A - B), observed_a, observed_b, p, p_fwe, null_mean, null_std
    (n_windows, m, m, n_bands) or (n_rec, n_windows, ...), n_valid (n_windows,) or (n_rec, n_windows), tested (m, m) and, for
    two or more recordings, group = {observed, p, p_fwe, null_mean, null_std (n_windows, m, m, n_bands), n_valid
    (n_windows,)}: the same test on the mean of A - B over the recordings.  Every recording needs at least one onset of each
    condition.  The arguments are checked before the GPU is touched."""
    single, n_rec, rec_a, start_a, counts_a, offsets = _onset_trials(x, onsets_a, pre, post, window_size, hop)
    _, _, rec_b, start_b, counts_b, _ = _onset_trials(x, onsets_b, pre, post, window_size, hop)
    m = int(np.shape(x)[-2])
    _contrast_args("sliding_ensemble_contrast", p, bands, measure, n_surrogates, m, tail, split, counts_a, counts_b, check)
    eng = engine or default_engine()
    xd = _recordings_to_device(eng, x, single)
    return _contrast_run(eng, xd, rec_a, start_a, counts_a, rec_b, start_b, counts_b, offsets, window_size, p, freqs, fs, bands,
                         measure, n_surrogates, seed, tail, split, check, chunk, share_overlap, single)


def sliding_ensemble_epochs_contrast(epochs_a, epochs_b, window_size, hop, p, freqs, fs, bands, *, measure, n_surrogates, seed,
                                     tail="two-sided", split=None, check=True, chunk=None, share_overlap=True,
                                     engine: Engine | None = None):
    """`sliding_ensemble_contrast` for epochs that are already cut: two (m, L, trials) arrays, or two lists of such groups
    (one pair per dyad; same m and L, any numbers of trials), as `sliding_ensemble_epochs` takes them.  Returns the same dict,
    shaped (n_windows, ...) or (n_groups, n_windows, ...)."""
    single, groups_a, counts_a = _epoch_groups(epochs_a)
    single_b, groups_b, counts_b = _epoch_groups(epochs_b)
    if single != single_b or groups_a[0].shape[:2] != groups_b[0].shape[:2]:
        raise ValueError("epochs_a and epochs_b must both be arrays or both be lists, with the same channels and samples")
    m, L = groups_a[0].shape[:2]
    _contrast_args("sliding_ensemble_epochs_contrast", p, bands, measure, n_surrogates, m, tail, split, counts_a, counts_b, check)
    offsets = hop_positions(L, window_size, hop).astype(np.int64)
    eng = engine or default_engine()
    # every trial becomes one recording of L samples that starts at its own sample 0: A's groups, then B's
    xd = eng.to_device(np.concatenate([np.moveaxis(e, 2, 0) for e in groups_a + groups_b], axis=0))
    na, nb_ = int(sum(counts_a)), int(sum(counts_b))
    return _contrast_run(eng, xd, np.arange(na, dtype=np.int64), np.zeros(na, dtype=np.int64), counts_a,
                         na + np.arange(nb_, dtype=np.int64), np.zeros(nb_, dtype=np.int64), counts_b, offsets, window_size, p,
                         freqs, fs, bands, measure, n_surrogates, seed, tail, split, check, chunk, share_overlap, single)
