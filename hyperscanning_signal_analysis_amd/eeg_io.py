"""NetCDF front-end feeding the MVAR engine: the semantics of the reference's `load_eeg_signals`
(/root/reference/src/mne_bridge.py:113-223) -- Butterworth-4 zero-phase high/low-pass, 50 Hz notch
(Q = 15) when 50 Hz is below Nyquist, trim to [0, event_duration], drop the M1/M2 mastoids, optional channel
subset, per-channel z-score -- split into a pure-array function (`preprocess_eeg`, testable without
xarray) and thin file readers (xarray imported lazily; the reference's files are NETCDF4_CLASSIC written by
`DataArray.to_netcdf`, /root/reference/src/export.py:606).

Host-side O(n) DSP with the same SciPy calls as the reference; this is SURVEY.md section 8(f) row 2 (the
caller side of the hot path), not GPU work.
"""
from __future__ import annotations

import numpy as np

__all__ = ["filter_eeg", "preprocess_eeg", "load_eeg_signals", "load_dyad_block", "decimation_taps", "DECIMATION_DESIGNS",
           "band_response", "PHASE_MEASURES", "resolve_phase_measures", "PHASE_LAG_MEASURES", "resolve_phase_lag_measures",
           "check_phase_lag_split", "resolve_bands_hz"]


def filter_eeg(data_tc, fs, low_cutoff_hz=None, high_cutoff_hz=None):
    """The filter sequence of `load_eeg_signals` (mne_bridge.py:152-183) on (time, channel) samples: zero-phase
    Butterworth-4 high-pass, low-pass, then the 50 Hz notch (Q = 15) when 50 Hz is below Nyquist."""
    from scipy.signal import butter, filtfilt, iirnotch
    # filtered channel by channel along a CONTIGUOUS time axis: the same recurrences on the same numbers as
    # filtfilt(..., axis=0) on the (time, channel) array -- bit-identical -- at half the time (110 001 x 34: 0.56 -> 0.28 s
    # per filter), which is what bounds a config-5 batch once the GPU work is out of the way
    x = np.ascontiguousarray(np.asarray(data_tc, dtype=np.float64).T)
    nyq = fs / 2.0
    for cutoff, kind, label in ((low_cutoff_hz, "highpass", "low_cutoff_hz"), (high_cutoff_hz, "lowpass", "high_cutoff_hz")):
        if cutoff is None:
            continue
        wn = float(cutoff) / nyq
        if not 0.0 < wn < 1.0:
            raise ValueError(f"Invalid {label}={cutoff}. Must satisfy 0 < cutoff < {nyq:.3f} Hz.")
        b, a = butter(4, wn, btype=kind)
        x = filtfilt(b, a, x, axis=-1)
    if 50.0 < nyq:
        b, a = iirnotch(50.0, Q=15, fs=fs)
        x = filtfilt(b, a, x, axis=-1)
    return x.T


DECIMATION_DESIGNS = ("decimate", "resample_poly")


def decimation_taps(q, design="decimate"):
    """The anti-aliasing FIR of an integer-factor decimation by q, as float64 taps on the host (SciPy's own calls).
        "decimate"       scipy.signal.decimate(x, q, ftype='fir', zero_phase=True) -- what the reference's
                         `MultimodalData._decimate_signals` calls (data_structures.py:792):
                         firwin(20 q + 1, 1 / q, window="hamming")
        "resample_poly"  scipy.signal.resample_poly(x, 1, q) -- `_downsample_signal` (eeg_alpha_ibi_ffdtf.py:404):
                         firwin(20 q + 1, 1 / q, window=("kaiser", 5.0))
    A 1-D array is taken as the taps themselves (odd length, 3 .. 641)."""
    from . import _lib
    q = int(q)
    if not 2 <= q <= _lib.MAX_DECIMATE:
        raise ValueError(f"decimation factor must be in 2..{_lib.MAX_DECIMATE}, got {q}")
    if isinstance(design, str):
        from scipy.signal import firwin
        if design == "decimate":
            return firwin(20 * q + 1, 1.0 / q, window="hamming")
        if design == "resample_poly":
            return firwin(20 * q + 1, 1.0 / q, window=("kaiser", 5.0))
        raise ValueError(f"design must be one of {DECIMATION_DESIGNS} or a 1-D array of taps, got {design!r}")
    h = np.ascontiguousarray(np.asarray(design, dtype=np.float64))
    if h.ndim != 1 or h.size % 2 == 0 or not 3 <= h.size <= _lib.MAX_DECIMATE_TAPS:
        raise ValueError(f"taps must be a 1-D array of odd length in 3..{_lib.MAX_DECIMATE_TAPS}, got shape {h.shape}")
    return h


PHASE_MEASURES = ("plv", "ciplv", "coh", "imcoh")


def resolve_phase_measures(measures):
    """`measures` of the phase-synchrony calls -> a tuple without repeats, in the caller's order.  Needs no GPU."""
    if isinstance(measures, str):
        measures = (measures,)
    out = tuple(dict.fromkeys(measures))
    unknown = [q for q in out if q not in PHASE_MEASURES]
    if not out or unknown:
        raise ValueError(f"phase synchrony measures must be a non-empty subset of {PHASE_MEASURES}, got {tuple(measures)!r}")
    return out


PHASE_LAG_MEASURES = ("pli", "wpli", "dwpli")


def resolve_phase_lag_measures(measures):
    """`measures` of the phase-lag calls (PLI, weighted PLI, debiased squared weighted PLI) -> a tuple without repeats, in
    the caller's order.  A family of its own: `PHASE_MEASURES` does not list these names.  Needs no GPU."""
    if isinstance(measures, str):
        measures = (measures,)
    out = tuple(dict.fromkeys(measures))
    unknown = [q for q in out if q not in PHASE_LAG_MEASURES]
    if not out or unknown:
        raise ValueError(f"phase-lag measures must be a non-empty subset of {PHASE_LAG_MEASURES}, got {tuple(measures)!r}")
    return out


def check_phase_lag_split(split, m, who):
    """`split` of the phase-lag calls -> int: 0 (all pairs) or 1..m-1 (the pairs i < split <= j only).  Needs no GPU."""
    if isinstance(split, bool) or not isinstance(split, (int, np.integer)) or not 0 <= int(split) <= max(0, int(m) - 1):
        raise ValueError(f"{who}: split must be 0 (all pairs) or an integer in 1..{int(m) - 1} (the inter-brain pairs "
                         f"i < split <= j only), got {split!r}")
    return int(split)


def resolve_bands_hz(bands_hz, fs):
    """`bands_hz` -> a tuple of (lo, hi) in Hz with None for an edge that is not there (lo <= 0, hi >= fs / 2), as
    `band_response` reads them.  ValueError for an empty list, an entry that is not a pair, or lo >= hi.  Needs no GPU."""
    nyq = float(fs) / 2.0
    if not nyq > 0.0:
        raise ValueError(f"the sampling rate must be positive, got {fs!r}")
    out = []
    for band in bands_hz:
        if np.ndim(band) != 1 or len(band) != 2:
            raise ValueError(f"bands_hz must be a sequence of (lo, hi) pairs in Hz, got the entry {band!r}")
        lo, hi = band
        lo = None if lo is None or float(lo) <= 0.0 else float(lo)
        hi = None if hi is None or float(hi) >= nyq else float(hi)
        if hi is not None and not hi > 0.0 or (lo is not None and not lo < nyq) or (lo is not None and hi is not None and lo >= hi):
            raise ValueError(f"band {band!r}: the lower edge must lie below the upper edge and both inside (0, {nyq:g}) Hz")
        out.append((lo, hi))
    if not out:
        raise ValueError("bands_hz is empty: at least one (lo, hi) band is needed")
    return tuple(out)


def band_response(T, fs, lo=None, hi=None, order=4):
    """The one-sided zero-phase response of a Butterworth band on the FFT grid f_k = np.fft.fftfreq(T, 1 / fs), as (T,)
    float64:  resp[k] = |H(|f_k|)|^2 * w[k].  H is the response (`sosfreqz`) of `butter(order, [lo, hi] / (fs / 2),
    btype="band", output="sos")`, squared in magnitude as forward-backward filtering applies it; w holds the weights of
    `scipy.signal.hilbert`: 1 at k = 0 and (T even) k = T / 2, 2 for 0 < k < T / 2, 0 on the negative frequencies.
    lo None or <= 0: a low-pass at hi; hi None or >= fs / 2: a high-pass at lo; both: w alone, the plain Hilbert transform.

    The analytic band signal of a row x is z = ifft(fft(x) * resp)  (`Engine.analytic_signal`).  It is CIRCULAR: the
    samples within the filter's transient of either end of the recording see the other end.  Nothing is padded; keep the
    windows away from the two ends by the transient (a few periods of the lower band edge), or accept the wrap.  This is
    a definition of its own, not `sosfiltfilt` followed by `hilbert`: the two agree away from the ends (PLV to < 1e-3 on
    the planted dyad of tests/test_phase_sync_cpu.py) and differ in how they treat the ends."""
    T = int(T)
    fs = float(fs)
    if T < 1 or not fs > 0.0 or int(order) < 1:
        raise ValueError(f"band_response: need T >= 1, fs > 0 and order >= 1, got T={T}, fs={fs}, order={order}")
    nyq = fs / 2.0
    lo = None if lo is None or float(lo) <= 0.0 else float(lo)
    hi = None if hi is None or float(hi) >= nyq else float(hi)
    if lo is not None and hi is not None and lo >= hi:
        raise ValueError(f"band_response: the lower edge ({lo:g} Hz) must lie below the upper edge ({hi:g} Hz)")
    k = np.arange(T)
    w = np.zeros(T)
    w[0] = 1.0
    w[(k > 0) & (2 * k < T)] = 2.0
    if T % 2 == 0:
        w[T // 2] = 1.0
    if lo is None and hi is None:
        return w
    from scipy.signal import butter, sosfreqz
    try:
        if lo is None:
            sos = butter(int(order), hi / nyq, btype="low", output="sos")
        elif hi is None:
            sos = butter(int(order), lo / nyq, btype="high", output="sos")
        else:
            sos = butter(int(order), [lo / nyq, hi / nyq], btype="band", output="sos")
    except ValueError as e:
        raise ValueError(f"band_response: no Butterworth filter for the band ({lo}, {hi}) Hz at fs = {fs:g} Hz: {e}") from None
    _, h = sosfreqz(sos, worN=2.0 * np.pi * np.abs(np.fft.fftfreq(T, 1.0 / fs)) / fs)
    return np.abs(h) ** 2 * w


def preprocess_eeg(data_tc, time_s, channel_names, fs, event_duration_s=None, channel_subset=None,
                   low_cutoff_hz=None, high_cutoff_hz=None, source="<array>"):
    """(time, channel) samples -> (signals (n_chan, n_samp) z-scored, names, time_s trimmed)."""
    x = filter_eeg(data_tc, fs, low_cutoff_hz, high_cutoff_hz)
    t = np.asarray(time_s, dtype=np.float64)
    names = [str(c) for c in channel_names]
    if event_duration_s is None:
        event_duration_s = float(t[-1])
    keep_t = (t >= 0.0) & (t <= event_duration_s)
    x, t = x[keep_t], t[keep_t]
    keep_c = [k for k, c in enumerate(names) if c not in ("M1", "M2")]
    if channel_subset is not None:
        avail = [names[k] for k in keep_c]
        keep_c = [names.index(c) for c in channel_subset if c in avail]
        if not keep_c:
            raise ValueError(f"None of the requested channels {channel_subset} found in {source}. Available: {avail}")
    sig = np.ascontiguousarray(x[:, keep_c].T)
    sd = np.std(sig, axis=1, keepdims=True)
    sd[sd == 0] = 1.0
    sig = (sig - np.mean(sig, axis=1, keepdims=True)) / sd
    return sig, [names[k] for k in keep_c], t


def load_eeg_signals(ncdf_path, channel_subset=None, low_cutoff_hz=None, high_cutoff_hz=None):
    """(signals, channel_names, fs, time_s, event_duration_s) of one exported EEG NetCDF file."""
    try:
        import xarray as xr
    except ImportError as e:  # pragma: no cover
        raise ImportError("load_eeg_signals needs xarray + netCDF4 to read the reference's .nc files") from e
    da = xr.open_dataarray(ncdf_path)
    try:
        if "time" not in da.dims or "channel" not in da.dims:
            raise ValueError(f"Expected 'time' and 'channel' dimensions in {ncdf_path}, got {da.dims}")
        fs = float(da.attrs.get("sampling_freq", da.attrs.get("sampling_frequency_Hz", 128.0)))
        t = da.coords["time"].values
        dur = float(da.attrs.get("event_duration", t[-1]))
        sig, names, t = preprocess_eeg(da.transpose("time", "channel").values, t, da.coords["channel"].values, fs,
                                       dur, channel_subset, low_cutoff_hz, high_cutoff_hz, source=str(ncdf_path))
    finally:
        da.close()
    return sig, names, fs, t, dur


def load_dyad_block(child_path, caregiver_path, **kw):
    """np.vstack([child, caregiver]) on their common length: the (2 x n_chan, T) block the sliding-window
    engine takes (BASELINE.json config 2); returns (block, names, fs)."""
    a, na, fs_a, _, _ = load_eeg_signals(child_path, **kw)
    b, nb, fs_b, _, _ = load_eeg_signals(caregiver_path, **kw)
    if fs_a != fs_b:
        raise ValueError(f"sampling rates differ: {fs_a} vs {fs_b}")
    T = min(a.shape[1], b.shape[1])
    return np.vstack([a[:, :T], b[:, :T]]), [f"ch_{c}" for c in na] + [f"cg_{c}" for c in nb], fs_a
