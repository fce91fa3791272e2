"""The phase family behind `Engine.phase_sync`, `.phase_sync_pairs`, `.phase_lag`, `.phase_slabs`, `.sliding_phase_sync`,
`.sliding_phase_lag` and `.sliding_phase`: the functions of those names below, each taking the engine first.

What the family shares is here once: which measures one kernel call of which mode gives (`MODES`), what an info code means
(`SYNC_WHY`, `LAG_WHY`), the checks of z and x, the sentence that names the first refused window, the slabs of the analytic
signal, and the one sliding driver over them that feeds both kernels.  The raw callers of the three C entries
(`Engine._phase_sync`, `._phase_sync_pairs`, `._phase_lag`) stay methods of the engine, like every other entry's; the null
tests of phase synchrony are `significance`'s and build on the names here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

__all__ = ["MODES", "SYNC_WHY", "LAG_WHY", "check_z", "check_x", "raise_first_refused", "phase_sync", "phase_sync_pairs",
           "phase_lag", "phase_slabs", "sliding_phase"]

# mode of a synchrony call -> the measures its (mag, lagged) outputs are: unit phasors, the signal itself
MODES = ((_lib.PHASE_UNIT, ("plv", "ciplv")), (_lib.PHASE_RAW, ("coh", "imcoh")))
SYNC_WHY = {1: "a non-finite sample in the window", 2: "a channel of zero power in the window"}
LAG_WHY = {1: "a non-finite sample in the window",
           2: "a pair of channels whose sum |Im(z_i conj z_j)| over the window is zero: a flat or duplicated channel"}


def check_z(who, eng, z, min_m=1):
    """z must be complex128 (n_rec, m >= min_m, T) on the engine's device -> z as the kernels read it: itself where time has
    unit stride and the rows and recordings do not overlap (a strided view is read in place), else a contiguous copy."""
    if (not isinstance(z, torch.Tensor) or z.dtype != torch.complex128 or z.device != eng.device or z.dim() != 3
            or z.shape[1] < min_m):
        raise ValueError(f"{who}: z must be a complex128 tensor (n_rec, {'m' if min_m == 1 else f'm >= {min_m}'}, T) on "
                         f"{eng.device}")
    n_rec, m, T = z.shape
    if n_rec > 0 and (z.stride(2) != 1 or z.stride(1) < T or z.stride(0) < m * z.stride(1)):
        return z.contiguous()
    return z


def check_x(who, eng, x):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != eng.device or x.dim() != 3:
        raise ValueError(f"{who}: x must be a float64 tensor (n_rec, m, T) on {eng.device}")


def raise_first_refused(who, info, item_rec, item_start, bands, why, then, sel=slice(None), b0=0):
    """ValueError naming the first (recording, window, band) whose info is not 0, if there is one.  info: (rows, bands of
    the slab), row k = item sel[k] (sel as `phase_slabs` yields it), column j = band b0 + j; `then`: what check='nan' does."""
    info = info.cpu()
    bad = torch.nonzero(info)
    if bad.numel():
        k, j = (int(v) for v in bad[0])
        it, b, code = k if isinstance(sel, slice) else int(sel[k]), b0 + j, int(info[k, j])
        raise ValueError(f"{who}: recording {int(item_rec[it])}, window at sample {int(item_start[it])} (item {it}), band {b} "
                         f"{bands[b]!r} Hz: info = {code} ({why.get(code, '?')}); check='nan' {then}")


def phase_sync(eng, z, item_rec, item_start, n, mode, *, want=("mag", "lagged"), coherency=False):
    from .engine import validate_items
    z = check_z("phase_sync", eng, z)
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in ("mag", "lagged") for w in want) or not (want or coherency):
        raise ValueError(f"phase_sync: want must name 'mag' and / or 'lagged' (or coherency=True), got {want!r}")
    if int(mode) not in (_lib.PHASE_UNIT, _lib.PHASE_RAW):
        raise ValueError(f"phase_sync: mode must be PHASE_UNIT (0) or PHASE_RAW (1), got {mode!r}")
    eng.pad(z.shape[1])
    validate_items(z, item_rec, item_start, n, 0)
    return eng._phase_sync(z, item_rec, item_start, n, mode, "mag" in want, "lagged" in want, bool(coherency))


def phase_sync_pairs(eng, z, rec_a, rec_b, item_start, n, mode, *, split, shift_b=None, out=None, cols=(0, 1)):
    from .engine import validate_items
    z = check_z("phase_sync_pairs", eng, z, 2)
    n_rec, m, T = z.shape
    if int(mode) not in (_lib.PHASE_UNIT, _lib.PHASE_RAW):
        raise ValueError(f"phase_sync_pairs: mode must be PHASE_UNIT (0) or PHASE_RAW (1), got {mode!r}")
    if isinstance(split, bool) or not isinstance(split, (int, np.integer)) or not 1 <= int(split) <= m - 1:
        raise ValueError(f"phase_sync_pairs: split must be an integer in 1..{m - 1}, got {split!r}")
    cols = tuple(int(c) for c in cols)
    if len(cols) != 2 or min(cols) < -1 or max(cols) < 0 or cols[0] == cols[1]:
        raise ValueError(f"phase_sync_pairs: cols must be two different columns (col_mag, col_lagged), -1 for an output "
                         f"that is not wanted and not both, got {cols!r}")
    eng.pad(m)
    for name, rec in (("rec_a", rec_a), ("rec_b", rec_b)):
        try:
            validate_items(z, rec, item_start, n, 0)
        except ValueError as err:                      # the message names the table that is wrong
            raise ValueError("phase_sync_pairs: " + str(err).replace("item_rec", name)) from None
    n_items = int(rec_a.numel())
    if shift_b is not None:
        if (not isinstance(shift_b, torch.Tensor) or shift_b.dtype != torch.int64 or shift_b.device != z.device
                or shift_b.shape != (n_items,)):
            raise ValueError(f"phase_sync_pairs: shift_b must be a 1-D int64 tensor on {z.device}, one entry per item")
        if n_items:
            lo, hi = torch.stack([shift_b.min(), shift_b.max()]).cpu().tolist()
            if lo < 0 or hi >= T:
                raise ValueError(f"phase_sync_pairs: shift_b must lie in [0, {T}), got [{lo}, {hi}]")
        shift_b = shift_b.contiguous()
    if out is None:
        out = torch.full((n_items, m, m, 1 + max(cols)), float("nan"), dtype=torch.float64, device=eng.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != eng.device or out.dim() != 4
          or tuple(out.shape[:3]) != (n_items, m, m) or out.shape[3] <= max(cols) or not out.is_contiguous()):
        raise ValueError(f"phase_sync_pairs: out must be a contiguous float64 tensor ({n_items}, {m}, {m}, K) on "
                         f"{eng.device} with K > {max(cols)}")
    return eng._phase_sync_pairs(z, rec_a.contiguous(), rec_b.contiguous(), item_start.contiguous(), n, mode, split,
                                 shift_b, out, cols)


def phase_lag(eng, z, item_rec, item_start, n, *, want=("wpli",), split=0):
    from .eeg_io import check_phase_lag_split, resolve_phase_lag_measures
    from .engine import validate_items
    z = check_z("phase_lag", eng, z)
    want = resolve_phase_lag_measures(want)
    split = check_phase_lag_split(split, z.shape[1], "phase_lag")
    eng.pad(z.shape[1])
    validate_items(z, item_rec, item_start, n, 0)
    return eng._phase_lag(z, item_rec, item_start, n, want, split)


def phase_slabs(eng, x, item_rec, item_start, resp, max_workspace_bytes):
    n_rec, m, T = x.shape
    nb = int(resp.shape[0])
    if item_rec.numel() == 0:
        return
    unit = 16 * m * T
    B = int(max(1, min(nb, int(max_workspace_bytes) // unit - 2)))
    R = int(max(1, min(n_rec, (int(max_workspace_bytes) // unit - 2) // nb))) if B == nb else 1
    rec_host = item_rec.cpu()
    for r0 in range(0, n_rec, R):
        r1 = min(n_rec, r0 + R)
        if R >= n_rec:
            sel, rec_s, start_s = slice(None), item_rec, item_start
        else:
            sel = torch.nonzero((rec_host >= r0) & (rec_host < r1)).flatten().to(eng.device)
            if sel.numel() == 0:
                continue
            rec_s, start_s = item_rec[sel] - r0, item_start[sel]
        for b0 in range(0, nb, B):
            b1 = min(nb, b0 + B)
            z = eng.analytic_signal(x[r0:r1], resp[b0:b1]).view(-1, m, T)       # recording (r, b) = (r - r0) * (b1 - b0) + b
            bb = torch.arange(b1 - b0, dtype=torch.int64, device=eng.device)
            rec_z = (rec_s[:, None] * (b1 - b0) + bb[None, :]).reshape(-1)
            start_z = start_s[:, None].expand(-1, b1 - b0).reshape(-1)
            yield sel, b0, b1, z, rec_z, start_z
            del z


def sliding_phase(eng, who, x, item_rec, item_start, n, fs, bands_hz, *, sync=None, lag=None, split=0, order=4, check=True,
                  max_workspace_bytes=8 << 30):
    from .eeg_io import check_phase_lag_split, resolve_bands_hz
    from .engine import validate_items
    check_x(who, eng, x)
    if check is not True and check != "nan":
        raise ValueError(f"{who}: check must be True or 'nan', got {check!r}")
    n_rec, m, T = x.shape
    if lag:
        split = check_phase_lag_split(split, m, who)
    eng.pad(m)
    bands = resolve_bands_hz(bands_hz, fs)
    validate_items(x, item_rec, item_start, n, 0)
    nb, n_items = len(bands), int(item_rec.numel())
    resp = torch.stack([eng.band_response(T, fs, lo, hi, order) for lo, hi in bands])
    modes = [(mode, [q for q in sync or () if q in names], names) for mode, names in MODES]
    modes = [(mode, qs, names) for mode, qs, names in modes if qs]
    outs = [{q: eng.empty(n_items, nb, m, m) for q in qs or ()} for qs in (sync, lag)]
    infos = [torch.zeros(n_items, nb, dtype=torch.int32, device=eng.device) for _ in range(2)]
    for sel, b0, b1, z, rec_z, start_z in phase_slabs(eng, x, item_rec, item_start, resp, max_workspace_bytes):
        for mode, qs, names in modes:
            res = eng._phase_sync(z, rec_z, start_z, n, mode, names[0] in qs, names[1] in qs, False)
            for q, key in zip(names, ("mag", "lagged")):
                if q in qs:
                    outs[0][q][sel, b0:b1] = res[key].view(-1, b1 - b0, m, m)
            infos[0][sel, b0:b1] = torch.maximum(infos[0][sel, b0:b1], res["info"].view(-1, b1 - b0))
        if lag:
            res = eng._phase_lag(z, rec_z, start_z, n, lag, split)
            for q in lag:
                outs[1][q][sel, b0:b1] = res[q].view(-1, b1 - b0, m, m)
            infos[1][sel, b0:b1] = res["info"].view(-1, b1 - b0)
        del z
    for qs, info, why, name in ((sync, infos[0], SYNC_WHY, "sliding_phase_sync"), (lag, infos[1], LAG_WHY, "sliding_phase_lag")):
        if qs and check is True and n_items:
            raise_first_refused(name, info, item_rec, item_start, bands, why, "returns the arrays with their NaNs")
    for out, info in zip(outs, infos):
        out["info"] = info
    return (outs[0] if sync else None), (outs[1] if lag else None)
