"""Device-side engine: stages buffers with PyTorch-ROCm and drives the HIP kernels through the C ABI.

PyTorch is plumbing here (device memory, streams, H2D/D2H copies); all arithmetic of the hot path
runs in libhypermvar.so.  Every method takes / returns torch tensors that live on the engine's device;
`hyperscanning_signal_analysis_amd.mtmvar` wraps them into the reference's NumPy signatures.

Layouts ("MP layout": channels padded to MP = 16*ceil(m/16)):
    R       (items, p+1, MP, MP)      lag covariances                               K1
    ar      (items, MP, MP, p)        AR coefficients, lag fastest                  K2
    V       (items, MP, MP)           residual covariance                           K2
    P/H/A/S (items, F, MP, MP)        kernel-natural per-frequency matrices         K3 / K5
    ffdtf   (items, m, m, F)          the reference's (m, m, F) array per window    K4
"""
from __future__ import annotations

import dataclasses
import types
import typing
from typing import Callable

import numpy as np
import torch

from . import _lib, phase, significance
from . import surrogates as sg

__all__ = ["Engine", "default_engine", "SingularMatrixError", "validate_items", "validate_trials", "check_block_split"]


# Pivot threshold of the per-frequency inverses of A(f) (K3): a row interchange happens only when some row's |re| + |im|
# exceeds the diagonal's by more than a factor 1 / tau (threshold partial pivoting: multipliers bounded by 1 / tau).
# tau = 1 is LAPACK's partial pivoting.  A(f) = I - sum_k A_k z_k is close to the identity; with tau = 1 nine per cent of
# its pivot columns interchange two rows whose candidates differ by a few per cent -- an interchange that buys no
# accuracy (max-norm distance to numpy.linalg.inv 2.2e-15 either way, measured on the north-star dyad) and costs every
# wave of the workgroup a trip through LDS: K3 8.19 -> 7.64 ms at tau = 0.25, where 0.2 % of the columns still
# interchange (profiles/r03_k3_ab_notes.md).  `Engine(pivot_tau=1.0)` or HYPERMVAR_PIVOT_TAU=1 restores LAPACK's rule;
# the general complex inverse (partial coherence of arbitrary spectral matrices) always uses tau = 1.
DEFAULT_PIVOT_TAU = 0.25


class SingularMatrixError(np.linalg.LinAlgError):
    """Raised where the reference's np.linalg.solve / np.linalg.inv raise LinAlgError('Singular matrix')."""


def validate_items(x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int):
    """Refuse window descriptors the kernels would read out of bounds with, BEFORE anything is launched: wrong
    dtype / device, a recording index outside x, a window that does not lie inside its recording (one tiny
    reduction on the tensors' device).  x: (n_rec, m, T).  Pure tensor logic: also runs on CPU tensors."""
    n_rec, m, T = x.shape
    for name, t in (("item_rec", item_rec), ("item_start", item_start)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != x.device or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D int64 tensor on {x.device}")
    if item_rec.numel() != item_start.numel():
        raise ValueError("item_rec and item_start must have the same length")
    if int(n) <= int(p):
        raise ValueError(f"window length ({n}) must exceed the model order ({p})")
    if int(n) > T:
        raise ValueError(f"window length ({n}) exceeds the recording length ({T})")
    if item_rec.numel() == 0:
        return
    lim = torch.stack([item_rec.min(), item_rec.max(), item_start.min(), item_start.max()]).cpu().tolist()
    if lim[0] < 0 or lim[1] >= n_rec:
        raise ValueError(f"item_rec must lie in [0, {n_rec}), got [{lim[0]}, {lim[1]}]")
    if lim[2] < 0 or lim[3] + int(n) > T:
        raise ValueError(f"windows [start, start + {n}) must lie in [0, {T}), got starts in [{lim[2]}, {lim[3]}]")


def validate_trials(x: torch.Tensor, trial_rec: torch.Tensor, trial_start: torch.Tensor, group_ptr: torch.Tensor,
                    item_group: torch.Tensor, item_offset: torch.Tensor, n: int, p: int):
    """Refuse an event-locked ensemble the kernels would read out of bounds with, BEFORE anything is launched (the
    counterpart of `validate_items` for `Engine.lagcov_ensemble` / `sliding_ensemble`).  x: (n_rec, m, T); trial e is the
    epoch starting at trial_start[e] of recording trial_rec[e]; group g owns the trials group_ptr[g] .. group_ptr[g+1]-1;
    item `it` is the window of n samples item_offset[it] samples after every trial start of group item_group[it].
    Checked: int64 1-D tensors on x's device, group_ptr non-decreasing from 0 to the number of trials with no empty group,
    trial_rec and item_group in range, every window of every trial inside its recording, n > p.  The ValueError names the
    first offender.  Pure tensor logic: also runs on CPU tensors."""
    n_rec, m, T = x.shape
    n, p = int(n), int(p)
    named = (("trial_rec", trial_rec), ("trial_start", trial_start), ("group_ptr", group_ptr), ("item_group", item_group),
             ("item_offset", item_offset))
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != x.device or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D int64 tensor on {x.device}")
    if trial_rec.numel() != trial_start.numel():
        raise ValueError("trial_rec and trial_start must have the same length")
    if item_group.numel() != item_offset.numel():
        raise ValueError("item_group and item_offset must have the same length")
    if n <= p:
        raise ValueError(f"window length ({n}) must exceed the model order ({p})")
    if n > T:
        raise ValueError(f"window length ({n}) exceeds the recording length ({T})")
    n_trials, n_groups = int(trial_rec.numel()), int(group_ptr.numel()) - 1
    if n_groups < 1:
        raise ValueError("group_ptr must have at least two entries (one group)")
    gp = group_ptr.cpu()
    if int(gp[0]) != 0 or int(gp[-1]) != n_trials:
        raise ValueError(f"group_ptr must run from 0 to the number of trials ({n_trials}), got {int(gp[0])} .. {int(gp[-1])}")
    counts = gp[1:] - gp[:-1]
    if bool((counts < 0).any()):
        g = int(torch.nonzero(counts < 0)[0])
        raise ValueError(f"group_ptr must be non-decreasing (group {g}: {int(gp[g])} > {int(gp[g + 1])})")
    if bool((counts == 0).any()):
        raise ValueError(f"group {int(torch.nonzero(counts == 0)[0])} is empty: every group needs at least one trial")
    bad = torch.nonzero((trial_rec < 0) | (trial_rec >= n_rec)).flatten()
    if bad.numel():
        e = int(bad[0])
        raise ValueError(f"trial_rec must lie in [0, {n_rec}), got {int(trial_rec[e])} for trial {e}")
    if item_group.numel() == 0:
        return
    bad = torch.nonzero((item_group < 0) | (item_group >= n_groups)).flatten()
    if bad.numel():
        it = int(bad[0])
        raise ValueError(f"item_group must lie in [0, {n_groups}), got {int(item_group[it])} for item {it}")
    # earliest and latest trial start of every group: a window lies inside for all trials iff it does for these two
    gid = torch.repeat_interleave(torch.arange(n_groups, dtype=torch.int64), counts).to(x.device)
    lo = torch.full((n_groups,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=x.device)
    hi = torch.full((n_groups,), torch.iinfo(torch.int64).min, dtype=torch.int64, device=x.device)
    lo = lo.scatter_reduce(0, gid, trial_start, "amin")
    hi = hi.scatter_reduce(0, gid, trial_start, "amax")
    bad = torch.nonzero((lo[item_group] + item_offset < 0) | (hi[item_group] + item_offset + n > T)).flatten()
    if bad.numel():
        it = int(bad[0])
        g, off = int(item_group[it]), int(item_offset[it])
        st = trial_start[int(gp[g]):int(gp[g + 1])] + off
        e = int(gp[g]) + int(torch.nonzero((st < 0) | (st + n > T))[0])
        s0 = int(trial_start[e]) + off
        raise ValueError(f"windows [start, start + {n}) must lie in [0, {T}): item {it} (group {g}, offset {off}) of "
                         f"trial {e} covers [{s0}, {s0 + n})")


MAX_ORDER = 32          # HMV_MAX_ORDER of include/hypermvar.h


def auto_order_args(max_model_order, crit_type, n):
    """Arguments of the automatic model order (`p=None`), checked before the GPU is touched: the reference's ValueError
    for an unknown criterion (mtmvar.py:588-589), the largest order within 1..32, a window longer than it.  Returns
    (pmax, criterion number of the C ABI)."""
    if crit_type not in _lib.CRITERIA:
        raise ValueError("Invalid criterion type. Choose from 'AIC', 'HQ', 'SC'.")
    if isinstance(max_model_order, bool) or int(max_model_order) != max_model_order:
        raise ValueError(f"max_model_order must be an integer in 1..{MAX_ORDER}, got {max_model_order!r}")
    pmax = int(max_model_order)
    if not 1 <= pmax <= MAX_ORDER:
        raise ValueError(f"max_model_order must be an integer in 1..{MAX_ORDER}, got {max_model_order!r}")
    if int(n) <= pmax:
        raise ValueError(f"window length ({n}) must exceed max_model_order ({pmax})")
    return pmax, _lib.CRITERIA[crit_type]


def no_auto_order(p, where: str):
    """`p=None` where the automatic order is not offered yet."""
    if p is None:
        raise ValueError(f"{where}: the automatic model order (p=None) is not offered here yet; pass an integer p "
                         "(sliding_ffdtf / sliding_ddtf / sliding_gpdc / sliding_ffdtf_spectra select it per window)")


def check_block_split(split, m: int, where: str) -> int:
    """`split` of the block measures, checked before the GPU is touched: an integer with 1 <= split <= m - 1 (channels
    < split are block A, the others block B; both need a channel)."""
    if isinstance(split, (bool, float)) or not isinstance(split, (int, np.integer)):
        raise ValueError(f"{where}: split must be an integer in 1..m-1, got {split!r}")
    if not 1 <= int(split) <= int(m) - 1:
        raise ValueError(f"{where}: split must be an integer in 1..m-1 = 1..{int(m) - 1}, got {int(split)}")
    return int(split)


def no_block_auto_order(p, where: str):
    """`p=None` of the block Granger calls: the restricted fits need the full fit's order, which is fixed."""
    if p is None:
        raise ValueError(f"{where}: the automatic model order (p=None) is not available for this call; pass an integer p")
    if isinstance(p, (bool, float)) or int(p) != p or not 1 <= int(p) <= MAX_ORDER:
        raise ValueError(f"{where}: p must be an integer in 1..{MAX_ORDER}, got {p!r}")
    return int(p)


def resolve_pivoted_yw(pivoted_yw) -> bool:
    """`Engine(pivoted_yw=...)`: a bool, or None for the environment variable HYPERMVAR_YW_PIVOTED (unset, empty, "0",
    "false", "no", "off": off; anything else: on).  Needs no GPU."""
    if pivoted_yw is None:
        import os
        return os.environ.get("HYPERMVAR_YW_PIVOTED", "").strip().lower() not in ("", "0", "false", "no", "off")
    if not isinstance(pivoted_yw, (bool, np.bool_)):
        raise ValueError(f"pivoted_yw must be True, False or None, got {pivoted_yw!r}")
    return bool(pivoted_yw)


def no_pivoted_auto_order(pivoted: bool, where: str):
    """The automatic model order compares the criterion curve of the recursion; the pivoted LU has none."""
    if pivoted:
        raise ValueError(f"{where}: the automatic model order (p=None) is not available with the pivoted Yule-Walker "
                         "fallback (pivoted_yw / HYPERMVAR_YW_PIVOTED / FLAG_YW_PIVOTED): an LU gives no criterion curve; "
                         "pass an integer p")


def route_counts(route) -> dict:
    """{"recursion", "ldlt", "lu"}: how many windows each K2 solver took, from their route words (0 / 1 / 2)."""
    r = np.asarray(route.cpu() if isinstance(route, torch.Tensor) else route).reshape(-1)
    return {"recursion": int((r == 0).sum()), "ldlt": int((r == 1).sum()), "lu": int((r == 2).sum())}


_MEASURES = {"ffdtf": _lib.MEASURE_FFDTF, "ddtf": _lib.MEASURE_DDTF, "gpdc": _lib.MEASURE_GPDC}
_NO_ENSEMBLE_ORDER = ("ensemble fits need an integer model order p: the reference's mvar_criterion does not take "
                      "(channels, samples, trials) input, so there is no automatic order to reproduce")


class _Info(typing.NamedTuple):
    """One LAPACK-style info array of a fused C entry."""
    name: str                   # `call` finds its pointer as info_<name>
    text: str                   # the stage as `raise_on_info` words it
    per_item: int | None = 1    # entries per item; None: one per frequency
    rows: bool = False          # handed out as (items, per_item), not flat


class _More(typing.NamedTuple):
    """One output of a fused C entry behind `out`."""
    name: str                   # `call` finds its pointer under this name
    shape: Callable             # (items, m, F) -> the buffer the C entry writes
    nan: bool = True            # check="nan" fills the failed items
    give: Callable = lambda buf, info: buf      # (the buffer, the info arrays by name) -> its place in the result tuple


_SPECTRA = _More("S", lambda items, m, F: (items, m, m, F, 2), give=lambda S, info: torch.view_as_complex(S))
_BLOCK_TIME = _More("time", lambda items, m, F: (items, 4))
_BLOCK_RED = _More("red", lambda items, m, F: (items, 2), nan=False, give=lambda red, info: (red, info["red"]))
_YW_TEXT = "ar_coeff (Yule-Walker solve; a negative info: residual covariance not positive definite)"
_BLOCK_INFO_RED = _Info("red", "block Granger causality (Yule-Walker solve of one block alone)", per_item=2, rows=True)
_BLOCK_INFO_GC = _Info("gc", "block Granger causality (per-frequency factorisation)", per_item=None)
# what `call` sees for an output or an info array its route does not have: a null pointer
_ABSENT = dict(S=0, time=0, red=0, info_tf=0, info_red=0, info_gc=0)


def _measure_infos(measure, yw_text):
    """info_yw, and info_tf behind it unless the measure is GPDC, which never inverts A(f)."""
    yw = _Info("yw", yw_text)
    return (yw,) if measure == "gpdc" else (yw, _Info("tf", "mvar_transfer_function (inverse of A(f))", per_item=None))


@dataclasses.dataclass(frozen=True)
class _Route:
    """What is particular to one fused C entry (`Engine._route`, `_ensemble_route`, `_mix_route`, `_pairs_route`,
    `_block_route`, `_block_pairs_route`); `Engine._sliding_call` is everything the entries share.  A new entry is a new
    route, not a new driver."""
    name: str                   # who the "bad sizes" refusal says it is (sliding_<measure>, with or without spectra)
    measure: str                # "ffdtf", "ddtf", "gpdc" or "block_gc"
    p: int                      # lags of the coefficient arrays: the order, or max_model_order of the automatic order
    order_text: str             # the order (and what else sizes the workspace) as the "bad sizes" refusal words it
    infos: tuple                # the `_Info` arrays, info_yw first, in the order check=True raises; None: not asked for
    validate: Callable          # (x, items): the descriptors against x, ValueError before anything is launched
    grid: Callable              # (x, items, n_items, grid, compare) -> the grid arguments of the C entry
    ws_bytes: Callable          # (chunk, m, F, n_bands, grid arguments) -> hmv_sliding_*_workspace_bytes
    call: Callable              # (the driver's pointers and sizes) -> (name of the C entry, its argument tuple)
    more: tuple = ()            # the `_More` outputs behind `out`, in the result's order; None: not asked for
    row: tuple | None = None    # an output row in front of the frequency axis, where not (m, m)
    zero_infos: bool = False    # the info arrays start at zero, where the entry's kernels are not known to write them all
    automatic: bool = False     # the order is selected per window: `orders` and `crit` exist
    per_item: Callable | None = None    # (m, F, n_bands) -> bytes that size the chunk, where not ws_bytes(1, ...)
    blame: Callable | None = None       # (SingularMatrixError, items): what the route adds to the error
    m: int | None = None                # the channel count, where x does not carry it (the mix route: x is the stack)

    @property
    def bands_in_k3(self) -> bool:      # ffDTF: K3's row workers add the bands up (where `bands_in_kernel` allows)
        return self.measure == "ffdtf"


class Engine:
    def __init__(self, device=None, pivot_tau: float | None = None, max_workspace_bytes: int = 24 << 30,
                 pivoted_yw: bool | None = None):
        """pivoted_yw: windows that the Yule-Walker solvers refuse (info != 0: a pivot that rounding made non-positive,
        from cond ~ 1e13 on) are solved again by the dense LU with partial pivoting, like the reference's
        `np.linalg.solve`; the engine ORs `FLAG_YW_PIVOTED` into every fixed-order call.  None: HYPERMVAR_YW_PIVOTED."""
        import os
        self.pivoted_yw = resolve_pivoted_yw(pivoted_yw)
        self.yw_flag = _lib.FLAG_YW_PIVOTED if self.pivoted_yw else 0
        if pivot_tau is None:
            pivot_tau = float(os.environ.get("HYPERMVAR_PIVOT_TAU", DEFAULT_PIVOT_TAU))
        self.lib = _lib.load()                      # fails loudly when the HIP library is not built
        if not torch.cuda.is_available():
            raise RuntimeError("hypermvar needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.pivot_tau = float(pivot_tau)
        self.max_workspace_bytes = int(max_workspace_bytes)
        self._ws = {}
        self._aux = {}        # second HIP stream for chunk overlap in the fused path
        self._taps = {}       # decimation filters on the device, per (q, design)
        self._resp = {}       # band responses of the analytic signal on the device, per (T, fs, lo, hi, order)

    # ------------------------------------------------------------------ helpers
    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, entry, *args):
        """The C entry `entry` on the engine's device (`_lib.call`: tensors as their pointers, None as null; raises on a status
        other than 0).  The stream is an argument like any other."""
        with torch.cuda.device(self.device):
            _lib.call(self.lib, entry, *args)

    def to_device(self, a, dtype=torch.float64):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device)

    def empty(self, *shape, dtype=torch.float64):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def pad(self, m: int) -> int:
        mp = self.lib.hmv_pad(int(m))
        if mp < 0:
            raise ValueError(f"hypermvar supports 1..64 channels, got {m}")
        return mp

    def _workspace(self, nbytes: int):
        """Cached scratch of the fused call, one buffer per HIP stream: two calls on different streams never share
        (and so never race on) a workspace; calls on one stream are ordered by the stream."""
        key = self.stream()
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            self._ws.pop(key, None)
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    @staticmethod
    def raise_on_info(info: torch.Tensor, what: str, per_item: int = 1):
        """LAPACK-style info array -> the reference's LinAlgError("Singular matrix") (np.linalg.solve / inv).
        The exception additionally carries which items failed (`.items`, `.info`: first bad pivot column, 1-based;
        with `per_item` = F for the per-frequency inverses, `.freqs` too)."""
        bad = torch.nonzero(info != 0).flatten()
        if bad.numel() == 0:
            return
        idx = bad.cpu().numpy()
        err = SingularMatrixError("Singular matrix")
        err.stage = what
        err.items = np.unique(idx // per_item)
        err.freqs = (idx % per_item) if per_item > 1 else None
        err.info = info[bad].cpu().numpy()
        err.args = ("Singular matrix", f"{what}: {len(err.items)} item(s) failed, first: item {int(err.items[0])}"
                    + (f" frequency {int(err.freqs[0])}" if per_item > 1 else "") + f" pivot column {int(err.info[0])}")
        raise err

    def check_items(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int):
        validate_items(x, item_rec, item_start, n, p)

    # ------------------------------------------------------------------ K1
    def lagcov(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int):
        """x: (n_rec, m, T) float64 device tensor -> R (items, p+1, MP, MP)."""
        assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
        x = x if x.stride(2) == 1 else x.contiguous()
        n_rec, m, T = x.shape
        mp = self.pad(m)
        self.check_items(x, item_rec, item_start, n, p)
        n_items = int(item_rec.numel())
        R = self.empty(n_items, p + 1, mp, mp)
        self._call("hmv_lagcov_f64", x, x.stride(0), x.stride(1), item_rec, item_start, n_items, m, int(n), int(p), R,
                   self.stream())
        return R

    def lagcov_regular(self, x: torch.Tensor, first: int, hop: int, n_win: int, n: int, p: int):
        """x: (m, T) ONE recording; windows first + w*hop .. + n (n = k hops) -> R (n_win, p+1, MP, MP) with the hop
        blocks summed once and shared by the overlapping windows (`hmv_lagcov_regular_f64`)."""
        assert x.dim() == 2 and x.dtype == torch.float64 and x.is_cuda
        x = x if x.stride(1) == 1 else x.contiguous()
        m, T = x.shape
        mp = self.pad(m)
        nws = int(self.lib.hmv_lagcov_regular_workspace_doubles(n_win, m, int(n), int(hop), int(p)))
        if nws < 0:
            raise ValueError("the window must be a whole number of hops")
        ws = self.empty(max(nws, 1))
        R = self.empty(n_win, p + 1, mp, mp)
        self._call("hmv_lagcov_regular_f64", x, x.stride(0), T, int(first), int(hop), int(n_win), m, int(n), int(p), R, ws,
                   self.stream())
        return R

    def trial_mean(self, R: torch.Tensor, m: int):
        """(trials, p+1, MP, MP) -> (1, p+1, MP, MP): count_corr's average over trials (mtmvar.py:78-85)."""
        trials, p1, mp, _ = R.shape
        out = self.empty(1, p1, mp, mp)
        self._call("hmv_trial_mean_f64", R, trials, m, p1 - 1, out, self.stream())
        return out

    # ------------------------------------------------------------------ K2
    def yw_solve(self, R: torch.Tensor, m: int, want_logdet: bool = False, flags: int = 0, return_route: bool = False):
        """K2 -> (ar, V, logdet, info[, route]).  route (return_route=True): int32 per item, which solver took it --
        0 the recursion, 1 the LDL^T, 2 the pivoted LU (`FLAG_YW_PIVOTED`, or an engine with `pivoted_yw`)."""
        flags = int(flags) | self.yw_flag
        if want_logdet and (flags & _lib.FLAG_YW_PIVOTED):
            raise ValueError("yw_solve: want_logdet is not available with the pivoted Yule-Walker fallback (pivoted_yw / "
                             "FLAG_YW_PIVOTED): an LU gives no criterion curve")
        n_items, p1, mp, _ = R.shape
        p = p1 - 1
        ws = self.empty(n_items * int(self.lib.hmv_yw_workspace_doubles(m, p)))
        ar = self.empty(n_items, mp, mp, p)
        V = self.empty(n_items, mp, mp)
        info = self.empty(n_items, dtype=torch.int32)
        logdet = self.empty(n_items, p) if want_logdet else None
        self._call("hmv_yw_solve_f64", R, n_items, m, p, ws, ar, V, logdet, info, int(flags), self.stream())
        if return_route:
            return ar, V, logdet, info, self.yw_routes(ws, n_items, m, p)
        return ar, V, logdet, info

    def window_routes(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int,
                      chunk: int = 128):
        """K1 + K2 with the pivoted fallback on, `chunk` windows at a time -> (route int32 per item: 0 recursion, 1 LDL^T,
        2 LU; info int32 per item, not zero where even the LU met an exactly zero pivot column)."""
        n_items = int(item_rec.numel())
        route = self.empty(n_items, dtype=torch.int32)
        info = self.empty(n_items, dtype=torch.int32)
        for i0 in range(0, n_items, int(chunk)):
            sl = slice(i0, min(n_items, i0 + int(chunk)))
            R = self.lagcov(x, item_rec[sl], item_start[sl], n, p)
            _, _, _, info[sl], route[sl] = self.yw_solve(R, x.shape[1], flags=_lib.FLAG_YW_PIVOTED, return_route=True)
        return route, info

    def yw_routes(self, ws: torch.Tensor, n_items: int, m: int, p: int):
        """The route words of a K2 workspace (`hmv_yw_routes_i32`): int32 per item, 0 recursion, 1 LDL^T, 2 LU."""
        route = self.empty(n_items, dtype=torch.int32)
        if n_items:
            self._call("hmv_yw_routes_i32", ws, n_items, int(m), int(p), route, self.stream())
        return route

    def yw_solve_auto(self, R: torch.Tensor, m: int, n: int, crit_type: str = "AIC"):
        """K2 with the order chosen per item (`hmv_yw_solve_auto_f64`): R (items, pmax+1, MP, MP) from K1 at p = pmax, n the
        window length -> (ar (items, MP, MP, pmax) of the selected order, zero beyond it; V; orders int32, 0 for a failed
        item; crit (items, pmax), the criterion curve of `mvar_criterion` (mtmvar.py:551-601); info)."""
        no_pivoted_auto_order(self.pivoted_yw, "yw_solve_auto")
        n_items, p1, mp, _ = R.shape
        pmax, crit = auto_order_args(p1 - 1, crit_type, n)
        ws = self.empty(max(1, n_items * int(self.lib.hmv_yw_workspace_doubles(m, pmax))))
        ar = self.empty(n_items, mp, mp, pmax)
        V = self.empty(n_items, mp, mp)
        orders = self.empty(n_items, dtype=torch.int32)
        curve = self.empty(n_items, pmax)
        info = self.empty(n_items, dtype=torch.int32)
        try:
            self._call("hmv_yw_solve_auto_f64", R, n_items, m, pmax, int(n), crit, ws, ar, V, orders, curve, None, info, 0,
                       self.stream())
        except (ValueError, RuntimeError):
            if n_items:         # the status of an empty batch is not looked at: its tensors have null pointers, which the
                raise           # entry refuses, and there is nothing it could have solved
        return ar, V, orders, curve, info

    # ------------------------------------------------------------------ K3 (+K4/K5 layout kernels)
    def twiddles(self, freqs, fs: float, p: int):
        f = self.to_device(np.asarray(freqs, dtype=np.float64))
        tw = self.empty(f.numel(), p, 2)
        self._call("hmv_twiddles_f64", f, f.numel(), float(fs), p, tw, self.stream())
        return tw

    def transfer(self, ar: torch.Tensor, m: int, tw: torch.Tensor, want_P=True, want_H=False, want_A=False):
        """ar (items, MP, MP, p) -> dict of kernel-natural (items, F, MP, MP) tensors + info."""
        n_items, mp, _, p = ar.shape
        F = tw.shape[0]
        out = {}
        P = self.empty(n_items, F, mp, mp) if want_P else None
        rowsum = self.empty(n_items, F, mp) if want_P else None
        H = self.empty(n_items, F, mp, mp, 2) if want_H else None
        A = self.empty(n_items, F, mp, mp, 2) if want_A else None
        info = self.empty(n_items * F, dtype=torch.int32)
        ws = self.empty(max(1, int(self.lib.hmv_tf_workspace_doubles(n_items, m, p))))
        self._call("hmv_tf_f64", ar, n_items, m, p, tw, F, P, rowsum, H, A, info, self.pivot_tau, ws, self.stream())
        out.update(P=P, rowsum=rowsum, H=H, A=A, info=info)
        return out

    def normalise(self, P, rowsum, m: int, normalise: bool = True):
        n_items, F, mp, _ = P.shape
        den = self.empty(n_items, mp)
        out = self.empty(n_items, m, m, F)
        self._call("hmv_ffdtf_norm_f64", P, rowsum, den, out, n_items, F, m, 1 if normalise else 0, self.stream())
        return out, den

    def to_mmf_complex(self, Z: torch.Tensor, m: int):
        """(items, F, MP, MP, 2) -> complex128 (items, m, m, F), the reference's H / A / spectra layout."""
        n_items, F, mp, _, _ = Z.shape
        out = self.empty(n_items, m, m, F, 2)
        self._call("hmv_transpose_c128", Z, out, n_items, F, m, self.stream())
        return torch.view_as_complex(out)

    def spectra(self, H: torch.Tensor, V: torch.Tensor, m: int):
        n_items, F, mp, _, _ = H.shape
        S = self.empty(n_items, F, mp, mp, 2)
        self._call("hmv_spectra_f64", H, V, S, n_items, m, F, self.stream())
        return S

    # ------------------------------------------------------------------ measures on top of K3 / K5
    def pack_complex(self, Z: torch.Tensor):
        """complex128 (items, m, m, F) -> kernel layout (items, F, MP, MP, 2), identity on the padding."""
        n_items, m, _, F = Z.shape
        mp = self.pad(m)
        zin = torch.view_as_real(Z.contiguous())
        out = self.empty(n_items, F, mp, mp, 2)
        self._call("hmv_pack_c128", zin, out, n_items, F, m, self.stream())
        return out

    def complex_inverse(self, Z: torch.Tensor, m: int):
        """Z (items, F, MP, MP, 2) -> (inverse, det/|det| (items*F, 2), info)."""
        n_items, F, mp, _, _ = Z.shape
        Zi = self.empty(n_items, F, mp, mp, 2)
        detph = self.empty(n_items * F, 2)
        info = self.empty(n_items * F, dtype=torch.int32)
        self._call("hmv_cinv_c128", Z, n_items, m, F, Zi, detph, info, 1.0, self.stream())
        return Zi, detph, info

    def partial_coherence(self, S: torch.Tensor, m: int):
        """S spectral matrices (items, F, MP, MP, 2) in kernel layout -> kappa complex128 (items, m, m, F)."""
        n_items, F, mp, _, _ = S.shape
        Si, detph, info = self.complex_inverse(S, m)
        kap = self.empty(n_items, F, mp, mp, 2)
        self._call("hmv_partial_coherence_c128", Si, detph, kap, n_items, m, F, self.stream())
        return self.to_mmf_complex(kap, m), info

    def ddtf(self, ff: torch.Tensor, kappa: torch.Tensor):
        """ffDTF (items, m, m, F) real x |partial coherence| (items, m, m, F) complex128 -> dDTF (mtmvar.py:341-385)."""
        n_items, m, _, F = ff.shape
        ff = ff.contiguous()
        kr = torch.view_as_real(kappa.contiguous())
        out = self.empty(n_items, m, m, F)
        self._call("hmv_ddtf_f64", ff, kr, out, n_items, m, F, self.stream())
        return out

    def band_tables(self, bin_lo, bin_hi, F: int):
        """Device copies (int32) of the bin ranges [bin_lo[b], bin_hi[b]) of a band set on an F-point grid, cached."""
        lo_h, hi_h = np.asarray(bin_lo, dtype=np.int32), np.asarray(bin_hi, dtype=np.int32)
        if (lo_h < 0).any() or (hi_h > F).any() or (hi_h < lo_h).any() or lo_h.shape != hi_h.shape or lo_h.ndim != 1:
            raise ValueError("band bin ranges must satisfy 0 <= lo <= hi <= F")
        # the bin tables live on the device per distinct band set: a fresh pageable-memory copy per call is a synchronous
        # copy on the compute stream, i.e. a host wait for everything queued before it (the streamed path's stall)
        key = (lo_h.tobytes(), hi_h.tobytes())
        cache = self.__dict__.setdefault("_band_tables", {})
        if key not in cache:
            if len(cache) >= 16:
                cache.pop(next(iter(cache)))
            cache[key] = (torch.as_tensor(lo_h).to(self.device), torch.as_tensor(hi_h).to(self.device))
        return cache[key]

    def bands_in_kernel(self, m: int, F: int) -> bool:
        """Can K3's row workers add up the bands themselves (`sliding_ffdtf(bands=...)` without the full array)?"""
        cap = {16: 640, 32: 1280, 48: 1984, 64: 2688}[self.pad(m)]     # doubles of LDS the row worker has, whole 32s
        return F % 32 == 0 and F <= cap

    def band_sums(self, ff: torch.Tensor, bin_lo, bin_hi):
        """(..., F) -> (..., n_bands): sums over the bin ranges [bin_lo[b], bin_hi[b])."""
        F = ff.shape[-1]
        ff = ff.contiguous()
        lo, hi = self.band_tables(bin_lo, bin_hi, F)
        nb = int(lo.numel())
        rows = ff.numel() // F if F else 0
        out = self.empty(*ff.shape[:-1], nb)
        self._call("hmv_band_sums_f64", ff, rows, F, lo, hi, nb, out, self.stream())
        return out

    def gpdc(self, A: torch.Tensor, V: torch.Tensor, m: int):
        """A (items, F, MP, MP, 2) from `transfer(want_A=True)`, V (items, MP, MP) -> GPDC (items, m, m, F)."""
        n_items, F, mp, _, _ = A.shape
        G = self.empty(n_items, F, mp, mp)
        self._call("hmv_gpdc_f64", A, V, G, n_items, m, F, self.stream())
        out, _ = self.normalise(G, None, m, normalise=False)
        return out

    # ------------------------------------------------------------------ fused sliding-window path
    @staticmethod
    def _chunk(n_items: int, per_item: int, cap_bytes: int) -> int:
        """Items per chunk of a fused call: all of them, unless their workspace would exceed cap_bytes."""
        return max(1, min(n_items, max(1, cap_bytes // max(per_item, 1))))

    def sliding_chunk(self, n_items: int, m: int, p: int, F: int, lanes: int = 1) -> int:
        per_item = int(self.lib.hmv_sliding_workspace_bytes(1, m, p, F))
        return self._chunk(n_items, per_item * lanes, self.max_workspace_bytes)

    def copy_streams(self):
        """The upload and the download stream of `stream_dyads`, created ONCE per engine.  HIP streams share a handful of
        hardware queues (four by default) and two streams on one queue run one after the other: with fresh streams per
        call the download of recording d and the upload of recording d + 1 ended up on the compute stream's queue and
        the whole pipeline ran serially (device timeline, `tools/dbg/e2e_depth.py`: compute -> download -> upload ->
        compute, 12.2 ms per dyad instead of 10.4).  High priority: their own queues, apart from the compute streams'."""
        if "_copy" not in self.__dict__:
            self._copy = (torch.cuda.Stream(self.device, priority=-1), torch.cuda.Stream(self.device, priority=-1))
        return self._copy

    def aux_stream(self):
        """Second stream of the fused call (the tiled form of K2 runs as two half-batches), one per calling stream."""
        key = self.stream()
        if key not in self._aux:
            self._aux[key] = torch.cuda.Stream(device=self.device)
        return self._aux[key]

    # The routes: what is particular to one fused C entry, written down once each.  `_sliding_call` is all they share.
    # `_route` and `_ensemble_route` follow; `_mix_route`, `_pairs_route`, `_block_route` and `_block_pairs_route` stand in
    # front of the entries they serve.  A route's `call` reads the driver's buffers by name (`a.out`, `a.info_yw`, ...);
    # an output or info array the route does not list in `more` / `infos` reads as a null pointer (`_ABSENT`).
    def _window_grid(self, x, items, n_items, grid, compare):
        """grid = (hop, first, n_win) of the single-trial routes -> the three grid arguments of the C call."""
        if grid is None:
            return 0, 0, 0
        g_hop, g_first, g_nwin = (int(v) for v in grid)
        # With a declared grid K1 addresses the windows by (item // n_win, first + (item % n_win) * hop) and never
        # reads item_rec / item_start: they must say the same thing, or the results belong to other windows (and a
        # recording index past n_rec would be read out of bounds).  One device comparison per call.
        if g_nwin < 1 or n_items % g_nwin or g_hop < 1 or n_items // g_nwin > x.shape[0]:
            raise ValueError("grid = (hop, first, n_win) does not match the number of items / recordings")
        if compare:
            k = torch.arange(n_items, dtype=torch.int64, device=self.device)
            if not (torch.equal(items[0], k // g_nwin) and torch.equal(items[1], g_first + (k % g_nwin) * g_hop)):
                raise ValueError("grid = (hop, first, n_win) contradicts item_rec / item_start "
                                 "(items must be recording-major, window-minor on the declared grid)")
        return g_hop, g_first, g_nwin

    def _ensemble_grid(self, n_groups, items, n_items, grid, compare):
        """grid = (hop, n_win) of the ensemble routes -> the two grid arguments of the C call."""
        g_hop, g_nwin = (int(v) for v in grid) if grid is not None else (0, 0)
        if grid is not None and n_items:
            # with a declared grid the shared form addresses by (item // n_win, (item % n_win) * hop) and never reads
            # item_group / item_offset: they must say the same thing
            if g_hop < 1 or g_nwin < 1 or n_items != n_groups * g_nwin:
                raise ValueError("grid = (hop, n_win) does not match the number of items / groups")
            k = torch.arange(n_items, dtype=torch.int64, device=self.device)
            if compare and not (torch.equal(items[0], k // g_nwin) and torch.equal(items[1], (k % g_nwin) * g_hop)):
                raise ValueError("grid = (hop, n_win) contradicts item_group / item_offset "
                                 "(items must be group-major, window-minor on the declared grid)")
        return g_hop, g_nwin

    def _route(self, measure, n, p, max_model_order=20, crit_type="AIC", spectra=False):
        """Route of a single-trial call: `hmv_sliding_<measure>_f64` at the fixed order p, or with p=None
        `hmv_sliding_auto_f64` -- K1 sums max_model_order + 1 lags, K2 walks every order, keeps the criterion's first
        arg-min per window and leaves that order's coefficients zero-padded to max_model_order lags; the later stages run
        at max_model_order on them."""
        lib, n, code = self.lib, int(n), _MEASURES[measure]
        common = dict(measure=measure, more=(_SPECTRA,) if spectra else (), grid=self._window_grid)

        def windows(a, order):
            return (*a.x, *a.items, a.n_items, a.m, n, *order, a.f, a.F, a.fs)

        def tail(a):
            return (*a.grid, a.T, a.stream, a.aux)
        if p is None:
            pmax, crit = auto_order_args(max_model_order, crit_type, n)
            return _Route(
                name=f"sliding_{measure}", p=pmax, order_text=f"max_model_order={pmax}", automatic=True,
                infos=_measure_infos(measure, "ar_coeff (Yule-Walker solve at the automatic order; a negative info: residual "
                                              "covariance not positive definite)"),
                validate=lambda x, items: self.check_items(x, items[0], items[1], n, pmax),
                ws_bytes=lambda chunk, m, F, nb, g: lib.hmv_sliding_auto_workspace_bytes(code, chunk, m, pmax, F,
                                                                                           -1 if spectra else nb),
                call=lambda a: ("hmv_sliding_auto_f64", (
                    code, *windows(a, (pmax, crit)), a.out, a.lo, a.hi, a.nb, a.S, a.ar, a.V, a.orders, a.curve, a.info_yw,
                    a.info_tf, a.ws, a.nbytes, a.chunk, a.tau, a.flags, *tail(a))),
                **common)
        p = int(p)
        fixed = dict(name=f"sliding_{measure}", p=p, order_text=f"p={p}",
                     validate=lambda x, items: self.check_items(x, items[0], items[1], n, p), **common)
        if measure != "ffdtf":
            wsf = lib.hmv_sliding_ddtf_workspace_bytes if measure == "ddtf" else lib.hmv_sliding_gpdc_workspace_bytes

            def call(a):
                front = (*windows(a, (p,)), a.out, a.lo, a.hi, a.nb, a.ar, a.V, a.info_yw)
                if measure == "gpdc":           # no inverse of A(f): neither info_tf nor the pivot threshold
                    return "hmv_sliding_gpdc_f64", (*front, a.ws, a.nbytes, a.chunk, a.flags, *tail(a))
                return "hmv_sliding_ddtf_f64", (*front, a.info_tf, a.ws, a.nbytes, a.chunk, a.tau, a.flags, *tail(a))
            return _Route(infos=_measure_infos(measure, _YW_TEXT), ws_bytes=lambda chunk, m, F, nb, g: wsf(chunk, m, p, F, nb),
                          call=call, **fixed)

        def ws_bytes(chunk, m, F, nb, g):
            if spectra:
                return lib.hmv_sliding_spectra_workspace_bytes(chunk, m, p, F)
            return (lib.hmv_sliding_bands_workspace_bytes if nb else lib.hmv_sliding_workspace_bytes)(chunk, m, p, F)

        def call(a):
            work = (a.info_yw, a.info_tf, a.ws, a.nbytes, a.chunk, a.tau, a.flags, *a.grid, a.T)
            if spectra:
                return "hmv_sliding_ffdtf_spectra_f64", (*windows(a, (p,)), a.out, a.S, a.ar, a.V, *work, a.stream, a.aux)
            if a.nb:
                return "hmv_sliding_ffdtf_bands_f64", (*windows(a, (p,)), a.out, a.lo, a.hi, a.nb, a.ar, a.V, *work, *a.k3,
                                                       a.stream, a.aux)
            return "hmv_sliding_ffdtf_f64", (*windows(a, (p,)), a.out, a.ar, a.V, *work, *a.k3, a.stream, a.aux)
        # (the chunk of the full and the band form is sized by the full form's workspace: `sliding_chunk`'s rule)
        return _Route(infos=_measure_infos(measure, "ar_coeff (Yule-Walker solve)"), ws_bytes=ws_bytes, call=call,
                      per_item=None if spectra else lambda m, F, nb: lib.hmv_sliding_workspace_bytes(1, m, p, F), **fixed)

    def _ensemble_route(self, measure, n, p, trial_rec, trial_start, group_ptr, spectra=False, shuffle=None):
        """Route of `sliding_ensemble` (`hmv_sliding_ensemble_f64`): the items are (group, offset) pairs, the validation
        is `validate_trials`, the grid has two parts, and a failed fit is reported with its group and offset.
        shuffle = (trial_rec_b, trial_start_b, split, R_base, item_base): `hmv_sliding_ensemble_split_f64` instead -- K1
        reads the channels >= split through the second trial table (no grid: the direct form only)."""
        if p is None:
            raise ValueError(_NO_ENSEMBLE_ORDER)
        lib, n, p, code = self.lib, int(n), int(p), _MEASURES[measure]
        n_groups = int(group_ptr.numel()) - 1

        def blame(err, items):       # say which group and which window of the epoch
            idx = torch.as_tensor(err.items, dtype=torch.int64, device=items[0].device)
            err.groups = items[0][idx].cpu().numpy()
            err.offsets = items[1][idx].cpu().numpy()
            err.args = (err.args[0], err.args[1] + f" (group {int(err.groups[0])}, window at offset {int(err.offsets[0])})")

        def call(a):
            front = (code, *a.x, a.T, trial_rec, trial_start, group_ptr, n_groups, *a.items,
                     a.n_items, a.m, n, p, a.f, a.F, a.fs, a.out, a.lo, a.hi, a.nb, a.S, a.ar, a.V, a.info_yw, a.info_tf, a.ws,
                     a.nbytes, a.chunk, a.tau, a.flags)
            if shuffle is None:
                return "hmv_sliding_ensemble_f64", (*front, *a.grid, a.stream, a.aux)
            rec_b, start_b, split, R_base, item_base = shuffle
            return "hmv_sliding_ensemble_split_f64", (*front, rec_b, start_b, int(split), R_base, item_base, a.stream, a.aux)
        return _Route(
            name="sliding_ensemble", measure=measure, p=p, order_text=f"n={n}, p={p}", more=(_SPECTRA,) if spectra else (),
            blame=blame, infos=_measure_infos(measure, "ar_coeff (Yule-Walker solve of the trial-averaged covariances; a negative "
                                                       "info: residual covariance not positive definite)"),
            validate=lambda x, items: validate_trials(x, trial_rec, trial_start, group_ptr, items[0], items[1], n, p),
            grid=lambda x, items, n_items, grid, compare: self._ensemble_grid(n_groups, items, n_items, grid, compare),
            ws_bytes=lambda chunk, m, F, nb, g: lib.hmv_sliding_ensemble_workspace_bytes(
                code, chunk, m, n, p, F, -1 if spectra else nb, *g),
            call=call)

    def _sliding_call(self, rt, x, items, freqs, fs, *, bands=None, out=None, out_more=None, return_ar=False,
                      return_orders=False, check=True, chunk=None, overlap=False, flags=0, grid=None, validate=True,
                      k3_events=None):
        """The one driver of the fused entries; `rt` (a `_Route`) carries what differs between them.  Top to bottom: the
        inputs, the empty batch, the grid, `out`, chunk and workspace, what else the C call writes (`buffers`), the call, the
        band sums of the two-step form, `check`, the result `(out, *more[, bad][, ar, V, infos][, orders, crit])`.
        freqs=None: there is no frequency grid (F = 0) and no `out`; out_more: {name: buffer} for outputs behind `out`
        that the caller brings along."""
        flags = int(flags) | self.yw_flag
        if rt.automatic:
            no_pivoted_auto_order(bool(flags & _lib.FLAG_YW_PIVOTED), rt.name)
        if rt.m is None:
            assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
            x = x if x.stride(2) == 1 else x.contiguous()
            n_rec, m, T = x.shape
        else:                                 # the mix route: x is the per-trial stack, there are no samples
            m, T = rt.m, 0
        mp = self.pad(m)
        if validate:
            rt.validate(x, items)
        n_items = int(items[0].numel())
        f, F, nb = None, 0, 0
        if freqs is not None:
            f = freqs if isinstance(freqs, torch.Tensor) else self.to_device(np.asarray(freqs, dtype=np.float64))
            F = int(f.numel())
        if bands is not None:
            b_lo, b_hi = self.band_tables(bands[0], bands[1], F)
            nb = int(b_lo.numel())
        row = (m, m) if rt.row is None else rt.row
        return_orders = return_orders and rt.automatic
        per_item = [0 if i is None else F if i.per_item is None else i.per_item for i in rt.infos]

        def buffers():                        # what the C call writes besides `out`, in the order it is allocated
            given = out_more or {}
            more = [None if mo is None else given[mo.name] if given.get(mo.name) is not None
                    else self.empty(*mo.shape(n_items, m, F)) for mo in rt.more]
            ar = self.empty(n_items, mp, mp, rt.p) if return_ar else None
            V = self.empty(n_items, mp, mp) if return_ar else None
            orders = self.empty(n_items, dtype=torch.int32) if rt.automatic else None
            curve = self.empty(n_items, rt.p) if return_orders else None
            new_info = torch.zeros if rt.zero_infos else torch.empty
            infos = [None if i is None else new_info(n_items * k, dtype=torch.int32, device=self.device)
                     for i, k in zip(rt.infos, per_item)]
            return more, ar, V, orders, curve, infos

        def result(out, bad):
            info = {i.name: buf.view(n_items, k) if i.rows else buf
                    for i, k, buf in zip(rt.infos, per_item, infos) if i is not None}
            r = (out, *(None if mo is None else mo.give(buf, info) for mo, buf in zip(rt.more, more)))
            if check == "mask":
                r += (bad,)
            if return_ar:
                r += (ar, V, tuple(None if i is None else info[i.name] for i in rt.infos) if len(infos) > 1 else infos[0])
            if return_orders:
                r += (orders, curve)
            return r if len(r) > 1 else r[0]
        if n_items == 0:                      # empty batch (torch gives empty tensors a null data pointer)
            more, ar, V, orders, curve, infos = buffers()
            return result(None if freqs is None else self.empty(0, *row, nb if bands is not None else F),
                          torch.zeros(0, dtype=torch.bool, device=self.device))
        g = rt.grid(x, items, n_items, grid, validate)
        # Two steps -- the full array (scratch), then its band sums -- where the kernels cannot add the bands up themselves:
        # an empty band set, and for the ffDTF a frequency grid that does not suit K3's row workers or the unfused norm
        two_step = bands is not None and (nb == 0 or (rt.bands_in_k3 and (
            not self.bands_in_kernel(m, F) or (flags & _lib.FLAG_UNFUSED_NORM))))
        knb = 0 if two_step else nb           # the bands the C call sums itself
        res = None
        if freqs is not None:
            res = self.empty(n_items, *row, knb or F) if out is None or two_step else out
            assert res.is_contiguous() and tuple(res.shape) == (n_items, *row, knb or F)
        if chunk is None:
            size = rt.ws_bytes(1, m, F, knb, (0,) * len(g)) if rt.per_item is None else rt.per_item(m, F, knb)
            chunk = self._chunk(n_items, int(size), self.max_workspace_bytes)
        chunk = int(chunk)
        nbytes = int(rt.ws_bytes(chunk, m, F, knb, g))
        if nbytes < 0:
            raise ValueError(f"{rt.name}: bad sizes (m={m}, {rt.order_text}, F={F}, chunk={chunk})")
        ws = self._workspace(nbytes)
        more, ar, V, orders, curve, infos = buffers()
        ptrs = dict(_ABSENT)
        ptrs.update((mo.name, buf) for mo, buf in zip(rt.more, more) if mo is not None)
        ptrs.update(("info_" + i.name, buf) for i, buf in zip(rt.infos, infos) if i is not None)
        a = types.SimpleNamespace(
            **ptrs, x=(x, x.stride(0), x.stride(1)), T=T, items=tuple(items), n_items=n_items, m=m, f=f, F=F, fs=float(fs),
            out=res, nb=knb, lo=b_lo if knb else None, hi=b_hi if knb else None, ar=ar, V=V, orders=orders, curve=curve, ws=ws,
            nbytes=nbytes, chunk=chunk, tau=self.pivot_tau, flags=int(flags), grid=g,
            k3=tuple(k3_events) if k3_events else (0, 0), stream=self.stream(), aux=self.aux_stream().cuda_stream if overlap else 0)
        entry, args = rt.call(a)
        self._call(entry, *args)
        if two_step:
            res = self.band_sums(res, bands[0], bands[1])
            if out is not None:
                out.copy_(res)
                res = out
        bad = None
        if check == "nan" or check == "mask":   # "mask": no host synchronisation, the caller decides what to NaN-fill
            for k, buf in zip(per_item, infos):
                if buf is not None:
                    b = buf != 0 if k == 1 else (buf.view(n_items, k) != 0).any(dim=1)
                    bad = b if bad is None else bad | b
        if check == "nan":          # keep the good windows, NaN-fill the ones whose fit or inverse was singular
            if bool(bad.any()):
                for buf in (res, *(buf for mo, buf in zip(rt.more, more) if mo is not None and mo.nan)):
                    if buf is not None:
                        buf[bad] = float("nan")
        elif check and check != "mask":
            try:
                for i, k, buf in zip(rt.infos, per_item, infos):
                    if buf is not None:
                        self.raise_on_info(buf, i.text, per_item=k)
            except SingularMatrixError as err:
                if rt.blame is not None:
                    rt.blame(err, items)
                raise
        return result(res, bad)

    def sliding_ffdtf(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int,
                      freqs, fs: float, out: torch.Tensor | None = None, return_ar: bool = False,
                      check: bool = True, chunk: int | None = None, k3_events=None, overlap: bool = True,
                      flags: int = 0, grid=None, validate: bool = True, bands=None, max_model_order: int = 20,
                      crit_type: str = "AIC", return_orders: bool = False):
        """ffDTF of every window: x (n_rec, m, T) -> (items, m, m, F).  One C-ABI call (K1->K2->K3->K4).

        p=None: the reference's default, `optimal_model_order=None` -- every window gets the order that
        `mvar_criterion(window, max_model_order, crit_type)` (mtmvar.py:551-601) picks for it, selected on the device in
        the same single call (`hmv_sliding_auto_f64`).  `return_orders=True` then appends `orders` (items,) int32, 0 for
        a failed window, and `crit` (items, max_model_order) to whatever the call returns; `return_ar` gives the
        coefficients zero-padded to max_model_order lags.  With an integer p these three keywords are not looked at.

        check: True raises numpy.linalg.LinAlgError("Singular matrix") if ANY window failed, like the reference's
        np.linalg.solve / inv (the exception names the windows); "nan" returns every window and NaN-fills the
        failed ones; False skips the check (and its synchronisation); "mask" returns (out, bad) with `bad` the boolean
        device mask of the failed windows and no synchronisation (the caller NaN-fills what it keeps).
        validate=False skips the bounds check of the window descriptors and of a declared grid (two host
        synchronisations): for callers that validated the same descriptors before (`stream_dyads`).
        overlap: give the library a second stream: the Yule-Walker stage (K2), whose launches cannot fill the
        chip, then runs as two half-batches that interleave on the device (see include/hypermvar.h).
        flags: option bits of include/hypermvar.h (`_lib.FLAG_*`); 0 = the fast defaults.
        grid: (hop, first, n_win) when the items are a REGULAR grid -- item = rec * n_win + w is the window starting
        at first + w * hop of recording rec (`sliding.regular_grid` derives it from the start positions): K1 then sums
        every hop block once and shares it between the overlapping windows (half its flops at 50 % overlap; equal to
        the direct form to rounding, not bitwise -- `_lib.FLAG_DIRECT_LAGCOV` keeps the direct form).
        k3_events: optional pair of raw hipEvent_t handles (`torch.cuda.Event.cuda_event` of events that
        have been recorded once) which the library records around the dominant kernel.
        bands: (bin_lo, bin_hi) -- the REDUCED product: instead of the (items, m, m, F) array the call returns its band
        sums (items, m, m, n_bands), band b = sum over the bins bin_lo[b] <= f < bin_hi[b] (`distributed.band_bins`).
        The row workers inside K3 add them up and the full array is never written (`hmv_sliding_ffdtf_bands_f64`); the
        same bits as `band_sums(sliding_ffdtf(...))`, which is also what runs when the grid does not suit the kernel
        (`bands_in_kernel`).  `out`, if given, is the band array.
        """
        rt = self._route("ffdtf", n, p, max_model_order, crit_type)
        return self._sliding_call(rt, x, (item_rec, item_start), freqs, fs, bands=bands, out=out, return_ar=return_ar,
                                  return_orders=return_orders, check=check, chunk=chunk, overlap=overlap, flags=flags,
                                  grid=grid, validate=validate, k3_events=k3_events)

    def sliding_ddtf(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int, freqs,
                     fs: float, out: torch.Tensor | None = None, return_ar: bool = False, check=True,
                     chunk: int | None = None, overlap: bool = True, flags: int = 0, grid=None, validate: bool = True,
                     bands=None, max_model_order: int = 20, crit_type: str = "AIC", return_orders: bool = False):
        """dDTF of every window (`direct_dtf`, mtmvar.py:341-385): x (n_rec, m, T) -> (items, m, m, F), or its band sums
        (items, m, m, n_bands) with `bands=(bin_lo, bin_hi)`.  One C-ABI call (`hmv_sliding_ddtf_f64`): K1 -> K2 -> K3's
        fused ffDTF -> |kappa| from W(f) = A^T V^-1 A (sliding_conn.hip).  The keywords mean what they mean for
        `sliding_ffdtf`; a window also fails where its residual covariance is not positive definite (info_yw < 0).
        Equal to the reference's minors-based dDTF to rounding, not bitwise (no minors, no second inversion).
        p=None / max_model_order / crit_type / return_orders: the automatic order, as in `sliding_ffdtf`."""
        rt = self._route("ddtf", n, p, max_model_order, crit_type)
        return self._sliding_call(rt, x, (item_rec, item_start), freqs, fs, bands=bands, out=out, return_ar=return_ar,
                                  return_orders=return_orders, check=check, chunk=chunk, overlap=overlap, flags=flags,
                                  grid=grid, validate=validate)

    def sliding_gpdc(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int, freqs,
                     fs: float, out: torch.Tensor | None = None, return_ar: bool = False, check=True,
                     chunk: int | None = None, overlap: bool = True, flags: int = 0, grid=None, validate: bool = True,
                     bands=None, max_model_order: int = 20, crit_type: str = "AIC", return_orders: bool = False):
        """GPDC of every window (`gen_partial_directed_coherence`, mtmvar.py:388-468): x (n_rec, m, T) -> (items, m, m, F),
        or its band sums with `bands=(bin_lo, bin_hi)`.  One C-ABI call (`hmv_sliding_gpdc_f64`): K1 -> K2 -> one kernel
        that builds A(f) on chip; no K3.  The keywords mean what they mean for `sliding_ffdtf`.  Only the Yule-Walker
        failure is reported: A(f) is never inverted, so an exactly singular A(f), on which the reference's
        mvar_transfer_function raises, goes through (`return_ar` gives (out, ar, V, info_yw)).
        p=None / max_model_order / crit_type / return_orders: the automatic order, as in `sliding_ffdtf`."""
        rt = self._route("gpdc", n, p, max_model_order, crit_type)
        return self._sliding_call(rt, x, (item_rec, item_start), freqs, fs, bands=bands, out=out, return_ar=return_ar,
                                  return_orders=return_orders, check=check, chunk=chunk, overlap=overlap, flags=flags,
                                  grid=grid, validate=validate)

    # ------------------------------------------------------------------ block Granger causality (block_gc.hip)
    def block_granger(self, ar: torch.Tensor, V: torch.Tensor, m: int, split: int, freqs, fs: float, check=True):
        """Geweke's spectral block Granger causality of fitted models: ar (items, MP, MP, p), V (items, MP, MP) in K2's
        layouts -> (items, 2, F); index 0 is A -> B (channels < split drive the others), 1 is B -> A.  The stage of
        `sliding_block_granger` on its own (`hmv_block_gc_f64`), the same kernels and the same bits.  The spectrum behind
        it is S(f) = H V H^H with the CONJUGATE transpose, not the plain transpose of `spectra` / `multivariate_spectra`.
        check: True raises SingularMatrixError where V is not positive definite or a per-frequency pivot fails; False
        returns (out, info_v, info_gc)."""
        split = check_block_split(split, m, "block_granger")
        n_items, mp, _, p = ar.shape
        assert mp == self.pad(m) and tuple(V.shape) == (n_items, mp, mp) and ar.is_contiguous() and V.is_contiguous()
        f = freqs if isinstance(freqs, torch.Tensor) else self.to_device(np.asarray(freqs, dtype=np.float64))
        F = int(f.numel())
        out = self.empty(n_items, 2, F)
        info_v = torch.zeros(n_items, dtype=torch.int32, device=self.device)
        info_gc = torch.zeros(n_items * F, dtype=torch.int32, device=self.device)
        if n_items:
            nbytes = int(self.lib.hmv_block_gc_workspace_bytes(n_items, m, p, split, F))
            if nbytes < 0:
                raise ValueError(f"block_granger: bad sizes (m={m}, p={p}, split={split}, F={F})")
            ws = self._workspace(nbytes)
            self._call("hmv_block_gc_f64", ar, V, n_items, m, p, split, f, F, float(fs), out, info_v, info_gc, ws, nbytes,
                       self.stream())
        if not check:
            return out, info_v, info_gc
        self.raise_on_info(info_v, "block_granger (residual covariance not positive definite)")
        self.raise_on_info(info_gc, "block_granger (per-frequency factorisation)", per_item=F)
        return out

    def _block_route(self, n, p, split):
        """Route of `sliding_block_granger` (`hmv_sliding_block_gc_f64`): an output row is the two directions, `time` comes
        out behind it, the restricted fits and the per-frequency factorisation report infos of their own; the grid is that of
        the single-trial routes; neither a second stream nor K3 (and its events) is involved."""
        lib, n = self.lib, int(n)

        def call(a):
            return "hmv_sliding_block_gc_f64", (
                *a.x, *a.items, a.n_items, a.m, n, p, split, a.f, a.F, a.fs, a.out, a.lo, a.hi, a.nb, a.time, a.ar, a.V, a.info_yw,
                a.info_red, a.info_gc, a.ws, a.nbytes, a.chunk, a.flags, *a.grid, a.T, a.stream)
        return _Route(
            name="sliding_block_granger", measure="block_gc", p=p, order_text=f"p={p}, split={split}", row=(2,),
            more=(_BLOCK_TIME,), infos=(_Info("yw", _YW_TEXT), _BLOCK_INFO_RED, _BLOCK_INFO_GC), zero_infos=True,
            validate=lambda x, items: self.check_items(x, items[0], items[1], n, p), grid=self._window_grid,
            ws_bytes=lambda chunk, m, F, nb, g: lib.hmv_block_gc_sliding_workspace_bytes(chunk, m, p, split, F, nb), call=call)

    def sliding_block_granger(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int, freqs,
                              fs: float, *, split: int, bands=None, out=None, return_ar: bool = False, check=True,
                              chunk: int | None = None, flags: int = 0, grid=None, validate: bool = True):
        """Block (multivariate) Granger causality between the channels < split (block A) and the channels >= split
        (block B) of every window: x (n_rec, m, T) -> (spectral, time).  One C-ABI call (`hmv_sliding_block_gc_f64`): K1 and
        K2 once per window, the two restricted fits from the same lag covariances, then the kernels of block_gc.hip.
            spectral (items, 2, F)   Geweke's spectral decomposition, index 0 = A -> B, 1 = B -> A; with
                                     `bands=(bin_lo, bin_hi)` its band sums (items, 2, n_bands), the bits of `band_sums` of
                                     the full output.  Defined on S(f) = H V H^H (conjugate transpose -- not the plain
                                     transpose of `sliding_ffdtf_spectra`).
            time (items, 4)          (F_{A->B}, F_{B->A}, F_{A.B} instantaneous, F_{A,B} total): log-determinant ratios of
                                     the residual covariances of the full fit and of the order-p Yule-Walker fits of each
                                     block alone -- the classical Geweke estimator, which differs from the state-space /
                                     spectral-factorisation estimators.
        `out`, if given, receives `spectral`.  check / chunk / flags / grid / validate mean what they mean for
        `sliding_ffdtf`: check=True raises SingularMatrixError naming the failed windows, "nan" NaN-fills them, "mask"
        appends the boolean device mask, False skips the check.  return_ar appends (ar, V, (info_yw, info_red, info_gc)).
        An integer p is required: the automatic order (p=None) is not available for this call."""
        p = no_block_auto_order(p, "sliding_block_granger")
        rt = self._block_route(n, p, check_block_split(split, x.shape[1], "sliding_block_granger"))
        return self._sliding_call(rt, x, (item_rec, item_start), freqs, fs, bands=bands, out=out, return_ar=return_ar,
                                  check=check, chunk=chunk, flags=flags, grid=grid, validate=validate)

    # ------------------------------------------------------------------ event-locked ensembles (lagcov_ensemble.hip)
    def lagcov_ensemble(self, x: torch.Tensor, trial_rec: torch.Tensor, trial_start: torch.Tensor, group_ptr: torch.Tensor,
                        item_group: torch.Tensor, item_offset: torch.Tensor, n: int, p: int, grid=None, flags: int = 0,
                        validate: bool = True):
        """K1 of an event-locked ensemble: x (n_rec, m, T) -> R (items, p+1, MP, MP), the lag covariances of the window
        item_offset[it] samples after every trial start of group item_group[it], averaged over the group's trials
        (`count_corr` on 3-D input, mtmvar.py:54-85).  Index tensors as in `validate_trials`.  grid = (hop, n_win) declares
        item = g * n_win + w at offset w * hop and lets the library share the overlap between windows
        (`hmv_lagcov_ensemble_f64`; `_lib.FLAG_DIRECT_LAGCOV` keeps the direct form)."""
        if p is None:
            raise ValueError(_NO_ENSEMBLE_ORDER)
        assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
        x = x if x.stride(2) == 1 else x.contiguous()
        if validate:
            validate_trials(x, trial_rec, trial_start, group_ptr, item_group, item_offset, n, p)
        n_groups, n_items = int(group_ptr.numel()) - 1, int(item_group.numel())
        g_hop, g_nwin = self._ensemble_grid(n_groups, (item_group, item_offset), n_items, grid, validate)
        n_rec, m, T = x.shape
        mp = self.pad(m)
        R = self.empty(n_items, p + 1, mp, mp)
        if n_items == 0:
            return R
        nws = int(self.lib.hmv_lagcov_ensemble_workspace_doubles(n_items, m, int(n), int(p), g_hop, g_nwin))
        if nws < 0:
            raise ValueError(f"lagcov_ensemble: bad sizes (m={m}, n={n}, p={p})")
        ws = self.empty(max(nws, 1))
        self._call("hmv_lagcov_ensemble_f64", x, x.stride(0), x.stride(1), T, trial_rec, trial_start, group_ptr, n_groups,
                   item_group, item_offset, n_items, m, int(n), int(p), R, ws, nws, g_hop, g_nwin, int(flags), self.stream())
        return R

    def sliding_ensemble(self, x: torch.Tensor, trial_rec: torch.Tensor, trial_start: torch.Tensor, group_ptr: torch.Tensor,
                         item_group: torch.Tensor, item_offset: torch.Tensor, n: int, p: int, freqs, fs: float,
                         measure: str = "ffdtf", bands=None, spectra: bool = False, out: torch.Tensor | None = None,
                         return_ar: bool = False, check=True, chunk: int | None = None, grid=None, flags: int = 0,
                         validate: bool = True):
        """Connectivity of event-locked ensembles: for every item (group, offset) ONE model of order p is fitted to the lag
        covariances averaged over the group's trials and `measure` ("ffdtf", "ddtf", "gpdc") is computed from it -- what the
        reference's full_freq_dtf / direct_dtf / gen_partial_directed_coherence give for
        `np.stack([trial windows], axis=2)` with `optimal_model_order=p`.  x (n_rec, m, T) -> (items, m, m, F), or the band
        sums (items, m, m, n_bands) with `bands=(bin_lo, bin_hi)`.  One C-ABI call (`hmv_sliding_ensemble_f64`); only K1
        differs from the single-trial calls.  Index tensors as in `validate_trials`, grid as in `lagcov_ensemble`.
        spectra=True (ffdtf, no bands): returns (out, S) with S (items, m, m, F) complex, `multivariate_spectra` of the
        same fit.  check: True raises SingularMatrixError naming item, group and offset of the failed fits; "nan"
        NaN-fills them; "mask" appends the boolean mask of the failed items without synchronising; False skips the check.
        return_ar appends (ar, V, infos).  p=None raises ValueError (no automatic order for ensembles)."""
        if measure not in ("ffdtf", "ddtf", "gpdc"):
            raise ValueError(f"measure must be 'ffdtf', 'ddtf' or 'gpdc', got {measure!r}")
        if spectra and (measure != "ffdtf" or bands is not None):
            raise ValueError("spectra come with the full ffDTF only")
        rt = self._ensemble_route(measure, n, p, trial_rec, trial_start, group_ptr, spectra)
        return self._sliding_call(rt, x, (item_group, item_offset), freqs, fs, bands=bands, out=out, return_ar=return_ar,
                                  check=check, chunk=chunk, flags=flags, grid=grid, validate=validate)

    # ------------------------------------------------------------------ trial-shuffle significance of ensembles
    def _check_shuffle(self, x, n_items, p, split, R_base, item_base):
        """The arguments of the split K1 that `validate_trials` does not see, before anything is launched."""
        m, mp = x.shape[1], self.pad(x.shape[1])
        if isinstance(split, bool) or int(split) != split or not 1 <= int(split) <= m - 1:
            raise ValueError(f"split must be an integer in 1..{m - 1}, got {split!r}")
        if (R_base is None) != (item_base is None):
            raise ValueError("R_base and item_base go together")
        if R_base is None:
            return
        if not (isinstance(R_base, torch.Tensor) and R_base.dtype == torch.float64 and R_base.device == x.device
                and R_base.dim() == 4 and tuple(R_base.shape[1:]) == (int(p) + 1, mp, mp) and R_base.is_contiguous()):
            raise ValueError(f"R_base must be a contiguous float64 tensor (n_base, {int(p) + 1}, {mp}, {mp}) on {x.device}")
        if not (isinstance(item_base, torch.Tensor) and item_base.dtype == torch.int64 and item_base.device == x.device
                and item_base.dim() == 1 and item_base.numel() == n_items and item_base.is_contiguous()):
            raise ValueError(f"item_base must be a contiguous 1-D int64 tensor of {n_items} entries on {x.device}")
        if n_items:
            lo, hi = int(item_base.min()), int(item_base.max())
            if lo < 0 or hi >= R_base.shape[0]:
                raise ValueError(f"item_base must lie in [0, {R_base.shape[0]}), got [{lo}, {hi}]")

    def lagcov_ensemble_split(self, x: torch.Tensor, trial_rec: torch.Tensor, trial_start: torch.Tensor,
                              trial_rec_b: torch.Tensor, trial_start_b: torch.Tensor, group_ptr: torch.Tensor,
                              item_group: torch.Tensor, item_offset: torch.Tensor, n: int, p: int, split: int,
                              R_base: torch.Tensor | None = None, item_base: torch.Tensor | None = None,
                              validate: bool = True):
        """K1 of a trial-shuffled ensemble (`hmv_lagcov_ensemble_split_f64`): as `lagcov_ensemble` in the direct form, but
        trial step e of a group reads the channels >= split from trial (trial_rec_b[e], trial_start_b[e]) -- table B,
        indexed through the same group_ptr, is table A with the second participant's trials reordered.  With R_base
        (n_base, p+1, MP, MP) and item_base (items,) the within-participant elements (both indices < split, or both
        >= split, padding included) are copied from R_base[item_base[it]] and only the cross blocks are computed.
        Both tables are checked with `validate_trials`."""
        if p is None:
            raise ValueError(_NO_ENSEMBLE_ORDER)
        assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
        x = x if x.stride(2) == 1 else x.contiguous()
        n_groups, n_items = int(group_ptr.numel()) - 1, int(item_group.numel())
        if validate:
            validate_trials(x, trial_rec, trial_start, group_ptr, item_group, item_offset, n, p)
            validate_trials(x, trial_rec_b, trial_start_b, group_ptr, item_group, item_offset, n, p)
            self._check_shuffle(x, n_items, p, split, R_base, item_base)
        n_rec, m, T = x.shape
        mp = self.pad(m)
        R = self.empty(n_items, int(p) + 1, mp, mp)
        if n_items == 0:
            return R
        self._call("hmv_lagcov_ensemble_split_f64", x, x.stride(0), x.stride(1), T, trial_rec, trial_start, group_ptr,
                   n_groups, item_group, item_offset, n_items, m, int(n), int(p), R, trial_rec_b, trial_start_b, int(split),
                   R_base, item_base, 0, self.stream())
        return R

    def ensemble_significance_chunk(self, measure: str, m: int, n: int, p: int, F: int, nb: int) -> int:
        """Items (surrogate x item) per block of `ensemble_significance`: `max_workspace_bytes` over what one item needs --
        the fused call's workspace, the surrogate's band values and its index entries.  No window is ever written."""
        ws = int(self.lib.hmv_sliding_ensemble_workspace_bytes(_MEASURES[measure], 1, m, n, p, F, nb, 0, 0))
        return max(1, self.max_workspace_bytes // (ws + 8 * m * m * nb + 8 * nb + 1 + 3 * 8))

    def ensemble_significance(self, x: torch.Tensor, trial_rec: torch.Tensor, trial_start: torch.Tensor,
                              group_ptr: torch.Tensor, item_group: torch.Tensor, item_offset: torch.Tensor, n: int, p: int,
                              freqs, fs: float, bands, *, measure: str, n_surrogates: int, seed, split=None, check=True,
                              chunk: int | None = None, grid=None):
        """Trial-shuffle test of the band values of `sliding_ensemble(..., measure=measure, bands=bands, grid=grid)`.

        Surrogate s pairs trial e of group g (channels < split, participant A) with trial pi[s][g][e] of the same group
        (channels >= split, participant B); one permutation per (s, g) serves every window of the group
        (`surrogates.trial_permutations` from numpy.random.default_rng(seed)).  Every participant's evoked response and
        within-brain dynamics are those of the observed fit -- the within-participant blocks of the trial-averaged lag
        covariances are copied from it --; the trial-by-trial pairing of the two is not.  No surrogate window is
        written: K1 reads the permuted trials in place (`hmv_sliding_ensemble_split_f64`).  Tests the pairs with exactly
        one index < split.  Statistics, `check` (True or "nan") and the returned dict as `sliding_significance`, with
        one entry per item.  chunk: items (surrogate x item) per block (default `ensemble_significance_chunk`); where
        the items of one surrogate exceed it, a block holds whole groups of one surrogate.  The results are the same
        bits for any chunk.  p=None raises ValueError (no automatic order for ensembles)."""
        return significance.ensemble_significance(self, x, trial_rec, trial_start, group_ptr, item_group, item_offset, n, p,
                                                  freqs, fs, bands, measure=measure, n_surrogates=n_surrogates, seed=seed,
                                                  split=split, check=check, chunk=chunk, grid=grid)

    # ------------------------------------------------------------------ condition contrast of ensembles (lagcov_mix.hip)
    def lagcov_trials(self, x: torch.Tensor, trial_rec: torch.Tensor, trial_start: torch.Tensor, offsets: torch.Tensor, n: int,
                      p: int, grid=None, validate: bool = True):
        """The per-trial stack of an event-locked ensemble: x (n_rec, m, T) -> Rt (E, W, p+1, MP, MP), the lag covariances of
        the window offsets[w] samples after the start of trial e, every trial on its own -- `lagcov_ensemble` with E groups
        of one trial, items group-major.  grid = (hop, n_win) declares offsets[w] = w * hop and lets the library share the
        overlap between the windows of a trial where `lagcov_ensemble`'s rule allows it."""
        if p is None:
            raise ValueError(_NO_ENSEMBLE_ORDER)
        E, W = int(trial_rec.numel()), int(offsets.numel())
        i64 = dict(dtype=torch.int64, device=self.device)
        R = self.lagcov_ensemble(x, trial_rec, trial_start, torch.arange(E + 1, **i64), torch.arange(E, **i64).repeat_interleave(W),
                                 offsets.repeat(E), n, p, grid=grid, validate=validate)
        return R.view(E, W, int(p) + 1, R.shape[-1], R.shape[-1])

    def _check_mix(self, Rt, W, scale, m):
        """Stack, weights and scales of the mix K1 against one another, before anything is launched."""
        mp = self.pad(m)
        if not (isinstance(Rt, torch.Tensor) and Rt.dtype == torch.float64 and Rt.device == self.device and Rt.dim() == 5
                and Rt.is_contiguous() and tuple(Rt.shape[3:]) == (mp, mp) and Rt.shape[2] >= 2):
            raise ValueError(f"Rt must be a contiguous float64 tensor (trials, windows, p + 1, {mp}, {mp}) on {self.device}")
        if not (isinstance(W, torch.Tensor) and W.dtype == torch.float64 and W.device == self.device and W.dim() == 2
                and W.is_contiguous() and W.shape[1] == Rt.shape[0]):
            raise ValueError(f"W must be a contiguous float64 tensor (rows, {Rt.shape[0]}) on {self.device}")
        if scale is not None and not (isinstance(scale, torch.Tensor) and scale.dtype == torch.float64
                                      and scale.device == self.device and tuple(scale.shape) == (W.shape[0],)
                                      and scale.is_contiguous()):
            raise ValueError(f"scale must be a contiguous float64 tensor of {W.shape[0]} entries on {self.device}")

    def lagcov_mix(self, Rt: torch.Tensor, W: torch.Tensor, scale: torch.Tensor | None = None, *, m: int):
        """K1 as a weighted sum over trials (`hmv_lagcov_mix_f64`): Rt (E, n_win, p+1, MP, MP) from `lagcov_trials`, W (rows,
        E), scale (rows,) or None -> R (rows * n_win, p+1, MP, MP), item k * n_win + w = scale[k] * sum_e W[k, e] Rt[e, w] on
        the m x m real elements, trials in ascending order; the padding is written (zero, identity at lag 0), not read.
        m: the channel count, which the padded stack does not carry."""
        self._check_mix(Rt, W, scale, m)
        E, n_win, p1, mp, _ = Rt.shape
        rows = int(W.shape[0])
        R = self.empty(rows * n_win, p1, mp, mp)
        if rows == 0 or n_win == 0 or E == 0:
            if E == 0 and R.numel():
                raise ValueError("lagcov_mix needs at least one trial")
            return R
        self._call("hmv_lagcov_mix_f64", Rt, E, n_win, W, scale, rows, int(m), p1 - 1, R, self.stream())
        return R

    def _mix_route(self, measure, n, m, Rt, W, scale, spectra=False):
        """Route of `sliding_mix` (`hmv_sliding_mix_f64`): the driver's x is the per-trial stack, which carries the order but
        not the channel count; the items are (mix row, window) pairs that only name a failed fit; there is no grid."""
        lib, n, code = self.lib, int(n), _MEASURES[measure]
        E, n_win, p1 = (int(v) for v in Rt.shape[:3])
        p, rows = p1 - 1, int(W.shape[0])

        def blame(err, items):       # say which mix row and which window
            idx = torch.as_tensor(err.items, dtype=torch.int64, device=items[0].device)
            err.rows, err.windows = items[0][idx].cpu().numpy(), items[1][idx].cpu().numpy()
            err.args = (err.args[0], err.args[1] + f" (mix row {int(err.rows[0])}, window {int(err.windows[0])})")

        def call(a):
            return "hmv_sliding_mix_f64", (
                code, a.x[0], E, n_win, W, scale, rows, a.m, n, p, a.f, a.F, a.fs, a.out, a.lo, a.hi, a.nb, a.S,
                a.ar, a.V, a.info_yw, a.info_tf, a.ws, a.nbytes, a.chunk, a.tau, a.flags, a.stream, a.aux)
        return _Route(
            name="sliding_mix", measure=measure, p=p, order_text=f"n={n}, p={p}", more=(_SPECTRA,) if spectra else (),
            blame=blame, m=int(m), infos=_measure_infos(measure, "ar_coeff (Yule-Walker solve of the mixed covariances; a negative "
                                                                 "info: residual covariance not positive definite)"),
            validate=lambda x, items: self._check_mix(x, W, scale, m), grid=lambda x, items, n_items, grid, compare: (),
            ws_bytes=lambda chunk, m_, F, nb, g: lib.hmv_mix_workspace_bytes(code, chunk, m_, p, F, -1 if spectra else nb),
            call=call)

    def sliding_mix(self, Rt: torch.Tensor, W: torch.Tensor, scale: torch.Tensor | None, n: int, freqs, fs: float, *, m: int,
                    measure: str = "ffdtf", bands=None, spectra: bool = False, out: torch.Tensor | None = None,
                    return_ar: bool = False, check=True, chunk: int | None = None, flags: int = 0, validate: bool = True):
        """Connectivity of weighted trial sums: for every mix row k and window w ONE model of the stack's order is fitted to
        scale[k] * sum_e W[k, e] Rt[e, w] and `measure` is computed from it -- with 0 / 1 label rows and scale = 1 / E_c what
        `sliding_ensemble` gives for the trials labelled c, to rounding.  Rt (E, n_win, p+1, MP, MP) from `lagcov_trials` at
        window length n (K1 does not use n; the C entry checks it against the order) -> (rows * n_win, m, m, F), item k *
        n_win + w, or the band sums with `bands=(bin_lo, bin_hi)`.  One C-ABI call (`hmv_sliding_mix_f64`); only K1
        differs from `sliding_ensemble`, whose conventions for spectra, out, return_ar, check and chunk hold; the
        SingularMatrixError of check=True names the mix row and the window.  m: the channel count, which the padded stack
        does not carry.  validate=False skips the shape checks of Rt, W and scale."""
        if measure not in _MEASURES:
            raise ValueError(f"measure must be 'ffdtf', 'ddtf' or 'gpdc', got {measure!r}")
        if spectra and (measure != "ffdtf" or bands is not None):
            raise ValueError("spectra come with the full ffDTF only")
        if validate:
            self._check_mix(Rt, W, scale, m)
        rows, n_win = int(W.shape[0]), int(Rt.shape[1])
        if Rt.shape[0] == 0 and rows * n_win:
            raise ValueError("sliding_mix needs at least one trial")
        rt = self._mix_route(measure, n, m, Rt, W, scale, spectra)
        i64 = dict(dtype=torch.int64, device=self.device)
        items = (torch.arange(rows, **i64).repeat_interleave(n_win), torch.arange(n_win, **i64).repeat(rows))
        return self._sliding_call(rt, Rt, items, freqs, fs, bands=bands, out=out, return_ar=return_ar, check=check, chunk=chunk,
                                  flags=flags, validate=False)

    def ensemble_contrast_chunk(self, measure: str, m: int, p: int, F: int, nb: int) -> int:
        """Items (mix row x window) per block of `ensemble_contrast`: half of `max_workspace_bytes` (the other half is the
        per-trial stack's) over what one item needs -- the fused call's workspace and the item's band values."""
        ws = int(self.lib.hmv_mix_workspace_bytes(_MEASURES[measure], 1, m, p, F, nb))
        return max(1, (self.max_workspace_bytes // 2) // (ws + 3 * 8 * m * m * nb + 8 * nb + 2))

    def ensemble_contrast(self, x: torch.Tensor, trial_rec: torch.Tensor, trial_start: torch.Tensor, group_ptr: torch.Tensor,
                          cond: torch.Tensor, offsets: torch.Tensor, n: int, p: int, freqs, fs: float, bands, *, measure: str,
                          n_surrogates: int, seed, tail: str = "two-sided", split=None, group=None, check=True,
                          chunk: int | None = None, grid=None):
        """Label-permutation test of the difference between two conditions of an event-locked ensemble (Maris & Oostenveld
        2007): does the band value of `sliding_ensemble(..., measure=measure, bands=bands)` differ between the trials
        labelled A (cond == 0) and those labelled B (cond == 1)?

        x (n_rec, m, T); trial e is the epoch starting at trial_start[e] of recording trial_rec[e]; group g (a dyad) owns the
        trials group_ptr[g] .. group_ptr[g+1]-1 and needs at least one of each condition; offsets (W,) int64 are the window
        offsets, common to all groups (grid = (hop, W) declares offsets[w] = w * hop, as for `lagcov_ensemble`).  The pool of
        a group is its A trials in their order, then its B trials.  Surrogate s relabels the pool keeping both sizes
        (`surrogates.label_draws` from numpy.random.default_rng(seed)); one relabelling per (s, g) serves every window.
        The samples are read once per group: `lagcov_trials` gives the per-trial stack and every relabelling -- the observed
        labels included, as two weight rows -- is a row of `sliding_mix`.
        Per group and window: D = band(A) - band(B); T = |D| (tail="two-sided"), D ("greater") or -D ("less"); p, p_fwe
        (maximum over the tested pairs), null_mean, null_std of T as in `sliding_significance`, over the n_valid surrogates
        both of whose fits succeeded.  Tested pairs: i != j without a split, the pairs with exactly one index < split with
        one; NaN elsewhere.  group (G >= 2, or group=True): the observed value is the mean of D over the groups, surrogate s
        the mean of its D over the groups (summed in ascending group order), invalid for a window where any group's fit
        failed; conventions of `pseudo_dyad_significance`.
        check: True raises LinAlgError for a failed observed fit, naming group and window; "nan" gives NaN statistics for
        it.  chunk: items (mix row x window) per block; the results are the same bits for any chunk.  Where the stack of a
        group would exceed half of `max_workspace_bytes` it is built per block of windows.  p=None raises ValueError.
        Returns a dict of device tensors: observed (= D), observed_a, observed_b, p, p_fwe, null_mean, null_std (G, W, m, m,
        n_bands), n_valid (G, W) int32, tested (m, m) bool and, where built, group = {observed, p, p_fwe, null_mean,
        null_std (W, m, m, n_bands), n_valid (W,)}."""
        return significance.ensemble_contrast(self, x, trial_rec, trial_start, group_ptr, cond, offsets, n, p, freqs, fs, bands,
                                              measure=measure, n_surrogates=n_surrogates, seed=seed, tail=tail, split=split,
                                              group=group, check=check, chunk=chunk, grid=grid)

    # ------------------------------------------------------------------ pairs of recordings, pseudo-dyad significance
    def _check_pairs(self, x, n_items, p, split, R_base, base_a, base_b):
        """The arguments of the pair K1 that `validate_items` does not see, before anything is launched."""
        m, mp = x.shape[1], self.pad(x.shape[1])
        if isinstance(split, bool) or int(split) != split or not 1 <= int(split) <= m - 1:
            raise ValueError(f"split must be an integer in 1..{m - 1}, got {split!r}")
        if len({R_base is None, base_a is None, base_b is None}) != 1:
            raise ValueError("R_base, base_a and base_b go together")
        if R_base is None:
            return
        if not (isinstance(R_base, torch.Tensor) and R_base.dtype == torch.float64 and R_base.device == x.device
                and R_base.dim() == 4 and tuple(R_base.shape[1:]) == (int(p) + 1, mp, mp) and R_base.is_contiguous()):
            raise ValueError(f"R_base must be a contiguous float64 tensor (n_base, {int(p) + 1}, {mp}, {mp}) on {x.device}")
        for name, t in (("base_a", base_a), ("base_b", base_b)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.device == x.device and t.dim() == 1
                    and t.numel() == n_items and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous 1-D int64 tensor of {n_items} entries on {x.device}")
            if n_items:
                lo, hi = int(t.min()), int(t.max())
                if lo < 0 or hi >= R_base.shape[0]:
                    raise ValueError(f"{name} must lie in [0, {R_base.shape[0]}), got [{lo}, {hi}]")

    def _validate_pairs(self, x, rec_a, rec_b, item_start, n, p, split, R_base, base_a, base_b):
        validate_items(x, rec_a, item_start, n, p)
        validate_items(x, rec_b, item_start, n, p)
        self._check_pairs(x, int(rec_a.numel()), p, split, R_base, base_a, base_b)

    def lagcov_pairs(self, x: torch.Tensor, rec_a: torch.Tensor, rec_b: torch.Tensor, item_start: torch.Tensor, n: int, p: int,
                     split: int, R_base: torch.Tensor | None = None, base_a: torch.Tensor | None = None,
                     base_b: torch.Tensor | None = None, out: torch.Tensor | None = None, validate: bool = True):
        """K1 for pairs of recordings (`hmv_lagcov_pairs_f64`): x (n_rec, m, T) -> R (items, p+1, MP, MP) of the window of n
        samples at item_start[it] whose channels < split come from recording rec_a[it] and whose channels >= split come
        from recording rec_b[it].  Every computed element has the bits of `lagcov` on that window written out as one
        recording.  With R_base (n_base, p+1, MP, MP), base_a and base_b (items,) the elements with both indices < split
        are copied from R_base[base_a[it]], those with both indices >= split (padding included) from R_base[base_b[it]],
        and only the cross blocks are computed.  Both recording tables are checked with `validate_items`.  `out`, if given,
        is the contiguous (items, p+1, MP, MP) tensor the result is written to."""
        no_auto_order(p, "lagcov_pairs")
        assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
        x = x if x.stride(2) == 1 else x.contiguous()
        if validate:
            self._validate_pairs(x, rec_a, rec_b, item_start, n, p, split, R_base, base_a, base_b)
        n_rec, m, T = x.shape
        mp = self.pad(m)
        n_items = int(rec_a.numel())
        R = self.empty(n_items, int(p) + 1, mp, mp) if out is None else out
        assert R.is_contiguous() and R.dtype == torch.float64 and tuple(R.shape) == (n_items, int(p) + 1, mp, mp)
        if n_items == 0:
            return R
        self._call("hmv_lagcov_pairs_f64", x, x.stride(0), x.stride(1), T, rec_a, rec_b, item_start, n_items, m, int(n),
                   int(p), int(split), R, R_base, base_a, base_b, 0, self.stream())
        return R

    @staticmethod
    def _blame_pair(err, rec_a, rec_b, item_start, split):
        """Say which pair of recordings and which window a SingularMatrixError is about."""
        idx = torch.as_tensor(err.items, dtype=torch.int64, device=rec_a.device)
        err.rec_a, err.rec_b = rec_a[idx].cpu().numpy(), rec_b[idx].cpu().numpy()
        err.starts = item_start[idx].cpu().numpy()
        err.args = (err.args[0], err.args[1] + f" (channels < {int(split)} of recording {int(err.rec_a[0])} with channels "
                    f">= {int(split)} of recording {int(err.rec_b[0])}, window at sample {int(err.starts[0])})")

    def _pairs_route(self, measure, n, p, rec_b, split, R_base, base_a, base_b):
        """Route of `sliding_pairs` (`hmv_sliding_pairs_f64`): the items are (rec_a, item_start), the second recording table
        and the bases ride along, there is no grid, and a failed fit is reported with its pair of recordings."""
        lib, n, p, code = self.lib, int(n), int(p), _MEASURES[measure]

        def blame(err, items):
            self._blame_pair(err, items[0], rec_b, items[1], split)

        def call(a):
            return "hmv_sliding_pairs_f64", (
                code, *a.x, a.T, a.items[0], rec_b, a.items[1], a.n_items, a.m, n, p, a.f, a.F, a.fs, a.out, a.lo,
                a.hi, a.nb, a.S, a.ar, a.V, a.info_yw, a.info_tf, a.ws, a.nbytes, a.chunk, a.tau, a.flags, int(split),
                R_base, base_a, base_b, a.stream, a.aux)
        return _Route(
            name="sliding_pairs", measure=measure, p=p, order_text=f"n={n}, p={p}", blame=blame,
            infos=_measure_infos(measure, _YW_TEXT),
            validate=lambda x, items: self._validate_pairs(x, items[0], rec_b, items[1], n, p, split, R_base, base_a, base_b),
            grid=lambda x, items, n_items, grid, compare: (),
            ws_bytes=lambda chunk, m, F, nb, g: lib.hmv_pairs_workspace_bytes(code, chunk, m, n, p, F, nb),
            call=call)

    def sliding_pairs(self, x: torch.Tensor, rec_a: torch.Tensor, rec_b: torch.Tensor, item_start: torch.Tensor, n: int,
                      p: int, freqs, fs: float, *, measure: str = "ffdtf", split: int, bands=None,
                      R_base: torch.Tensor | None = None, base_a: torch.Tensor | None = None,
                      base_b: torch.Tensor | None = None, out: torch.Tensor | None = None, return_ar: bool = False,
                      check=True, chunk: int | None = None, flags: int = 0, validate: bool = True):
        """Connectivity of pairs of recordings: `measure` ("ffdtf", "ddtf", "gpdc") of the window at item_start[it] whose
        channels < split are those of recording rec_a[it] and whose channels >= split are those of recording rec_b[it] --
        what `sliding_<measure>` gives for the two halves written out as one recording, bit for bit, without writing it.
        x (n_rec, m, T) -> (items, m, m, F), or the band sums (items, m, m, n_bands) with `bands=(bin_lo, bin_hi)`.  One
        C-ABI call (`hmv_sliding_pairs_f64`); only K1 differs from the single-recording calls.  R_base / base_a / base_b
        as in `lagcov_pairs`.  out, return_ar, check, chunk, flags as in `sliding_ffdtf`; the SingularMatrixError of
        check=True names the pair.  p=None raises ValueError (no automatic order here)."""
        if measure not in _MEASURES:
            raise ValueError(f"measure must be 'ffdtf', 'ddtf' or 'gpdc', got {measure!r}")
        no_auto_order(p, "sliding_pairs")
        rt = self._pairs_route(measure, n, p, rec_b, split, R_base, base_a, base_b)
        return self._sliding_call(rt, x, (rec_a, item_start), freqs, fs, bands=bands, out=out, return_ar=return_ar,
                                  check=check, chunk=chunk, flags=flags, validate=validate)

    @staticmethod
    def _check_red_base(red_base, R_base):
        """red_base = (red, info_red) of `sliding_block_granger_pairs(..., return_red=True)`, one row per row of R_base."""
        if R_base is None:
            raise ValueError("red_base needs R_base, base_a and base_b: its rows are the observed windows of R_base")
        ok = isinstance(red_base, (tuple, list)) and len(red_base) == 2 and all(isinstance(t, torch.Tensor) for t in red_base)
        ok = ok and red_base[0].dtype == torch.float64 and red_base[1].dtype == torch.int32
        if not (ok and all(t.device == R_base.device and tuple(t.shape) == (R_base.shape[0], 2) and t.is_contiguous()
                           for t in red_base)):
            raise ValueError(f"red_base must be (red float64, info_red int32), contiguous ({R_base.shape[0]}, 2) tensors on "
                             f"{R_base.device}")

    def block_significance_chunk(self, null: str, m: int, n: int, p: int, split: int, F: int, nb: int, want) -> int:
        """Items (surrogate x window) per block of `block_granger_significance`: `max_workspace_bytes` over what one item
        needs -- the call's workspace, the item buffer (m n doubles; the phase null also its spectrum) and its values."""
        spec, timed = sg.block_want(want)
        ws = int(self.lib.hmv_block_gc_pairs_workspace_bytes(1, m, n, p, split, F, nb, (1 if spec else 0) | (2 if timed else 0)))
        per_item = ws + 8 * m * n + 8 * 4 * (nb + 1) + 8 * (nb + 1) + 64
        if null == "phase":
            per_item += 16 * m * (n // 2 + 1)
        return max(1, self.max_workspace_bytes // per_item)

    def _block_pairs_route(self, n, p, split, rec_b, spec, timed, R_base, base_a, base_b, red_base, return_red):
        """Route of `sliding_block_granger_pairs` (`hmv_sliding_block_gc_pairs_f64`): `_block_route` with the items, the
        validation and the blame of `_pairs_route` and no grid.  Of `spectral` (spec) and `time` (timed) the one not asked
        for is None, with its info array; `red` comes out behind them on request, and the looked-up fits ride along."""
        lib, n, code = self.lib, int(n), (1 if spec else 0) | (2 if timed else 0)
        red_in = (None, None) if red_base is None else tuple(red_base)

        def call(a):
            return "hmv_sliding_block_gc_pairs_f64", (
                *a.x, a.T, a.items[0], rec_b, a.items[1], a.n_items, a.m, n, p, split, a.f, a.F, a.fs, a.out, a.lo, a.hi,
                a.nb, a.time, a.ar, a.V, a.info_yw, a.info_red, a.info_gc, a.ws, a.nbytes, a.chunk, a.flags, R_base, base_a,
                base_b, code, a.red, *red_in, a.stream)
        return _Route(
            name="sliding_block_granger_pairs", measure="block_gc", p=p, order_text=f"n={n}, p={p}, split={split}", row=(2,),
            more=(_BLOCK_TIME if timed else None,) + ((_BLOCK_RED,) if return_red else ()), zero_infos=True,
            infos=(_Info("yw", _YW_TEXT), _BLOCK_INFO_RED if timed else None, _BLOCK_INFO_GC if spec else None),
            blame=lambda err, items: self._blame_pair(err, items[0], rec_b, items[1], split),
            validate=lambda x, items: self._validate_pairs(x, items[0], rec_b, items[1], n, p, split, R_base, base_a, base_b),
            grid=lambda x, items, n_items, grid, compare: (),
            ws_bytes=lambda chunk, m, F, nb, g: lib.hmv_block_gc_pairs_workspace_bytes(chunk, m, n, p, split, F, nb, code),
            call=call)

    def sliding_block_granger_pairs(self, x: torch.Tensor, rec_a: torch.Tensor, rec_b: torch.Tensor, item_start: torch.Tensor,
                                    n: int, p: int, freqs, fs: float, *, split: int, want=("spectral", "time"), bands=None,
                                    R_base: torch.Tensor | None = None, base_a: torch.Tensor | None = None,
                                    base_b: torch.Tensor | None = None, red_base=None, return_red: bool = False,
                                    return_ar: bool = False, check=True, chunk: int | None = None, flags: int = 0,
                                    validate: bool = True):
        """Block Granger causality of pairs of recordings: `sliding_block_granger` of the window at item_start[it] whose
        channels < split are those of recording rec_a[it] and whose channels >= split are those of recording rec_b[it] --
        bit for bit what that call gives for the two halves written out as one recording (with rec_b = rec_a: for the
        recording itself), without writing it.  One C-ABI call (`hmv_sliding_block_gc_pairs_f64`).  -> (spectral, time).
            want      which of the two: "spectral" and / or "time"; the other one is returned as None and none of its
                      kernels runs.  ("time",) needs no frequency grid: freqs may be None, and the call is K1, K2, the two
                      restricted fits and one small kernel.
            bands     (bin_lo, bin_hi): the band sums (items, 2, n_bands) in place of the full (items, 2, F) array.
            R_base, base_a, base_b    as in `lagcov_pairs`: both within-recording covariance blocks are copied from
                      observed windows.
            return_red   appends (red, info_red): red (items, 2) = (ln det Sr_AA, ln det Sr_BB) of the restricted fits
                      and their infos -- what `red_base` takes.
            red_base  (red, info_red) of a call on the observed windows that R_base holds (row = window): the restricted
                      fit of block A is then that of window base_a[it], the one of block B that of window base_b[it]; they
                      are looked up, not computed.  Needs R_base.  Same bits.
        check, chunk, flags as in `sliding_block_granger`; the SingularMatrixError of check=True names the pair, "mask"
        appends the boolean device mask (behind (red, info_red)).  return_ar appends (ar, V, (info_yw, info_red, info_gc)),
        an info that was not asked for being None.  An integer p is required."""
        p = no_block_auto_order(p, "sliding_block_granger_pairs")
        spec, timed = sg.block_want(want)
        split = check_block_split(split, x.shape[1], "sliding_block_granger_pairs")
        if red_base is not None:
            self._check_red_base(red_base, R_base)
        if (red_base is not None or return_red) and not timed:
            raise ValueError("red_base and return_red belong to the time-domain values: want must include 'time'")
        rt = self._block_pairs_route(n, p, split, rec_b, spec, timed, R_base, base_a, base_b, red_base, return_red)
        return self._sliding_call(rt, x, (rec_a, item_start), freqs if spec else None, fs, bands=bands if spec else None,
                                  return_ar=return_ar, check=check, chunk=chunk, flags=flags, validate=validate)

    def block_granger_significance(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int,
                                   freqs, fs: float, bands, *, split: int, null: str, n_surrogates: int, seed,
                                   values=("time", "bands"), min_shift=None, check=True, chunk: int | None = None):
        """Surrogate test of the block Granger causality of `sliding_block_granger` for every window: the time-domain
        values F_{A->B}, F_{B->A} and / or the band sums of the spectral decomposition against null="shift" (block B
        circularly shifted against block A) or null="phase" (every channel phase-randomised).  The surrogate windows are
        those of `sliding_significance`: `surrogates.shift_offsets` / `phase_draws` from numpy.random.default_rng(seed), in
        the same order.  values: "time" and / or "bands"; with ("time",) no frequency-domain kernel runs (bands and freqs
        may be None) and a surrogate costs K1, K2, two restricted fits and one small kernel.
        Statistics as in `sliding_significance` over the two directions: p = (1 + #{T_s >= T_obs}) / (1 + n_valid), p_fwe
        with the maximum over the two directions (per value column), null_mean, null_std (ddof 1).  F_{A.B} and the total
        are returned as observed and not tested.  check: True raises LinAlgError for a failed observed window, "nan" gives
        NaN statistics for it; chunk: items (surrogate x window) per block, the same bits for any chunk.
        Returns a dict of device tensors, index 0 = A -> B, 1 = B -> A: time = {observed, p, p_fwe, null_mean, null_std
        (W, 2)}, bands = {the same, (W, 2, n_bands)}, observed_time (W, 4), n_valid (W,) int32; a leaf that was not asked
        for is absent."""
        return significance.block_granger_significance(self, x, item_rec, item_start, n, p, freqs, fs, bands, split=split,
                                                       null=null, n_surrogates=n_surrogates, seed=seed, values=values,
                                                       min_shift=min_shift, check=check, chunk=chunk)

    def block_granger_pseudo_dyad_significance(self, x: torch.Tensor, item_start: torch.Tensor, n: int, p: int, freqs,
                                               fs: float, bands, *, split: int, n_surrogates=None, seed=None,
                                               values=("time", "bands"), check=True, chunk: int | None = None):
        """Pseudo-dyad (shuffled-partner) test of block Granger causality: `pseudo_dyad_significance` with the two block
        values per window in place of the (m, m) band array.  x (D, m, T), recording d = dyad d, channels < split its
        participant A; surrogate s analyses A of dyad d with B of dyad pi[s][d] (`surrogates.partner_derangements`).  A pseudo
        dyad changes only the cross-participant covariance blocks, so both within-participant blocks (R_base) and both
        restricted fits (red_base) are those of the observed windows: a surrogate of the time-domain values is a cross-block
        K1, one K2 and three small Cholesky log-determinants.  values as in `block_granger_significance`.
        Returns its dict with a leading (D, W) in place of (W,) -- per dyad over the 2 S A-anchored and B-anchored values
        -- plus group = {time, bands, n_valid (W,)} for the mean over the dyads, and partners (S, D) int64."""
        return significance.block_granger_pseudo_dyad_significance(self, x, item_start, n, p, freqs, fs, bands, split=split,
                                                                   n_surrogates=n_surrogates, seed=seed, values=values,
                                                                   check=check, chunk=chunk)

    def pseudo_dyad_significance(self, x: torch.Tensor, item_start: torch.Tensor, n: int, p: int, freqs, fs: float, bands, *,
                                 measure: str, split=None, n_surrogates=None, seed=None, check=True,
                                 chunk: int | None = None):
        """Pseudo-dyad (shuffled-partner) test of the band values of `sliding_<measure>(..., bands=bands)`.

        x (D, m, T): recording d is dyad d, its channels < split participant A, the others participant B; every dyad went
        through the same stimulus, and item_start (W,) names the windows common to all of them.  Surrogate s analyses A of
        dyad d with B of dyad pi[s][d] != d at the same time points (`surrogates.partner_derangements`: n_surrogates=None
        is the exhaustive set of the D - 1 cyclic offsets and uses no seed; an integer draws that many derangements from
        numpy.random.default_rng(seed)).  What the real dyads share with the pseudo dyads is the stimulus; what they do not
        share is the interaction.  No pseudo recording is written: K1 reads the two halves in place
        (`hmv_sliding_pairs_f64`) and copies both within-participant covariance blocks from the observed fits.
        Per dyad ("window" = (d, w)): surrogate s gives dyad d two null values, index 2s A-anchored (A_d with B_pi(d)) and
        index 2s+1 B-anchored (A_{pi^-1(d)} with B_d); p, p_fwe, null_mean, null_std as in `sliding_significance` over the
        n_valid of them whose fit succeeded.  Group ("window" = w): the observed value is the mean over the D dyads,
        surrogate s the mean over its D pseudo dyads, invalid for a window where any of the D fits failed; the observed
        group value is NaN where an observed fit of the window failed.  Tests the pairs with exactly one index < split.
        check: True raises LinAlgError for a failed observed window, "nan" gives NaN statistics for it.  chunk: items per
        fused call (default: a whole surrogate, as far as the workspace allows); the results are the same bits for any chunk.
        Returns a dict of device tensors: observed, p, p_fwe, null_mean, null_std (D, W, m, m, n_bands), n_valid (D, W) int32,
        tested (m, m) bool, partners (S, D) int64 and group = {observed, p, p_fwe, null_mean, null_std (W, m, m, n_bands),
        n_valid (W,)}."""
        return significance.pseudo_dyad_significance(self, x, item_start, n, p, freqs, fs, bands, measure=measure, split=split,
                                                     n_surrogates=n_surrogates, seed=seed, check=check, chunk=chunk)

    # ------------------------------------------------------------------ surrogate significance (surrogate.hip)
    def surrogate_shift(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, shift: torch.Tensor,
                        split: int, out: torch.Tensor | None = None):
        """Shift surrogates of a block (`hmv_surrogate_shift_f64`): x (n_rec, m, T), shift int64 (S_blk, n_rec) ->
        (S_blk * W, m, n), item s * W + w = window w with the channels >= split circularly shifted by shift[s, rec]."""
        n_rec, m, T = x.shape
        x = x if x.stride(2) == 1 else x.contiguous()
        Sb, W = int(shift.shape[0]), int(item_rec.numel())
        out = self.empty(Sb * W, m, int(n)) if out is None else out
        self._call("hmv_surrogate_shift_f64", x, x.stride(0), x.stride(1), T, item_rec, item_start, W, shift, n_rec, Sb, m,
                   int(n), int(split), out, self.stream())
        return out

    def window_spectra(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int):
        """rfft of every window, raw samples as K1 reads them: (W, m, n // 2 + 1) complex128 (one batched transform)."""
        win = x.unfold(2, int(n), 1)[item_rec, :, item_start]            # (W, m, n): the windows only, not the recordings
        return torch.fft.rfft(win, dim=-1)

    def surrogate_phase_spectra(self, spec: torch.Tensor, phi: torch.Tensor, n: int):
        """spec (W, m, nf) complex128, phi (S_blk, m, nf) -> (S_blk * W, m, nf) complex128 (`hmv_surrogate_phase_c128`)."""
        W, m, nf = spec.shape
        Sb = int(phi.shape[0])
        sr = torch.view_as_real(spec.contiguous())
        out = self.empty(Sb * W, m, nf, 2)
        self._call("hmv_surrogate_phase_c128", sr, W, phi, Sb, m, int(n), out, self.stream())
        return torch.view_as_complex(out)

    def surrogate_phase(self, spec: torch.Tensor, phi: torch.Tensor, n: int):
        """Phase surrogates of a block: irfft(rfft(window) exp(i phi[s]), n) -> (S_blk * W, m, n), item s * W + w.  The
        inverse transform runs on the whole block at once: rocFFT's result for one transform does not depend on the
        batch it is planned with (measured on the MI355X), so neither do the surrogates' bits."""
        return torch.fft.irfft(self.surrogate_phase_spectra(spec, phi, n), n=int(n), dim=-1)

    def null_accumulate(self, observed, surr, bad, tested, state, finalize: bool, n_surr: int):
        """One block of surrogates (`hmv_null_accumulate_f64`): observed (W, m, m, nb), surr (n_surr * W, m, m, nb), bad
        (n_surr * W,) bool, tested (m, m) uint8; `state` is the running dict of `null_state`, updated in place.
        finalize: also write state["p"], ["p_fwe"], ["null_mean"], ["null_std"]."""
        W, m, _, nb = observed.shape
        bad8 = bad.to(torch.uint8).contiguous()
        M = self.empty(n_surr * W, nb)
        fin = [state[k] for k in ("p", "p_fwe", "null_mean", "null_std")] if finalize else [None] * 4
        self._call("hmv_null_accumulate_f64", observed, surr, bad8, tested, W, int(n_surr), m, nb, M, state["n_valid"],
                   state["count"], state["count_fwe"], state["n_cell"], state["mean"], state["m2"], *fin, self.stream())
        return M

    def null_state(self, W: int, m: int, nb: int):
        z = dict(dtype=torch.int32, device=self.device)
        st = {"n_valid": torch.zeros(W, **z), "count": torch.zeros(W, m, m, nb, **z), "count_fwe": torch.zeros(W, m, m, nb, **z),
              "n_cell": torch.zeros(W, m, m, nb, **z)}
        for k in ("mean", "m2"):
            st[k] = torch.zeros(W, m, m, nb, dtype=torch.float64, device=self.device)
        for k in ("p", "p_fwe", "null_mean", "null_std"):
            st[k] = self.empty(W, m, m, nb)
        return st

    def significance_chunk(self, measure: str, null: str, W: int, m: int, n: int, p: int, F: int, nb: int) -> int:
        """Items (surrogate x window) per block: `max_workspace_bytes` over what one item needs -- the measure's
        workspace, the item buffer (m n doubles; the phase null also its spectrum) and the surrogate's band values."""
        wsf = {"ffdtf": None, "ddtf": self.lib.hmv_sliding_ddtf_workspace_bytes,
               "gpdc": self.lib.hmv_sliding_gpdc_workspace_bytes}[measure]
        ws = int(self.lib.hmv_sliding_bands_workspace_bytes(1, m, p, F)) if wsf is None else int(wsf(1, m, p, F, nb))
        per_item = ws + 8 * m * n + 8 * m * m * nb + 8 * nb + 1
        if null == "phase":
            per_item += 16 * m * (n // 2 + 1)
        return max(1, self.max_workspace_bytes // per_item)

    def sliding_significance(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int, freqs,
                             fs: float, bands, *, measure: str, null: str, n_surrogates: int, seed, split=None,
                             min_shift=None, check=True, chunk: int | None = None, grid=None):
        """Surrogate test of the band values of `sliding_<measure>(..., bands=bands)` for every window.

        null="shift": surrogate s of window (r, w) keeps the channels < split and reads the channels >= split circularly
        shifted by d[s, r] (the second participant against the first); tests the pairs with exactly one index < split.
        null="phase": every channel of the window with the phases of its rfft replaced (Kaminski et al. 2001); tests i != j.
        The draws are `surrogates.shift_offsets` / `phase_draws` from numpy.random.default_rng(seed).  Per tested cell,
        over the n_valid surrogates whose fit succeeded: p = (1 + #{T_s >= T_obs}) / (1 + n_valid), p_fwe the same with
        the maximum over the tested pairs, null_mean and null_std (ddof 1, Welford in surrogate order); untested cells NaN.
        check: True raises LinAlgError for a failed observed window, "nan" gives NaN statistics for it.  chunk: items
        (surrogate x window) per block (default: `significance_chunk`); the results are the same bits for any chunk.
        grid: (hop, first, n_win) for the OBSERVED call only (`sliding_ffdtf(grid=...)`); the surrogates are separate
        recordings.  Returns a dict of device tensors: observed, p, p_fwe, null_mean, null_std (W, m, m, n_bands),
        n_valid (W,) int32, tested (m, m) bool."""
        return significance.sliding_significance(self, x, item_rec, item_start, n, p, freqs, fs, bands, measure=measure,
                                                 null=null, n_surrogates=n_surrogates, seed=seed, split=split,
                                                 min_shift=min_shift, check=check, chunk=chunk, grid=grid)

    # ------------------------------------------------------------------ recordings streamed from the host
    def stream_dyads(self, dyads, n: int, positions, p: int, freqs, fs: float, bands=None, reduce=None, depth: int = 3,
                     check="nan", keep_full=None, timeline=None, out=None):
        """The reference's outer loop -- load a recording, compute, save, next (eeg_alpha_ibi_ffdtf.py:661-806) -- as a
        pipeline: while recording d computes, recording d + 1 crosses PCIe on a copy stream and the reduced result of
        recording d - 1 goes back on another one.  `dyads`: an iterable of host arrays (m, T) float64 -- NumPy arrays
        (staged through pinned buffers) or pinned torch tensors (copied as they are).  Every recording gets the windows
        `positions` (length n).  What leaves the device per recording is `reduce(ffdtf)` -- by default the band-integrated
        ffDTF (windows, m, m, n_bands) of `bands` (`distributed.DEFAULT_BANDS`): full-resolution ffDTF is 5 GB per
        10-minute dyad, i.e. >= 80 ms of PCIe against ~10 ms of compute.  `keep_full(d, ffdtf_device)` is called (on the
        compute stream's timeline) for callers that want to consume the full array on the device.
        `depth`: recordings in flight (buffer slots).  With two, "result of d - 2 on the host -> upload of d -> compute of
        d" is a chain as long as a dyad's compute and the compute stream waits for its input (0.84 of the resident rate,
        measured); the third slot takes the copies off the critical path.
        Returns the list of reduced results as NumPy arrays, in order.  `out`: optional pinned host tensor
        (n_recordings, *reduced shape) that receives the results directly (no host-side copy: at 98 MB per 10-minute
        dyad that copy alone takes longer than the dyad's compute); the returned arrays are then views of it.  Same
        bits as the resident path: the arithmetic does not know where its input came from (tests/test_gpu_pipeline.py)."""
        from . import distributed as hdist
        from .sliding import regular_grid, window_items
        no_auto_order(p, "stream_dyads")
        dev = self.device
        f = freqs if isinstance(freqs, torch.Tensor) else self.to_device(np.asarray(freqs, dtype=np.float64))
        fhost = f.cpu().numpy()
        lo, hi = hdist.band_bins(fhost, hdist.DEFAULT_BANDS if bands is None else bands)
        # default product without a consumer of the full array: K3's row workers add the bands up themselves and the 5 GB
        # per dyad are never written (`sliding_ffdtf(bands=...)`); same bits as band_sums(full array)
        in_kernel_bands = (reduce is None and keep_full is None)
        if reduce is None:
            def reduce(ff):
                return self.band_sums(ff, lo, hi)
        pos = np.asarray(positions, dtype=np.int64)
        item_rec, item_start = window_items(1, pos, dev)
        grid = regular_grid(pos, n, p)
        validated = False                    # the descriptors are the same for every recording: checked once
        import collections
        import time
        comp = torch.cuda.current_stream(dev)
        s_in, s_out = self.copy_streams()
        slots, results, pending, deferred = [], [], collections.deque(), None
        # timeline: besides the host-side marks, the device-side intervals of every recording (HIP events on the three
        # streams, read after the last recording): when its upload, its kernels and its download started and ended
        tev = [] if timeline is not None else None
        if tev is not None:
            t_base = torch.cuda.Event(enable_timing=True)
            t_base.record(comp)

        def mark(stream):
            e = torch.cuda.Event(enable_timing=True)
            e.record(stream)
            return e

        def collect_one():
            d, k = pending.popleft()
            slots[k]["d2h"].synchronize()
            results.append(out[d].numpy() if out is not None else slots[k]["out_pin"].numpy().copy())
            if timeline is not None:
                timeline.append(("collected", d, time.perf_counter()))

        for d, arr in enumerate(dyads):
            k = d % depth
            while pending and pending[0][0] <= d - depth:      # slot k's previous recording: result on the host first
                if deferred is not None and pending[0][0] == d - 1:     # (depth 1: its download is not even queued yet)
                    deferred()
                    deferred = None
                collect_one()
            pinned_in = isinstance(arr, torch.Tensor) and arr.is_pinned()
            host = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64))
            m, T = host.shape
            if len(slots) <= k:
                slots.append({"x": self.empty(1, m, T),
                              "ff": None if in_kernel_bands else self.empty(len(pos), m, m, int(f.numel())), "in_pin": None,
                              "h2d": torch.cuda.Event(), "done": torch.cuda.Event(), "d2h": torch.cuda.Event(),
                              "red": None, "out_pin": None})
            sl = slots[k]
            if tuple(sl["x"].shape[1:]) != (m, T):
                raise ValueError("stream_dyads: every recording must have the same shape")
            if pinned_in:
                src = host
            else:
                if sl["in_pin"] is None:
                    sl["in_pin"] = torch.empty(m, T, dtype=torch.float64).pin_memory()
                elif d >= depth:
                    sl["h2d"].synchronize()                    # the copy out of this staging buffer has finished
                sl["in_pin"].copy_(host)                       # host memcpy, under the GPU's work on earlier recordings
                src = sl["in_pin"]
            with torch.cuda.stream(s_in):
                if d >= depth:
                    s_in.wait_event(sl["done"])                # the kernels that read x[k] have finished
                if tev is not None:
                    tev.append({"d": d, "h0": mark(s_in)})
                sl["x"][0].copy_(src, non_blocking=True)
                sl["h2d"].record(s_in)
                if tev is not None:
                    tev[-1]["h1"] = mark(s_in)
            # The download of the PREVIOUS recording is queued only now, behind this recording's upload: both directions
            # go through one in-order copy queue, and a download queued first -- it waits for its kernels -- keeps the
            # next upload, and with it the next recording's kernels, waiting too (device timeline of the first
            # recordings, tools/dbg/e2e_depth.py: compute -> download -> upload -> compute, nothing overlapped)
            if deferred is not None:
                deferred()
                deferred = None
            comp.wait_event(sl["h2d"])
            if tev is not None:
                tev[-1]["c0"] = mark(comp)
            if in_kernel_bands:
                if sl["red"] is None:
                    sl["red"] = self.empty(len(pos), m, m, len(lo))
                elif d >= depth:
                    comp.wait_event(sl["d2h"])                 # (already collected on the host: a formality)
                red, bad = self.sliding_ffdtf(sl["x"], item_rec, item_start, n, p, f, fs, out=sl["red"], check="mask",
                                              grid=grid, validate=not validated, bands=(lo, hi))
            else:
                ff, bad = self.sliding_ffdtf(sl["x"], item_rec, item_start, n, p, f, fs, out=sl["ff"], check="mask", grid=grid,
                                             validate=not validated)
                if keep_full is not None:
                    if check == "nan":
                        ff.masked_fill_(bad.view(-1, 1, 1, 1), float("nan"))
                    keep_full(d, ff)
                red = reduce(ff)
            validated = True
            if check == "nan" and red.shape[0] == bad.shape[0]:     # NaN-fill what leaves the device (98 MB, not 5 GB)
                red.masked_fill_(bad.view(-1, *([1] * (red.dim() - 1))), float("nan"))
            if d < depth:                                      # first use of this slot: where the result goes on the host
                if out is None:
                    sl["out_pin"] = torch.empty(red.shape, dtype=red.dtype).pin_memory()
                elif not (out.is_pinned() and tuple(out.shape[1:]) == tuple(red.shape) and out.dtype == red.dtype):
                    raise ValueError("stream_dyads: `out` must be a pinned host tensor (recordings, *%s)" % (tuple(red.shape),))
            if not in_kernel_bands:                            # (in-kernel bands: `red` IS the slot's buffer)
                if sl["red"] is None or sl["red"].shape != red.shape:
                    sl["red"] = torch.empty_like(red)
                elif d >= depth:
                    comp.wait_event(sl["d2h"])                 # (already collected on the host: a formality)
                sl["red"].copy_(red)
            sl["done"].record(comp)
            if tev is not None:
                tev[-1]["c1"] = mark(comp)
            def download(sl=sl, d=d, te=(tev[-1] if tev is not None else None)):
                with torch.cuda.stream(s_out):
                    s_out.wait_event(sl["done"])
                    if te is not None:
                        te["o0"] = mark(s_out)
                    (out[d] if out is not None else sl["out_pin"]).copy_(sl["red"], non_blocking=True)
                    sl["d2h"].record(s_out)
                    if te is not None:
                        te["o1"] = mark(s_out)
            deferred = download
            pending.append((d, k))
            if timeline is not None:
                timeline.append(("queued", d, time.perf_counter()))
        if deferred is not None:
            deferred()
        while pending:
            collect_one()
        if tev is not None:
            torch.cuda.synchronize(dev)
            for t in tev:
                timeline.append(("device_ms", t["d"], {k: t_base.elapsed_time(t[k]) for k in ("h0", "h1", "c0", "c1", "o0", "o1")}))
        return results

    # ------------------------------------------------------------------ ffDTF + spectra from ONE fit
    def sliding_ffdtf_spectra(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, p: int,
                              freqs, fs: float, chunk: int | None = None, check: bool = True, out_ff=None, out_S=None,
                              grid=None, flags: int = 0, max_model_order: int = 20, crit_type: str = "AIC",
                              return_orders: bool = False):
        """Both products the reference's orchestrators always compute together (full_freq_dtf + multivariate_spectra,
        /root/reference/src/eeg_alpha_ibi_ffdtf.py:592-604, src/mtmvar.py:1100-1113) from ONE fit and ONE set of
        inverses per window, in ONE C-ABI call (`hmv_sliding_ffdtf_spectra_f64`): K1 -> K2 -> K3 (ffDTF normalised
        in-kernel, H left in the workspace) -> K5 (S written in the reference's (m, m, F) layout), `chunk` windows at a
        time (H is 16.8 MB per window; default: as many as `max_workspace_bytes` allows).  grid / flags as in
        `sliding_ffdtf`.  Returns (ffdtf (items, m, m, F) real, S (items, m, m, F) complex).
        p=None / max_model_order / crit_type: the automatic order, as in `sliding_ffdtf`; `return_orders=True` appends
        `orders` and `crit`."""
        rt = self._route("ffdtf", n, p, max_model_order, crit_type, spectra=True)
        return self._sliding_call(rt, x, (item_rec, item_start), freqs, fs, out=out_ff, out_more={"S": out_S},
                                  return_orders=return_orders, check=check, chunk=chunk, overlap=True, flags=flags, grid=grid)

    # ------------------------------------------------------------------ FAD (fad.hip)
    FAD_CRIT = {"AIC": 0, "HQ": 1, "SC": 2}

    def _fad_outputs(self, S: int, P: int):
        e = self.empty
        return dict(poles=e(S, P, 2), C=e(S, P, 2), alpha=e(S, P, 2), freq_hz=e(S, P), beta=e(S, P),
                    bandwidth_hz=e(S, P), phi=e(S, P), B=e(S, P), osc_mask=e(S, P, dtype=torch.uint8),
                    paired_index=e(S, P, dtype=torch.int32), n_paired=e(S, dtype=torch.int32),
                    info=e(S, dtype=torch.int32))

    @staticmethod
    def _fad_finish(o: dict):
        for k in ("poles", "C", "alpha"):
            o[k] = torch.view_as_complex(o[k])
        o["osc_mask"] = o["osc_mask"].bool()
        return o

    def fad(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, pmax: int, order: int = 0,
            crit: int = 0, fs: float = 1.0, imag_tol: float = 1e-8, pair_conjugates: bool = True):
        """FAD decomposition of every channel of every window (`hmv_fad_f64`).  x: (n_rec, m, T) float64 device tensor;
        series s = item * m + ch.  order 0 = automatic (crit 0/1/2 = AIC/HQ/SC over 1..pmax).  Returns a dict of device
        tensors with rows of pmax entries per series (NaN / False / -1 past the series' order): order, crit (automatic
        mode), ar, noise_variance, poles / C / alpha (complex128), freq_hz, beta, bandwidth_hz, phi, B, osc_mask (bool),
        paired_index (int32) + n_paired, info (bit 0 fit breakdown, bit 1 no convergence, bit 2 ambiguous grouping)."""
        assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
        x = x if x.stride(2) == 1 else x.contiguous()
        n_rec, m, T = x.shape
        self.check_items(x, item_rec, item_start, n, pmax)
        n_items = int(item_rec.numel())
        S, P = n_items * m, int(pmax)
        o = self._fad_outputs(S, P)
        o["order"] = self.empty(S, dtype=torch.int32)
        o["crit"] = self.empty(S, P) if int(order) == 0 else None
        o["ar"] = self.empty(S, P)
        o["noise_variance"] = self.empty(S)
        self._call("hmv_fad_f64", x, x.stride(0), x.stride(1), item_rec, item_start, n_items, m, int(n), P, int(order),
                   int(crit), float(fs), float(imag_tol), int(bool(pair_conjugates)), o["order"], o["crit"], o["ar"],
                   o["noise_variance"], o["poles"], o["C"], o["alpha"], o["freq_hz"], o["beta"], o["bandwidth_hz"], o["phi"],
                   o["B"], o["osc_mask"], o["paired_index"], o["n_paired"], o["info"], self.stream())
        return self._fad_finish(o)

    def fad_decompose(self, ar: torch.Tensor, fs: float, imag_tol: float = 1e-8, pair_conjugates: bool = True):
        """Poles, residues and FAD parameters of given AR coefficients ar (S, p) (`hmv_fad_decompose_f64`): the same
        outputs as `fad` minus the fit (order, crit, ar, noise_variance)."""
        ar = self.to_device(ar)
        assert ar.dim() == 2
        S, p = ar.shape
        o = self._fad_outputs(S, p)
        self._call("hmv_fad_decompose_f64", ar, S, p, float(fs), float(imag_tol), int(bool(pair_conjugates)), o["poles"],
                   o["C"], o["alpha"], o["freq_hz"], o["beta"], o["bandwidth_hz"], o["phi"], o["B"], o["osc_mask"],
                   o["paired_index"], o["n_paired"], o["info"], self.stream())
        return self._fad_finish(o)

    # ------------------------------------------------------------------ model validation (csrc/validate.hip)
    def _validation_inputs(self, x, item_rec, item_start, n, ar, validate):
        assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
        x = x if x.stride(2) == 1 else x.contiguous()
        m = x.shape[1]
        mp = self.pad(m)
        assert ar.dim() == 4 and ar.dtype == torch.float64 and ar.is_cuda and ar.is_contiguous()
        p = int(ar.shape[3])
        if validate:
            self.check_items(x, item_rec, item_start, n, p)
        n_items = int(item_rec.numel())
        if tuple(ar.shape) != (n_items, mp, mp, p) or not 1 <= p <= MAX_ORDER:
            raise ValueError(f"ar must have shape (items, MP, MP, p) = ({n_items}, {mp}, {mp}, 1..{MAX_ORDER}), "
                             f"got {tuple(ar.shape)}")
        return x, m, mp, p, n_items

    def residuals(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, ar: torch.Tensor,
                  validate: bool = True):
        """Residuals of every window's fit (`hmv_residuals_f64`): x (n_rec, m, T), ar (items, MP, MP, p) from `yw_solve`
        (or `yw_solve_auto`: zero-padded to pmax lags, p = pmax) -> E (items, m, n - p), E[:, :, c] the residual at
        sample p + c of the window:  E = X[:, p:] - sum_k ar[:, :, k-1] X[:, p-k : n-k].  The products run in a fixed
        order, so a window's residuals do not depend on the batch it is computed in."""
        x, m, mp, p, n_items = self._validation_inputs(x, item_rec, item_start, n, ar, validate)
        N = int(n) - p
        E = self.empty(n_items, m, N)
        if n_items == 0:
            return E
        per_item = int(self.lib.hmv_residuals_workspace_bytes(1, m, p))
        nbytes = per_item * self._chunk(n_items, per_item, self.max_workspace_bytes)
        ws = self._workspace(nbytes)
        self._call("hmv_residuals_f64", x, x.stride(0), x.stride(1), item_rec, item_start, n_items, m, int(n), p, ar, E, N,
                   ws, nbytes, self.stream())
        return E

    def whiteness(self, C: torch.Tensor, m: int, N: int, acf_thr: float):
        """The whiteness statistics (`hmv_whiteness_f64`) of lag covariances C (items, h+1, MP, MP) of residuals -- `lagcov`
        over E as `items` recordings of N samples.  Returns the dict of `model_validation` without resid_cov."""
        assert C.dim() == 4 and C.dtype == torch.float64 and C.is_cuda and C.is_contiguous()
        n_items, h = int(C.shape[0]), int(C.shape[1]) - 1
        o = dict(s=self.empty(n_items, h), q=self.empty(n_items, 3), q_channel=self.empty(n_items, m),
                 acf_count=self.empty(n_items, dtype=torch.int32), info=self.empty(n_items, dtype=torch.int32))
        if n_items == 0:
            return o
        self._call("hmv_whiteness_f64", C, n_items, int(m), int(N), h, float(acf_thr), o["s"], o["q"], o["q_channel"],
                   o["acf_count"], o["info"], self.stream())
        return o

    def model_validation(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, ar: torch.Tensor,
                         max_lag: int, *, acf_z: float = 1.96, return_residuals: bool = False, chunk: int | None = None,
                         validate: bool = True):
        """Residual whiteness of every window's fit in one call (`hmv_model_validation_f64`): the residuals E of `residuals`,
        their lag covariances C_l = E[:, :N-l] E[:, l:]^T / N (K1 itself, l = 0..max_lag, N = n - p) and from them, with
        C_0 = L L^T,
            s (items, h)            s_l = ||L^-1 C_l L^-T||_F^2, l = 1..h = max_lag
            q (items, 3)            Box-Pierce N sum s_l, Li-McLeod + m^2 h (h+1) / (2N), Hosking N^2 sum s_l / (N - l)
            q_channel (items, m)    per-channel Ljung-Box N (N+2) sum_l r_l[i,i]^2 / (N - l)
            acf_count (items,)      residual correlations r_l[i,j] = C_l[i,j] / sqrt(C_0[i,i] C_0[j,j]) beyond acf_z / sqrt(N)
            info (items,)           0, or c + 1 where C_0 is not positive definite at column c (statistics NaN, count -1)
            resid_cov (items, m, m) C_0
        and with return_residuals `residuals` (items, m, N).  All device tensors; the chi-square tails are the caller's
        (`sliding.sliding_model_validation`).  The windows are processed `chunk` at a time (default: what
        `max_workspace_bytes` allows)."""
        x, m, mp, p, n_items = self._validation_inputs(x, item_rec, item_start, n, ar, validate)
        h, N = int(max_lag), int(n) - p
        if isinstance(max_lag, bool) or h != max_lag or not 1 <= h <= MAX_ORDER:
            raise ValueError(f"max_lag must be an integer in 1..{MAX_ORDER}, got {max_lag!r}")
        if N <= h:
            raise ValueError(f"n - p ({N}) residuals must exceed max_lag ({h})")
        o = dict(s=self.empty(n_items, h), q=self.empty(n_items, 3), q_channel=self.empty(n_items, m),
                 acf_count=self.empty(n_items, dtype=torch.int32), info=self.empty(n_items, dtype=torch.int32))
        cov = self.empty(n_items, mp, mp)
        E = self.empty(n_items, m, N) if return_residuals else None
        o["resid_cov"] = cov[:, :m, :m]
        if return_residuals:
            o["residuals"] = E
        if n_items == 0:
            return o
        if chunk is None:
            per_item = int(self.lib.hmv_model_validation_workspace_bytes(1, m, int(n), p, h))
            chunk = self._chunk(n_items, per_item, self.max_workspace_bytes)
        chunk = int(chunk)
        nbytes = int(self.lib.hmv_model_validation_workspace_bytes(chunk, m, int(n), p, h))
        if nbytes < 0:
            raise ValueError(f"model_validation: bad sizes (m={m}, n={n}, p={p}, max_lag={h}, chunk={chunk})")
        ws = self._workspace(nbytes)
        self._call("hmv_model_validation_f64", x, x.stride(0), x.stride(1), item_rec, item_start, n_items, m, int(n), p, ar,
                   h, float(acf_z) / float(np.sqrt(N)), o["s"], o["q"], o["q_channel"], o["acf_count"], o["info"], cov, E, N,
                   ws, nbytes, chunk, self.stream())
        return o

    # ------------------------------------------------------------------ FIR decimation (decimate.hip)
    def decimation_taps(self, q: int, design="decimate"):
        """Device copy of `eeg_io.decimation_taps(q, design)`; the two named designs are uploaded once per q."""
        from .eeg_io import decimation_taps
        key = (int(q), design) if isinstance(design, str) else None
        h = self._taps.get(key) if key is not None else None
        if h is None:
            h = self.to_device(decimation_taps(q, design))
            if key is not None:
                self._taps[key] = h
        return h

    def decimate(self, x: torch.Tensor, q: int, design="decimate", out: torch.Tensor | None = None):
        """Anti-aliased decimation by the integer q (`hmv_decimate_fir_f64`): x (n_rec, m, T) or (m, T) float64 on the
        device -> (.., ceil(T / q)), what `scipy.signal.decimate(x, q, ftype='fir', zero_phase=True)` (design="decimate") or
        `scipy.signal.resample_poly(x, 1, q)` (design="resample_poly") return on the host; a 1-D array as `design` is taken
        as the taps.  x may be a strided view (unit stride along time); `out` (optional) a float64 device tensor of the
        result's shape, strided likewise.  On the engine's stream, no host synchronisation.  m is not limited to 64."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != self.device or x.dim() not in (2, 3):
            raise ValueError(f"decimate: x must be a float64 tensor (n_rec, m, T) or (m, T) on {self.device}")
        q = int(q)
        h = self.decimation_taps(q, design)
        x3 = x[None] if x.dim() == 2 else x
        n_rec, m, T = x3.shape
        T_out = int(self.lib.hmv_decimate_out_len(T, q))
        if T_out < 0 or m < 1:
            raise ValueError(f"decimate: bad shape {tuple(x.shape)} for q={q}")
        if n_rec > 0 and (x3.stride(2) != 1 or x3.stride(1) < T or x3.stride(0) < 0):
            x3 = x3.contiguous()
        if out is None:
            y3 = self.empty(n_rec, m, T_out)
        else:
            y3 = out[None] if out.dim() == 2 else out
            if (out.dtype != torch.float64 or out.device != self.device or out.dim() != x.dim()
                    or tuple(y3.shape) != (n_rec, m, T_out) or (n_rec > 0 and (y3.stride(2) != 1 or y3.stride(1) < T_out))):
                raise ValueError(f"decimate: out must be a float64 tensor of shape {(*x.shape[:-1], T_out)} on {self.device}, "
                                 "unit stride along time")
        self._call("hmv_decimate_fir_f64", x3, x3.stride(0), x3.stride(1), T, n_rec, m, q, h, int(h.numel()), y3,
                   y3.stride(0), y3.stride(1), self.stream())
        return (y3[0] if x.dim() == 2 else y3) if out is None else out

    # ------------------------------------------------------------------ phase synchrony (phase_sync.hip)
    def band_response(self, T: int, fs: float, lo=None, hi=None, order: int = 4):
        """Device copy of `eeg_io.band_response(T, fs, lo, hi, order)`, built and uploaded once per argument tuple."""
        from .eeg_io import band_response
        key = (int(T), float(fs), None if lo is None else float(lo), None if hi is None else float(hi), int(order))
        r = self._resp.get(key)
        if r is None:
            r = self._resp[key] = self.to_device(band_response(*key))
        return r

    def analytic_signal(self, x: torch.Tensor, resp: torch.Tensor, out: torch.Tensor | None = None):
        """z = ifft(fft(x) * resp) along time: x (n_rec, m, T) or (m, T) float64 on the device, resp (T,) or (n_bands, T)
        float64 (`band_response`) -> complex128 (n_rec, [n_bands,] m, T), without the recording axis for a 2-D x.  Circular
        (see `eeg_io.band_response`).  `torch.fft` on the engine's stream, one forward transform per recording and one
        inverse per recording and band, each over that recording's m rows alone: a recording's bits do not depend on what
        else is in the call.  m is not limited to 64."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != self.device or x.dim() not in (2, 3):
            raise ValueError(f"analytic_signal: x must be a float64 tensor (n_rec, m, T) or (m, T) on {self.device}")
        x3 = x[None] if x.dim() == 2 else x
        n_rec, m, T = x3.shape
        if (not isinstance(resp, torch.Tensor) or resp.dtype != torch.float64 or resp.device != self.device
                or resp.dim() not in (1, 2) or resp.shape[-1] != T or T < 1):
            raise ValueError(f"analytic_signal: resp must be a float64 tensor (T,) or (n_bands, T) with T = {T} on {self.device}")
        r2 = resp[None] if resp.dim() == 1 else resp
        nb = int(r2.shape[0])
        z = torch.empty(n_rec, nb, m, T, dtype=torch.complex128, device=self.device) if out is None else out
        for r in range(n_rec):
            X = torch.fft.fft(x3[r].contiguous(), dim=-1)
            for b in range(nb):
                torch.fft.ifft(X * r2[b], dim=-1, out=z[r, b])
        if out is not None:
            return out
        z = z[:, 0] if resp.dim() == 1 else z
        return z[0] if x.dim() == 2 else z

    def _phase_sync(self, z, item_rec, item_start, n, mode, mag, lagged, coherency):
        n_rec, m, T = z.shape
        n_items = int(item_rec.numel())
        info = torch.empty(n_items, dtype=torch.int32, device=self.device)
        out = {}
        if mag:
            out["mag"] = self.empty(n_items, m, m)
        if lagged:
            out["lagged"] = self.empty(n_items, m, m)
        if coherency:
            out["coherency"] = self.empty(n_items, 2, m, m)
        self._call("hmv_phase_sync_c128", z, z.stride(0), z.stride(1), T, n_rec, m, item_rec, item_start, n_items, int(n),
                   int(mode), out.get("coherency"), out.get("mag"), out.get("lagged"), info, self.stream())
        out["info"] = info
        return out

    def phase_sync(self, z: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, mode: int, *,
                   want=("mag", "lagged"), coherency: bool = False):
        """Phase synchrony of every window (`hmv_phase_sync_c128`): z (n_rec, m, T) complex128 on the device (unit stride
        along time; a strided view is read in place), item i = the n samples of recording item_rec[i] from item_start[i].
        mode `_lib.PHASE_UNIT`: mag = PLV, lagged = ciPLV of the unit phasors; `_lib.PHASE_RAW`: mag = coherence, lagged =
        imaginary coherence of z itself.  -> {"mag", "lagged": (n_items, m, m) as named in `want`, "coherency": (n_items, 2,
        m, m) (Re R, Im R) if asked, "info": int32 (n_items,)}: 1 = a non-finite sample (the item is NaN), 2 = RAW only, a
        channel of zero power (its row and column are NaN).  On the engine's stream; nothing is read back after the check
        of the item tables."""
        return phase.phase_sync(self, z, item_rec, item_start, n, mode, want=want, coherency=coherency)

    def _phase_sync_pairs(self, z, rec_a, rec_b, item_start, n, mode, split, shift_b, values, cols, info=None):
        n_rec, m, T = z.shape
        n_items = int(rec_a.numel())
        info = torch.empty(n_items, dtype=torch.int32, device=self.device) if info is None else info
        self._call("hmv_phase_sync_pairs_c128", z, z.stride(0), z.stride(1), T, n_rec, m, int(split), rec_a, rec_b,
                   item_start, shift_b, n_items, int(n), int(mode), values, int(values.shape[-1]), int(cols[0]),
                   int(cols[1]), info, self.stream())
        return values, info

    def phase_sync_pairs(self, z: torch.Tensor, rec_a: torch.Tensor, rec_b: torch.Tensor, item_start: torch.Tensor, n: int,
                         mode: int, *, split: int, shift_b: torch.Tensor | None = None, out: torch.Tensor | None = None,
                         cols=(0, 1)):
        """The inter-brain cells of `phase_sync` for items put together from two places (`hmv_phase_sync_pairs_c128`): item
        i = the channels < split of recording rec_a[i] at item_start[i] .. + n with the channels >= split of recording
        rec_b[i] read shift_b[i] samples later, modulo T (shift_b None: 0).  z as for `phase_sync`.  rec_b = rec_a with a
        shift is the shift surrogate of the window (the analytic signal is a circular filter, so shifting the recording
        shifts z), another rec_b at shift 0 the pseudo dyad; neither is ever written out.
        cols = (col_mag, col_lagged): the columns of `out` (n_items, m, m, K) float64 that receive mag and lagged, -1 for an
        output that is not wanted; the other columns of `out` are left alone.  out None: a new (n_items, m, m, 1 + max(cols))
        tensor, NaN in the columns not written.  In the written columns a cross cell (one index < split) has the bits
        `phase_sync` gives on the written-out window and every other cell is NaN.  -> (out, info int32 (n_items,)), info as
        in `phase_sync`.  Both recording tables and the shifts (0..T-1) are checked before the call."""
        return phase.phase_sync_pairs(self, z, rec_a, rec_b, item_start, n, mode, split=split, shift_b=shift_b, out=out,
                                      cols=cols)

    def phase_sync_significance(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, fs: float,
                                bands_hz, *, measures=("plv",), n_surrogates: int, seed, split=None, min_shift=None,
                                order: int = 4, check=True, chunk: int | None = None, full: bool = False,
                                max_workspace_bytes: int = 8 << 30):
        """Shift-surrogate test of the inter-brain cells of `sliding_phase_sync`: x (n_rec, m, T) float64 on the device,
        channels < split participant A.  Surrogate s reads participant B of recording r d[s, r] samples later, circularly,
        with d = `surrogates.shift_offsets(numpy.random.default_rng(seed), S, n_rec, T, min_shift)` modulo T (min_shift = 0 can
        draw T itself, which reads B as it lies).  The analytic signal is a
        circular filter, so that is the observed analytic signal of B read d samples later: z is formed once per slab of
        recordings x bands (the slabs of `sliding_phase_sync`) and a surrogate is a table of shifts for `phase_sync_pairs` --
        no surrogate signal, FFT or window exists.  Per window and band the statistics of `sliding_significance` over the
        measures as value columns: p = (1 + #{v_s >= v_obs}) / (1 + n_valid), p_fwe with the maximum over the tested pairs per
        window, band and measure, null_mean, null_std (ddof 1).  A surrogate item with a non-finite sample is left out of
        n_valid.  check=True: ValueError naming the first (recording, window, band) whose observed info is not 0; "nan": its
        row is NaN.  chunk: items (surrogate x window x band) per call; the same bits for any chunk and any slab size.
        -> {"tested": (m, m) bool, "n_valid": int32 (n_items, n_bands), "info": int32 (n_items, n_bands), measure: {"observed",
        "p", "p_fwe", "null_mean", "null_std": (n_items, n_bands, m, m)}}; observed holds the cross cells and NaN elsewhere;
        full=True adds "full": the dict of `sliding_phase_sync` on the same z."""
        return significance.phase_sync_significance(self, x, item_rec, item_start, n, fs, bands_hz, measures=measures,
                                                    n_surrogates=n_surrogates, seed=seed, split=split, min_shift=min_shift,
                                                    order=order, check=check, chunk=chunk, full=full,
                                                    max_workspace_bytes=max_workspace_bytes)

    def phase_sync_pseudo_dyad_significance(self, x: torch.Tensor, item_start: torch.Tensor, n: int, fs: float, bands_hz, *,
                                            measures=("plv",), split=None, n_surrogates=None, seed=None, order: int = 4,
                                            check=True, chunk: int | None = None, max_workspace_bytes: int = 8 << 30):
        """Pseudo-dyad test of the inter-brain cells of `sliding_phase_sync`: x (D, m, T), recording d = dyad d, item_start
        (W,) the windows common to all dyads.  Surrogate s analyses A of dyad d with B of dyad pi[s][d] at the same samples
        (`surrogates.partner_derangements`, as `pseudo_dyad_significance`): one `phase_sync_pairs` call per mode on the
        resident analytic signals, rec_b = pi[s][rec_a], no shift.  The bands run outermost, with the analytic signals of all
        D dyads of one band resident together; ValueError (with the bytes needed) if they do not fit max_workspace_bytes.
        -> {"tested", "partners" (S, D), "n_valid" (D, W, n_bands), "info" (D, W, n_bands), measure: {"observed", "p",
        "p_fwe", "null_mean", "null_std": (D, W, n_bands, m, m)}, "group": {"n_valid" (W, n_bands), measure: {the same five,
        (W, n_bands, m, m)}}} -- per dyad over the 2 S A-anchored and B-anchored values, and for the mean over the dyads."""
        return significance.phase_sync_pseudo_dyad_significance(self, x, item_start, n, fs, bands_hz, measures=measures,
                                                                split=split, n_surrogates=n_surrogates, seed=seed,
                                                                order=order, check=check, chunk=chunk,
                                                                max_workspace_bytes=max_workspace_bytes)

    def phase_slabs(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, resp: torch.Tensor,
                    max_workspace_bytes: int):
        """The analytic signal of x (n_rec, m, T) for the responses resp (n_bands, T), slab by slab: B bands of R recordings, as
        many as keep the complex arrays alive at one time -- the slab's z, one recording's spectrum and one product -- under
        `max_workspace_bytes` (at least one recording and one band).  Yields (sel, b0, b1, z, rec_z, start_z): the slab holds
        the bands b0 .. b1 - 1 of the items `sel` (a slice or an index tensor into the item tables), z ((recordings of the
        slab) * (b1 - b0), m, T) is its analytic signal with the bands as recordings, and rec_z / start_z are its item tables,
        window-major and band-minor.  The caller drops its z before asking for the next slab."""
        return phase.phase_slabs(self, x, item_rec, item_start, resp, max_workspace_bytes)

    def sliding_phase_sync(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, fs: float,
                           bands_hz, *, measures=("plv",), order: int = 4, check=True, max_workspace_bytes: int = 8 << 30):
        """Band-limited phase synchrony per window: x (n_rec, m, T) float64 on the device -> {measure: (n_items, n_bands, m,
        m), "info": int32 (n_items, n_bands)} for `measures` out of ("plv", "ciplv", "coh", "imcoh") and the bands
        `bands_hz` = ((lo, hi), ...) in Hz (Butterworth of `order`, applied in the frequency domain: `eeg_io.band_response`).
        The analytic signal is formed slab by slab -- some recordings times some bands, as many as keep the complex arrays
        alive at one time under `max_workspace_bytes` -- and each slab is one kernel call per mode (PLV / ciPLV: unit
        phasors; coh / imcoh: the signal itself), both on the same z.  Bit-identical to `phase_sync(analytic_signal(..))`
        by hand.  check=True: ValueError naming the first (recording, window, band) whose info is not 0; check="nan": the
        arrays come back with their NaNs."""
        from .eeg_io import resolve_phase_measures
        measures = resolve_phase_measures(measures)
        return self.sliding_phase("sliding_phase_sync", x, item_rec, item_start, n, fs, bands_hz, sync=measures, order=order,
                                  check=check, max_workspace_bytes=max_workspace_bytes)[0]

    # ------------------------------------------------------------------ phase-lag family (phase_lag.hip)
    def _phase_lag(self, z, item_rec, item_start, n, want, split):
        n_rec, m, T = z.shape
        n_items = int(item_rec.numel())
        info = torch.empty(n_items, dtype=torch.int32, device=self.device)
        out = {q: self.empty(n_items, m, m) for q in want}
        self._call("hmv_phase_lag_c128", z, z.stride(0), z.stride(1), T, n_rec, m, int(split), item_rec, item_start, n_items,
                   int(n), out.get("pli"), out.get("wpli"), out.get("dwpli"), info, self.stream())
        out["info"] = info
        return out

    def phase_lag(self, z: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, *, want=("wpli",),
                  split: int = 0):
        """The phase-lag family of every window (`hmv_phase_lag_c128`): z (n_rec, m, T) complex128 on the device (unit
        stride along time; a strided view is read in place), item i = the n samples of recording item_rec[i] from
        item_start[i].  With x[t] = Im(z_i[t] conj z_j[t]) (two rounded products, one subtraction):
        "pli" = |#{x > 0} - #{x < 0}| / n (Stam 2007), "wpli" = |sum x| / sum |x|, "dwpli" = (S^2 - Q) / (A^2 - Q) with
        S = sum x, A = sum |x|, Q = sum x^2 (Vinck 2011; may be slightly negative, NaN where A^2 - Q <= 0).  The diagonal is
        0.  split = 0: all pairs; 1..m-1: the pairs i < split <= j only, every other off-diagonal cell NaN.
        -> {the measures named in `want`: (n_items, m, m), "info": int32 (n_items,)}: 1 = a non-finite sample (the item is
        NaN), 2 = a computed pair with sum |x| == 0 (a flat or duplicated channel; those cells pli 0, wpli / dwpli NaN).
        PLI is exactly what NumPy gives; every cell's bits depend on the n samples of its two channels only.  On the
        engine's stream; nothing is read back after the check of the item tables."""
        return phase.phase_lag(self, z, item_rec, item_start, n, want=want, split=split)

    def sliding_phase_lag(self, x: torch.Tensor, item_rec: torch.Tensor, item_start: torch.Tensor, n: int, fs: float,
                          bands_hz, *, measures=("wpli",), split: int = 0, order: int = 4, check=True,
                          max_workspace_bytes: int = 8 << 30):
        """Band-limited phase-lag measures per window: x (n_rec, m, T) float64 on the device -> {measure: (n_items,
        n_bands, m, m), "info": int32 (n_items, n_bands)} for `measures` out of ("pli", "wpli", "dwpli") (`phase_lag`), the
        bands and the slabs of the analytic signal as in `sliding_phase_sync`, one kernel call per slab.  Bit-identical
        to `phase_lag(analytic_signal(..))` by hand.  split as in `phase_lag`.  check=True: ValueError naming the first
        (recording, window, band) whose info is not 0; check="nan": the arrays come back with their NaNs."""
        from .eeg_io import resolve_phase_lag_measures
        measures = resolve_phase_lag_measures(measures)
        return self.sliding_phase("sliding_phase_lag", x, item_rec, item_start, n, fs, bands_hz, lag=measures, split=split,
                                  order=order, check=check, max_workspace_bytes=max_workspace_bytes)[1]

    PHASE_SYNC_WHY, PHASE_LAG_WHY = phase.SYNC_WHY, phase.LAG_WHY

    def sliding_phase(self, who, x, item_rec, item_start, n, fs, bands_hz, *, sync=None, lag=None, split=0, order=4,
                      check=True, max_workspace_bytes=8 << 30):
        """The one driver of `sliding_phase_sync` (sync: its resolved measures) and `sliding_phase_lag` (lag: its resolved
        measures, with `split`), for a caller `who` that wants both: every slab of `phase_slabs` is formed once and handed
        to the kernels of both families, so the two cost one analytic signal.  -> (dict of `sliding_phase_sync` or None,
        dict of `sliding_phase_lag` or None), each with its own "info" and the bits its own call gives.  check=True raises
        for the first window refused, the synchrony family's first."""
        return phase.sliding_phase(self, who, x, item_rec, item_start, n, fs, bands_hz, sync=sync, lag=lag, split=split,
                                   order=order, check=check, max_workspace_bytes=max_workspace_bytes)


_default = None


def default_engine() -> Engine:
    global _default
    if _default is None:
        _default = Engine()
    return _default
