"""The null tests behind `Engine.sliding_significance`, `.pseudo_dyad_significance`, `.block_granger_significance`,
`.block_granger_pseudo_dyad_significance`, `.ensemble_significance`, `.ensemble_contrast`, `.phase_sync_significance` and
`.phase_sync_pseudo_dyad_significance`: the functions of those names below, each taking the engine first.

What they share is here once: the block planners (integers in, integers out), the preamble, `NullAccumulator`, which owns the
running state of `hmv_null_accumulate_f64` and builds every returned dict, and one loop per null -- `surrogate_null` (shift and
phase surrogates of sliding windows) and `partner_null` (pseudo dyads).  A loop does not know what a value is: the test hands
it the observed values as (rows, mv, mv, nv) and a closure that turns a block of surrogate items into (values, bad).  For
the connectivity measures that is the (m, m, n_bands) band array of the fused call itself; for block Granger causality it is
the 2 x 2 meta array of `block_meta`, taken apart again by `block_leaves`.  So a test is: check the arguments, make the
observed call, run its loop, shape the result.  The two ensemble tests plan their blocks differently and keep loops of their
own.  Phase synchrony has no model and no surrogate window: its shift surrogate is a table of shifts for the pairs kernel
on the observed analytic signal, so its shift test walks `sliding_plan`'s blocks itself, slab by slab of the analytic
signal (`phase.phase_slabs`; the mode table, the check of x and the sentence that names a refused window are `phase`'s
too), and its pseudo-dyad test is `partner_null` without the lag-covariance base (p = None).  The draws and the argument
checks are `surrogates`; everything that wraps one C call is a method of the engine.
"""
from __future__ import annotations

import numpy as np
import torch

from . import engine as _engine
from . import phase
from . import surrogates as sg

__all__ = ["sliding_plan", "ensemble_plan", "stack_plan", "window_ranges", "surrogate_blocks", "NullAccumulator",
           "surrogate_null", "partner_null", "sliding_significance", "ensemble_significance", "pseudo_dyad_significance",
           "ensemble_contrast", "block_meta", "block_leaves", "block_granger_significance",
           "block_granger_pseudo_dyad_significance", "phase_calls", "phase_pairs", "phase_chunk", "phase_sync_significance",
           "phase_sync_pseudo_dyad_significance"]

STATS = ("p", "p_fwe", "null_mean", "null_std")


# ------------------------------------------------------------------ block planning: integers and host arrays only
def sliding_plan(S: int, W: int, chunk: int):
    """S surrogates of W >= 1 rows each, at most `chunk` >= 1 items (surrogate x row) per block -> (Sb, Wb): whole
    surrogates, Sb at a time, where one fits (Wb = W); else one surrogate in blocks of Wb rows."""
    Wb = min(W, chunk)
    Sb = min(S, max(1, chunk // W)) if Wb == W else 1
    return Sb, Wb


def ensemble_plan(first, S: int, chunk: int):
    """The items of group g are first[g] .. first[g+1]-1 (N = first[-1] >= 1 in all) -> (Sb, [(g0, g1), ...]): whole
    surrogates, Sb at a time, where the N items fit in `chunk`; else whole groups of one surrogate, as many as fit and at
    least one -- a group larger than the chunk still goes whole."""
    G, N = len(first) - 1, int(first[-1])
    if N <= chunk:
        return min(S, chunk // N), [(0, G)]
    blocks, g0 = [], 0
    while g0 < G:
        g1 = g0 + 1
        while g1 < G and first[g1 + 1] - first[g0] <= chunk:
            g1 += 1
        blocks.append((g0, g1))
        g0 = g1
    return 1, blocks


def stack_plan(E: int, W: int, per_window: int, cap_bytes: int) -> int:
    """Windows per block of a per-trial stack of E trials x W windows of `per_window` bytes each: all of them where the
    stack fits in cap_bytes, else as many as fit (at least one)."""
    return W if E * W * per_window <= cap_bytes else max(1, cap_bytes // (E * per_window))


def window_ranges(W: int, Wb: int):
    return [(w0, min(W, w0 + Wb)) for w0 in range(0, W, Wb)]


def surrogate_blocks(S: int, Sb: int, ranges):
    """The blocks in the order they run: (s0, sb, r0, r1, last) for the surrogates s0 .. s0+sb-1 of the range (r0, r1),
    surrogate blocks ascending (Welford's order) and every range under each; last: the block ends at surrogate S."""
    for s0 in range(0, S, Sb):
        sb = min(Sb, S - s0)
        for r0, r1 in ranges:
            yield s0, sb, r0, r1, s0 + sb >= S


# ------------------------------------------------------------------ what every test does before and after its surrogates
def device_x(x):
    assert x.dim() == 3 and x.dtype == torch.float64 and x.is_cuda
    return x if x.stride(2) == 1 else x.contiguous()


def band_bins(bands, who: str):
    lo, hi = (np.asarray(b, dtype=np.int32) for b in bands)
    nb = int(lo.size)
    if nb < 1:
        raise ValueError(f"{who} needs at least one band")
    return lo, hi, nb


def prepare(eng, freqs, bands, who: str, m: int, null: str, split):
    """-> f (device), F, lo, hi, nb, tested_h (host bool), tested (device uint8); refuses an empty or ill-formed band set."""
    f = freqs if isinstance(freqs, torch.Tensor) else eng.to_device(np.asarray(freqs, dtype=np.float64))
    F = int(f.numel())
    lo, hi, nb = band_bins(bands, who)
    eng.band_tables(lo, hi, F)
    tested_h = sg.tested_mask(m, null, split)
    return f, F, lo, hi, nb, tested_h, torch.as_tensor(tested_h.astype(np.uint8)).to(eng.device)


def observed_run(run, check):
    """run(check) is the observed call -> (observed, None) under check=True, (observed, bad) under "nan"."""
    obs = run(True if check is True else "mask")
    return (obs, None) if check is True else obs


class NullAccumulator:
    """The running statistics of N rows ("windows" of `hmv_null_accumulate_f64`) of (m, m, nb) band values, and the dicts
    a test returns from them."""

    def __init__(self, eng, N: int, m: int, nb: int, tested_h, tested):
        self.eng, self.m, self.nb, self.tested = eng, m, nb, tested
        self.tested_out = torch.as_tensor(tested_h).to(eng.device)
        self.st = eng.null_state(N, m, nb)
        self._failed = None

    def add(self, observed_rows, vals, bad, rows: slice, n_surr: int, last: bool):
        """n_surr surrogates of the rows `rows`: vals (n_surr * rows, m, m, nb) surrogate-major, bad alike."""
        sub = {k: v[rows] for k, v in self.st.items()}                  # row-major: contiguous views
        self.eng.null_accumulate(observed_rows, vals, bad, self.tested, sub, last, n_surr)

    def failed(self, obs_bad) -> bool:
        """Did an observed fit fail?  The one host synchronisation of a run, at its first use."""
        if self._failed is None:
            self._failed = obs_bad is not None and bool(obs_bad.any())
        return self._failed

    def empty(self, lead, extra_observed=(), group: bool = False):
        """The result of a run without rows: lead = the leading shape, one dimension of it 0."""
        def new(*lead):
            return self.eng.empty(*lead, self.m, self.m, self.nb)
        res = self.result(lead, new(*lead), None, {k: new(*lead) for k in extra_observed})
        if group:
            res["group"] = dict({k: new(*lead[1:]) for k in ("observed",) + STATS},
                                n_valid=self.eng.empty(*lead[1:], dtype=torch.int32))
        return res

    def result(self, lead, observed, obs_bad, extra_observed=(), index=None):
        """The per-row dict, rows viewed as `lead` (or gathered by `index`): NaN where obs_bad says an observed fit failed,
        in `observed`, in extra_observed (a dict of further observed tensors) and in the four statistics."""
        shape = (*lead, self.m, self.m, self.nb)
        res = {"tested": self.tested_out, "observed": observed.view(shape), **dict(extra_observed)}
        res["n_valid"] = self.st["n_valid"].view(lead) if index is None else self.st["n_valid"][index]
        for k in STATS:
            res[k] = self.st[k].view(shape) if index is None else self.st[k][index]
        if self.failed(obs_bad):
            for k in ("observed", *dict(extra_observed), *STATS):
                res[k][obs_bad.view(lead)] = float("nan")
        return res

    def group(self, observed, surr, bad, S: int, obs_bad, tested_value=None):
        """The one-shot test of the group value: observed (W, m, m, nb), surr (S, W, m, m, nb), bad (S, W); the statistic
        tested is `tested_value` where it is not `observed` itself.  NaN for a window where an observed fit (obs_bad,
        (rows / W, W)) failed."""
        W = int(observed.shape[0])
        gst = self.eng.null_state(W, self.m, self.nb)
        self.eng.null_accumulate(observed if tested_value is None else tested_value, surr.view(S * W, self.m, self.m, self.nb),
                                 bad.view(S * W), self.tested, gst, True, S)
        grp = {"observed": observed, "n_valid": gst["n_valid"], **{k: gst[k] for k in STATS}}
        if self.failed(obs_bad):
            bad_w = obs_bad.view(-1, W).any(dim=0)
            for k in ("observed",) + STATS:
                grp[k][bad_w] = float("nan")
        return grp


# ------------------------------------------------------------------ the loops: one per null
def surrogate_null(eng, acc, x, item_rec, item_start, n, null, S, seed, split, min_shift, chunk, obs, surrogate):
    """The shift / phase null of the W windows (item_rec, item_start) of x: the draws (`shift_offsets` once up front,
    `phase_draws` per surrogate block), the blocks of `sliding_plan(S, W, chunk)`, every block's surrogate windows written
    out as recordings of their own, `surrogate(xs (items, m, n), item_rec, item_start) -> (values, bad)` on them, and the
    values into `acc` against the observed rows `obs`, surrogate blocks ascending (Welford's order)."""
    n_rec, m, T = x.shape
    W = int(item_rec.numel())
    rng = np.random.default_rng(seed)
    if null == "shift":
        d_all = torch.as_tensor(sg.shift_offsets(rng, S, n_rec, T, min_shift)).to(eng.device)
    else:
        spec = eng.window_spectra(x, item_rec, item_start, n)
    Sb, Wb = sliding_plan(S, W, max(1, int(chunk)))
    zeros = torch.zeros(Sb * Wb, dtype=torch.int64, device=eng.device)          # the largest block's descriptors
    ar_items = torch.arange(Sb * Wb, dtype=torch.int64, device=eng.device)
    for s0, sb, w0, w1, last in surrogate_blocks(S, Sb, window_ranges(W, Wb)):
        if null == "phase" and w0 == 0:                                         # drawn per surrogate block
            phi = torch.as_tensor(sg.phase_draws(rng, sb, m, n)).to(eng.device)
        ws = slice(w0, w1)
        if null == "shift":
            xs = eng.surrogate_shift(x, item_rec[ws], item_start[ws], n, d_all[s0:s0 + sb], split)
        else:
            xs = eng.surrogate_phase(spec[ws], phi, n)
        items = sb * (w1 - w0)
        vals, bad = surrogate(xs.view(items, m, n), ar_items[:items], zeros[:items])
        acc.add(obs[ws], vals, bad, ws, sb, last)


def dyad_items(eng, x, item_start, n, p):
    """x (D, m, T), the W windows common to the dyads -> (dy, starts): item (d, w) = d * W + w, checked against x."""
    D, W = int(x.shape[0]), int(item_start.numel())
    dy = torch.arange(D, dtype=torch.int64, device=eng.device).repeat_interleave(W)
    starts = item_start.repeat(D) if isinstance(item_start, torch.Tensor) else item_start
    eng.check_items(x, dy, starts, n, p)
    return dy, starts


def partner_null(eng, acc, x, dy, starts, n, p, partners, chunk, obs, obs_bad, surrogate):
    """The pseudo-dyad null of the N = D W items (dy, starts): K1 over the real windows for the within-participant blocks
    (not with p = None: the value has no model order and `base` carries R_base = None), then per derangement
    `surrogate(block, rec_b, base, out) -> bad` on blocks of at most `chunk` items -- `out` (block, mv, mv, nv) receives the
    values of A of dyad dy with B of dyad rec_b, `base` is R_base / base_a / base_b of the block --, the A- and the
    B-anchored value of every dyad into `acc` against `obs`, and the mean over the dyads aside.  -> the group dict of
    `NullAccumulator.group`."""
    N, mv, _, nv = obs.shape
    S, D = partners.shape
    W = N // D
    i64 = dict(dtype=torch.int64, device=eng.device)
    # (K1 over the D W real windows a second time -- the observed fused call does not hand its R out; a few per cent of it)
    # p None: a value without a model (phase synchrony) has no within-participant blocks to copy, and R_base is None
    R_base = None if p is None else eng.lagcov(x, dy, starts, n, p)
    base_a = torch.arange(N, **i64)
    wrep = torch.arange(W, **i64).repeat(D)
    blk = N if chunk is None else max(1, min(N, int(chunk)))
    gmean = eng.empty(S, W, mv, mv, nv)
    gbad = torch.empty(S, W, dtype=torch.bool, device=eng.device)
    both = eng.empty(2, N, mv, mv, nv)                                 # the two surrogates one s gives every dyad
    both_bad = torch.empty(2, N, dtype=torch.bool, device=eng.device)
    for s in range(S):
        pi = torch.as_tensor(partners[s]).to(eng.device)
        inv = torch.empty_like(pi)
        inv[pi] = torch.arange(D, **i64)
        rec_b = pi[dy].contiguous()
        base_b = (rec_b * W + wrep).contiguous()
        for i0, i1 in window_ranges(N, blk):
            sl = slice(i0, i1)
            both_bad[0, sl] = surrogate(sl, rec_b[sl], dict(R_base=R_base, base_a=base_a[sl], base_b=base_b[sl]), both[0, sl])
        # whole surrogates only: the B-anchored value of dyad d is the item of dyad pi^-1(d), wherever its block was
        both[1] = both[0].view(D, W, mv, mv, nv)[inv].view(N, mv, mv, nv)
        both_bad[1] = both_bad[0].view(D, W)[inv].view(N)
        acc.add(obs, both.view(2 * N, mv, mv, nv), both_bad.view(2 * N), slice(0, N), 2, s == S - 1)
        gmean[s] = both[0].view(D, W, mv, mv, nv).mean(dim=0)
        gbad[s] = both_bad[0].view(D, W).any(dim=0)
    return acc.group(obs.view(D, W, mv, mv, nv).mean(dim=0), gmean, gbad, S, obs_bad)


# ------------------------------------------------------------------ the tests (docstrings: the Engine methods)
def sliding_significance(eng, x, item_rec, item_start, n, p, freqs, fs, bands, *, measure, null, n_surrogates, seed, split=None,
                         min_shift=None, check=True, chunk=None, grid=None):
    _engine.no_auto_order(p, "sliding_significance")
    if null in sg.ENSEMBLE_NULLS:
        raise ValueError(f"null={null!r} is the test of event-locked ensembles (ensemble_significance); "
                         f"sliding_significance takes one of {sg.NULLS}")
    x = device_x(x)
    n_rec, m, T = x.shape
    n = int(n)
    S, split, min_shift = sg.significance_args(measure, null, n_surrogates, m, T, n, split, min_shift)
    if check is not True and check != "nan":
        raise ValueError(f"check must be True or 'nan', got {check!r}")
    eng.pad(m)
    eng.check_items(x, item_rec, item_start, n, p)
    W = int(item_rec.numel())
    f, F, lo, hi, nb, tested_h, tested = prepare(eng, freqs, bands, "sliding_significance", m, null, split)
    run = {"ffdtf": eng.sliding_ffdtf, "ddtf": eng.sliding_ddtf, "gpdc": eng.sliding_gpdc}[measure]
    acc = NullAccumulator(eng, W, m, nb, tested_h, tested)
    if W == 0:
        return acc.empty((0,))
    obs, obs_bad = observed_run(lambda c: run(x, item_rec, item_start, n, p, f, fs, bands=(lo, hi), check=c, grid=grid), check)
    surrogate_null(eng, acc, x, item_rec, item_start, n, null, S, seed, split, min_shift,
                   eng.significance_chunk(measure, null, W, m, n, p, F, nb) if chunk is None else chunk, obs,
                   lambda xs, rec, st: run(xs, rec, st, n, p, f, fs, bands=(lo, hi), check="mask", validate=False))
    return acc.result((W,), obs, obs_bad)


def ensemble_significance(eng, x, trial_rec, trial_start, group_ptr, item_group, item_offset, n, p, freqs, fs, bands, *, measure,
                          n_surrogates, seed, split=None, check=True, chunk=None, grid=None):
    if p is None:
        raise ValueError(_engine._NO_ENSEMBLE_ORDER)
    x = device_x(x)
    n_rec, m, T = x.shape
    n, p = int(n), int(p)
    S, split, _ = sg.significance_args(measure, "trial", n_surrogates, m, T, n, split)
    if check is not True and check != "nan":
        raise ValueError(f"check must be True or 'nan', got {check!r}")
    eng.pad(m)
    _engine.validate_trials(x, trial_rec, trial_start, group_ptr, item_group, item_offset, n, p)
    gp = group_ptr.cpu().numpy()
    counts = np.diff(gp)
    G, N = len(counts), int(item_group.numel())
    eng._ensemble_grid(G, (item_group, item_offset), N, grid, True)            # checked once, for both observed calls
    f, F, lo, hi, nb, tested_h, tested = prepare(eng, freqs, bands, "ensemble_significance", m, "trial", split)
    perms = sg.trial_permutations(np.random.default_rng(seed), S, counts)     # (also: every group has >= 2 trials)
    acc = NullAccumulator(eng, N, m, nb, tested_h, tested)
    if N == 0:
        return acc.empty((0,))
    ens = (x, trial_rec, trial_start, group_ptr, item_group, item_offset, n, p)
    obs, obs_bad = observed_run(lambda c: eng.sliding_ensemble(*ens, f, fs, measure=measure, bands=(lo, hi), grid=grid,
                                                               validate=False, check=c), check)
    R_base = eng.lagcov_ensemble(*ens, grid=grid, validate=False)
    # table B of every surrogate: the trials of each group in the order of its permutation
    rec_h, start_h = trial_rec.cpu().numpy(), trial_start.cpu().numpy()
    src = np.stack([np.concatenate([gp[g] + perms[s][g] for g in range(G)]) for s in range(S)])       # (S, trials)
    rec_b = torch.as_tensor(rec_h[src]).to(eng.device)
    start_b = torch.as_tensor(start_h[src]).to(eng.device)
    # the items group-major (a stable sort: nothing moves where they already are), so that a block of whole groups is
    # a contiguous run of items and of the running state
    order = torch.argsort(item_group, stable=True)
    grp, offs = item_group[order].contiguous(), item_offset[order].contiguous()
    first = np.searchsorted(grp.cpu().numpy(), np.arange(G + 1))           # items of group g: first[g] .. first[g+1]
    obs_s = obs[order].contiguous()
    chunk = eng.ensemble_significance_chunk(measure, m, n, p, F, nb) if chunk is None else max(1, int(chunk))
    i64 = dict(dtype=torch.int64, device=eng.device)
    for s0, sb, g0, g1, last in surrogate_blocks(S, *ensemble_plan(first, S, chunk)):
        i0, i1, e0, e1 = int(first[g0]), int(first[g1]), int(gp[g0]), int(gp[g1])
        wb, gb = i1 - i0, g1 - g0
        if wb == 0:
            continue
        srep = torch.arange(sb, **i64).repeat_interleave(wb)
        d = dict(trial_rec=trial_rec[e0:e1].repeat(sb), trial_start=trial_start[e0:e1].repeat(sb),
                 group_ptr=torch.as_tensor(np.concatenate([[0], np.cumsum(np.tile(counts[g0:g1], sb))]), **i64),
                 item_group=(grp[i0:i1] - g0).repeat(sb) + srep * gb, item_offset=offs[i0:i1].repeat(sb))
        shuffle = (rec_b[s0:s0 + sb, e0:e1].reshape(-1).contiguous(), start_b[s0:s0 + sb, e0:e1].reshape(-1).contiguous(),
                   split, R_base, order[i0:i1].repeat(sb))
        rt = eng._ensemble_route(measure, n, p, d["trial_rec"], d["trial_start"], d["group_ptr"], shuffle=shuffle)
        vals, bad = eng._sliding_call(rt, x, (d["item_group"], d["item_offset"]), f, fs, bands=(lo, hi), check="mask",
                                      chunk=min(sb * wb, chunk), validate=False)
        acc.add(obs_s[i0:i1], vals, bad, slice(i0, i1), sb, last)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(N, **i64)
    return acc.result((N,), obs, obs_bad, index=inv)


def ensemble_contrast(eng, x, trial_rec, trial_start, group_ptr, cond, offsets, n, p, freqs, fs, bands, *, measure, n_surrogates,
                      seed, tail="two-sided", split=None, group=None, check=True, chunk=None, grid=None):
    if p is None:
        raise ValueError(_engine._NO_ENSEMBLE_ORDER)
    x = device_x(x)
    n_rec, m, T = x.shape
    n, p = int(n), int(p)
    mp = eng.pad(m)
    i64 = dict(dtype=torch.int64, device=eng.device)
    if not (isinstance(cond, torch.Tensor) and cond.dim() == 1 and cond.numel() == trial_rec.numel()
            and not cond.dtype.is_floating_point):
        raise ValueError("cond must be a 1-D integer tensor with one entry per trial")
    gp = group_ptr.cpu().numpy()
    G, W = len(gp) - 1, int(offsets.numel())
    _engine.validate_trials(x, trial_rec, trial_start, group_ptr, torch.arange(G, **i64).repeat_interleave(W),
                            offsets.repeat(G), n, p)
    cond_h = cond.cpu().numpy().astype(np.int64)
    if ((cond_h != 0) & (cond_h != 1)).any():
        raise ValueError("cond must hold 0 (condition A) or 1 (condition B)")
    counts_a = [int((cond_h[gp[g]:gp[g + 1]] == 0).sum()) for g in range(G)]
    counts_b = [int((cond_h[gp[g]:gp[g + 1]] == 1).sum()) for g in range(G)]
    S, split = sg.contrast_args(measure, n_surrogates, m, tail, split, check, bands, counts_a, counts_b)
    eng._ensemble_grid(1, (torch.zeros(W, **i64), offsets), W, grid, True)
    f, F, lo, hi, nb, tested_h, tested = prepare(eng, freqs, bands, "ensemble_contrast", m,
                                                 "phase" if split is None else "shift", 0 if split is None else split)
    draws = sg.label_draws(np.random.default_rng(seed), S, counts_a, counts_b)
    acc = NullAccumulator(eng, G * W, m, nb, tested_h, tested)
    want_group = (G >= 2) if group is None else bool(group)
    stat = {"two-sided": torch.abs, "greater": lambda d: d, "less": torch.neg}[tail]
    if W == 0:
        return acc.empty((G, 0), ("observed_a", "observed_b"), group=want_group)
    chunk = eng.ensemble_contrast_chunk(measure, m, p, F, nb) if chunk is None else max(1, int(chunk))
    obs_ab = eng.empty(2, G, W, m, m, nb)
    obs_bad = torch.zeros(G, W, dtype=torch.bool, device=eng.device)
    if want_group:
        gsum = eng.empty(S, W, m, m, nb)
        gbad = torch.zeros(S, W, dtype=torch.bool, device=eng.device)
    per_window = (p + 1) * mp * mp * 8
    for g in range(G):
        e0, e1, EA, EB = int(gp[g]), int(gp[g + 1]), counts_a[g], counts_b[g]
        E = EA + EB
        pool = torch.as_tensor(e0 + np.argsort(cond_h[e0:e1], kind="stable")).to(eng.device)      # A's trials, then B's
        rec_g, start_g = trial_rec[pool].contiguous(), trial_start[pool].contiguous()
        # weight rows: 2 s = the trials relabelled A in surrogate s, 2 s + 1 = the others; the observed labels alike
        Wh = np.zeros((2 * S + 2, E))
        for s in range(S + 1):
            a = np.arange(EA) if s == S else draws[s][g]
            Wh[2 * s, a] = 1.0
            Wh[2 * s + 1] = 1.0 - Wh[2 * s]
        Wd = eng.to_device(Wh)
        sc = eng.to_device(np.tile([1.0 / EA, 1.0 / EB], S + 1))
        for w0, w1 in window_ranges(W, stack_plan(E, W, per_window, eng.max_workspace_bytes // 2)):
            wb = w1 - w0
            if grid is not None:        # a block of a regular grid is a regular grid that starts offsets[w0] later
                Rt = eng.lagcov_trials(x, rec_g, start_g + int(grid[0]) * w0, offsets[:wb], n, p, grid=(int(grid[0]), wb),
                                       validate=False)
            else:
                Rt = eng.lagcov_trials(x, rec_g, start_g, offsets[w0:w1].contiguous(), n, p, validate=False)
            run = dict(m=m, measure=measure, bands=(lo, hi), validate=False)
            try:
                o = eng.sliding_mix(Rt, Wd[2 * S:], sc[2 * S:], n, f, fs, check=True if check is True else "mask",
                                    chunk=min(chunk, 2 * wb), **run)
            except _engine.SingularMatrixError as err:
                err.group, err.windows = g, err.windows + w0
                err.args = (err.args[0], err.args[1] + f" (group {g}, condition {'AB'[int(err.rows[0])]}, window "
                            f"{int(err.windows[0])} of the observed labels)")
                raise
            if check is not True:
                o, bad = o
                obs_bad[g, w0:w1] = bad.view(2, wb).any(dim=0)
            obs_ab[:, g, w0:w1] = o.view(2, wb, m, m, nb)
            obs_t = stat(o[:wb] - o[wb:])
            Sb, _ = sliding_plan(S, 2 * wb, chunk)                  # a surrogate is two mix rows of every window
            for s0, sb, _, _, last in surrogate_blocks(S, Sb, [(w0, w1)]):
                vals, bad = eng.sliding_mix(Rt, Wd[2 * s0:2 * (s0 + sb)], sc[2 * s0:2 * (s0 + sb)], n, f, fs, check="mask",
                                            chunk=min(chunk, 2 * sb * wb), **run)
                vals, bad = vals.view(sb, 2, wb, m, m, nb), bad.view(sb, 2, wb).any(dim=1)
                d = vals[:, 0] - vals[:, 1]
                acc.add(obs_t, stat(d).view(sb * wb, m, m, nb), bad.reshape(sb * wb), slice(g * W + w0, g * W + w1), sb, last)
                if want_group:
                    if g == 0:
                        gsum[s0:s0 + sb, w0:w1] = d
                    else:
                        gsum[s0:s0 + sb, w0:w1] += d
                    gbad[s0:s0 + sb, w0:w1] |= bad
    obs_bad = None if check is True else obs_bad
    res = acc.result((G, W), obs_ab[0] - obs_ab[1], obs_bad, {"observed_a": obs_ab[0], "observed_b": obs_ab[1]})
    if want_group:
        gobs = obs_ab[0, 0] - obs_ab[1, 0]
        for g in range(1, G):                           # the order of the surrogates' sums
            gobs = gobs + (obs_ab[0, g] - obs_ab[1, g])
        gobs = gobs / G
        res["group"] = acc.group(gobs, stat(gsum / G), gbad, S, obs_bad, tested_value=stat(gobs))
    return res


def pseudo_dyad_significance(eng, x, item_start, n, p, freqs, fs, bands, *, measure, split=None, n_surrogates=None, seed=None,
                             check=True, chunk=None):
    _engine.no_auto_order(p, "pseudo_dyad_significance")
    D, m, T = x.shape
    n, p = int(n), int(p)
    S, split = sg.pseudo_dyad_args(measure, D, m, n_surrogates, seed, split, check)
    bands = band_bins(bands if bands is not None else ((), ()), "pseudo_dyad_significance")[:2]
    x = device_x(x)
    eng.pad(m)
    W = int(item_start.numel())
    dy, starts = dyad_items(eng, x, item_start, n, p)
    f, F, lo, hi, nb, tested_h, tested = prepare(eng, freqs, bands, "pseudo_dyad_significance", m, "shift", split)
    partners = sg.partner_derangements(None if S is None else np.random.default_rng(seed), S, D)
    acc = NullAccumulator(eng, D * W, m, nb, tested_h, tested)
    partners_out = torch.as_tensor(partners).to(eng.device)
    if W == 0:
        return dict(acc.empty((D, 0), group=True), partners=partners_out)
    run = {"ffdtf": eng.sliding_ffdtf, "ddtf": eng.sliding_ddtf, "gpdc": eng.sliding_gpdc}[measure]
    obs, obs_bad = observed_run(lambda c: run(x, dy, starts, n, p, f, fs, bands=(lo, hi), check=c, validate=False), check)

    def surrogate(sl, rec_b, base, out):            # the fused call writes the block's values where they belong
        return eng.sliding_pairs(x, dy[sl], rec_b, starts[sl], n, p, f, fs, measure=measure, split=split, bands=(lo, hi), out=out,
                                 check="mask", validate=False, **base)[1]
    group = partner_null(eng, acc, x, dy, starts, n, p, partners, chunk, obs, obs_bad, surrogate)
    return dict(acc.result((D, W), obs, obs_bad), group=group, partners=partners_out)


# ------------------------------------------------------------------ block Granger causality: two values per window
def block_meta(time, band_vals):
    """The block values of every item as a 2 x 2 "meta-channel" array for `hmv_null_accumulate_f64` (m = 2, channel 0 =
    block A, 1 = block B, cell [destination][source]): time (items, >= 2) with F_{A->B}, F_{B->A} in front and / or band_vals
    (items, 2, nb) with index 0 = A -> B -> (items, 2, 2, nv).  Cell [1][0] is A -> B, cell [0][1] is B -> A, the diagonal is
    NaN and never tested; the value columns are the time-domain value (if given), then the bands.  Pure tensor code."""
    cols = ([] if time is None else [time[:, :2, None]]) + ([] if band_vals is None else [band_vals])
    v = torch.cat(cols, dim=2)
    out = v.new_full((v.shape[0], 2, 2, v.shape[2]), float("nan"))
    out[:, 1, 0] = v[:, 0]
    out[:, 0, 1] = v[:, 1]
    return out


def block_leaves(res, values):
    """A `NullAccumulator` dict over meta arrays (..., 2, 2, nv) -> {"time": {observed, p, ... (..., 2)}, "bands": {...
    (..., 2, nb)}} for the leaves in `values`; index 0 = A -> B."""
    out, col = {}, 0
    per_dir = {k: torch.stack((res[k][..., 1, 0, :], res[k][..., 0, 1, :]), dim=-2) for k in ("observed",) + STATS}
    if "time" in values:
        out["time"] = {k: v[..., 0] for k, v in per_dir.items()}
        col = 1
    if "bands" in values:
        out["bands"] = {k: v[..., col:] for k, v in per_dir.items()}
    return out


def _block_test(eng, freqs, bands, values, who, N):
    """What the two block tests share around their loops -> (acc over N rows of the 2 x 2 meta array; the keywords of
    `sliding_block_granger_pairs` for `values`; f; finish(res, time, obs_bad, lead, group=None, **extra) -> the test's dict)."""
    tested_h = sg.tested_mask(2, "phase", 0)                         # the off-diagonal: the two directions
    tested = torch.as_tensor(tested_h.astype(np.uint8)).to(eng.device)
    f, bins, nv, want = None, None, 1, ("time",)
    if "bands" in values:
        f, _, lo, hi, nb, _, _ = prepare(eng, freqs, bands, who, 2, "phase", 0)
        bins, nv, want = (lo, hi), nb + int("time" in values), ("spectral", "time") if "time" in values else ("spectral",)
    acc = NullAccumulator(eng, N, 2, nv, tested_h, tested)

    def finish(res, time, obs_bad, lead, group=None, **extra):
        out = dict(block_leaves(res, values), n_valid=res["n_valid"], **extra)
        if group is not None:
            out["group"] = dict(block_leaves(group, values), n_valid=group["n_valid"])
        if "time" in values:
            out["observed_time"] = time.view(*lead, 4)
            if acc.failed(obs_bad):
                out["observed_time"][obs_bad.view(lead)] = float("nan")
        return out
    return acc, dict(want=want, bands=bins, validate=False), f, finish


def block_granger_significance(eng, x, item_rec, item_start, n, p, freqs, fs, bands, *, split, null, n_surrogates, seed,
                               values=sg.BLOCK_VALUES, min_shift=None, check=True, chunk=None):
    p = _engine.no_block_auto_order(p, "block_granger_significance")
    x = device_x(x)
    n_rec, m, T = x.shape
    n = int(n)
    S, split, min_shift, values = sg.block_significance_args(null, n_surrogates, m, T, n, split, min_shift, values, bands, check)
    eng.pad(m)
    eng.check_items(x, item_rec, item_start, n, p)
    W = int(item_rec.numel())
    acc, kw, f, finish = _block_test(eng, freqs, bands, values, "block_granger_significance", W)
    if W == 0:
        return finish(acc.empty((0,)), eng.empty(0, 4), None, (0,))

    def pairs(x, rec, st, **more):                  # the recording with itself: rec_b = rec_a
        return eng.sliding_block_granger_pairs(x, rec, rec, st, n, p, f, fs, split=split, **kw, **more)
    obs = pairs(x, item_rec, item_start, check=True if check is True else "mask")
    obs_bad = None if check is True else obs[2]
    obs_meta = block_meta(obs[1], obs[0])

    def surrogate(xs, rec, st):
        sp, tm, bad = pairs(xs, rec, st, check="mask")
        return block_meta(tm, sp), bad
    if chunk is None:
        F, nb = (0, 0) if f is None else (int(f.numel()), len(kw["bands"][0]))
        chunk = eng.block_significance_chunk(null, m, n, p, split, F, nb, kw["want"])
    surrogate_null(eng, acc, x, item_rec, item_start, n, null, S, seed, split, min_shift, chunk, obs_meta, surrogate)
    return finish(acc.result((W,), obs_meta, obs_bad), obs[1], obs_bad, (W,))


def block_granger_pseudo_dyad_significance(eng, x, item_start, n, p, freqs, fs, bands, *, split, n_surrogates=None, seed=None,
                                           values=sg.BLOCK_VALUES, check=True, chunk=None):
    p = _engine.no_block_auto_order(p, "block_granger_pseudo_dyad_significance")
    D, m, T = x.shape
    n = int(n)
    S, split, values = sg.block_pseudo_dyad_args(D, m, n_surrogates, seed, split, values, bands, check)
    x = device_x(x)
    eng.pad(m)
    W = int(item_start.numel())
    dy, starts = dyad_items(eng, x, item_start, n, p)
    acc, kw, f, finish = _block_test(eng, freqs, bands, values, "block_granger_pseudo_dyad_significance", D * W)
    timed = "time" in values
    partners = sg.partner_derangements(None if S is None else np.random.default_rng(seed), S, D)
    partners_out = torch.as_tensor(partners).to(eng.device)
    if W == 0:
        res = acc.empty((D, 0), group=True)
        return finish(res, eng.empty(0, 4), None, (D, 0), group=res.pop("group"), partners=partners_out)
    # the observed dyads through the same entry (rec_b = rec_a), which also hands out the restricted fits' log-determinants
    obs = eng.sliding_block_granger_pairs(x, dy, dy, starts, n, p, f, fs, split=split, return_red=timed,
                                          check=True if check is True else "mask", **kw)
    obs_bad = None if check is True else obs[-1]
    red = obs[2] if timed else None
    obs_meta = block_meta(obs[1], obs[0])

    def surrogate(sl, rec_b, base, out):
        sp, tm, bad = eng.sliding_block_granger_pairs(x, dy[sl], rec_b, starts[sl], n, p, f, fs, split=split, red_base=red,
                                                      check="mask", **kw, **base)
        out[:] = block_meta(tm, sp)
        return bad
    group = partner_null(eng, acc, x, dy, starts, n, p, partners, chunk, obs_meta, obs_bad, surrogate)
    return finish(acc.result((D, W), obs_meta, obs_bad), obs[1], obs_bad, (D, W), group=group, partners=partners_out)


# ------------------------------------------------------------------ phase synchrony: no model, the measures as value columns
def phase_calls(measures):
    """The kernel calls that fill the value columns `measures`: [(mode, (col_mag, col_lagged))], a column of -1 for a measure
    that was not asked for; one call per mode in use (PLV / ciPLV: unit phasors, coh / imcoh: the signal itself)."""
    calls = []
    for mode, names in phase.MODES:
        cols = tuple(measures.index(q) if q in measures else -1 for q in names)
        if max(cols) >= 0:
            calls.append((mode, cols))
    return calls


def phase_pairs(eng, calls, z, rec_a, rec_b, start, n, split, shift, out):
    """Every mode's call of `hmv_phase_sync_pairs_c128` into the columns of `out` (items, m, m, nq) -> info, the largest of
    the modes' (1 = a non-finite sample, in either mode)."""
    info = None
    for mode, cols in calls:
        i = eng._phase_sync_pairs(z, rec_a, rec_b, start, n, mode, split, shift, out, cols)[1]
        info = i if info is None else torch.maximum(info, i)
    return info


def phase_chunk(m: int, nq: int, max_workspace_bytes: int) -> int:
    """Items per pairs call: a quarter of the workspace over an item's values, tables and flags."""
    return max(1, (int(max_workspace_bytes) // 4) // (8 * m * m * nq + 64))


def _phase_leaves(res, measures, extra=()):
    """A `NullAccumulator` dict over (..., m, m, nq) -> {measure: {observed, p, p_fwe, null_mean, null_std (..., m, m)}}."""
    out = {k: res[k] for k in ("n_valid", *extra)}
    for i, q in enumerate(measures):
        out[q] = {k: res[k][..., i] for k in ("observed",) + STATS}
    return out


def phase_sync_significance(eng, x, item_rec, item_start, n, fs, bands_hz, *, measures, n_surrogates, seed, split=None,
                            min_shift=None, order=4, check=True, chunk=None, full=False, max_workspace_bytes=8 << 30):
    from .eeg_io import resolve_bands_hz
    who = "phase_sync_significance"
    phase.check_x(who, eng, x)
    n_rec, m, T = x.shape
    n = int(n)
    measures, S, split, min_shift = sg.phase_significance_args(measures, n_surrogates, m, T, n, split, min_shift, check)
    eng.pad(m)
    bands = resolve_bands_hz(bands_hz, fs)
    _engine.validate_items(x, item_rec, item_start, n, 0)
    nb, nq, W = len(bands), len(measures), int(item_rec.numel())
    calls = phase_calls(measures)
    tested_h = sg.tested_mask(m, "shift", split)
    tested = torch.as_tensor(tested_h.astype(np.uint8)).to(eng.device)
    keys = ("observed",) + STATS
    res = {k: eng.empty(W, nb, m, m, nq) for k in keys}
    res["n_valid"] = torch.zeros(W, nb, dtype=torch.int32, device=eng.device)
    info = torch.zeros(W, nb, dtype=torch.int32, device=eng.device)
    full_out = {q: eng.empty(W, nb, m, m) for q in measures} if full else None
    if W:
        # a draw may be T itself (min_shift = 0: the draws are from [min_shift, T - min_shift] with both ends); reading B T
        # samples later modulo T is reading it as it lies, and the kernel takes shifts in 0..T-1
        d_all = torch.as_tensor(sg.shift_offsets(np.random.default_rng(seed), S, n_rec, T, min_shift) % T).to(eng.device)
        resp = torch.stack([eng.band_response(T, fs, lo, hi, order) for lo, hi in bands])
        chunk = phase_chunk(m, nq, max_workspace_bytes) if chunk is None else max(1, int(chunk))
        for sel, b0, b1, z, rec_z, start_z in eng.phase_slabs(x, item_rec, item_start, resp, max_workspace_bytes):
            bs = b1 - b0
            start_z = start_z.contiguous()
            rec_x = item_rec[sel][:, None].expand(-1, bs).reshape(-1)                     # the row's recording in x: its draws
            N = int(rec_z.numel())
            Ws = N // bs
            obs = eng.empty(N, m, m, nq)
            info_s = phase_pairs(eng, calls, z, rec_z, rec_z, start_z, n, split, None, obs)
            info[sel, b0:b1] = info_s.view(Ws, bs)
            if check is True:                                # before any surrogate of the slab
                phase.raise_first_refused(who, info_s.view(Ws, bs), item_rec, item_start, bands, phase.SYNC_WHY,
                                          "returns that row as NaN", sel, b0)
            if full:
                for mode, cols in calls:
                    r = eng._phase_sync(z, rec_z, start_z, n, mode, cols[0] >= 0, cols[1] >= 0, False)
                    for key, c in zip(("mag", "lagged"), cols):
                        if c >= 0:
                            full_out[measures[c]][sel, b0:b1] = r[key].view(Ws, bs, m, m)
            acc = NullAccumulator(eng, N, m, nq, tested_h, tested)
            Sb, Wb = sliding_plan(S, N, chunk)
            vals = eng.empty(Sb * Wb, m, m, nq)
            for s0, sb, w0, w1, last in surrogate_blocks(S, Sb, window_ranges(N, Wb)):
                items = sb * (w1 - w0)
                rec_k, start_k = rec_z[w0:w1].repeat(sb), start_z[w0:w1].repeat(sb)
                shift = d_all[s0:s0 + sb][:, rec_x[w0:w1]].reshape(-1).contiguous()       # surrogate-major, as the items
                v = vals[:items]
                bad = phase_pairs(eng, calls, z, rec_k, rec_k, start_k, n, split, shift, v) == 1
                acc.add(obs[w0:w1], v, bad, slice(w0, w1), sb, last)
            del z
            res["observed"][sel, b0:b1] = obs.view(Ws, bs, m, m, nq)
            res["n_valid"][sel, b0:b1] = acc.st["n_valid"].view(Ws, bs)
            for k in STATS:
                res[k][sel, b0:b1] = acc.st[k].view(Ws, bs, m, m, nq)
        if check is not True:
            for k in keys:
                res[k][info != 0] = float("nan")
    out = dict(_phase_leaves(res, measures), tested=torch.as_tensor(tested_h).to(eng.device), info=info)
    if full:
        out["full"] = dict(full_out, info=info)
    return out


def phase_sync_pseudo_dyad_significance(eng, x, item_start, n, fs, bands_hz, *, measures, split=None, n_surrogates=None,
                                        seed=None, order=4, check=True, chunk=None, max_workspace_bytes=8 << 30):
    from .eeg_io import resolve_bands_hz
    who = "phase_sync_pseudo_dyad_significance"
    phase.check_x(who, eng, x)
    D, m, T = x.shape
    n = int(n)
    measures, S, split = sg.phase_pseudo_dyad_args(measures, D, m, n_surrogates, seed, split, check)
    eng.pad(m)
    bands = resolve_bands_hz(bands_hz, fs)
    need = 16 * m * T * (D + 2)                    # one band of every dyad, one recording's spectrum and one product
    if need > int(max_workspace_bytes):
        raise ValueError(f"{who}: the analytic signals of all {D} dyads of one band must be resident together, which needs "
                         f"{need} bytes; max_workspace_bytes is {int(max_workspace_bytes)}")
    W = int(item_start.numel())
    dy, starts = dyad_items(eng, x, item_start, n, 0)
    nb, nq, N = len(bands), len(measures), D * W
    calls = phase_calls(measures)
    tested_h = sg.tested_mask(m, "shift", split)
    tested = torch.as_tensor(tested_h.astype(np.uint8)).to(eng.device)
    partners = sg.partner_derangements(None if S is None else np.random.default_rng(seed), S, D)
    keys = ("observed",) + STATS
    res = {k: eng.empty(D, W, nb, m, m, nq) for k in keys}
    res["n_valid"] = torch.zeros(D, W, nb, dtype=torch.int32, device=eng.device)
    grp = {k: eng.empty(W, nb, m, m, nq) for k in keys}
    grp["n_valid"] = torch.zeros(W, nb, dtype=torch.int32, device=eng.device)
    info = torch.zeros(D, W, nb, dtype=torch.int32, device=eng.device)
    for b, (lo, hi) in enumerate(bands if W else ()):
        z = eng.analytic_signal(x, eng.band_response(T, fs, lo, hi, order))              # (D, m, T): every dyad of the band
        obs = eng.empty(N, m, m, nq)
        info_b = phase_pairs(eng, calls, z, dy, dy, starts, n, split, None, obs)
        info[:, :, b] = info_b.view(D, W)
        obs_bad = None
        if bool(info_b.any()):
            if check is True:
                it = int(torch.nonzero(info_b)[0])
                code = int(info_b[it])
                raise ValueError(f"{who}: dyad {it // W}, window at sample {int(starts[it])} (window {it % W}), band {b} "
                                 f"{bands[b]!r} Hz: info = {code} ({phase.SYNC_WHY.get(code, '?')}); check='nan' returns that "
                                 f"row as NaN")
            obs_bad = info_b != 0
        acc = NullAccumulator(eng, N, m, nq, tested_h, tested)

        def surrogate(sl, rec_b, base, out):
            return phase_pairs(eng, calls, z, dy[sl], rec_b, starts[sl], n, split, None, out) == 1
        g = partner_null(eng, acc, z, dy, starts, n, None, partners,
                         phase_chunk(m, nq, max_workspace_bytes) if chunk is None else chunk, obs, obs_bad, surrogate)
        r = acc.result((D, W), obs, obs_bad)
        for k in keys + ("n_valid",):
            res[k][:, :, b] = r[k]
            grp[k][:, b] = g[k]
        del z
    return dict(_phase_leaves(res, measures), tested=torch.as_tensor(tested_h).to(eng.device), info=info,
                partners=torch.as_tensor(partners).to(eng.device), group=_phase_leaves(grp, measures))
