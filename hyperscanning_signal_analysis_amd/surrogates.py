"""Host side of the surrogate significance tests: argument checks, the random draws and the tested family.  Pure NumPy,
so that every surrogate can be rebuilt on the host from the seed.  The draws are consumed by `significance.py`, which
drives the four tests (`Engine.sliding_significance`, `.ensemble_significance`, `.pseudo_dyad_significance`,
`.ensemble_contrast`); where and how often each is drawn relative to the others is part of the result's bits.

All randomness comes from `rng = numpy.random.default_rng(seed)`, in this order:
    null="shift":  d = rng.integers(min_shift, T - min_shift, size=(S, n_rec), endpoint=True)        (once; also the draws of
                   `Engine.phase_sync_significance`, whose pseudo-dyad test takes the partners below)
    null="phase":  phi = 2 pi rng.random((S, m, n // 2 + 1)), phi[..., 0] = 0, phi[..., n // 2] = 0 for even n
                   (drawn in consecutive surrogate blocks: one double per draw, so the stream is the same)
    null="trial":  for s = 0..S-1, then g = 0..G-1: pi[s][g] = rng.permutation(counts[g]), drawn again while it is the
                   identity (`trial_permutations`; event-locked ensembles only)
    pseudo dyads:  for s = 0..S-1: pi[s] = rng.permutation(D), drawn again while any pi[s][d] == d (`partner_derangements`
                   with an integer S; `Engine.pseudo_dyad_significance` only).  S = None draws nothing: the exhaustive set is
                   the D - 1 cyclic offsets pi[k-1][d] = (d + k) mod D, k = 1..D-1, and no seed is used
    contrast:      for s = 0..S-1, then g = 0..G-1: a[s][g] = sort(rng.permutation(E_g)[:EA_g]), the positions of the pooled
                   trials of group g (its EA_g trials of condition A, then its EB_g of condition B; E_g = EA_g + EB_g) that
                   surrogate s labels A, drawn again while it is the observed set 0..EA_g-1 (`label_draws`;
                   `Engine.ensemble_contrast` only)
"""
from __future__ import annotations

import numpy as np

__all__ = ["NULLS", "ENSEMBLE_NULLS", "MEASURES", "TAILS", "significance_args", "shift_offsets", "phase_draws",
           "trial_permutations", "label_draws", "contrast_args", "partner_count", "partner_derangements", "pseudo_dyad_args",
           "tested_mask", "check_significance_dict", "BLOCK_VALUES", "BLOCK_WANT", "block_want", "block_values",
           "block_significance_args", "block_pseudo_dyad_args", "phase_significance_args", "phase_pseudo_dyad_args"]

NULLS = ("shift", "phase")          # of continuous recordings (`sliding_significance`)
ENSEMBLE_NULLS = ("trial",)         # of event-locked ensembles (`ensemble_significance`)
MEASURES = ("ffdtf", "ddtf", "gpdc")
BLOCK_VALUES = ("time", "bands")    # of the block Granger tests: the time-domain value, the band sums of the spectral one
BLOCK_WANT = ("spectral", "time")   # outputs of `Engine.sliding_block_granger_pairs`
TAILS = ("two-sided", "greater", "less")    # of the condition contrast: T = |D|, D, -D with D = band(A) - band(B)


def _int(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def significance_args(measure, null, n_surrogates, m, T, n, split=None, min_shift=None):
    """Check the arguments of a significance run BEFORE anything is drawn or launched; returns (S, split, min_shift) with
    the defaults filled in: split = m // 2 for even m (odd m must pass it; the phase null does not use it), min_shift = n
    (the window length).  ValueError for an unknown measure or null, S < 1, a split outside 1..m-1 and, under the shift
    null, T < 2 min_shift.  null="trial" (the trial shuffle of an event-locked ensemble) takes the split of the shift
    null and uses neither T nor min_shift."""
    if measure not in MEASURES:
        raise ValueError(f"measure must be one of {MEASURES}, got {measure!r}")
    if null not in NULLS + ENSEMBLE_NULLS:
        raise ValueError(f"null must be one of {NULLS + ENSEMBLE_NULLS}, got {null!r}")
    S = _int(n_surrogates, "n_surrogates")
    if S < 1:
        raise ValueError(f"n_surrogates must be >= 1, got {S}")
    m, T, n = int(m), int(T), int(n)
    if split is None:
        if null in ("shift", "trial") and m % 2:
            raise ValueError(f"an odd channel count ({m}) needs an explicit split")
        split = m // 2
    else:
        split = _int(split, "split")
    if null in ("shift", "trial") and not 1 <= split <= m - 1:
        raise ValueError(f"split must be in 1..{m - 1}, got {split}")
    if null == "phase" and not 0 <= split <= m:
        raise ValueError(f"split must be in 0..{m}, got {split}")
    min_shift = n if min_shift is None else _int(min_shift, "min_shift")
    if min_shift < 0:
        raise ValueError(f"min_shift must be >= 0, got {min_shift}")
    if null == "shift" and T < 2 * min_shift:
        raise ValueError(f"the shift null needs T >= 2 min_shift (T = {T}, min_shift = {min_shift})")
    return S, split, min_shift


def shift_offsets(rng, S: int, n_rec: int, T: int, min_shift: int):
    """(S, n_rec) int64 circular shifts of the second participant, in [min_shift, T - min_shift]."""
    return np.asarray(rng.integers(min_shift, T - min_shift, size=(S, n_rec), endpoint=True), dtype=np.int64)


def phase_draws(rng, S: int, m: int, n: int):
    """(S, m, n // 2 + 1) phases of the next S surrogates; 0 at bin 0 and, for even n, at bin n / 2."""
    phi = 2.0 * np.pi * rng.random((S, m, n // 2 + 1))
    phi[..., 0] = 0.0
    if n % 2 == 0:
        phi[..., n // 2] = 0.0
    return phi


def trial_permutations(rng, S: int, counts):
    """The trial shuffles of S surrogates: perms[s][g] = rng.permutation(counts[g]), drawn for s = 0..S-1 and inside a
    surrogate for g = 0..G-1, in that order.  Trial e of group g (participant A, channels < split) is paired with trial
    perms[s][g][e] of the same group (participant B).  A draw that is the identity is drawn again: it is the observed
    arrangement, which the (1 + count) / (1 + n_valid) estimator already counts.  ValueError for a group of fewer than
    2 trials, which has no other arrangement."""
    counts = [int(c) for c in counts]
    for g, c in enumerate(counts):
        if c < 2:
            raise ValueError(f"the trial shuffle needs at least 2 trials per group, group {g} has {c}")
    perms = []
    for _ in range(int(S)):
        row = []
        for c in counts:
            pi = rng.permutation(c)
            while np.array_equal(pi, np.arange(c)):
                pi = rng.permutation(c)
            row.append(np.asarray(pi, dtype=np.int64))
        perms.append(row)
    return perms


def label_draws(rng, S: int, counts_a, counts_b):
    """The relabellings of S surrogates of the condition contrast: draws[s][g] = np.sort(rng.permutation(E_g)[:EA_g]) with
    E_g = counts_a[g] + counts_b[g], drawn for s = 0..S-1 and inside a surrogate for g = 0..G-1, in that order -- the
    positions in group g's pool (A's trials, then B's) that surrogate s labels A; the others are labelled B, so both group
    sizes are kept.  A draw equal to the observed set 0..EA_g-1 is drawn again: it is the observed labelling, which the
    (1 + count) / (1 + n_valid) estimator already counts.  ValueError for a group with an empty condition."""
    counts_a, counts_b = [int(c) for c in counts_a], [int(c) for c in counts_b]
    if len(counts_a) != len(counts_b):
        raise ValueError("counts_a and counts_b must have one entry per group each")
    for g, (ea, eb) in enumerate(zip(counts_a, counts_b)):
        if ea < 1 or eb < 1:
            raise ValueError(f"the condition contrast needs at least one trial of each condition per group, group {g} has "
                             f"{ea} of A and {eb} of B")
    draws = []
    for _ in range(int(S)):
        row = []
        for ea, eb in zip(counts_a, counts_b):
            a = np.sort(rng.permutation(ea + eb)[:ea])
            while np.array_equal(a, np.arange(ea)):
                a = np.sort(rng.permutation(ea + eb)[:ea])
            row.append(np.asarray(a, dtype=np.int64))
        draws.append(row)
    return draws


def contrast_args(measure, n_surrogates, m, tail, split, check, bands, counts_a, counts_b):
    """Check the arguments of a condition contrast BEFORE anything is drawn or launched; returns (S, split), split None
    (every pair i != j is tested) or the integer in 1..m-1 (the inter-brain pairs are).  ValueError for an unknown measure
    or tail, S < 1, a split outside 1..m-1, a `check` other than True / "nan", bands that are not (bin_lo, bin_hi) with at
    least one band, no group, and a group with an empty condition."""
    if measure not in MEASURES:
        raise ValueError(f"measure must be one of {MEASURES}, got {measure!r}")
    if tail not in TAILS:
        raise ValueError(f"tail must be one of {TAILS}, got {tail!r}")
    S = _int(n_surrogates, "n_surrogates")
    if S < 1:
        raise ValueError(f"n_surrogates must be >= 1, got {S}")
    m = int(m)
    if split is not None:
        split = _int(split, "split")
        if not 1 <= split <= m - 1:
            raise ValueError(f"split must be in 1..{m - 1}, got {split}")
    if check is not True and check != "nan":
        raise ValueError(f"check must be True or 'nan', got {check!r}")
    if bands is None or len(bands) != 2 or len(np.atleast_1d(bands[0])) < 1 or \
            len(np.atleast_1d(bands[0])) != len(np.atleast_1d(bands[1])):
        raise ValueError("the condition contrast needs bands = (bin_lo, bin_hi) with at least one band")
    counts_a, counts_b = list(counts_a), list(counts_b)
    if len(counts_a) != len(counts_b) or len(counts_a) < 1:
        raise ValueError("the condition contrast needs at least one group, with both conditions")
    for g, (ea, eb) in enumerate(zip(counts_a, counts_b)):
        if int(ea) < 1 or int(eb) < 1:
            raise ValueError(f"the condition contrast needs at least one trial of each condition per group, group {g} has "
                             f"{int(ea)} of A and {int(eb)} of B")
    return S, split


def _n_dyads(D):
    D = _int(D, "the number of dyads")
    if D < 2:
        raise ValueError(f"the pseudo-dyad test needs at least 2 dyads, got {D}")
    return D


def partner_count(n_surrogates, seed=None, *, seeded=True):
    """The number of partner sets asked for: None for the exhaustive set, else the integer S >= 1.  ValueError for S < 1 and,
    with `seeded`, for an integer S without a seed."""
    if n_surrogates is None:
        return None
    S = _int(n_surrogates, "n_surrogates")
    if S < 1:
        raise ValueError(f"n_surrogates must be >= 1, got {S}")
    if seeded and seed is None:
        raise ValueError("seeded partner draws (an integer n_surrogates) need a seed; n_surrogates=None takes the "
                         "exhaustive set of cyclic offsets")
    return S


def partner_derangements(rng, S, D: int):
    """(S, D) int64 partners of the pseudo-dyad test: in surrogate s participant A of dyad d is analysed with participant
    B of dyad pi[s][d] != d.  S = None: the exhaustive set of the D - 1 cyclic offsets pi[k-1][d] = (d + k) mod D -- every
    ordered pair (d, j != d) exactly once, every other partner once on each side; `rng` is not used.  An integer S >= 1:
    pi[s] = rng.permutation(D) for s = 0..S-1 in that order, drawn again while it has a fixed point (a dyad paired with
    itself is the observed arrangement).  ValueError for D < 2, which has no other partner, and for S < 1."""
    D = _n_dyads(D)
    d = np.arange(D, dtype=np.int64)
    S = partner_count(S, seeded=False)
    if S is None:
        return np.stack([(d + k) % D for k in range(1, D)])
    if rng is None:
        raise ValueError("seeded partner draws need a random generator")
    out = np.empty((S, D), dtype=np.int64)
    for s in range(S):
        pi = rng.permutation(D)
        while np.any(pi == d):
            pi = rng.permutation(D)
        out[s] = pi
    return out


def pseudo_dyad_args(measure, D, m, n_surrogates, seed, split=None, check=True):
    """Check the arguments of a pseudo-dyad run BEFORE anything is drawn or launched; returns (S or None, split) with the
    default split = m // 2 for even m filled in.  ValueError for an unknown measure, fewer than 2 dyads, an odd channel
    count without a split, a split outside 1..m-1, an integer n_surrogates < 1 or without a seed, a `check` other than
    True / "nan"."""
    if measure not in MEASURES:
        raise ValueError(f"measure must be one of {MEASURES}, got {measure!r}")
    _n_dyads(int(D))
    S = partner_count(n_surrogates, seed)
    m = int(m)
    if split is None:
        if m % 2:
            raise ValueError(f"an odd channel count ({m}) needs an explicit split")
        split = m // 2
    else:
        split = _int(split, "split")
    if not 1 <= split <= m - 1:
        raise ValueError(f"split must be in 1..{m - 1}, got {split}")
    if check is not True and check != "nan":
        raise ValueError(f"check must be True or 'nan', got {check!r}")
    return S, split


def tested_mask(m: int, null: str, split: int):
    """(m, m) bool: the pairs a null tests.  shift and trial: exactly one index < split (the inter-brain pairs); phase:
    i != j."""
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    if null in ("shift", "trial"):
        return (i < split) != (j < split)
    return i != j


def check_significance_dict(sig):
    """escan_batch.run(significance=...): dict(null=..., n_surrogates=..., seed=..., min_shift=None), checked before
    anything is read.  Returns a normalised copy."""
    if not isinstance(sig, dict):
        raise ValueError(f"significance must be a dict(null=..., n_surrogates=..., seed=..., min_shift=None), got {sig!r}")
    allowed = {"null", "n_surrogates", "seed", "min_shift"}
    extra = sorted(set(sig) - allowed)
    missing = sorted({"null", "n_surrogates", "seed"} - set(sig))
    if extra or missing:
        raise ValueError(f"significance: unknown keys {extra}, missing keys {missing}")
    if sig["null"] not in NULLS:
        raise ValueError(f"significance: null must be one of {NULLS}, got {sig['null']!r}")
    S = _int(sig["n_surrogates"], "significance: n_surrogates")
    if S < 1:
        raise ValueError(f"significance: n_surrogates must be >= 1, got {S}")
    seed = _int(sig["seed"], "significance: seed")
    ms = sig.get("min_shift")
    if ms is not None and _int(ms, "significance: min_shift") < 0:
        raise ValueError(f"significance: min_shift must be >= 0, got {ms}")
    return {"null": sig["null"], "n_surrogates": S, "seed": seed, "min_shift": None if ms is None else int(ms)}


# ------------------------------------------------------------------ block Granger causality (two values per window)
def _subset(given, allowed, name):
    given = (given,) if isinstance(given, str) else tuple(given)
    if not given or len(set(given)) != len(given) or any(v not in allowed for v in given):
        raise ValueError(f"{name} must be a non-empty selection of {allowed} without repeats, got {given!r}")
    return given


def block_want(want):
    """want of `Engine.sliding_block_granger_pairs` -> (spectral, time) booleans; ValueError for anything that is not a
    non-empty selection of "spectral" and "time"."""
    want = _subset(want, BLOCK_WANT, "want")
    return "spectral" in want, "time" in want


def block_values(values, bands):
    """values of the block Granger tests, in the order of the value columns: the time-domain value first, then the band
    sums.  ValueError for anything that is not a non-empty selection of "time" and "bands", and for "bands" without
    bands = (bin_lo, bin_hi) of at least one band."""
    values = _subset(values, BLOCK_VALUES, "values")
    if "bands" in values and (bands is None or len(bands) != 2 or len(np.atleast_1d(bands[0])) < 1
                              or len(np.atleast_1d(bands[0])) != len(np.atleast_1d(bands[1]))):
        raise ValueError('values with "bands" needs bands = (bin_lo, bin_hi) with at least one band')
    return tuple(v for v in BLOCK_VALUES if v in values)


def _block_split(split, m):
    split = _int(split, "split")
    if not 1 <= split <= int(m) - 1:
        raise ValueError(f"split must be in 1..{int(m) - 1}, got {split}")
    return split


def _check_mode(check):
    if check is not True and check != "nan":
        raise ValueError(f"check must be True or 'nan', got {check!r}")


def block_significance_args(null, n_surrogates, m, T, n, split, min_shift=None, values=BLOCK_VALUES, bands=None, check=True):
    """Check the arguments of `Engine.block_granger_significance` BEFORE anything is drawn or launched; returns
    (S, split, min_shift, values) with min_shift = n filled in and `values` in column order.  The split is that of the
    blocks and has no default; both nulls need it.  ValueError for a null outside NULLS, S < 1, a split outside 1..m-1, T < 2
    min_shift under the shift null, ill-formed values / bands and a `check` other than True / "nan"."""
    if null not in NULLS:
        raise ValueError(f"null must be one of {NULLS}, got {null!r}")
    S = _int(n_surrogates, "n_surrogates")
    if S < 1:
        raise ValueError(f"n_surrogates must be >= 1, got {S}")
    split = _block_split(split, m)
    min_shift = int(n) if min_shift is None else _int(min_shift, "min_shift")
    if min_shift < 0:
        raise ValueError(f"min_shift must be >= 0, got {min_shift}")
    if null == "shift" and int(T) < 2 * min_shift:
        raise ValueError(f"the shift null needs T >= 2 min_shift (T = {int(T)}, min_shift = {min_shift})")
    _check_mode(check)
    return S, split, min_shift, block_values(values, bands)


def _default_split(split, m):
    m = int(m)
    if split is None:
        if m % 2:
            raise ValueError(f"an odd channel count ({m}) needs an explicit split")
        return m // 2
    return _block_split(split, m)


def phase_significance_args(measures, n_surrogates, m, T, n, split=None, min_shift=None, check=True):
    """Check the arguments of `Engine.phase_sync_significance` BEFORE anything is drawn or launched; returns (measures, S,
    split, min_shift) with the measures resolved (`eeg_io.resolve_phase_measures`) and the defaults filled in: split = m // 2
    for even m (odd m must pass it), min_shift = n (the window length).  ValueError for unknown or no measures, S < 1, a split
    outside 1..m-1, min_shift < 0, T < 2 min_shift and a `check` other than True / "nan"."""
    from .eeg_io import resolve_phase_measures
    measures = resolve_phase_measures(measures)
    S = _int(n_surrogates, "n_surrogates")
    if S < 1:
        raise ValueError(f"n_surrogates must be >= 1, got {S}")
    split = _default_split(split, m)
    min_shift = int(n) if min_shift is None else _int(min_shift, "min_shift")
    if min_shift < 0:
        raise ValueError(f"min_shift must be >= 0, got {min_shift}")
    if int(T) < 2 * min_shift:
        raise ValueError(f"the shift null needs T >= 2 min_shift (T = {int(T)}, min_shift = {min_shift})")
    _check_mode(check)
    return measures, S, split, min_shift


def phase_pseudo_dyad_args(measures, D, m, n_surrogates, seed, split=None, check=True):
    """Check the arguments of `Engine.phase_sync_pseudo_dyad_significance` BEFORE anything is drawn or launched; returns
    (measures, S or None, split).  ValueError for unknown or no measures, fewer than 2 dyads, an odd channel count without a
    split, a split outside 1..m-1, an integer n_surrogates < 1 or without a seed and a `check` other than True / "nan"."""
    from .eeg_io import resolve_phase_measures
    measures = resolve_phase_measures(measures)
    _n_dyads(int(D))
    S = partner_count(n_surrogates, seed)
    split = _default_split(split, m)
    _check_mode(check)
    return measures, S, split


def block_pseudo_dyad_args(D, m, n_surrogates, seed, split, values=BLOCK_VALUES, bands=None, check=True):
    """Check the arguments of `Engine.block_granger_pseudo_dyad_significance` BEFORE anything is drawn or launched; returns
    (S or None, split, values).  ValueError for fewer than 2 dyads, a split outside 1..m-1, an integer n_surrogates < 1 or
    without a seed, ill-formed values / bands and a `check` other than True / "nan"."""
    _n_dyads(int(D))
    S = partner_count(n_surrogates, seed)
    split = _block_split(split, m)
    _check_mode(check)
    return S, split, block_values(values, bands)
