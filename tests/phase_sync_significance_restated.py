"""NumPy restatement of the null tests of phase synchrony (`Engine.phase_sync_significance`,
`Engine.phase_sync_pseudo_dyad_significance`, include/hypermvar.h: hmv_phase_sync_pairs_c128): the surrogate written out --
participant A's rows as they lie, participant B's rows rolled by -shift or taken from another recording --, the measures of
tests/phase_sync_restated.py on it, and the p / p_fwe / mean / std formulas of hmv_null_accumulate_f64.  No GPU: shared by
tests/test_phase_sync_significance_cpu.py and tests/test_gpu_phase_sync_significance.py; nothing here is the code under test.

Why a shift surrogate needs no new analytic signal: z = ifft(fft(x) resp) is a circular filter and commutes with a circular
shift, so the analytic signal of the recording whose participant B is shifted by d samples is B's observed analytic signal
read d samples later, modulo T."""
import numpy as np

from tests import phase_sync_restated as PR

MEASURES = ("plv", "ciplv", "coh", "imcoh")
KEY = {"plv": (PR.UNIT, "mag"), "ciplv": (PR.UNIT, "lagged"), "coh": (PR.RAW, "mag"), "imcoh": (PR.RAW, "lagged")}
STATS = ("p", "p_fwe", "null_mean", "null_std")


def tested_mask(m, split):
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    return (i < split) != (j < split)


def written_out(z, rec_a, rec_b, shift, split):
    """The recording (m, T) of an item: rows < split of z[rec_a], rows >= split of z[rec_b] read `shift` samples later mod T."""
    w = np.array(z[rec_a], copy=True)
    w[split:] = np.roll(z[rec_b][split:], -int(shift), axis=-1)
    return w


def window_values(zw, start, n, measures):
    """(m, m, nq): the measures of the window start .. start + n of the written-out recording zw, and its info per mode."""
    res = {mode: PR.measures_restated(zw, start, n, mode) for mode in {KEY[q][0] for q in measures}}
    vals = np.stack([res[KEY[q][0]][KEY[q][1]] for q in measures], axis=-1)
    return vals, max(r["info"] for r in res.values())


def null_stats(obs, surr, tested, bad=None):
    """hmv_null_accumulate_f64 on the host: obs (rows, m, m, nv), surr (S, rows, m, m, nv), bad (S, rows) bool -> dict of
    p, p_fwe, null_mean, null_std (rows, m, m, nv; NaN on untested cells) and n_valid (rows,).  A bad surrogate is left out
    of everything; a NaN value is left out of count, mean and std of its cell but its surrogate still counts in n_valid and
    in p_fwe; M is the maximum over the tested cells, NaN skipped."""
    S, rows = surr.shape[:2]
    bad = np.zeros((S, rows), dtype=bool) if bad is None else np.asarray(bad, dtype=bool)
    ok = ~bad[:, :, None, None, None]
    with np.errstate(invalid="ignore"):
        M = np.where(tested[None, None, :, :, None] & ~np.isnan(surr), surr, -np.inf).max(axis=(2, 3))       # (S, rows, nv)
        n_valid = (~bad).sum(0)
        den = 1.0 + n_valid[:, None, None, None]
        use = ok & ~np.isnan(surr)
        cnt = (use & (surr >= obs[None])).sum(0)
        cnt_fwe = (ok & (M[:, :, None, None, :] >= obs[None])).sum(0)
        k = use.sum(0)
        v0 = np.where(use, surr, 0.0)
        mean = np.where(k > 0, v0.sum(0) / np.maximum(k, 1), np.nan)
        dev = np.where(use, surr - mean[None], 0.0)
        std = np.where(k > 1, np.sqrt((dev ** 2).sum(0) / np.maximum(k - 1, 1)), np.nan)
    out = {"p": (1.0 + cnt) / den, "p_fwe": (1.0 + cnt_fwe) / den, "null_mean": mean, "null_std": std}
    for a in out.values():
        a[:, ~tested] = np.nan
    out["n_valid"] = n_valid
    return out


def check_planted_significance(p, p_fwe, n_valid, S, seed):
    """The three statements about the planted dyad of tests/phase_sync_restated.py under the shift null with split 4 and S
    surrogates, on p, p_fwe (W, 8, 8, the four MEASURES): the lagged pair (0, 5) has the smallest possible p = p_fwe =
    1 / (1 + S) in every window for all four measures; the zero-lag pair (2, 6) has it for PLV and coherence; no other tested
    cell has p_fwe <= 0.05.  Prints the smallest other p_fwe."""
    assert (n_valid == S).all()
    small = 1.0 / (1.0 + S)
    hit = np.zeros(p.shape[1:], dtype=bool)
    for i, j in ((0, 5), (5, 0)):
        hit[i, j, :] = True
    for i, j in ((2, 6), (6, 2)):
        hit[i, j, MEASURES.index("plv")] = hit[i, j, MEASURES.index("coh")] = True
    assert np.array_equal(p[:, hit], np.full_like(p[:, hit], small)), seed
    assert np.array_equal(p_fwe[:, hit], np.full_like(p_fwe[:, hit], small)), seed
    tested = tested_mask(8, 4)
    other = tested[:, :, None] & ~hit
    assert np.isnan(p[:, ~tested]).all() and np.isnan(p_fwe[:, ~tested]).all()
    least = float(p_fwe[:, other].min())
    print(f"seed {seed}: smallest p_fwe outside the planted cells = {least:.3g}")
    assert least > 0.05, (seed, least)


def shift_test(z, starts, n, split, d, measures):
    """The shift test of one recording's analytic signal z (m, T) on the host: windows `starts`, draws d (S,) ->
    {observed, p, p_fwe, null_mean, null_std: (W, m, m, nq), n_valid (W,)}, observed NaN on untested cells."""
    m = z.shape[0]
    tested = tested_mask(m, split)
    obs = np.stack([window_values(z, s, n, measures)[0] for s in starts])
    surr = np.stack([np.stack([window_values(written_out(z[None], 0, 0, ds, split), s, n, measures)[0] for s in starts])
                     for ds in d])
    out = null_stats(obs, surr, tested)
    obs[:, ~tested] = np.nan
    out["observed"] = obs
    return out
