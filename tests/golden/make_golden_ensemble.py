"""Generate tests/golden/g10_ensemble.npz by RUNNING THE REFERENCE on (channels, samples, trials) input in the build container.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ensemble.py

The reference (`/root/reference/src/mtmvar.py`: full_freq_dtf, multivariate_spectra, direct_dtf,
gen_partial_directed_coherence, ar_coeff, mvar_criterion) is imported read-only; only seeded inputs and its OUTPUTS are
written.  The tests read the .npz only.  Layout: case <c> in ("a", "b") stores the recording `<c>__x` (m, T), the onsets
`<c>__onsets`, the scalars `<c>__p / n / hop / L / fs`, the frequency grid `<c>__freqs`, the stored window indices
`<c>__windows` (window w covers the samples onset + w * hop .. + n of every trial) and, per stored window in that order,
`<c>__ffdtf / spectra / ddtf / gpdc` (W, m, m, F), `<c>__ar` (W, m, m, p), `<c>__V` (W, m, m).  `criterion_error` is the
text of the ValueError of mvar_criterion on 3-D input.
"""
import io
import os
import sys
from contextlib import redirect_stdout

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from src import mtmvar as ref  # noqa: E402  (the reference itself)

# (m, p, n, trials, hop, epoch length, stored windows: None = every window)
CASES = {"a": (3, 1, 24, 12, 6, 120, None), "b": (8, 4, 60, 40, 10, 200, (0, 5, 9, 14))}
T = 1200
FS = 100.0
FREQS = np.linspace(1.0, 45.0, 8)


def signal(m, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, T))
    x[:, 1:] += 0.5 * x[:, :-1]
    x[1:] += 0.3 * x[:-1]
    return x


def main():
    out = {}
    for c, (m, p, n, E, hop, L, keep) in CASES.items():
        x = signal(m, T, 7 * m + p)
        onsets = np.sort(np.random.default_rng(1).choice(np.arange(0, T - L + 1), E, replace=False))
        n_win = (L - n) // hop + 1
        windows = np.arange(n_win) if keep is None else np.asarray(keep)
        res = {k: [] for k in ("ffdtf", "spectra", "ddtf", "gpdc", "ar", "V")}
        for w in windows:
            stack = np.stack([x[:, s + w * hop:s + w * hop + n] for s in onsets], axis=2)
            with redirect_stdout(io.StringIO()):
                res["ffdtf"].append(ref.full_freq_dtf(stack, FREQS, FS, optimal_model_order=p))
                res["spectra"].append(ref.multivariate_spectra(stack, FREQS, FS, optimal_model_order=p))
                res["ddtf"].append(ref.direct_dtf(stack, FREQS, FS, optimal_model_order=p))
                res["gpdc"].append(ref.gen_partial_directed_coherence(stack, FREQS, FS, optimal_model_order=p))
                ar, V = ref.ar_coeff(stack, p)
            res["ar"].append(ar)
            res["V"].append(V)
        out[f"{c}__x"] = x
        out[f"{c}__onsets"] = onsets.astype(np.int64)
        for k, v in (("p", p), ("n", n), ("hop", hop), ("L", L)):
            out[f"{c}__{k}"] = np.int64(v)
        out[f"{c}__fs"] = np.float64(FS)
        out[f"{c}__freqs"] = FREQS
        out[f"{c}__windows"] = windows.astype(np.int64)
        for k, v in res.items():
            out[f"{c}__{k}"] = np.stack(v)
    try:
        with redirect_stdout(io.StringIO()):
            ref.mvar_criterion(np.zeros((3, 24, 4)), 5, "AIC")
        raise SystemExit("mvar_criterion accepted 3-D input: the fixture's premise does not hold")
    except ValueError as e:
        out["criterion_error"] = np.array(str(e))
    path = os.path.join(HERE, "g10_ensemble.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
