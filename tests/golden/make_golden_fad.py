"""Generate tests/golden/g9_fad.npz by RUNNING THE REFERENCE's FAD decomposition in the build container.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fad.py

The reference (`/root/reference/src/mtmvar.py`: fad_decomposition, mvar_criterion, ar_coeff) and
scipy.signal.residuez are imported read-only; only seeded inputs and their OUTPUTS are written.  The GPU tests read
the .npz only.  Layout: every case <c> stores its inputs under `<c>__in_*` and the reference's dict under
`<c>__<key>` (`<c>__pc_<key>` for paired_components), the criterion curve in automatic mode (`<c>__crit`), the
printed line (`<c>__printed`) and the condition number of the Toeplitz matrix of the fit (`<c>__kappa`).
Decomposition-only cases `d_<name>` store AR coefficients and residuez's (C, poles).
"""
import io
import os
import sys
from contextlib import redirect_stdout

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
import numpy as np
from scipy.linalg import toeplitz
from scipy.signal import lfilter, residuez

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from src import mtmvar as ref  # noqa: E402  (the reference itself)

KEYS = ("poles", "C", "alpha", "freq_hz", "omega_rad_s", "beta", "bandwidth_hz", "phi", "B", "osc_mask", "ar_coeffs")
PC_KEYS = ("pole_index", "poles", "C", "alpha", "freq_hz", "omega_rad_s", "beta", "bandwidth_hz", "phi", "B")
CRIT = {"AIC": 0, "HQ": 1, "SC": 2}


def ar_signal(seed, poles_hz, radii, fs, n, burn=500, extra_real=()):
    rng = np.random.default_rng(seed)
    z = []
    for f, r in zip(poles_hz, radii):
        w = r * np.exp(2j * np.pi * f / fs)
        z += [w, np.conj(w)]
    z += list(extra_real)
    a = np.real(np.poly(z))                         # [1, -a_1, .., -a_p]
    e = rng.standard_normal(n + burn)
    return lfilter([1.0], a, e)[burn:]


def kappa(x, p):
    n = len(x)
    r = np.array([x[:n - k] @ x[k:] / n for k in range(p + 1)])
    return float(np.linalg.cond(toeplitz(r[:p])))


def main():
    out = {}

    def run(name, x, fs, model_order=None, max_model_order=20, crit_type="AIC", pair_conjugates=True):
        buf = io.StringIO()
        with redirect_stdout(buf):
            d = ref.fad_decomposition(x, fs, model_order=model_order, max_model_order=max_model_order,
                                      crit_type=crit_type, pair_conjugates=pair_conjugates)
        out[f"{name}__in_x"] = np.asarray(x, dtype=np.float64)
        out[f"{name}__in_fs"] = np.float64(fs)
        out[f"{name}__in_model_order"] = np.int64(0 if model_order is None else model_order)
        out[f"{name}__in_max_model_order"] = np.int64(max_model_order)
        out[f"{name}__in_crit"] = np.int64(CRIT[crit_type])
        out[f"{name}__in_pair"] = np.bool_(pair_conjugates)
        out[f"{name}__model_order"] = np.int64(d["model_order"])
        out[f"{name}__noise_variance"] = np.float64(d["noise_variance"])
        for k in KEYS:
            out[f"{name}__{k}"] = np.asarray(d[k])
        for k in PC_KEYS:
            out[f"{name}__pc_{k}"] = np.asarray(d["paired_components"][k])
        out[f"{name}__printed"] = np.array(buf.getvalue())
        out[f"{name}__kappa"] = np.float64(kappa(np.ravel(x), int(d["model_order"])))
        if model_order is None:
            with redirect_stdout(io.StringIO()):
                crit, _, _ = ref.mvar_criterion(np.atleast_2d(x), max_model_order, crit_type)
            out[f"{name}__crit"] = crit

    fs = 250.0
    x6 = ar_signal(9, (10.0, 22.0, 3.0), (0.97, 0.93, 0.95), fs, 2000)
    run("ar6_p8", x6, fs, model_order=8)
    for c in ("AIC", "HQ", "SC"):
        run(f"ar6_{c.lower()}", x6, fs, crit_type=c)
    run("short", ar_signal(10, (12.0, 40.0), (0.9, 0.85), fs, 200), fs)
    run("unpaired", x6, fs, model_order=8, pair_conjugates=False)
    run("negpole", ar_signal(11, (15.0,), (0.9,), fs, 1500, extra_real=(-0.8, 0.5)), fs, model_order=4)

    # the reference looped over the windows x channels of an 8-channel recording (_create_windows geometry:
    # 3 windows of 1000 samples spread over 2600)
    rng = np.random.default_rng(12)
    rec = np.stack([ar_signal(100 + c, (rng.uniform(4, 40), rng.uniform(40, 90)), (0.95, 0.9), fs, 2600)
                    for c in range(8)])
    starts = np.linspace(0, 2600 - 1000, 3, dtype=int)
    out["rec__in_x"] = rec
    out["rec__in_starts"] = starts
    out["rec__in_window"] = np.int64(1000)
    P = 20
    ref_rows = {k: np.full((3, 8, P), np.nan, dtype=complex if k in ("poles", "C", "alpha") else float) for k in KEYS}
    orders = np.zeros((3, 8), dtype=np.int64)
    noise = np.zeros((3, 8))
    for w, s0 in enumerate(starts):
        for c in range(8):
            with redirect_stdout(io.StringIO()):
                d = ref.fad_decomposition(rec[c, s0:s0 + 1000], fs)
            p = int(d["model_order"])
            orders[w, c] = p
            noise[w, c] = d["noise_variance"]
            for k in KEYS:
                ref_rows[k][w, c, :p] = d[k]
    out["rec__model_order"] = orders
    out["rec__noise_variance"] = noise
    for k in KEYS:
        out[f"rec__{k}"] = ref_rows[k]

    # decomposition only: residuez on given coefficients
    def dec(name, a):
        a = np.asarray(a, dtype=np.float64)
        C, z, _ = residuez([1.0], np.r_[1.0, -a])
        out[f"d_{name}__ar"] = a
        out[f"d_{name}__C"] = C
        out[f"d_{name}__poles"] = z

    drng = np.random.default_rng(13)
    for p in (1, 2, 3, 8, 16, 20, 32):
        nc = p // 2
        ang = drng.uniform(0.05, 3.0, nc)
        rad = drng.uniform(0.3, 0.97, nc)
        z = list(rad * np.exp(1j * ang)) + list(rad * np.exp(-1j * ang))
        z += list(drng.uniform(-0.9, 0.9, p - 2 * nc))
        dec(f"rand{p}", -np.real(np.poly(z))[1:])
    w = 0.8 * np.exp(0.5j)
    dec("double_real", -np.real(np.poly([0.6, 0.6, -0.3, w, np.conj(w)]))[1:])
    dec("double_pair", -np.real(np.poly([w, w, np.conj(w), np.conj(w), 0.3]))[1:])
    dec("grouped", -np.real(np.poly([0.6, 0.6005, 0.9 * np.exp(1j), 0.9 * np.exp(-1j)]))[1:])
    dec("odd7", -np.real(np.poly([0.95 * np.exp(0.2j), 0.95 * np.exp(-0.2j), 0.7 * np.exp(2.0j), 0.7 * np.exp(-2.0j),
                                  0.4, -0.5, 0.1]))[1:])

    path = os.path.join(HERE, "g9_fad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
