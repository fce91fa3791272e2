"""NumPy restatement of the phase-synchrony formulas of include/hypermvar.h (hmv_phase_sync_c128), of the analytic signal
z = ifft(fft(x) * resp), the derived rounding bound the GPU tests hold the kernel to, and the planted dyad.  `resp` is an
input: `eeg_io.band_response` is not restated here.  No GPU: shared by tests/test_phase_sync_cpu.py and
tests/test_gpu_phase_sync.py.

    UNIT (0):  u_i[t] = z_i[t] / |z_i[t]|  (0 where |z_i[t]| == 0)        RAW (1):  u_i[t] = z_i[t]
    C_ij = sum_t u_i[t] conj(u_j[t])
    UNIT:  R = C / n                   mag = |R| (PLV)         lagged = ciPLV = den > 0 ? min(1, |Im R| / sqrt(den)) : 0
    RAW:   R = C / sqrt(C_ii C_jj)     mag = |R| (coherence)   lagged = |Im R|              den = 1 - (Re R)^2
    diagonal: Im R = 0; mag = 1, lagged = 0 where the channel has a non-zero sample in the window."""
import numpy as np

EPS = 2.0 ** -52
UNIT, RAW = 0, 1
FS, BAND, WINDOW = 250.0, (8.0, 12.0), 2500
STARTS = tuple(range(1000, 8501, 500))             # the 16 interior windows of the planted dyad


def analytic_restated(x, resp, dtype=np.float64):
    """ifft(fft(x) * resp) along the last axis by scipy.fft in `dtype` (float64 or np.longdouble)."""
    import scipy.fft
    x = np.asarray(x, dtype=dtype)
    return scipy.fft.ifft(scipy.fft.fft(x, axis=-1) * np.asarray(resp, dtype=dtype), axis=-1)


def _operand(z, start, n, mode):
    w = np.asarray(z)[:, start:start + n]
    re, im = w.real.astype(np.float64), w.imag.astype(np.float64)
    if mode == UNIT:
        a = np.hypot(re, im)
        with np.errstate(invalid="ignore", divide="ignore"):
            re, im = np.where(a == 0.0, 0.0, re / a), np.where(a == 0.0, 0.0, im / a)
    return re, im


def gram_restated(z, start, n, mode):
    """C (m, m) complex128 of the window z[:, start : start + n], summed by NumPy's matrix product (not the kernel's
    order: equal to it to `gram_bound` only)."""
    re, im = _operand(z, start, n, mode)
    with np.errstate(invalid="ignore", over="ignore"):
        return (re @ re.T + im @ im.T) + 1j * (im @ re.T - re @ im.T)


def measures_restated(z, start, n, mode):
    """{"coherency": (2, m, m) = (Re R, Im R), "mag", "lagged": (m, m), "info": 0 | 1 | 2} as the entry defines them."""
    C = gram_restated(z, start, n, mode)
    m = C.shape[0]
    d = C.real.diagonal().copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        R = C / n if mode == UNIT else C / np.sqrt(np.outer(d, d))
        R[np.arange(m), np.arange(m)] = R.real.diagonal()                       # Im R_ii = 0
        mag = np.abs(R)
        if mode == UNIT:
            den = 1.0 - R.real ** 2
            lagged = np.where(den > 0.0, np.minimum(1.0, np.abs(R.imag) / np.sqrt(np.where(den > 0.0, den, 1.0))), 0.0)
        else:
            lagged = np.abs(R.imag)
    live = d > 0.0
    mag[live, live], lagged[live, live] = 1.0, 0.0
    info = 0
    coh = np.stack([R.real, R.imag])
    if not np.isfinite(d).all():
        info = 1
        coh[:], mag[:], lagged[:] = np.nan, np.nan, np.nan
    elif mode == RAW and (d == 0.0).any():
        info = 2
        dead = d == 0.0
        for a in (coh[0], coh[1], mag, lagged):
            a[dead, :] = np.nan
            a[:, dead] = np.nan
    return {"coherency": coh, "mag": mag, "lagged": lagged, "info": info}


def plv(z, start, n):
    return measures_restated(z, start, n, UNIT)["mag"]


def ciplv(z, start, n):
    return measures_restated(z, start, n, UNIT)["lagged"]


def coh(z, start, n):
    return measures_restated(z, start, n, RAW)["mag"]


def imcoh(z, start, n):
    return measures_restated(z, start, n, RAW)["lagged"]


def gram_bound(z, start, n, mode):
    """How far two float64 evaluations of the formulas may lie apart, per element: {"coherency": (2, m, m), "mag",
    "lagged", "den": (m, m)}.
    Two summations of the same 2 n products in different orders, each product rounded once or fused, differ by at most
    2 n 2^-52 sum |products| (each side below 2 n u sum |terms|, u = 2^-53, to first order; 2 n eps = 4 n u leaves the
    higher-order terms room), and 16 more eps of that sum cover the few ulps by which two roundings of the phasor
    z / |z| (hypot or sqrt of the squares, a division each) move every product, and the final roundings:
        dRe C_ij = (2 n + 16) 2^-52 sum_t (|re_i re_j| + |im_i im_j|),   dIm C_ij likewise with |im_i re_j| + |re_i im_j|.
    To first order:  UNIT  dR = dC / n;   RAW  dR = dC / s + |R| (dC_ii / (2 C_ii) + dC_jj / (2 C_jj)),  s = sqrt(C_ii C_jj);
    |dmag| <= |dR|;  |dciPLV| <= |dIm| / sqrt(den) + |Im| |Re| |dRe| / den^(3/2);  |dimcoh| <= |dIm R|."""
    re, im = _operand(z, start, n, mode)
    are, aim = np.abs(re), np.abs(im)
    f = (2 * n + 16) * EPS
    bre = f * (are @ are.T + aim @ aim.T)
    bim = f * (aim @ are.T + are @ aim.T)
    r = measures_restated(z, start, n, mode)
    Rre, Rim = r["coherency"]
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == UNIT:
            dre, dim = bre / n, bim / n
        else:
            d = (re * re + im * im).sum(axis=1)
            s = np.sqrt(np.outer(d, d))
            rel = bre.diagonal() / (2.0 * d)
            dre = bre / s + np.abs(Rre) * (rel[:, None] + rel[None, :])
            dim = bim / s + np.abs(Rim) * (rel[:, None] + rel[None, :])
        den = 1.0 - Rre ** 2
        dmag = np.hypot(dre, dim)
        if mode == UNIT:
            dlag = dim / np.sqrt(den) + np.abs(Rim) * np.abs(Rre) * dre / den ** 1.5
        else:
            dlag = dim
    return {"coherency": np.stack([dre, dim]), "mag": dmag, "lagged": dlag, "den": den}


def planted_dyad(seed):
    """(x (8, 12000) float64, fs): noise in physical-unit and mixed amplitudes with a pi/2-lagged 10 Hz coupling between
    channels 0 and 5 and a zero-lag mixing between channels 2 and 6."""
    rng = np.random.default_rng(seed)
    fs, T = 250.0, 12000
    t = np.arange(T) / fs
    x = rng.standard_normal((8, T))
    ph = 2.0 * np.pi * 10.0 * t + 0.05 * np.cumsum(rng.standard_normal(T))
    x[0] += 2.0 * np.cos(ph)
    x[5] += 2.0 * np.cos(ph - np.pi / 2.0)                       # lagged coupling 0 <-> 5
    c = 10.0 * rng.standard_normal(T)
    x[2] += c
    x[6] += c                                                    # zero-lag mixing 2 <-> 6
    x *= np.array((1e-6, 3e-6, 1.0, 5.0, 20.0, 1e-5, 2.0, 1.0))[:, None]      # physical-unit and mixed amplitudes
    return x, fs


def check_planted(plv_w, ciplv_w):
    """The thresholds of the planted dyad on PLV and ciPLV of one window (8, 8); returns the largest other PLV."""
    assert plv_w[0, 5] > 0.95 and ciplv_w[0, 5] > 0.95, (plv_w[0, 5], ciplv_w[0, 5])
    assert plv_w[2, 6] > 0.9 and ciplv_w[2, 6] < 0.4, (plv_w[2, 6], ciplv_w[2, 6])
    other = np.ones((8, 8), dtype=bool)
    other[np.arange(8), np.arange(8)] = False
    for i, j in ((0, 5), (2, 6)):
        other[i, j] = other[j, i] = False
    assert plv_w[other].max() < 0.6, plv_w[other].max()
    return float(plv_w[other].max())
