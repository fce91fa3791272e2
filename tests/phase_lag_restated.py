"""NumPy restatement of the phase-lag family of include/hypermvar.h (hmv_phase_lag_c128), the derived rounding bound the GPU
tests hold the kernel to, and the condition on the input under which PLI is exactly reproducible.  No GPU: shared by
tests/test_phase_lag_cpu.py and tests/test_gpu_phase_lag.py.

    x[t]  = rn( rn(im_i[t] re_j[t]) - rn(re_i[t] im_j[t]) )        = Im(z_i conj z_j), which is what NumPy computes anyway
    P = #{x > 0}   N = #{x < 0}   S = sum x   A = sum |x|   Q = sum x^2
    pli = |P - N| / n      wpli = |S| / A (NaN where A == 0)      dwpli = (S^2 - Q) / (A^2 - Q) (NaN where A^2 - Q <= 0)
    diagonal 0;  split: only the cells i < split <= j (and their mirror), every other off-diagonal cell NaN
    info 1: a non-finite sample (everything NaN);  2: a computed off-diagonal pair with A == 0;  0 otherwise."""
import numpy as np

EPS = 2.0 ** -52
MEASURES = ("pli", "wpli", "dwpli")


def _window(z, start, n):
    """(re, im) float64 (m, n) of the window; samples past the end of the recording read as zero."""
    w = np.asarray(z)[:, start:start + n]
    if w.shape[1] < n:
        w = np.concatenate([w, np.zeros((w.shape[0], n - w.shape[1]), dtype=w.dtype)], axis=1)
    return np.ascontiguousarray(w.real, dtype=np.float64), np.ascontiguousarray(w.imag, dtype=np.float64)


def x_restated(z, start, n):
    """x (m, m, n) float64: two rounded products and one subtraction per sample, no FMA (NumPy has none here)."""
    re, im = _window(z, start, n)
    with np.errstate(invalid="ignore", over="ignore"):
        p0 = im[:, None, :] * re[None, :, :]
        p1 = re[:, None, :] * im[None, :, :]
        return p0 - p1


def computed_pairs(m, split=0):
    """(m, m) bool: the off-diagonal cells a call with `split` computes."""
    off = ~np.eye(m, dtype=bool)
    if split == 0:
        return off
    i = np.arange(m)
    cross = (i[:, None] < split) & (i[None, :] >= split)
    return cross | cross.T


def sums_restated(z, start, n):
    """(P - N, S, A, Q), each (m, m), summed by NumPy (not the kernel's order: equal to it to `lag_bound` only; P - N is
    an integer and exact)."""
    x = x_restated(z, start, n)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x > 0).sum(-1) - (x < 0).sum(-1)
        return d, x.sum(-1), np.abs(x).sum(-1), (x * x).sum(-1)


def measures_restated(z, start, n, split=0):
    """{"pli", "wpli", "dwpli": (m, m), "info": 0 | 1 | 2} as the entry defines them."""
    re, im = _window(z, start, n)
    m = re.shape[0]
    d, S, A, Q = sums_restated(z, start, n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pli = np.abs(d) / float(n)
        wpli = np.where(A == 0.0, np.nan, np.abs(S) / np.where(A == 0.0, 1.0, A))
        D = A * A - Q
        dwpli = np.where(D > 0.0, (S * S - Q) / np.where(D > 0.0, D, 1.0), np.nan)
    done = computed_pairs(m, split)
    info = 0
    out = {"pli": pli, "wpli": wpli, "dwpli": dwpli}
    if not (np.isfinite(re).all() and np.isfinite(im).all()):
        info = 1
        for a in out.values():
            a[:] = np.nan
    else:
        if (A[done] == 0.0).any():
            info = 2
        for a in out.values():
            a[~done] = np.nan
            a[np.arange(m), np.arange(m)] = 0.0
    out["info"] = info
    return out


def lag_bound(z, start, n):
    """How far two float64 evaluations of wpli and dwpli may lie apart, per cell: {"wpli", "dwpli", "D": (m, m)}.
    The x are common to both sides bit for bit (two rounded products, one subtraction), so only the order of the sums and
    the final roundings differ.  A sum of n terms in any order carries an error below (n - 1) u sum |terms|, u = 2^-53, to
    first order; two orders differ by at most twice that, (n - 1) eps sum |terms|, and 9 more eps of the sum leave room for
    the higher-order terms, for the rounding of x^2 where it is not fused into the sum, and for the few final operations.
    With  a = (n + 8) eps A  and  q = (n + 8) eps Q:   |dS|, |dA| <= a   and   |dQ| <= q.
        wpli = |S| / A:                 |dwpli|  <= a / A + wpli a / A = (1 + wpli) a / A
        N = S^2 - Q,  D = A^2 - Q:      dN <= 2 |S| a + a^2 + q,      dD <= 2 A a + a^2 + q
        dwpli = N / D:                  |ddwpli| <= (dN + |dwpli| dD) / D      (first order in dD / D)."""
    _, S, A, Q = sums_restated(z, start, n)
    f = (n + 8) * EPS
    a, q = f * A, f * Q
    with np.errstate(invalid="ignore", divide="ignore"):
        wpli = np.abs(S) / A
        N, D = S * S - Q, A * A - Q
        dN = 2.0 * np.abs(S) * a + a * a + q
        dD = 2.0 * A * a + a * a + q
        return {"wpli": (1.0 + wpli) * a / A, "dwpli": (dN + np.abs(N / D) * dD) / D, "D": D, "A": A}


def sign_margin(z, start, n):
    """The condition on the input under which the sign of every x is beyond doubt: the number of off-diagonal pair-samples
    with |x| <= 4 eps (|im_i re_j| + |re_i im_j|), i.e. whose sign the rounding of the two products could have decided.
    0 on generic data; identical or proportional channels and zero samples are counted."""
    re, im = _window(z, start, n)
    x = x_restated(z, start, n)
    mass = np.abs(im[:, None, :] * re[None, :, :]) + np.abs(re[:, None, :] * im[None, :, :])
    doubt = np.abs(x) <= 4.0 * EPS * mass
    doubt[np.arange(len(re)), np.arange(len(re))] = False
    return int(doubt.sum())


def measures_longdouble(z, start, n):
    """The definitions by brute force in np.longdouble, sample after sample: (pli, wpli, dwpli) (m, m) longdouble, NaN
    where the definition has none; the diagonal 0."""
    re, im = (a.astype(np.longdouble) for a in _window(z, start, n))
    m = re.shape[0]
    x = x_restated(z, start, n).astype(np.longdouble)            # the float64 x: that is the definition
    S = np.zeros((m, m), dtype=np.longdouble)
    A, Q = S.copy(), S.copy()
    d = np.zeros((m, m), dtype=np.int64)
    for t in range(n):
        S += x[..., t]
        A += np.abs(x[..., t])
        Q += x[..., t] * x[..., t]
        d += (x[..., t] > 0).astype(np.int64) - (x[..., t] < 0).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        pli = np.abs(d) / np.longdouble(n)
        wpli = np.where(A == 0, np.nan, np.abs(S) / A)
        D = A * A - Q
        dwpli = np.where(D > 0, (S * S - Q) / D, np.nan)
    for a in (pli, wpli, dwpli):
        a[np.arange(m), np.arange(m)] = 0
    return pli, wpli, dwpli


def measures_sequential(z, start, n):
    """wpli and dwpli with S, A, Q summed in float64 one term after the other from the window start (Q without the FMA):
    the order the kernel documents, on the host."""
    x = x_restated(z, start, n)
    m = x.shape[0]
    S = np.zeros((m, m))
    A, Q = S.copy(), S.copy()
    for t in range(n):
        S += x[..., t]
        A += np.abs(x[..., t])
        Q += x[..., t] * x[..., t]
    with np.errstate(invalid="ignore", divide="ignore"):
        wpli = np.where(A == 0.0, np.nan, np.abs(S) / A)
        D = A * A - Q
        dwpli = np.where(D > 0.0, (S * S - Q) / D, np.nan)
    return wpli, dwpli


def z64_recipe(T1=1400):
    """The z of tests/test_gpu_phase_sync.py: (3, 64, T1) complex128, independent noise in mixed amplitudes 10^-6 .. 10^1.5
    plus one pi/2-lagged pair (channels 0 and 1)."""
    rng = np.random.default_rng(2024)
    z = rng.standard_normal((3, 64, T1)) + 1j * rng.standard_normal((3, 64, T1))
    ph = 2.0 * np.pi * 0.04 * np.arange(T1) + 0.05 * np.cumsum(rng.standard_normal((3, T1)), axis=-1)
    z[:, 0] += 6.0 * np.exp(1j * ph)
    z[:, 1] += 6.0 * np.exp(1j * (ph - np.pi / 2.0))
    z *= (10.0 ** rng.uniform(-6.0, 1.5, 64))[None, :, None]
    return z


N_CASES = (1, 3, 4, 5, 63, 64, 65, 130, 1000)


def items_for(n, T1=1400):
    """Five items with odd starts, one window ending exactly at T1, recording 1 used twice."""
    return [(0, 1), (1, min(37, T1 - n)), (2, T1 - n), (1, min(333, T1 - n)), (0, min(399, T1 - n))]
