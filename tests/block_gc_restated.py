"""NumPy restatements of block (multivariate) Granger causality between the channels < split (block A) and the channels
>= split (block B) -- Geweke (1982) -- for tests/test_block_gc_cpu.py and tests/test_gpu_block_gc.py.  NumPy only:
importable without a GPU, and nothing here is the code under test.

Conventions: ar (m, m, p) and V (m, m) as `oracle.mvar_oracle.ar_coeff` returns them, A(f) = I - sum_k ar_k z^k with
z = exp(-2 pi i f / fs), H = A^-1, S = H V H^H (conjugate transpose).  Outputs (2, F): row 0 is A -> B, row 1 is B -> A."""
import numpy as np


def _blocks(m, split):
    a, b = np.arange(split), np.arange(split, m)
    return ((a, b), (b, a))                     # (src, dst) of direction 0 and of direction 1


def _A_of_f(ar, freqs, fs):
    m, _, p = ar.shape
    z = np.exp(-2j * np.pi * np.asarray(freqs, dtype=np.float64) / fs)
    A = np.broadcast_to(np.eye(m, dtype=complex), (len(z), m, m)).copy()
    for k in range(p):
        A -= ar[None, :, :, k] * (z ** (k + 1))[:, None, None]
    return A


def _partial(V, s, d):
    """Sigma_{s|d} = Sigma_ss - Sigma_sd Sigma_dd^-1 Sigma_ds and G = Sigma_sd Sigma_dd^-1."""
    G = np.linalg.solve(V[np.ix_(d, d)].T, V[np.ix_(s, d)].T).T
    return V[np.ix_(s, s)] - G @ V[np.ix_(d, s)], G


def definition(ar, V, split, freqs, fs):
    """f_{s->d} = ln det S_dd - ln det(S_dd - H_ds Sigma_{s|d} H_ds^H), with np.linalg.inv and slogdet."""
    m = ar.shape[0]
    A = _A_of_f(ar, freqs, fs)
    out = np.empty((2, len(A)))
    for k, Ak in enumerate(A):
        H = np.linalg.inv(Ak)
        S = H @ V @ H.conj().T
        for direction, (s, d) in enumerate(_blocks(m, split)):
            Sp, _ = _partial(V, s, d)
            Hds = H[np.ix_(d, s)]
            Sdd = S[np.ix_(d, d)]
            out[direction, k] = np.linalg.slogdet(Sdd)[1] - np.linalg.slogdet(Sdd - Hds @ Sp @ Hds.conj().T)[1]
    return out


def inversion_free(ar, V, split, freqs, fs):
    """f_{s->d} = ln det Sigma_{s|d} + ln det W_ss - 2 ln|det At_ss|, W = A^H Sigma^-1 A, At_ss = A_ss - G A_ds."""
    m = ar.shape[0]
    A = _A_of_f(ar, freqs, fs)
    L = np.linalg.cholesky(V)
    out = np.empty((2, len(A)))
    for k, Ak in enumerate(A):
        LA = np.linalg.solve(L, Ak)
        for direction, (s, d) in enumerate(_blocks(m, split)):
            Sp, G = _partial(V, s, d)
            Ws = LA[:, s].conj().T @ LA[:, s]
            At = Ak[np.ix_(s, s)] - G @ Ak[np.ix_(d, s)]
            out[direction, k] = np.linalg.slogdet(Sp)[1] + np.linalg.slogdet(Ws)[1] - 2.0 * np.linalg.slogdet(At)[1]
    return out


def _restricted_cov(R, idx, p):
    """Residual covariance of the order-p Yule-Walker fit of the channels `idx` alone, from the lag covariances
    R (p+1, m, m), R_l = X[:, :n-l] X[:, l:]^T / n: the block-Toeplitz normal equations, solved densely."""
    Rx = R[np.ix_(np.arange(p + 1), idx, idx)]
    k = len(idx)
    left = np.zeros((k * p, k * p))
    right = np.zeros((k * p, k))
    for a in range(p):
        right[a * k:(a + 1) * k] = Rx[a + 1]
        for b in range(p):
            left[a * k:(a + 1) * k, b * k:(b + 1) * k] = Rx[a - b] if a >= b else Rx[b - a].T
    x = np.linalg.solve(left, right).T
    return Rx[0] - x @ right


def time_domain(R, V, split, p):
    """(F_{A->B}, F_{B->A}, F_{A.B}, F_{A,B}) from the lag covariances R (p+1, m, m) and the full fit's V."""
    m = V.shape[0]
    a, b = np.arange(split), np.arange(split, m)
    ld = lambda M: np.linalg.slogdet(M)[1]            # noqa: E731
    Vaa, Vbb = V[np.ix_(a, a)], V[np.ix_(b, b)]
    fab = ld(_restricted_cov(R, b, p)) - ld(Vbb)
    fba = ld(_restricted_cov(R, a, p)) - ld(Vaa)
    fi = ld(Vaa) + ld(Vbb) - ld(V)
    return np.array([fab, fba, fi, fab + fba + fi])
