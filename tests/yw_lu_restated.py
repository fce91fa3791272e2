"""NumPy restatement of csrc/yw_lu.hip (K2's pivoted fallback), and the inputs its tests share.  No GPU.

The kernel's algorithm with its blocking and its pivot rule, in float64:
  * [G | B] from the padded lag blocks R (p+1, MP, MP): G[a][b] = R_{a-b} (a >= b), R_{b-a}^T (a < b), B[a] = R_{a+1};
  * right-looking LU, 4 columns at a time: the panel column by column (pivot = largest |a| on or below the diagonal, the
    first on ties; the interchange on the whole augmented row; multipliers by division; an exactly zero column is left
    alone and reported as info = column + 1), the 4 x (rest) block row of U by a unit-lower 4 x 4 solve, the rank-4 update
    of the trailing matrix and of the B columns;
  * back substitution 4 rows at a time from the bottom;
  * ar[i][j][k] = X[k MP + j][i];  V = R_0 - X^T B.
It differs from the kernel only in how the sums inside a step are accumulated (fused multiply-adds and the matrix
instruction there, NumPy's products and sums here), which is what the ratio eta_restated / eta_numpy measures."""
import numpy as np

EPS = np.finfo(np.float64).eps


def pad_of(m: int) -> int:
    return (m + 15) // 16 * 16


def padded_lagcov(x: np.ndarray, p: int) -> np.ndarray:
    """K1 on the host: R_l = X[:, :n-l] X[:, l:]^T / n in the padded layout (identity on the padded diagonal of lag 0)."""
    x = np.asarray(x, dtype=np.float64)
    m, n = x.shape
    mp = pad_of(m)
    R = np.zeros((p + 1, mp, mp))
    for l in range(p + 1):
        R[l, :m, :m] = x[:, :n - l] @ x[:, l:].T * (1.0 / n)
    R[0, np.arange(m, mp), np.arange(m, mp)] = 1.0
    return R


def build_system(R: np.ndarray):
    """(G, B) of the padded lag blocks R (p+1, MP, MP)."""
    p, mp = R.shape[0] - 1, R.shape[1]
    G = np.zeros((mp * p, mp * p))
    B = np.zeros((mp * p, mp))
    for a in range(p):
        B[a * mp:(a + 1) * mp] = R[a + 1]
        for b in range(p):
            G[a * mp:(a + 1) * mp, b * mp:(b + 1) * mp] = R[a - b] if a >= b else R[b - a].T
    return G, B


def real_index(m: int, p: int) -> np.ndarray:
    """Rows / columns of G that belong to real channels."""
    mp = pad_of(m)
    return (np.arange(p)[:, None] * mp + np.arange(m)[None, :]).reshape(-1)


def lu_solve(R: np.ndarray):
    """The kernel's walk -> (ar (MP, MP, p), V (MP, MP), info, X (N, MP)).  info > 0: no solution is formed (NaN)."""
    p, mp = R.shape[0] - 1, R.shape[1]
    N = mp * p
    G, B = build_system(R)
    A = np.concatenate([G, B], axis=1)
    info = 0
    for k0 in range(0, N, 4):
        for k in range(k0, k0 + 4):
            piv = k + int(np.argmax(np.abs(A[k:, k])))            # the first of the largest
            if piv != k:
                A[[k, piv]] = A[[piv, k]]
            pv = A[k, k]
            if pv == 0.0:
                info = info or k + 1
                continue
            A[k + 1:, k] = A[k + 1:, k] / pv
            if k + 1 < k0 + 4:
                A[k + 1:, k + 1:k0 + 4] -= np.outer(A[k + 1:, k], A[k, k + 1:k0 + 4])
        for t in range(1, 4):                                      # block row of U: unit-lower 4 x 4 solve
            for s in range(t):
                A[k0 + t, k0 + 4:] -= A[k0 + t, k0 + s] * A[k0 + s, k0 + 4:]
        if k0 + 4 < N:
            A[k0 + 4:, k0 + 4:] -= A[k0 + 4:, k0:k0 + 4] @ A[k0:k0 + 4, k0 + 4:]
    if info:
        return np.full((mp, mp, p), np.nan), np.full((mp, mp), np.nan), info, np.full((N, mp), np.nan)
    for k0 in range(N - 4, -1, -4):
        for t in range(3, -1, -1):
            acc = A[k0 + t, N:].copy()
            for s in range(t + 1, 4):
                acc -= A[k0 + t, k0 + s] * A[k0 + s, N:]
            A[k0 + t, N:] = acc / A[k0 + t, k0 + t]
        if k0:
            A[:k0, N:] -= A[:k0, k0:k0 + 4] @ A[k0:k0 + 4, N:]
    X = A[:, N:].copy()
    V = R[0] - X.T @ B
    ar = X.reshape(p, mp, mp).transpose(2, 1, 0).copy()            # ar[i][j][k] = X[k MP + j][i]
    return ar, V, 0, X


def eta(G, B, X, idx=None):
    """Normwise backward error ||B - G X||_F / (||G||_F ||X||_F + ||B||_F), on the real channels' rows and columns only
    when `idx` (real_index) is given: the padded unit entries would swamp the norm of data in volts.  The residual is
    accumulated in extended precision."""
    if idx is not None:
        m = len(idx) // (G.shape[0] // B.shape[1])
        G, B, X = G[np.ix_(idx, idx)], B[idx][:, :m], X[idx][:, :m]
    r = (B.astype(np.longdouble) - G.astype(np.longdouble) @ X.astype(np.longdouble)).astype(np.float64)
    return float(np.linalg.norm(r) / (np.linalg.norm(G) * np.linalg.norm(X) + np.linalg.norm(B)))


# ---- inputs shared by tests/test_yw_pivoted_cpu.py and tests/test_gpu_yw_pivoted.py ------------------------------------
# (m, p, n) of the collinear batches: MP = 32, 48, 64, 64
COLLINEAR_SHAPES = [(19, 3, 200), (33, 2, 200), (48, 2, 256), (64, 2, 300)]
COLLINEAR_E = (1e-8, 0.0)
COLLINEAR_SEEDS = (0, 1, 2)
COLLINEAR_AMPLITUDES = (1.0, 1e-5)


def collinear_window(seed: int, m: int, n: int, e: float, amplitude: float = 1.0) -> np.ndarray:
    """A seeded VAR window whose last channel is ch0 + ch1 + e * noise, times `amplitude`."""
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad
    x = synthetic_var_dyad(500 + seed, m=m, p=2, T=n, burn=300)
    noise = np.random.default_rng(9000 + seed).standard_normal(n)
    x[m - 1] = x[0] + x[1] + e * noise
    return np.ascontiguousarray(x * amplitude)


def collinear_batch(m: int, n: int) -> np.ndarray:
    """(12, m, n): e x seed x amplitude, in that nesting."""
    return np.stack([collinear_window(s, m, n, e, a) for e in COLLINEAR_E for s in COLLINEAR_SEEDS
                     for a in COLLINEAR_AMPLITUDES])


# (m, p, n, low-pass in Hz at fs = 500) of the band-limited windows
BAND_LIMITED = [(19, 6, 1000, 30.0), (33, 5, 1000, 40.0)]


def band_limited_window(m: int, n: int, cutoff: float) -> np.ndarray:
    from hyperscanning_signal_analysis_amd.synthetic import band_limited_dyad
    return band_limited_dyad(7, m, n + 200, high_cutoff_hz=cutoff, burn=500)[:, 100:100 + n]


def ratio_cases():
    """(name, x (m, n), p) of every input the ratio eta_restated / eta_numpy is printed for."""
    for m, p, n in COLLINEAR_SHAPES:
        for i, x in enumerate(collinear_batch(m, n)):
            yield f"collinear m={m} p={p} #{i}", x, p
    for m, p, n, fc in BAND_LIMITED:
        yield f"band-limited m={m} p={p} {fc:g} Hz", band_limited_window(m, n, fc), p
