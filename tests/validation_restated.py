"""NumPy restatement of the model-validation definitions (include/hypermvar.h, "Model validation"):
residuals of an MVAR fit, their lag covariances and the whiteness statistics (Luetkepohl 2005, section 4.4.3; Hosking 1980;
Li & McLeod 1981).  The reference has nothing of the kind, so tests/test_validation_cpu.py pins this file by properties;
tests/test_gpu_validation.py compares the kernels with it.  Also the workloads both test files share."""
import numpy as np
from scipy.special import chdtrc

from hyperscanning_signal_analysis_amd.synthetic import mixed_order_recording, synthetic_var_dyad

EPS = np.finfo(np.float64).eps


def yule_walker(x, p):
    """Biased, not demeaned lag covariances and the block-Toeplitz normal equations (the reference's count_corr /
    ar_coeff): ar (m, m, p) with ar[:, :, k] multiplying x(t - k - 1), and the residual covariance."""
    m, n = x.shape
    R = [x[:, :n - l] @ x[:, l:].T / n for l in range(p + 1)]
    G = np.zeros((m * p, m * p))
    rhs = np.zeros((m * p, m))
    for a in range(p):
        rhs[a * m:(a + 1) * m] = R[a + 1]
        for b in range(p):
            G[a * m:(a + 1) * m, b * m:(b + 1) * m] = R[a - b] if a >= b else R[b - a].T
    sol = np.linalg.solve(G, rhs)
    ar = np.stack([sol[k * m:(k + 1) * m].T for k in range(p)], axis=2)
    return ar, R[0] - sol.T @ rhs


def residuals(x, ar):
    """E = X[:, p:] - sum_k A_k X[:, p-k : n-k], A_k = ar[:, :, k-1]: (m, n - p)."""
    m, n = x.shape
    p = ar.shape[2]
    E = x[:, p:].copy()
    for k in range(1, p + 1):
        E -= ar[:, :, k - 1] @ x[:, p - k:n - k]
    return E


def residual_bound(x, ar):
    """Elementwise forward bound of a dot product of m p + 1 terms, doubled because both sides round:
    2 (m p + 2) eps (|x_t| + sum_k |A_k| |x_{t-k}|)."""
    m, n = x.shape
    p = ar.shape[2]
    mag = np.abs(x[:, p:]).copy()
    for k in range(1, p + 1):
        mag += np.abs(ar[:, :, k - 1]) @ np.abs(x[:, p - k:n - k])
    return 2.0 * (m * p + 2) * EPS * mag


def lag_covariances(E, h):
    """C_l = E[:, :N-l] E[:, l:]^T / N, l = 0..h (K1's estimator: biased, not demeaned): (h+1, m, m)."""
    N = E.shape[1]
    return np.stack([E[:, :N - l] @ E[:, l:].T / N for l in range(h + 1)])


def acf(C):
    """r_l[i, j] = C_l[i, j] / sqrt(C_0[i, i] C_0[j, j]), l = 1..h: (h, m, m)."""
    d = np.diag(C[0])
    return C[1:] / np.sqrt(d[:, None] * d[None, :])


def whiteness(C, N, order, acf_z=1.96):
    """The statistics from lag covariances C (h+1, m, m) of N residuals of a model of order `order`."""
    h, m = C.shape[0] - 1, C.shape[1]
    L = np.linalg.cholesky(C[0])
    Li = np.linalg.inv(L)
    s = np.array([np.sum((Li @ C[l] @ Li.T) ** 2) for l in range(1, h + 1)])
    lags = np.arange(1, h + 1)
    q_bp = N * s.sum()
    q = np.array([q_bp, q_bp + m * m * h * (h + 1) / (2.0 * N), N * N * np.sum(s / (N - lags))])
    r = acf(C)
    rd = np.stack([np.diag(r[l]) for l in range(h)])                # (h, m)
    q_ch = N * (N + 2.0) * np.sum(rd ** 2 / (N - lags)[:, None], axis=0)
    df_ch = h - int(order)
    df = m * m * df_ch
    nan = float("nan")
    return dict(s=s, q=q, q_channel=q_ch, df=df, acf_count=int(np.sum(np.abs(r) > acf_z / np.sqrt(N))),
                p_value=chdtrc(df, q) if df > 0 else np.full(3, nan),
                p_channel=chdtrc(df_ch, q_ch) if df_ch > 0 else np.full(m, nan))


def validate_window(x, ar, h, order=None, acf_z=1.96):
    """Residuals -> covariances -> statistics of one window x (m, n) under the coefficients ar (m, m, p)."""
    p = ar.shape[2]
    E = residuals(x, ar)
    C = lag_covariances(E, h)
    out = whiteness(C, x.shape[1] - p, p if order is None else order, acf_z)
    out["acf_fraction"] = out["acf_count"] / float(h * x.shape[0] ** 2)
    out["resid_cov"] = C[0]
    return out


# ---- the workloads of tests/test_gpu_validation.py (the CPU file checks their ACF cells against the threshold) -----------
SHAPES = [(3, 203, 4, 7), (4, 160, 5, 12), (19, 1000, 6, 12), (20, 131, 1, 3), (33, 300, 32, 32), (64, 1000, 8, 20)]


def workload(m, n, p, h):
    """Two recordings inside a wider array (so the leading dimension is not T), 5 and 6 windows at arbitrary starts, the
    last one ending at T.  Returns (wide (2, m, T + 37), T, item_rec, item_start)."""
    T = n + 517
    if m == 4:
        recs = [mixed_order_recording(40 + d, 4, (2, 6), (T + 1) // 2)[:, :T] for d in range(2)]
    else:
        recs = [synthetic_var_dyad(10 + d, m, p=min(p, 8), T=T, burn=300) for d in range(2)]
    wide = np.zeros((2, m, T + 37))
    wide[:, :, :T] = np.stack(recs)
    wide[:, :, T:] = 1e3                     # never read: a window reaching here would show
    starts0 = [0, 13, 101, 256, T - n]
    starts1 = [7, 64, 129, 300, 411, T - n]
    item_rec = np.array([0] * len(starts0) + [1] * len(starts1), dtype=np.int64)
    item_start = np.array(starts0 + starts1, dtype=np.int64)
    return wide, T, item_rec, item_start


def behaviour_recording():
    """The accept / reject table: stretches of order 2, 6, 2, 6, 1200 samples each; windows of 400 every 400 samples."""
    return mixed_order_recording(77, 4, (2, 6, 2, 6), 1200), 400, 12


def workload_coefficients(x_win, p, seed=5):
    """Coefficients (m, m, p) with every lag in use, for the kernel comparisons: the restated Yule-Walker fit of the
    window at order min(p, 4) (well-posed at every shape of SHAPES, where m p can exceed n) in the first lags and small
    seeded values in the others.  Residuals and their statistics are defined for any coefficients."""
    m = x_win.shape[0]
    q = min(p, 4)
    ar = np.zeros((m, m, p))
    ar[:, :, :q] = yule_walker(x_win, q)[0]
    rng = np.random.default_rng(seed)
    ar[:, :, q:] = rng.standard_normal((m, m, p - q)) * (0.05 / m)
    return ar


def workload_windows(m, n, p, h):
    """(wide, T, item_rec, item_start, ar (items, m, m, p)) of one shape."""
    wide, T, item_rec, item_start = workload(m, n, p, h)
    ar = np.stack([workload_coefficients(wide[r, :, s:s + n], p) for r, s in zip(item_rec, item_start)])
    return wide, T, item_rec, item_start, ar
