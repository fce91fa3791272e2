"""Model validation without a GPU: the NumPy restatement (tests/validation_restated.py) pinned by properties, the
behaviour of the whiteness test on a recording whose windows need different orders, the argument refusals of the four
new C entries, and the distance of every residual correlation of the GPU workloads from the counting threshold."""
import numpy as np
import pytest

from tests import validation_restated as VR


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def fitted():
    rng = np.random.default_rng(3)
    x = VR.mixed_order_recording(11, 5, (3,), 700)
    ar, _ = VR.yule_walker(x, 3)
    return rng, x, ar


def test_zero_coefficients_leave_the_signal():
    x = np.random.default_rng(0).standard_normal((6, 300))
    for p in (1, 5):
        E = VR.residuals(x, np.zeros((6, 6, p)))
        assert E.shape == (6, 300 - p) and np.array_equal(E, x[:, p:])


def test_portmanteau_identities(fitted):
    _, x, ar = fitted
    m, n = x.shape
    for h in (1, 7, 12):
        w = VR.validate_window(x, ar, h)
        N = n - 3
        assert w["q"][1] - w["q"][0] == pytest.approx(m * m * h * (h + 1) / (2.0 * N), rel=1e-10)
        assert w["q"][2] >= w["q"][0]
        assert w["df"] == m * m * (h - 3)
        assert np.all(w["s"] >= 0) and w["s"].shape == (h,)
        if h <= 3:
            assert np.isnan(w["p_value"]).all() and np.isnan(w["p_channel"]).all()
        else:
            assert np.all((w["p_value"] >= 0) & (w["p_value"] <= 1))
        assert 0 <= w["acf_count"] <= h * m * m


def test_channel_permutation_and_scaling(fitted):
    rng, x, ar = fitted
    base = VR.validate_window(x, ar, 9)
    perm = rng.permutation(x.shape[0])
    w = VR.validate_window(x[perm], ar[perm][:, perm], 9)
    assert np.allclose(w["q"], base["q"], rtol=1e-12, atol=0) and np.allclose(w["s"], base["s"], rtol=1e-12, atol=0)
    assert np.allclose(w["q_channel"], base["q_channel"][perm], rtol=1e-12, atol=0)
    assert w["acf_count"] == base["acf_count"]
    sc = np.array([1.0, 7.5, 0.01, 3.0, 120.0])
    w = VR.validate_window(x * sc[:, None], ar * sc[:, None, None] / sc[None, :, None], 9)
    assert np.allclose(w["q"], base["q"], rtol=1e-12, atol=0)
    assert np.allclose(w["q_channel"], base["q_channel"], rtol=1e-12, atol=0)
    assert w["acf_count"] == base["acf_count"]


def test_whiteness_accepts_the_right_order_and_rejects_the_wrong_one():
    """Stretches of order 2, 6, 2, 6 (1200 samples each), windows of 400 every 400 samples, h = 12, restated
    Yule-Walker fit.  Li-McLeod p-values measured with this file: p = 2: smallest accepted 0.12, largest rejected 2.3e-25;
    p = 6: smallest 0.018."""
    x, n, n_win = VR.behaviour_recording()
    pv = {p: np.array([VR.validate_window(x[:, w * n:(w + 1) * n], VR.yule_walker(x[:, w * n:(w + 1) * n], p)[0], 12)
                       ["p_value"][1] for w in range(n_win)]) for p in (2, 6)}
    print("p=2:", pv[2], "p=6:", pv[6])
    low = [0, 1, 2, 6, 7, 8]
    high = [3, 4, 5, 9, 10, 11]
    assert np.all(pv[2][low] > 0.01), pv[2]
    assert np.all(pv[2][high] < 1e-10), pv[2]
    assert np.all(pv[6] > 0.01), pv[6]


def test_argument_refusals(lib):
    P = 4096                                      # any non-null pointer: nothing is dereferenced before the refusal

    def resid(m=4, n=100, p=3, ar=P, E=P, ldE=97, ws=P, nbytes=1 << 20, x=P):
        return lib.hmv_residuals_f64(x, 0, 100, P, P, 1, m, n, p, ar, E, ldE, ws, nbytes, 0)

    def white(m=4, N=97, h=5, C=P, s=P):
        return lib.hmv_whiteness_f64(C, 1, m, N, h, 0.2, s, P, P, P, P, 0)

    def full(m=4, n=100, p=3, h=5, ar=P, s=P, E=0, ldE=0, ws=P, nbytes=1 << 24, chunk=1, info=P):
        return lib.hmv_model_validation_f64(P, 0, 100, P, P, 1, m, n, p, ar, h, 0.2, s, P, P, P, info, 0, E, ldE, ws, nbytes,
                                            chunk, 0)
    for bad_m in (0, 65):
        assert resid(m=bad_m) == -1 and b"hmv_residuals_f64: channel count" in lib.hmv_last_error()
        assert white(m=bad_m) == -1 and b"hmv_whiteness_f64: channel count" in lib.hmv_last_error()
        assert full(m=bad_m) == -1 and b"hmv_model_validation_f64: channel count" in lib.hmv_last_error()
    for bad_p in (0, 33):
        assert resid(p=bad_p) == -2 and b"model order" in lib.hmv_last_error()
        assert full(p=bad_p) == -2 and b"model order" in lib.hmv_last_error()
    for bad_h in (0, 33):
        assert white(h=bad_h) == -6 and b"tested lags" in lib.hmv_last_error()
        assert full(h=bad_h) == -6 and b"tested lags" in lib.hmv_last_error()
    assert resid(n=3) == -3
    assert white(N=5) == -3 and white(N=6) != -3
    assert full(n=8) == -3 and b"tested lags" in lib.hmv_last_error()       # n - p = 5 = h
    assert resid(ar=0) == -4 and resid(E=0) == -4 and resid(ws=0) == -4 and resid(x=0) == -4
    assert white(C=0) == -4 and white(s=0) == -4
    assert full(ar=0) == -4 and full(s=0) == -4 and full(ws=0) == -4 and full(info=0) == -4
    assert b"null pointer" in lib.hmv_last_error()
    need = lib.hmv_residuals_workspace_bytes(1, 4, 3)
    assert need == 8 * 16 * 16 * 3
    assert resid(nbytes=need - 1) == -7 and b"workspace too small" in lib.hmv_last_error()
    need = lib.hmv_model_validation_workspace_bytes(2, 4, 100, 3, 5)
    assert full(chunk=2, nbytes=need - 1) == -7 and full(chunk=0) == -7
    assert resid(ldE=96) == -8 and b"ldE" in lib.hmv_last_error()
    assert full(E=P, ldE=96) == -8 and b"ldE" in lib.hmv_last_error()


def test_workspace_sizes(lib):
    f = lib.hmv_model_validation_workspace_bytes
    for bad in ((1, 0, 100, 3, 5), (1, 65, 100, 3, 5), (1, 4, 100, 0, 5), (1, 4, 100, 33, 5), (1, 4, 100, 3, 0),
                (1, 4, 100, 3, 33), (1, 4, 8, 3, 5), (0, 4, 100, 3, 5)):
        assert f(*bad) == -1, bad
    sizes = [f(c, 19, 1000, 6, 12) for c in (1, 2, 5, 50)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 8 * (32 * 32 * 6 + 19 * 994 + 13 * 32 * 32)
    g = lib.hmv_residuals_workspace_bytes
    assert g(1, 64, 8) == 8 * 64 * 64 * 8 and g(3, 20, 5) == 3 * 8 * 32 * 32 * 5
    assert g(0, 4, 3) == -1 and g(1, 65, 3) == -1 and g(1, 4, 33) == -1


@pytest.mark.parametrize("shape", VR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_residual_correlation_sits_on_the_threshold(shape):
    """The GPU file compares acf_count exactly: that is sound because on its workloads no |r_l[i,j]| lies within 1e-12 of
    1.96 / sqrt(N)."""
    m, n, p, h = shape
    wide, T, item_rec, item_start, ar = VR.workload_windows(m, n, p, h)
    thr = 1.96 / np.sqrt(n - p)
    for r, s, a in zip(item_rec, item_start, ar):
        C = VR.lag_covariances(VR.residuals(wide[r, :, s:s + n], a), h)
        assert np.all(np.linalg.eigvalsh(C[0]) > 0)
        assert np.abs(np.abs(VR.acf(C)) - thr).min() > 1e-12
