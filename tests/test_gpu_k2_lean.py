"""K2 after the lean walk (csrc/yw_lwr_core.h): lower-lag updates paired, one inverse at order 0, and on the fused path no
emitted model -- K3's packing kernel reads the recursion's tiles.  Every result bit must be what the walk before it gave;
that walk is kept as HMV_TUNE_YW_FORM = 4 and is the reference here.  All @pytest.mark.gpu.

Shapes: channels 5 / 20 / 33 / 64 are the padded sizes 16 / 32 / 48 / 64 (48 is the staging path whose pairs per row do
not divide 256); p = 1 has no lower lags, p = 2 one pair, p = 3 an odd order whose middle lag pairs with itself
(k == q-1-k), p = 8 is the benchmark's order; 5 windows are more than one workgroup; with and without the log
determinants (two instantiations of the kernel).  The window length is 4 m p samples (at least 200): four samples per
unknown of a row keep the fits well conditioned, so that the 1e-9 of the oracle comparison is the same bound as in
tests/test_gpu_parity.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

CHANNELS = (5, 20, 33, 64)
ORDERS = (1, 2, 3, 8)
N_WIN = 5
LEGACY_FORM = 4


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def batch(m, p):
    """(x, n, starts, R) of the 5 windows of one (m, p) case; computed once, shared by the tests, never written."""
    eng = default_engine()
    n = max(200, 4 * m * p)
    hop = n // 4
    T = n + (N_WIN - 1) * hop
    x = synthetic_var_dyad(100 + m + p, m=m, p=min(p, 4), T=T, burn=300)
    starts = hop * np.arange(N_WIN)
    xd = eng.to_device(x[None])
    rec = torch.zeros(N_WIN, dtype=torch.int64, device=eng.device)
    st = torch.as_tensor(starts, dtype=torch.int64, device=eng.device)
    R = eng.lagcov(xd, rec, st, n, p)
    torch.cuda.synchronize()
    return x, n, starts, R


class yw_form:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        lib = default_engine().lib
        assert lib.hmv_set_tuning(_lib.TUNE_YW_FORM, self.form) == 0

    def __exit__(self, *exc):
        assert default_engine().lib.hmv_set_tuning(_lib.TUNE_YW_FORM, 0) == 0


def solve(R, m, vq, fill):
    """hmv_yw_solve_f64 with the scratch and every output pre-filled with `fill`."""
    eng = default_engine()
    n_items, p1, mp, _ = R.shape
    p = p1 - 1
    full = lambda *s: torch.full(s, fill, dtype=torch.float64, device=eng.device)      # noqa: E731
    ws = full(n_items * int(eng.lib.hmv_yw_workspace_doubles(m, p)))
    ar, V, ld = full(n_items, mp, mp, p), full(n_items, mp, mp), full(n_items, p)
    info = torch.full((n_items,), -77, dtype=torch.int32, device=eng.device)
    with torch.cuda.device(eng.device):
        rc = eng.lib.hmv_yw_solve_f64(R.data_ptr(), n_items, m, p, ws.data_ptr(), ar.data_ptr(), V.data_ptr(),
                                      ld.data_ptr() if vq else 0, info.data_ptr(), 0, eng.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return ar, V, ld, info


@pytest.mark.parametrize("vq", [False, True])
@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("m", CHANNELS)
def test_fixed_order_equals_the_kept_walk_bit_for_bit(m, p, vq):
    """Default walk against form 4: coefficients, V, log det V_q, info.  The scratch and the outputs are NaN-poisoned
    for the default and zeroed for the reference: nothing reads the Vf / Vb tiles of order 0 that are no longer written."""
    R = batch(m, p)[3]
    with yw_form(LEGACY_FORM):
        ar0, V0, ld0, i0 = solve(R, m, vq, 0.0)
    ar1, V1, ld1, i1 = solve(R, m, vq, float("nan"))
    assert int((i0 != 0).sum()) == 0 and torch.equal(i0, i1)
    assert not bool(torch.isnan(ar1).any()) and not bool(torch.isnan(V1).any())
    assert same_bits(ar0, ar1) and same_bits(V0, V1)
    if vq:
        assert not bool(torch.isnan(ld1).any()) and same_bits(ld0, ld1)


@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("m", CHANNELS)
def test_automatic_order_equals_the_kept_walk_bit_for_bit(m, p):
    """The selecting form (largest order p): orders, criterion curve, models, V, info."""
    eng = default_engine()
    _, n, _, R = batch(m, p)
    with yw_form(LEGACY_FORM):
        ref = eng.yw_solve_auto(R, m, n, "AIC")
        torch.cuda.synchronize()
    got = eng.yw_solve_auto(R, m, n, "AIC")
    torch.cuda.synchronize()
    assert int((ref[4] != 0).sum()) == 0 and int(ref[2].min()) >= 1
    for a, b in zip(ref, got):
        assert torch.equal(a, b) if a.dtype == torch.int32 else same_bits(a, b)


@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("m", CHANNELS)
def test_coefficients_against_the_oracle(m, p):
    x, n, starts, R = batch(m, p)
    ar, V, _, info = solve(R, m, False, float("nan"))
    assert int((info != 0).sum()) == 0
    for k in (0, N_WIN - 1):
        aro, Vo = O.ar_coeff(x[:, starts[k]:starts[k] + n], p)
        got = ar[k, :m, :m].cpu().numpy()
        err = np.abs(got - aro).max() / np.abs(aro).max()
        print(f"m={m} p={p} window {k}: ar rel err {err:.2e}")
        assert err < 1e-9
