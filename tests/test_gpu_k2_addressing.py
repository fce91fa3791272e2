"""K2's tile addressing (csrc/yw_lwr_core.h): every tile is a wave-uniform base plus an unsigned 32-bit per-lane byte
offset.  What can go wrong with that is position dependence -- a base or an offset that is right for one item of the
batch and wrong for another -- and wrap-around once an item's scratch lies more than 2^32 bytes behind the scratch base.
Equal inputs must therefore give equal BITS wherever they sit in the batch, whatever the scratch held before, and the
result must still be the oracle's.  All @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

GUARD = 1e-9      # the tolerance of test_levinson_whittle_solver_against_the_block_ldlt_and_the_oracle
STARTS = (0, 10, 20)
ORDER = (2, 0, 1, 1, 0, 2, 0)


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def assert_parity(out, ref, guard=GUARD):
    assert out.shape == ref.shape
    assert rel(out, ref) <= guard, rel(out, ref)
    row_max = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).min()
    assert np.allclose(out, ref, rtol=1e-5, atol=1e-5 * row_max)


def distinct_windows(eng, m, n, p, seed=43):
    """(x, R): the lag covariances of the windows x[:, s:s + n], s in STARTS."""
    x = synthetic_var_dyad(seed, m=m, p=min(p, 4), T=n + STARTS[-1], burn=300)
    xd = eng.to_device(x[None])
    rec = torch.zeros(len(STARTS), dtype=torch.int64, device=eng.device)
    st = torch.tensor(STARTS, dtype=torch.int64, device=eng.device)
    return x, eng.lagcov(xd, rec, st, n, p)


def solve_into(eng, R, m, ws):
    """hmv_yw_solve_f64 with the caller's scratch (Engine.yw_solve allocates its own)."""
    n_items, p1, mp, _ = R.shape
    p = p1 - 1
    ar, V, ld = eng.empty(n_items, mp, mp, p), eng.empty(n_items, mp, mp), eng.empty(n_items, p)
    info = eng.empty(n_items, dtype=torch.int32)
    with torch.cuda.device(eng.device):
        rc = eng.lib.hmv_yw_solve_f64(R.data_ptr(), n_items, m, p, ws.data_ptr(), ar.data_ptr(), V.data_ptr(), ld.data_ptr(),
                                      info.data_ptr(), 0, eng.stream())
    assert rc == 0
    return ar, V, ld, info


def assert_twins_agree(order, outs, pairs=None):
    """items with the same source window carry the same bits in every output"""
    first = {}
    for i, src in enumerate(order):
        j = first.setdefault(src, i)
        if j != i and (pairs is None or i in pairs):
            for t in outs:
                assert torch.equal(t[i], t[j]), (i, j)


@pytest.mark.parametrize("m,n,p", [(64, 700, 8), (33, 300, 1), (19, 400, 3), (5, 200, 9), (48, 600, 2)])
def test_equal_windows_give_equal_bits_wherever_they_sit(m, n, p):
    """Every padded size, p = 1 (no lower-lag loop), odd and even orders: three distinct windows repeated over a batch
    of seven in a shuffled order; a second call into the same scratch, poisoned with NaN in between, gives the same
    bits; the coefficients are the oracle's."""
    eng = default_engine()
    x, R3 = distinct_windows(eng, m, n, p)
    R = R3[list(ORDER)].contiguous()
    wsd = int(eng.lib.hmv_yw_workspace_doubles(m, p))
    ws = eng.empty(len(ORDER) * wsd)
    ws.fill_(float("nan"))
    first = solve_into(eng, R, m, ws)
    torch.cuda.synchronize()
    assert not bool(first[3].any())
    assert_twins_agree(ORDER, first)
    ws.fill_(float("nan"))
    again = solve_into(eng, R, m, ws)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # the engine's own call (its own scratch) computes the same
    for a, b in zip(first, eng.yw_solve(R, m, True)):
        assert torch.equal(a, b)
    for i, src in enumerate(ORDER[:3]):
        aro, Vo = O.ar_coeff(x[:, STARTS[src]:STARTS[src] + n], p)
        assert_parity(first[0][i, :m, :m].cpu().numpy(), aro)
        assert_parity(first[1][i, :m, :m].cpu().numpy(), Vo)


def test_scratch_of_the_last_items_lies_past_4_gib():
    """m = 64, p = 8 with as many items as it takes for the last ones' scratch to begin more than 2^32 bytes behind the
    scratch base (the per-item size is the library's own figure): the smallest batch at which a 32-bit offset, per lane
    or scalar, would wrap.  Two distinct windows tiled; the first and the last two items agree bit for bit with their
    twins and with a two-item call."""
    eng = default_engine()
    m, n, p = 64, 700, 8
    _, R3 = distinct_windows(eng, m, n, p)
    wsd = int(eng.lib.hmv_yw_workspace_doubles(m, p))
    n_items = (1 << 32) // (8 * wsd) + 3
    assert (n_items - 2) * wsd * 8 > (1 << 32)
    order = [i & 1 for i in range(n_items)]
    R = R3[:2].repeat((n_items + 1) // 2, 1, 1, 1)[:n_items].contiguous()
    big = solve_into(eng, R, m, eng.empty(n_items * wsd))
    small = solve_into(eng, R3[:2].contiguous(), m, eng.empty(2 * wsd))
    torch.cuda.synchronize()
    assert not bool(big[3].any())
    assert_twins_agree(order, big, pairs=(n_items - 2, n_items - 1))
    for b, s in zip(big, small):
        assert torch.equal(b[:2], s)
        assert torch.equal(b[n_items - 2 + (n_items & 1)], s[0]) and torch.equal(b[n_items - 1 - (n_items & 1)], s[1])


def test_automatic_order_call_shares_the_core():
    """hmv_yw_solve_auto_f64 walks the same recursion (same staging helpers): duplicate items, same bits."""
    eng = default_engine()
    m, n, p = 64, 700, 8
    _, R3 = distinct_windows(eng, m, n, p)
    R = R3[list(ORDER)].contiguous()
    outs = eng.yw_solve_auto(R, m, n, "AIC")
    torch.cuda.synchronize()
    assert not bool(outs[4].any()) and bool((outs[2] > 0).all())
    assert_twins_agree(ORDER, outs)
