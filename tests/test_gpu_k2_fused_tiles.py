"""The fused sliding call without an emitted model: when the caller does not ask for the coefficients, K2 leaves them in
the final generation's scratch tiles and K3's packing kernel reads them there; windows that the conditioning guard hands
to the LDL^T re-solve come through the `ar` array as before.  With `return_ar=True` K2 emits and the packing kernel reads
`ar` -- the path as it was.  Both must give the same output bits.  All @pytest.mark.gpu.

Grid: n = 200, hop 100, 7 windows of one recording, 16 frequencies, p = 3, one channel count per padded size.  Two more
windows ride in the batch: the first 200 samples of the cond-2e9 nearly collinear fixture (tests/golden/g6_errors.npz,
nc1) in channels 0..3 of an otherwise ordinary recording, which trips the guard, and the exactly rank-deficient fixture
(xs) likewise, which is singular and NaN-filled under check="nan".
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

N, HOP, N_GRID, F, P, FS = 200, 100, 7, 16, 3, 500.0


def bits(t):
    return t.contiguous().view(torch.int64)


def poison_workspaces(eng):
    for ws in eng._ws.values():
        ws.fill_(0xFF)                        # every double of the cached scratch a NaN


@pytest.mark.parametrize("m", [5, 20, 33, 64])
def test_fused_ffdtf_from_tiles_equals_fused_ffdtf_from_emitted_model(m, golden):
    eng = default_engine()
    g = golden("g6_errors.npz")
    T = N + (N_GRID - 1) * HOP
    x = np.stack([synthetic_var_dyad(7 + k + m, m=m, p=P, T=T, burn=300) for k in range(3)])
    x[1, :4, :N] = g["nc1_x"][:, :N]                      # item 7: nearly collinear, guarded
    x[2, :4, :N] = g["xs"][:, :N]                         # item 8: rank deficient, singular
    xd = eng.to_device(x)
    rec = torch.tensor([0] * N_GRID + [1, 2], dtype=torch.int64, device=eng.device)
    st = torch.tensor([HOP * w for w in range(N_GRID)] + [0, 0], dtype=torch.int64, device=eng.device)
    freqs = 2.0 * np.arange(1, F + 1)

    def run(**kw):
        poison_workspaces(eng)
        r = eng.sliding_ffdtf(xd, rec, st, N, P, freqs, FS, check="nan", **kw)
        torch.cuda.synchronize()
        return r

    run()                                                  # (allocates the cached scratch that the next calls poison)
    from_tiles = run()
    emitted, ar, V, (info_yw, info_tf) = run(return_ar=True)
    ldlt = run(return_ar=True, flags=_lib.FLAG_YW_ONE_LAUNCH)[1]
    # the batch is what it is meant to be: item 7 went through the LDL^T re-solve, the grid windows did not all, item 8 failed
    assert int(info_yw[7]) == 0 and torch.equal(bits(ar[7]), bits(ldlt[7]))
    recursion = [k for k in range(N_GRID) if int(info_yw[k]) == 0 and not torch.equal(bits(ar[k]), bits(ldlt[k]))]
    assert recursion, "no window of the grid kept the recursion's result: the tile source is not exercised"
    assert int(info_yw[8]) != 0
    assert bool(torch.isnan(emitted[8]).all()) and not bool(torch.isnan(emitted[:8]).any())
    assert from_tiles.shape == emitted.shape == (N_GRID + 2, m, m, F)
    assert torch.equal(bits(from_tiles), bits(emitted))


def test_fused_band_sums_from_tiles_equal_those_from_the_emitted_model():
    """The band-summing form of K3 takes the same packing kernel: one shape, 32 frequencies in two bands."""
    eng = default_engine()
    m, Fb = 20, 32
    T = N + (N_GRID - 1) * HOP
    xd = eng.to_device(synthetic_var_dyad(5, m=m, p=P, T=T, burn=300)[None])
    rec = torch.zeros(N_GRID, dtype=torch.int64, device=eng.device)
    st = HOP * torch.arange(N_GRID, dtype=torch.int64, device=eng.device)
    freqs = 1.0 * np.arange(1, Fb + 1)
    bands = (np.array([0, 10]), np.array([10, 32]))
    eng.sliding_ffdtf(xd, rec, st, N, P, freqs, FS, bands=bands)
    poison_workspaces(eng)
    a = eng.sliding_ffdtf(xd, rec, st, N, P, freqs, FS, bands=bands)
    poison_workspaces(eng)
    b = eng.sliding_ffdtf(xd, rec, st, N, P, freqs, FS, bands=bands, return_ar=True)[0]
    torch.cuda.synchronize()
    assert a.shape == (N_GRID, m, m, 2) and not bool(torch.isnan(a).any())
    assert torch.equal(bits(a), bits(b))
