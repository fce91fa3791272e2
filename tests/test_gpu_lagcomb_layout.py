"""The combine step of K1 on a regular grid (lagcomb_kernel, csrc/lagcov.hip) after the change of its LDS image: one
odd-stride image of the 2 l tail samples per channel, filled without a division.  Window lengths of k = 2 and 4 hops,
one and many lags, every lag the launcher accepts, a last window that ends exactly where the recording ends (the
samples that C_l reaches for past it are the zero fill) and one that does not (they are real samples).  All
@pytest.mark.gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

LC_HALO = 32          # csrc/lagcov.hip: the highest lag count launch_lagcov / launch_lagcomb accept


def check_grid(eng, x, m, n, hop, p, first):
    """x: (m, T) host array.  lagcov_regular against lagcov window by window over every window that fits."""
    T = x.shape[1]
    xd = eng.to_device(x[None])
    n_win = (T - first - n) // hop + 1
    st = first + hop * torch.arange(n_win, dtype=torch.int64, device=eng.device)
    rec = torch.zeros(n_win, dtype=torch.int64, device=eng.device)
    direct = eng.lagcov(xd, rec, st, n, p)
    shared = eng.lagcov_regular(xd[0], first, hop, n_win, n, p)
    again = eng.lagcov_regular(xd[0], first, hop, n_win, n, p)
    torch.cuda.synchronize()
    assert shared.shape == direct.shape == (n_win, p + 1, eng.pad(m), eng.pad(m))
    assert float((shared - direct).abs().max() / direct.abs().max()) < 1e-13
    assert torch.equal(shared, again)
    mp = direct.shape[-1]
    if mp > m:
        eye = torch.eye(mp - m, dtype=torch.float64, device=eng.device).expand(n_win, -1, -1)
        assert torch.equal(shared[:, 0, m:, m:], eye)
        assert not bool(shared[:, 1:, m:, :].any()) and not bool(shared[:, :, :m, m:].any()) and not bool(shared[:, 0, m:, :m].any())
    return n_win


@pytest.mark.parametrize("m,n,hop,p,T,first", [(64, 128, 32, 8, 700, 4), (5, 66, 33, 1, 300, 0), (33, 96, 24, 7, 600, 10)])
def test_combined_windows_equal_direct_windows(m, n, hop, p, T, first):
    eng = default_engine()
    x = synthetic_var_dyad(37, m=m, p=min(p, 4), T=T, burn=200)
    n_win = check_grid(eng, x, m, n, hop, p, first)                 # real samples follow the last window
    end = first + (n_win - 1) * hop + n
    assert check_grid(eng, x[:, :end], m, n, hop, p, first) == n_win    # the last window ends exactly at T: zero fill


def test_highest_lag_count_the_launcher_accepts():
    eng = default_engine()
    m, n, hop, p, first = 16, 120, 40, LC_HALO, 3          # (the hop must be longer than the order)
    x = synthetic_var_dyad(39, m=m, p=4, T=first + n + 5 * hop, burn=200)
    assert check_grid(eng, x, m, n, hop, p, first) == 6             # ends exactly at T
