"""CPU-side checks of block Granger causality: the two NumPy restatements agree, the C entries refuse bad arguments before
anything touches a GPU (each refusal with its own code and text), workspace sizing, and the Python wrappers' refusals."""
import os
import subprocess

import numpy as np
import pytest

from oracle import mvar_oracle as O
from tests import block_gc_restated as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")

# m, split, p, n
SHAPES = [(3, 1, 1, 500), (5, 2, 3, 500), (7, 3, 2, 300), (8, 4, 3, 400), (17, 16, 2, 500), (19, 7, 4, 500), (19, 9, 5, 600),
          (33, 17, 4, 800), (64, 32, 8, 1000)]


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


def _signal(m, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, T))
    x[:, 1:] += 0.5 * x[:, :-1]
    x[1:] += 0.3 * x[:-1]
    return x


@pytest.mark.parametrize("m,split,p,n", SHAPES, ids=lambda v: str(v))
def test_the_two_restatements_agree(m, split, p, n):
    if m >= 33:
        from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad
        x = synthetic_var_dyad(5, m=m, p=min(p, 4), T=n, burn=300)
    else:
        x = _signal(m, n, 11 + m)
    ar, V = O.ar_coeff(x, p)
    freqs = np.linspace(1.0, 45.0, 8)
    a, b = G.definition(ar, V, split, freqs, 100.0), G.inversion_free(ar, V, split, freqs, 100.0)
    assert np.isfinite(a).all() and (a > -1e-10).all()
    err = np.abs(a - b).max()
    print(f"m={m} split={split} p={p}: |definition - inversion_free| = {err:.2e}, max|f| = {np.abs(a).max():.3f}")
    assert err <= 1e-10 * (1.0 + np.abs(a).max())


def test_time_domain_restatement_matches_the_oracle_fits():
    x = _signal(7, 400, 3)
    p, split = 3, 3
    R = O.lag_covariances(x, p)
    _, V = O.ar_coeff(x, p)
    t = G.time_domain(R, V, split, p)
    ld = lambda M: np.linalg.slogdet(M)[1]            # noqa: E731
    _, Va = O.ar_coeff(x[:split], p)
    _, Vb = O.ar_coeff(x[split:], p)
    want = np.array([ld(Vb) - ld(V[split:, split:]), ld(Va) - ld(V[:split, :split])])
    assert np.abs(t[:2] - want).max() < 1e-12
    assert (t[:3] > -1e-12).all() and abs(t[3] - t[:3].sum()) < 1e-14


P = 0x1000


def _sliding(lib, m=8, n=100, p=4, split=3, F=16, n_bands=0, spectral=P, ws_bytes=1 << 40, chunk=4, n_items=1):
    return lib.hmv_sliding_block_gc_f64(P, 0, 100, P, P, n_items, m, n, p, split, P, F, 100.0, spectral, P, P, n_bands, P, 0, 0,
                                        P, P, P, P, ws_bytes, chunk, 0, 0, 0, 0, 100, 0)


def _stage(lib, m=8, p=4, split=3, F=16, spectral=P, ws_bytes=1 << 40, n_items=1):
    return lib.hmv_block_gc_f64(P, P, n_items, m, p, split, P, F, 100.0, spectral, P, P, P, ws_bytes, 0)


def test_c_entries_refuse_bad_arguments_without_a_gpu(lib):
    """Every pointer a fake non-zero address: the argument checks must refuse before any of them is read."""
    need = lib.hmv_block_gc_sliding_workspace_bytes(4, 8, 4, 3, 16, 0)
    need_b = lib.hmv_block_gc_sliding_workspace_bytes(4, 8, 4, 3, 16, 2)
    assert 0 < need < need_b
    cases = [(dict(split=0), -11, b"split"), (dict(split=8), -11, b"split"), (dict(m=65), -1, b"channel count"),
             (dict(p=0), -2, b"model order"), (dict(p=33), -2, b"model order"), (dict(n=4, p=4), -3, b"window shorter"),
             (dict(n=3, p=4), -3, b"window shorter"), (dict(F=0), -12, b"frequency grid"), (dict(n_bands=-1), -14, b"n_bands"),
             (dict(spectral=0), -13, b"spectral output"), (dict(ws_bytes=need - 1), -7, b"workspace too small"),
             (dict(ws_bytes=need_b - 1, n_bands=2), -7, b"workspace too small"), (dict(chunk=0), -4, b"null pointer")]
    seen = {}
    for kw, code, text in cases:
        assert _sliding(lib, **kw) == code, kw
        err = lib.hmv_last_error()
        assert text in err and err.startswith(b"hmv_sliding_block_gc_f64"), (kw, err)
        seen.setdefault(code, err)
        assert seen[code] == err                                   # one code, one text
    assert len({v for v in seen.values()}) == len(seen)            # and every refusal its own
    assert _sliding(lib, n_items=0, spectral=0) == 0               # empty batch: nothing to do
    for entry, name in ((_sliding, b"hmv_sliding_block_gc_f64"), (_stage, b"hmv_block_gc_f64")):
        assert entry(lib, n_items=-1) == -4                        # a negative count is refused, not read as empty
        assert lib.hmv_last_error().startswith(name) and b"n_items" in lib.hmv_last_error()
    need_s = lib.hmv_block_gc_workspace_bytes(1, 8, 4, 3, 16)
    stage = [(dict(split=0), -11, b"split"), (dict(split=8), -11, b"split"), (dict(m=65), -1, b"channel count"),
             (dict(p=0), -2, b"model order"), (dict(p=33), -2, b"model order"), (dict(F=0), -12, b"frequency grid"),
             (dict(spectral=0), -13, b"spectral output"), (dict(ws_bytes=need_s - 1), -7, b"workspace too small")]
    for kw, code, text in stage:
        assert _stage(lib, **kw) == code, kw
        err = lib.hmv_last_error()
        assert text in err and err.startswith(b"hmv_block_gc_f64"), (kw, err)
    assert _stage(lib, n_items=0, spectral=0) == 0


def test_workspace_sizes(lib):
    ws = lib.hmv_block_gc_sliding_workspace_bytes
    prev = 0
    for chunk in (1, 2, 3, 7, 64, 599):
        now = ws(chunk, 64, 8, 32, 256, 0)
        assert now > prev
        prev = now
    assert ws(7, 64, 8, 32, 256, 5) > ws(7, 64, 8, 32, 256, 0)          # the band form keeps the chunk's full array
    for bad in ((0, 8, 4, 3, 16, 0), (1, 65, 4, 3, 16, 0), (1, 0, 4, 3, 16, 0), (1, 8, 0, 3, 16, 0), (1, 8, 33, 3, 16, 0),
                (1, 8, 4, 0, 16, 0), (1, 8, 4, 8, 16, 0), (1, 8, 4, 3, 0, 0), (1, 8, 4, 3, 16, -1)):
        assert ws(*bad) == -1, bad
    st = lib.hmv_block_gc_workspace_bytes
    assert 0 < st(1, 64, 8, 32, 256) < st(2, 64, 8, 32, 256)
    for bad in ((0, 8, 4, 3, 16), (1, 65, 4, 3, 16), (1, 8, 0, 3, 16), (1, 8, 4, 0, 16), (1, 8, 4, 8, 16), (1, 8, 4, 3, 0)):
        assert st(*bad) == -1, bad
    # no K3 in this call: its scratch is left out of the layout
    assert ws(1, 64, 8, 32, 256, 0) < lib.hmv_sliding_workspace_bytes(1, 64, 8, 256)
    # the generic entries go on refusing measure code 3: block Granger causality is not a fourth HMV_MEASURE_*
    assert lib.hmv_sliding_auto_workspace_bytes(3, 1, 8, 4, 16, 0) == -1


def test_python_wrappers_refuse_before_the_gpu():
    from hyperscanning_signal_analysis_amd import mtmvar as M
    from hyperscanning_signal_analysis_amd import sliding as SL
    from hyperscanning_signal_analysis_amd.engine import check_block_split
    x = np.zeros((6, 300))
    f = np.arange(1.0, 9.0)
    for bad in (0, 6, -1, 7, 2.0, 2.5, "2", None, True):
        with pytest.raises(ValueError, match="split"):
            SL.sliding_block_granger(x, 100, 3, 2, f, 100.0, split=bad)
        with pytest.raises(ValueError, match="split"):
            M.block_granger_causality(x, f, 100.0, bad, optimal_model_order=2)
        with pytest.raises(ValueError, match="split"):
            check_block_split(bad, 6, "t")
    assert check_block_split(np.int64(5), 6, "t") == 5 and check_block_split(1, 2, "t") == 1
    with pytest.raises(ValueError, match="automatic model order"):
        SL.sliding_block_granger(x, 100, 3, None, f, 100.0, split=2)
    with pytest.raises(ValueError, match="p must be an integer"):
        SL.sliding_block_granger(x, 100, 3, 2.5, f, 100.0, split=2)


def test_escan_block_granger_on_a_missing_root_is_refused_first(tmp_path):
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    missing = tmp_path / "no_such_root"
    with pytest.raises(ValueError, match="measures"):
        EB.run(missing, tmp_path / "out", measures=("ffdtf", "pdc"), block_granger=True, verbose=False)
    with pytest.raises(ValueError, match="automatic model order"):
        EB.run(missing, tmp_path / "out", model_order=None, block_granger=True, verbose=False)
    assert not (tmp_path / "out").exists()                                  # refused before anything is read or made
    assert EB.MEASURES == ("ffdtf", "ddtf", "gpdc")
