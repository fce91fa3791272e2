"""Host side of the condition-contrast permutation test (`surrogates.label_draws`, `surrogates.contrast_args`, the two
front-ends' refusals, the C entries' refusals, the linearity the mix kernel rests on, and what the statistic means on a
planted contrast).  Runs without a GPU."""
import os
import re

import numpy as np
import pytest

from hyperscanning_signal_analysis_amd import _lib
from hyperscanning_signal_analysis_amd import surrogates as sg
from oracle import mvar_oracle as O
from tests.contrast_restated import PLANT, PLANT_FREQS, band_bins, coloured, planted_conditions, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- draws
def test_label_draws_reproduce_keep_the_sizes_and_never_return_the_observed_set():
    ca, cb = [3, 1, 5], [2, 1, 4]
    a = sg.label_draws(np.random.default_rng(7), 40, ca, cb)
    b = sg.label_draws(np.random.default_rng(7), 40, ca, cb)
    assert len(a) == 40 and all(len(row) == 3 for row in a)
    for ra, rb in zip(a, b):
        for g, (x, y) in enumerate(zip(ra, rb)):
            assert np.array_equal(x, y) and x.dtype == np.int64
            assert len(x) == ca[g] and len(np.unique(x)) == ca[g] and (np.diff(x) > 0).all()
            assert x.min() >= 0 and x.max() < ca[g] + cb[g]
            assert not np.array_equal(x, np.arange(ca[g]))
    assert any(not np.array_equal(a[0][2], row[2]) for row in a[1:])
    # the documented order: s outer, g inner, np.sort(rng.permutation(E)[:EA]), the observed set drawn again
    rng = np.random.default_rng(7)
    for s in range(3):
        for g in range(3):
            d = np.sort(rng.permutation(ca[g] + cb[g])[:ca[g]])
            while np.array_equal(d, np.arange(ca[g])):
                d = np.sort(rng.permutation(ca[g] + cb[g])[:ca[g]])
            assert np.array_equal(d, a[s][g])
    # E = 2: the only other labelling
    assert all(np.array_equal(r[0], [1]) for r in sg.label_draws(np.random.default_rng(0), 5, [1], [1]))
    for bad in (([0], [3]), ([3], [0]), ([2, 2], [1])):
        with pytest.raises(ValueError):
            sg.label_draws(np.random.default_rng(0), 2, *bad)


# ------------------------------------------------------------------------------------------------------- refusals
def test_contrast_args_refuses_before_the_gpu():
    bands = (np.array([0, 4]), np.array([4, 8]))
    ok = dict(measure="ffdtf", n_surrogates=10, m=6, tail="two-sided", split=None, check=True, bands=bands, counts_a=[3, 2],
              counts_b=[2, 4])
    assert sg.contrast_args(**ok) == (10, None)
    assert sg.contrast_args(**dict(ok, split=3, tail="less", check="nan")) == (10, 3)
    for over, msg in [(dict(measure="dtf"), "measure"), (dict(n_surrogates=0), "n_surrogates"),
                      (dict(n_surrogates=2.5), "n_surrogates"), (dict(n_surrogates=True), "n_surrogates"),
                      (dict(tail="both"), "tail"), (dict(split=0), "split"), (dict(split=6), "split"), (dict(split=2.0), "split"),
                      (dict(check=False), "check"), (dict(check="mask"), "check"), (dict(bands=None), "bands"),
                      (dict(bands=((), ())), "bands"), (dict(bands=(np.array([0, 1]), np.array([2]))), "bands"),
                      (dict(counts_a=[3, 0]), "group 1"), (dict(counts_b=[0, 4]), "group 0"),
                      (dict(counts_a=[], counts_b=[]), "at least one group")]:
        with pytest.raises(ValueError, match=msg):
            sg.contrast_args(**dict(ok, **over))
    assert np.array_equal(sg.tested_mask(4, "phase", 0), ~np.eye(4, dtype=bool))


def test_front_ends_refuse_before_the_gpu():
    """Nothing below reaches `default_engine()`: there is no GPU here and the engine would raise RuntimeError."""
    from hyperscanning_signal_analysis_amd.sliding import sliding_ensemble_contrast, sliding_ensemble_epochs_contrast
    import hyperscanning_signal_analysis_amd.sliding as sl
    assert "sliding_ensemble_contrast" in sl.__all__ and "sliding_ensemble_epochs_contrast" in sl.__all__
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4, 1000))
    oa, ob = np.array([100, 300, 500]), np.array([200, 400])
    freqs = np.linspace(1, 40, 8)
    bands = band_bins(freqs, ((0.0, 20.0), (20.0, 50.0)))
    kw = dict(pre=10, post=90, hop=20, measure="ffdtf", n_surrogates=5, seed=0)
    for over, args, msg in [(dict(), (x, oa, ob, 50, None, freqs, 100.0, bands), "integer model order"),
                            (dict(measure="pdc"), (x, oa, ob, 50, 2, freqs, 100.0, bands), "measure"),
                            (dict(n_surrogates=0), (x, oa, ob, 50, 2, freqs, 100.0, bands), "n_surrogates"),
                            (dict(tail="up"), (x, oa, ob, 50, 2, freqs, 100.0, bands), "tail"),
                            (dict(split=4), (x, oa, ob, 50, 2, freqs, 100.0, bands), "split"),
                            (dict(check="mask"), (x, oa, ob, 50, 2, freqs, 100.0, bands), "check"),
                            (dict(), (x, oa, ob, 50, 2, freqs, 100.0, None), "bands"),
                            (dict(), (x, oa, np.array([], dtype=int), 50, 2, freqs, 100.0, bands), "no onsets"),
                            (dict(), (np.stack([x, x]), [oa, oa], [ob], 50, 2, freqs, 100.0, bands), "onset array")]:
        with pytest.raises(ValueError, match=msg):
            sliding_ensemble_contrast(*args, **dict(kw, **over))
    ea, eb = rng.standard_normal((4, 100, 3)), rng.standard_normal((4, 100, 2))
    kw = dict(measure="gpdc", n_surrogates=5, seed=0)
    for over, args, msg in [(dict(), (ea, eb, 50, 20, None, freqs, 100.0, bands), "integer model order"),
                            (dict(tail=None), (ea, eb, 50, 20, 2, freqs, 100.0, bands), "tail"),
                            (dict(), (ea, [eb], 50, 20, 2, freqs, 100.0, bands), "both be arrays or both be lists"),
                            (dict(), (ea, eb[:3], 50, 20, 2, freqs, 100.0, bands), "same channels and samples"),
                            (dict(), ([ea, ea], [eb], 50, 20, 2, freqs, 100.0, bands), "same number of groups"),
                            (dict(), (ea, eb[:, :, :0], 50, 20, 2, freqs, 100.0, bands), "no trials")]:
        with pytest.raises(ValueError, match=msg):
            sliding_ensemble_epochs_contrast(*args, **dict(kw, **over))


def test_c_entries_refuse_without_a_gpu():
    """The codes of include/hypermvar.h, before any launch: -1 channels, -2 order, -3 n <= p, -4 null / misaligned pointers, -7
    workspace, -10 n_trials / n_win / n_mix < 1."""
    lib = _lib.load()
    D = 0x1000          # a non-null, 16-byte aligned "device pointer" that is never dereferenced on the host

    def mix(Rt=D, nt=2, nw=2, W=D, nm=2, m=6, p=3, R=D):
        return lib.hmv_lagcov_mix_f64(Rt, nt, nw, W, 0, nm, m, p, R, 0)
    assert mix(m=0) == -1 and mix(m=65) == -1 and b"channel count" in lib.hmv_last_error()
    assert mix(p=0) == -2 and mix(p=33) == -2
    assert mix(nt=0) == -10 and mix(nw=0) == -10 and mix(nm=0) == -10 and b"n_mix" in lib.hmv_last_error()
    assert mix(Rt=0) == -4 and mix(W=0) == -4 and mix(R=0) == -4 and mix(Rt=D + 8) == -4 and mix(R=D + 8) == -4

    def sm(meas=0, Rt=D, nt=2, nw=2, W=D, nm=2, m=6, n=60, p=3, f=D, F=8, out=D, nbands=0, S=0, iyw=D, itf=D, ws=D, nbytes=1 << 30,
           chunk=4):
        return lib.hmv_sliding_mix_f64(meas, Rt, nt, nw, W, 0, nm, m, n, p, f, F, 100.0, out, D if nbands else 0,
                                       D if nbands else 0, nbands, S, 0, 0, iyw, itf, ws, nbytes, chunk, 1.0, 0, 0, 0)
    assert sm(m=65) == -1 and sm(p=0) == -2 and sm(p=33) == -2 and sm(n=3) == -3
    assert sm(nt=0) == -10 and sm(nw=0) == -10 and sm(nm=0) == -10
    for bad in (dict(Rt=0), dict(W=0), dict(f=0), dict(out=0), dict(iyw=0), dict(itf=0), dict(ws=0), dict(F=0), dict(chunk=0),
                dict(meas=3), dict(meas=-1), dict(nbands=-1), dict(S=D, meas=1), dict(S=D, nbands=2), dict(Rt=D + 8)):
        assert sm(**bad) == -4, bad
    assert sm(meas=2, itf=0, nbytes=8) == -7           # GPDC has no info_tf: a null one passes the pointer checks
    need = lib.hmv_mix_workspace_bytes(0, 4, 6, 3, 8, 0)
    assert need > 0 and sm(nbytes=need - 1) == -7 and b"workspace" in lib.hmv_last_error()
    # the workspace is that of the pairs entry (no hop-block scratch); -1 for sizes no entry accepts
    for meas in (0, 1, 2):
        for nbands in (-1, 0, 3):
            assert lib.hmv_mix_workspace_bytes(meas, 5, 20, 4, 16, nbands) == lib.hmv_pairs_workspace_bytes(meas, 5, 20, 100, 4, 16, nbands)
    assert lib.hmv_mix_workspace_bytes(0, 0, 6, 3, 8, 0) == -1 and lib.hmv_mix_workspace_bytes(0, 4, 65, 3, 8, 0) == -1
    assert lib.hmv_mix_workspace_bytes(0, 4, 6, 33, 8, 0) == -1 and lib.hmv_mix_workspace_bytes(3, 4, 6, 3, 8, 0) == -1


def test_header_and_signatures_list_the_new_entries():
    txt = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in (("hmv_lagcov_mix_f64", 10), ("hmv_mix_workspace_bytes", 6), ("hmv_sliding_mix_f64", 29)):
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define HMV_VERSION (\d+)", txt).group(1)) == 160


# ------------------------------------------------------------------------------------------------------ linearity
@pytest.mark.parametrize("m,n,p,E", [(6, 70, 3, 5), (20, 100, 4, 9), (64, 100, 8, 4)])
def test_mix_of_per_trial_covariances_is_the_ensemble_estimator(m, n, p, E):
    """What the kernel rests on, on the pinned oracle: the weighted sum (numpy.einsum) of the per-trial lag covariances with
    weights 1 on the selected trials and scale 1 / E_c equals the oracle's lag covariances of the 3-D stack of those trials.
    Both are sums of the same E_c n products per element in two orders, so they differ by at most
    (E n + n + E + 6) eps / 2 mean_e sqrt(d_e[i] d_e[j]), d_e the lag-0 diagonal of trial e (the worst case of two
    orders of one sum: |x_i x_j| summed over a trial is at most n sqrt(d_i d_j) by Cauchy-Schwarz)."""
    rng = np.random.default_rng(100 * m + E)
    x = np.stack([coloured(rng, (m, n)) for _ in range(E)], axis=2)                  # (m, n, E)
    Rt = np.stack([O.lag_covariances(x[:, :, e], p) for e in range(E)])              # (E, p+1, m, m)
    for sel in (np.arange(E), np.arange(0, E, 2), np.array([E - 1])):
        W = np.zeros(E)
        W[sel] = 1.0
        got = np.einsum("e,elij->lij", W, Rt) * (1.0 / len(sel))
        want = O.lag_covariances(x[:, :, sel], p)
        d = np.stack([np.diag(Rt[e, 0]) for e in sel])
        bound = (len(sel) * n + n + len(sel) + 6) * np.finfo(float).eps / 2 * np.sqrt(d[:, :, None] * d[:, None, :]).mean(0)
        err = np.abs(got - want)
        print(f"m={m} n={n} p={p} E_c={len(sel)}: max err / bound {float((err / bound[None]).max()):.3f}")
        assert (err <= bound[None]).all()


# ----------------------------------------------------------------------------------------------- planted contrast
def test_planted_contrast_on_the_restatement():
    """What the statistic means.  0 -> 2 is coupled in condition A only, 1 -> 3 in both: the contrast at (2, 0) is significant
    after the max-statistic correction in every window, the cells (3, 1) and (0, 2) are not.  The other cells of row 2 are
    NOT asserted on: the ffDTF normalises every row by its total inflow, so the extra inflow from channel 0 in condition A
    lowers every other entry of row 2 as well and they come out significant too -- a significant cell localises the row,
    not necessarily the source."""
    n, hop, p, fs, S, seed = (PLANT[k] for k in ("n", "hop", "p", "fs", "S", "seed"))
    ep_a, ep_b = planted_conditions()
    lo, hi = band_bins(PLANT_FREQS, ((0.0, 50.0),))
    offsets = np.arange(0, PLANT["L"] - n + 1, hop)
    assert len(offsets) == 3
    r, _ = restate("ffdtf", [ep_a], [ep_b], offsets, n, p, PLANT_FREQS, fs, lo, hi, S, seed)
    assert "group" not in r and (r["n_valid"] == S).all()
    print("planted: D[2,0]", r["observed"][0, :, 2, 0, 0], "p_fwe[2,0]", r["p_fwe"][0, :, 2, 0, 0], "p[3,1]", r["p"][0, :, 3, 1, 0],
          "p[0,2]", r["p"][0, :, 0, 2, 0])
    assert (r["p_fwe"][0, :, 2, 0, 0] <= 0.05).all()
    assert (r["p"][0, :, 3, 1, 0] > 0.05).all() and (r["p"][0, :, 0, 2, 0] > 0.05).all()
    assert (r["observed"][0, :, 2, 0, 0] > 0.3).all()
