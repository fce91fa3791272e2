"""CPU side of the trial-shuffle significance test of event-locked ensembles: the documented draws, the tested family, the
argument checks of the Python entry points before any GPU is touched, and the refusals of the two C entries."""
import os
import re
import subprocess

import numpy as np
import pytest

from hyperscanning_signal_analysis_amd import surrogates as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
P = 0x1000            # a non-null "device pointer" that no refused call dereferences


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


def test_trial_permutations_draw_order_and_identity_redraw():
    counts = [2, 5, 3]
    perms = sg.trial_permutations(np.random.default_rng(7), 40, counts)
    # the documented order: surrogate-major, group-minor, one rng.permutation per (s, g), drawn again while the identity
    rng = np.random.default_rng(7)
    redraws = 0
    for s in range(40):
        for g, c in enumerate(counts):
            pi = rng.permutation(c)
            while np.array_equal(pi, np.arange(c)):
                pi = rng.permutation(c)
                redraws += 1
            assert perms[s][g].dtype == np.int64 and np.array_equal(perms[s][g], pi), (s, g)
            assert sorted(pi) == list(range(c)) and not np.array_equal(pi, np.arange(c))
    assert redraws > 0                                      # 40 draws of 2 trials: the identity does come up
    again = sg.trial_permutations(np.random.default_rng(7), 40, counts)
    assert all(np.array_equal(a, b) for ra, rb in zip(perms, again) for a, b in zip(ra, rb))
    other = sg.trial_permutations(np.random.default_rng(8), 40, counts)
    assert any(not np.array_equal(a, b) for ra, rb in zip(perms, other) for a, b in zip(ra, rb))
    assert all((p[0] == [1, 0]).all() for p in perms)       # two trials: the swap is the only other arrangement
    for bad in ([1], [4, 1, 3], [0, 2]):
        with pytest.raises(ValueError, match="at least 2 trials"):
            sg.trial_permutations(np.random.default_rng(0), 3, bad)


def test_tested_family_and_arguments_of_the_trial_null():
    assert np.array_equal(sg.tested_mask(6, "trial", 2), sg.tested_mask(6, "shift", 2))
    assert sg.tested_mask(5, "trial", 2).sum() == 2 * 2 * 3
    assert sg.significance_args("gpdc", "trial", 10, 8, 100, 60) == (10, 4, 60)
    assert sg.significance_args("ffdtf", "trial", 1, 7, 100, 60, split=3)[:2] == (1, 3)
    assert sg.significance_args("ffdtf", "trial", 5, 6, 100, 100)[1] == 3          # no T >= 2 min_shift rule: nothing is shifted
    for kw, msg in [(dict(m=7), "explicit split"), (dict(split=0), "split must be in"), (dict(split=6), "split must be in"),
                    (dict(split=2.0), "integer"), (dict(S=0), "n_surrogates"), (dict(measure="dtf"), "measure must be")]:
        a = dict(dict(measure="ffdtf", S=10, m=6, split=None), **kw)
        with pytest.raises(ValueError, match=msg):
            sg.significance_args(a["measure"], "trial", a["S"], a["m"], 100, 60, a["split"])
    with pytest.raises(ValueError, match="null must be one of"):
        sg.significance_args("ffdtf", "bootstrap", 10, 6, 100, 60)
    assert sg.NULLS == ("shift", "phase") and sg.ENSEMBLE_NULLS == ("trial",)
    with pytest.raises(ValueError, match="null must be one of"):        # the ESCan driver keeps to the continuous nulls
        sg.check_significance_dict(dict(null="trial", n_surrogates=5, seed=1))


def test_front_ends_refuse_bad_arguments_before_the_gpu():
    """Every refusal below comes before `default_engine()`, which raises RuntimeError where there is no GPU."""
    from hyperscanning_signal_analysis_amd.sliding import (sliding_ensemble_epochs_significance,
                                                           sliding_ensemble_significance, sliding_significance)
    rng = np.random.default_rng(0)
    ep = rng.standard_normal((6, 120, 5))
    x = rng.standard_normal((6, 2000))
    on = np.array([100, 400, 900])
    freqs = np.arange(1.0, 9.0)
    bands = ([0, 4], [4, 8])
    ok = dict(measure="ffdtf", n_surrogates=10, seed=1, split=3)
    cases = [(dict(split=0), "split must be in"), (dict(split=6), "split must be in"), (dict(split=True), "integer"),
             (dict(measure="coh"), "measure must be"), (dict(n_surrogates=0), "n_surrogates"),
             (dict(n_surrogates=2.5), "integer"), (dict(check="mask"), "check must be")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            sliding_ensemble_epochs_significance(ep, 60, 30, 3, freqs, 100.0, bands, **dict(ok, **kw))
        with pytest.raises(ValueError, match=msg):
            sliding_ensemble_significance(x, on, 60, 3, freqs, 100.0, bands, pre=20, post=100, hop=30, **dict(ok, **kw))
    for b in (None, ([], []), ([0, 4], [4])):
        with pytest.raises(ValueError, match="at least one band"):
            sliding_ensemble_epochs_significance(ep, 60, 30, 3, freqs, 100.0, b, **ok)
    with pytest.raises(ValueError, match="integer model order"):
        sliding_ensemble_epochs_significance(ep, 60, 30, None, freqs, 100.0, bands, **ok)
    with pytest.raises(ValueError, match="integer model order"):
        sliding_ensemble_significance(x, on, 60, None, freqs, 100.0, bands, pre=20, post=100, hop=30, **ok)
    with pytest.raises(ValueError, match="explicit split"):
        sliding_ensemble_epochs_significance(ep[:5], 60, 30, 3, freqs, 100.0, bands, **dict(ok, split=None))
    with pytest.raises(ValueError, match="at least 2 trials"):
        sliding_ensemble_epochs_significance([ep, ep[:, :, :1]], 60, 30, 3, freqs, 100.0, bands, **ok)
    with pytest.raises(ValueError, match="at least 2 trials"):
        sliding_ensemble_significance(x, on[:1], 60, 3, freqs, 100.0, bands, pre=20, post=100, hop=30, **ok)
    with pytest.raises(ValueError, match="shape"):
        sliding_ensemble_epochs_significance(ep[0], 60, 30, 3, freqs, 100.0, bands, **ok)
    # the trial shuffle is no null of a continuous recording
    with pytest.raises(ValueError, match="event-locked"):
        sliding_significance(x, 200, 3, 3, freqs, 100.0, bands, measure="ffdtf", null="trial", n_surrogates=5, seed=1)


def test_header_declares_the_two_entries_with_the_ctypes_arity(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, base, extra in (("hmv_lagcov_ensemble_split_f64", "hmv_lagcov_ensemble_f64", 5 - 4),
                              ("hmv_sliding_ensemble_split_f64", "hmv_sliding_ensemble_f64", 5 - 2)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl, name
        args = [a.strip() for a in decl.group(1).split(",") if a.strip()]
        assert len(_lib.SIGNATURES[name][1]) == len(args) == len(_lib.SIGNATURES[base][1]) + extra, name
        for new in ("trial_rec_b", "trial_start_b", "split", "R_base", "item_base"):
            assert any(a.split()[-1].lstrip("*") == new for a in args), (name, new)
        assert not any("grid" in a or "workspace_doubles" in a for a in args), name
        assert hasattr(lib, name)
    assert "validate_trials" in hdr[hdr.index("Trial-shuffle surrogates"):hdr.index("int hmv_lagcov_ensemble_split_f64")]


def _k1(lib, m=8, n=100, p=5, x=P, trials=P, groups=P, items=P, R=P, n_groups=2, n_items=6, rec_b=P, start_b=P, split=4, Rb=0,
        ib=0):
    return lib.hmv_lagcov_ensemble_split_f64(x, 1000, 1000, 1000, trials, trials, groups, n_groups, items, items, n_items, m, n,
                                             p, R, rec_b, start_b, split, Rb, ib, 0, 0)


def _sl(lib, measure=0, m=8, n=100, p=5, F=4, out=P, nb=0, n_groups=2, n_items=6, ws=1 << 40, rec_b=P, start_b=P, split=4,
        Rb=0, ib=0, trials=P):
    return lib.hmv_sliding_ensemble_split_f64(measure, P, 1000, 1000, 1000, trials, trials, P, n_groups, P, P, n_items, m, n, p,
                                              P, F, 100.0, out, 0, 0, nb, 0, 0, 0, P, P, P, ws, 2, 1.0, 0, rec_b, start_b,
                                              split, Rb, ib, 0, 0)


def test_entries_refuse_bad_arguments(lib):
    """Before any launch, with the code numbers of the entries they extend."""
    for call in (_k1, _sl):
        for kw, code, msg in [(dict(m=65), -1, b"channel count"), (dict(p=33), -2, b"model order"), (dict(n=5), -3, b"shorter"),
                              (dict(trials=0), -4, b"null pointer"), (dict(n_groups=0), -10, b"n_groups"),
                              (dict(split=0), -5, b"split must be in 1..m-1"), (dict(split=8), -5, b"split must be in 1..m-1"),
                              (dict(split=-2), -5, b"split must be in 1..m-1"), (dict(rec_b=0), -4, b"second trial table"),
                              (dict(start_b=0), -4, b"second trial table"), (dict(Rb=P), -4, b"go together"),
                              (dict(ib=P), -4, b"go together")]:
            assert call(lib, **kw) == code, (call.__name__, kw)
            err = lib.hmv_last_error()
            assert msg in err and (b"hmv_lagcov_ensemble_split_f64" if call is _k1 else b"hmv_sliding_ensemble_split_f64") in err
    assert _k1(lib, n_items=0) == 0 and _sl(lib, n_items=0) == 0              # empty batches: nothing to do
    assert _sl(lib, measure=3) == -4 and _sl(lib, ws=64) == -7 and b"workspace too small" in lib.hmv_last_error()
    assert _sl(lib, out=0) == -4
    # the workspace is that of the ensemble entry without a grid
    assert lib.hmv_sliding_ensemble_workspace_bytes(2, 7, 8, 100, 5, 4, 3, 0, 0) > 0
