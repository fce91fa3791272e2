"""CPU-side checks of the event-locked ensemble path: the new C-ABI entries are declared, bound and refuse bad arguments
before anything touches a GPU; `validate_trials` refuses every bad index description (one case per message);
`ensemble_items` gives the index lists one would write by hand; the oracle reproduces the reference's outputs on
(channels, samples, trials) input stored in tests/golden/g10_ensemble.npz; and there is no automatic order."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import mvar_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
NEW = ("hmv_lagcov_ensemble_workspace_doubles", "hmv_lagcov_ensemble_f64", "hmv_sliding_ensemble_workspace_bytes",
       "hmv_sliding_ensemble_f64")


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


P = 0x1000          # a fake non-zero device address: the checks must refuse before any pointer is read


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def assert_parity(out, ref, guard):
    """The rule of tests/test_gpu_parity.py, restated."""
    assert out.shape == ref.shape
    assert rel(out, ref) <= guard, rel(out, ref)
    if np.isrealobj(ref):
        row_max = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).min()
    else:
        row_max = np.abs(ref).max()
    assert np.allclose(out, ref, rtol=1e-5, atol=1e-5 * row_max)


def test_header_and_ctypes_table_agree_on_the_new_entries(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    assert int(re.search(r"#define HMV_VERSION (\d+)", hdr).group(1)) == 160 == lib.hmv_version()
    assert re.search(r"#define HMV_MAX_HOPS_ENSEMBLE 32\b", hdr) and re.search(r"#define HMV_MAX_HOPS_PER_WINDOW 8\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name)


def _k1(lib, m=8, n=100, p=5, x=P, trials=P, groups=P, items=P, R=P, n_groups=2, n_items=6, ws=P, ws_n=1 << 40, hop=0, nwin=0,
        flags=0, T=1000, ld=1000):
    return lib.hmv_lagcov_ensemble_f64(x, ld, ld, T, trials, trials, groups, n_groups, items, items, n_items, m, n, p, R, ws,
                                       ws_n, hop, nwin, flags, 0)


def _sl(lib, measure=0, m=8, n=100, p=5, F=4, out=P, nb=0, S=0, trials=P, groups=P, n_groups=2, n_items=6, ws=1 << 40, lo=0,
        hi=0, info_tf=P, hop=0, nwin=0, flags=0, T=1000, ld=1000):
    return lib.hmv_sliding_ensemble_f64(measure, P, ld, ld, T, trials, trials, groups, n_groups, P, P, n_items, m, n, p, P, F,
                                        100.0, out, lo, hi, nb, S, 0, 0, P, info_tf, P, ws, 2, 1.0, flags, hop, nwin, 0, 0)


def test_entries_refuse_bad_arguments(lib):
    grid = [(dict(hop=20, nwin=4), -9, b"inconsistent regular window grid"),          # 6 items != 2 groups x 4 windows
            (dict(hop=20, nwin=0), -9, b"inconsistent regular window grid"),
            (dict(hop=-1, nwin=3), -9, b"inconsistent regular window grid"),
            (dict(hop=20, nwin=3, T=130), -9, b"inconsistent regular window grid"),   # the last window ends at 140
            (dict(hop=20, nwin=3, ld=900), -9, b"inconsistent regular window grid")]
    common = [(dict(m=0), -1, b"channel count"), (dict(m=65), -1, b"channel count"), (dict(p=0), -2, b"model order"),
              (dict(p=33), -2, b"model order"), (dict(n=5), -3, b"window shorter"), (dict(trials=0), -4, b"null pointer"),
              (dict(groups=0), -4, b"null pointer"), (dict(n_groups=0), -10, b"n_groups")] + grid
    cases = [
        (_k1, b"hmv_lagcov_ensemble_f64", common + [(dict(x=0), -4, b"null pointer"), (dict(items=0), -4, b"null pointer"),
                                                    (dict(R=0), -4, b"null pointer"),
                                                    (dict(hop=20, nwin=3, ws_n=16), -7, b"workspace too small"),
                                                    (dict(hop=20, nwin=3, ws=0), -7, b"workspace too small")]),
        (_sl, b"hmv_sliding_ensemble_f64", common + [(dict(measure=3), -4, b"measure"), (dict(measure=-1), -4, b"measure"),
                                                     (dict(nb=-1), -4, b"n_bands"), (dict(out=0), -4, b"null pointer"),
                                                     (dict(nb=2), -4, b"band bins"), (dict(S=P, measure=1), -4, b"spectra"),
                                                     (dict(S=P, nb=2, lo=P, hi=P), -4, b"spectra"),
                                                     (dict(ws=16), -7, b"workspace too small"),
                                                     (dict(measure=1, info_tf=0), -4, b"null pointer")]),
    ]
    for fn, name, cs in cases:
        for kw, code, text in cs:
            assert fn(lib, **kw) == code, (name, kw, lib.hmv_last_error())
            err = lib.hmv_last_error()
            assert err.startswith(name) and text in err, (name, kw, err)
    # an empty batch is not an error, whatever the pointers
    assert _sl(lib, n_items=0, out=0) == 0
    assert _k1(lib, n_items=0) == 0


def test_workspace_sizing(lib):
    k1, sl = lib.hmv_lagcov_ensemble_workspace_doubles, lib.hmv_sliding_ensemble_workspace_bytes
    tile = 9 * 64 * 64
    assert k1(368, 64, 100, 8, 0, 0) == 0                                   # arbitrary offsets: the direct form, no scratch
    assert k1(368, 64, 100, 8, 5, 46) == 0                                  # hop <= p: direct by rule
    assert k1(368, 64, 100, 8, 30, 46) == 0                                 # not a whole number of hops
    assert k1(46, 64, 640, 8, 20, 46) == (46 + 32 - 1) * 2 * tile           # k = 32 is the limit ...
    assert k1(46, 64, 660, 8, 20, 46) == 0                                  # ... k = 33 goes direct
    assert k1(46, 64, 200, 8, 100, 46) == 0                                 # a hop block + lags wider than one LDS fill
    # 8 groups x 46 windows, k = 5: 50 hop blocks per group, one spare group for a chunk that starts inside one
    assert k1(368, 64, 100, 8, 20, 46) == (8 + 1) * 50 * tile
    for bad in ((368, 65, 100, 8, 20, 46), (368, 64, 100, 0, 20, 46), (368, 64, 8, 8, 20, 46), (-1, 64, 100, 8, 20, 46)):
        assert k1(*bad) == -1
    auto = lib.hmv_sliding_auto_workspace_bytes
    for meas in (0, 1, 2):
        for nb in (0, 3):
            direct = sl(meas, 16, 64, 100, 8, 64, nb, 0, 0)
            # no hop-block scratch at all in the direct form: less than the single-trial layout, which always carries it
            assert 0 < direct < auto(meas, 16, 64, 8, 64, nb)
            assert sl(meas, 16, 64, 100, 8, 64, nb, 20, 46) == direct + 8 * 2 * 50 * tile
    assert sl(0, 16, 64, 100, 8, 64, -1, 0, 0) > sl(0, 16, 64, 100, 8, 64, 0, 0, 0)       # spectra: H passes through
    assert sl(1, 16, 64, 100, 8, 64, -1, 0, 0) == -1 and sl(3, 16, 64, 100, 8, 64, 0, 0, 0) == -1
    assert sl(0, 0, 64, 100, 8, 64, 0, 0, 0) == -1 and sl(0, 16, 64, 8, 8, 64, 0, 0, 0) == -1


def _desc():
    x = torch.zeros(2, 4, 1000, dtype=torch.float64)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
    return dict(x=x, trial_rec=i64(0, 0, 1, 1, 1), trial_start=i64(10, 500, 0, 300, 700), group_ptr=i64(0, 2, 5),
                item_group=i64(0, 0, 1, 1), item_offset=i64(0, 100, 0, 200), n=100, p=5)


def test_validate_trials_names_the_first_offender():
    """Index contents go straight into kernel address arithmetic: they are checked on the host side first (pure tensor
    logic: runs on CPU tensors here), one case per message."""
    from hyperscanning_signal_analysis_amd.engine import validate_trials
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
    validate_trials(**_desc())                                        # fine: trial 4 ends at 700 + 200 + 100 = 1000
    validate_trials(**dict(_desc(), item_group=i64(), item_offset=i64()))     # empty batch
    validate_trials(**dict(_desc(), trial_start=i64(10, 500, 100, 300, 700), item_offset=i64(-10, 100, -100, 200)))
    for change, msg in [
        (dict(trial_rec=torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32)), "trial_rec must be a 1-D int64"),
        (dict(trial_start=torch.zeros(5)), "trial_start must be a 1-D int64"),
        (dict(group_ptr=torch.tensor([[0, 2, 5]])), "group_ptr must be a 1-D int64"),
        (dict(item_group=[0, 0, 1, 1]), "item_group must be a 1-D int64"),
        (dict(item_offset=torch.tensor([0, 100, 0, 200], dtype=torch.int32)), "item_offset must be a 1-D int64"),
        (dict(trial_start=i64(10, 500, 0, 300)), "trial_rec and trial_start must have the same length"),
        (dict(item_offset=i64(0, 100, 0)), "item_group and item_offset must have the same length"),
        (dict(n=5), r"window length \(5\) must exceed the model order \(5\)"),
        (dict(n=1001), "exceeds the recording length"),
        (dict(group_ptr=i64(0)), "at least two entries"),
        (dict(group_ptr=i64(1, 2, 5)), "must run from 0 to the number of trials"),
        (dict(group_ptr=i64(0, 2, 4)), "must run from 0 to the number of trials"),
        (dict(group_ptr=i64(0, 3, 2, 5)), r"non-decreasing \(group 1"),
        (dict(group_ptr=i64(0, 2, 2, 5)), "group 1 is empty"),
        (dict(trial_rec=i64(0, 0, 1, 2, 1)), r"trial_rec must lie in \[0, 2\), got 2 for trial 3"),
        (dict(trial_rec=i64(0, -1, 1, 1, 1)), r"trial_rec must lie in \[0, 2\), got -1 for trial 1"),
        (dict(item_group=i64(0, 0, 2, 1)), r"item_group must lie in \[0, 2\), got 2 for item 2"),
        (dict(item_offset=i64(0, 100, 0, 201)), r"item 3 \(group 1, offset 201\) of trial 4 covers \[901, 1001\)"),
        (dict(item_offset=i64(0, 100, -1, 200)), r"item 2 \(group 1, offset -1\) of trial 2 covers \[-1, 99\)"),
        (dict(trial_start=i64(10, 901, 0, 300, 700)), r"item 0 \(group 0, offset 0\) of trial 1 covers \[901, 1001\)"),
    ]:
        with pytest.raises(ValueError, match=msg):
            validate_trials(**dict(_desc(), **change))


def test_ensemble_items_against_hand_built_lists():
    from hyperscanning_signal_analysis_amd.sliding import ensemble_items, hop_positions
    st, off = ensemble_items([300, 120, 777], pre=20, post=100, window_size=50, hop=25)
    assert st.dtype == off.dtype == np.int64
    np.testing.assert_array_equal(st, [280, 100, 757])                    # onset - pre, in the order given
    np.testing.assert_array_equal(off, [0, 25, 50])                       # whole windows inside the 120-sample epoch
    st, off = ensemble_items(np.array([5]), 0, 24, 24, 6)
    np.testing.assert_array_equal(st, [5])
    np.testing.assert_array_equal(off, [0])
    assert len(ensemble_items([50], 0, 23, 24, 6)[1]) == 0                # the epoch is shorter than one window
    np.testing.assert_array_equal(ensemble_items([0], 10, 290, 100, 20)[1], hop_positions(300, 100, 20))
    with pytest.raises(ValueError, match="non-negative"):
        ensemble_items([50], -1, 24, 24, 6)
    with pytest.raises(ValueError, match="one-dimensional"):
        ensemble_items([[50]], 0, 24, 24, 6)
    with pytest.raises(ValueError, match="positive"):
        ensemble_items([50], 0, 24, 24, 0)


@pytest.mark.parametrize("case", ["a", "b"])
def test_oracle_reproduces_the_reference_on_trial_stacks(golden, case):
    """The oracle on `np.stack(trial windows, axis=2)` against the reference's stored outputs: the GPU tests may then
    use the oracle for every window of every shape."""
    g = golden("g10_ensemble.npz")
    x, onsets, freqs, fs = g[f"{case}__x"], g[f"{case}__onsets"], g[f"{case}__freqs"], float(g[f"{case}__fs"])
    p, n, hop = (int(g[f"{case}__{k}"]) for k in ("p", "n", "hop"))
    assert len(g[f"{case}__windows"]) == {"a": 17, "b": 4}[case]
    for k, w in enumerate(g[f"{case}__windows"]):
        stack = np.stack([x[:, s + w * hop:s + w * hop + n] for s in onsets], axis=2)
        ar, V = O.ar_coeff(stack, p)
        for got, key in ((O.full_freq_dtf(stack, freqs, fs, p), "ffdtf"), (O.multivariate_spectra(stack, freqs, fs, p), "spectra"),
                         (O.direct_dtf(stack, freqs, fs, p), "ddtf"),
                         (O.gen_partial_directed_coherence(stack, freqs, fs, p), "gpdc"), (ar, "ar"), (V, "V")):
            assert_parity(got, g[f"{case}__{key}"][k], 1e-12)


def test_no_automatic_order_for_ensembles(golden):
    """The reference's mvar_criterion unpacks `data.shape` into two names: ValueError on 3-D input.  There is no
    automatic order to reproduce, and p=None is refused before the GPU is touched."""
    from hyperscanning_signal_analysis_amd.sliding import sliding_ensemble, sliding_ensemble_epochs
    assert "too many values to unpack" in str(golden("g10_ensemble.npz")["criterion_error"])
    x = np.zeros((3, 400))
    with pytest.raises(ValueError, match="integer model order"):
        sliding_ensemble(x, [50, 100], 24, None, [1.0, 2.0], 100.0, pre=0, post=120, hop=6)
    with pytest.raises(ValueError, match="integer model order"):
        sliding_ensemble_epochs(np.zeros((3, 120, 4)), 24, 6, None, [1.0, 2.0], 100.0)
