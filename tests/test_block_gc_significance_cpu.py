"""CPU-side checks of the significance tests of block Granger causality: the new entry is declared, exported and bound; it
refuses bad arguments before any launch; the 2 x 2 meta-channel scatter and the argument checks are pure host code; and the
NumPy restatement of both tests (tests/block_gc_significance_restated.py) finds the planted coupling."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from hyperscanning_signal_analysis_amd import significance as S
from hyperscanning_signal_analysis_amd import surrogates as sg
from tests import block_gc_significance_restated as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
P = 0x1000            # a non-null "device pointer" that no refused call dereferences
ENTRY, WS = "hmv_sliding_block_gc_pairs_f64", "hmv_block_gc_pairs_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


def test_the_entry_is_declared_exported_and_bound(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hypermvar.h")).read(), flags=re.S)
    for name, n_args in ((ENTRY, 37), (WS, 8)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    # the arguments of hmv_sliding_block_gc_f64 with (T, rec_a, rec_b, item_start) for (item_rec, item_start) and the four
    # grid arguments, plus the three pair arguments, want, red_out, red_base, info_red_base
    assert len(_lib.SIGNATURES[ENTRY][1]) == len(_lib.SIGNATURES["hmv_sliding_block_gc_f64"][1]) + 2 - 4 + 3 + 4
    # not one of the closed table of hmv_sliding_*_workspace_bytes
    assert not (WS.startswith("hmv_sliding_") and WS.endswith("workspace_bytes"))


def _call(lib, **over):
    a = dict(x=P, rec_stride=8000, ld=1000, T=1000, rec_a=P, rec_b=P, item_start=P, n_items=6, m=8, n=100, p=5, split=4,
             freqs=P, F=4, fs=100.0, spectral=P, bin_lo=0, bin_hi=0, n_bands=0, time=P, ar_out=0, V_out=0, info_yw=P,
             info_red=P, info_gc=P, workspace=P, workspace_bytes=1 << 40, chunk=6, flags=0, R_base=0, base_a=0, base_b=0,
             want=3, red_out=0, red_base=0, info_red_base=0, stream=0)
    assert set(over) <= set(a)
    a.update(over)
    return getattr(lib, ENTRY)(*a.values())


def test_refusals_before_any_launch(lib):
    err = lambda: lib.hmv_last_error().decode()        # noqa: E731
    assert _call(lib, want=0) == -15 and "want" in err() and ENTRY in err()
    assert _call(lib, want=4) == -15
    # red_base: its rows are those of R_base, and it comes with its infos
    assert _call(lib, red_base=P, info_red_base=P) == -4 and "R_base" in err()
    assert _call(lib, red_base=P, info_red_base=P, R_base=P, base_a=P) == -4                 # (base_b missing: the pair check)
    assert _call(lib, red_base=P, R_base=P, base_a=P, base_b=P) == -4 and "info_red_base" in err()
    assert _call(lib, info_red_base=P, R_base=P, base_a=P, base_b=P) == -4
    for split in (0, 8, -1):
        assert _call(lib, split=split) == -11 and "split" in err()
    assert _call(lib, m=65) == -1 and _call(lib, p=33) == -2 and _call(lib, n=5) == -3
    assert _call(lib, n_items=-1) == -4 and _call(lib, rec_b=0) == -4
    assert _call(lib, F=0) == -12 and _call(lib, spectral=0) == -13 and _call(lib, n_bands=-1) == -14
    assert _call(lib, want=1, info_gc=0) == -4 and _call(lib, want=2, time=0) == -4 and _call(lib, want=2, info_red=0) == -4
    assert _call(lib, workspace_bytes=1024) == -7
    # an empty batch is nothing to do, with or without the frequency grid
    assert _call(lib, n_items=0) == 0 and _call(lib, n_items=0, want=2, F=0, freqs=0, spectral=0, info_gc=0) == 0


def test_workspace_sizes(lib):
    ws = getattr(lib, WS)
    both, spec, time = ws(7, 8, 100, 5, 4, 16, 0, 3), ws(7, 8, 100, 5, 4, 16, 0, 1), ws(7, 8, 100, 5, 4, 16, 0, 2)
    assert 0 < time < spec < both
    assert ws(7, 8, 100, 5, 4, 16, 2, 3) > both                   # the band form keeps the chunk's full array in scratch
    assert ws(7, 8, 100, 5, 4, 0, -3, 2) == time                  # time alone: F and n_bands are not looked at
    for bad in ((0, 8, 100, 5, 4, 16, 0, 3), (7, 65, 100, 5, 4, 16, 0, 3), (7, 8, 5, 5, 4, 16, 0, 3), (7, 8, 100, 33, 4, 16, 0, 3),
                (7, 8, 100, 5, 0, 16, 0, 3), (7, 8, 100, 5, 8, 16, 0, 3), (7, 8, 100, 5, 4, 0, 0, 3), (7, 8, 100, 5, 4, 16, -1, 1),
                (7, 8, 100, 5, 4, 16, 0, 0), (7, 8, 100, 5, 4, 16, 0, 4)):
        assert ws(*bad) < 0, bad


def test_meta_layout_on_cpu_tensors():
    time = torch.arange(12, dtype=torch.float64).view(3, 4) + 100.0          # (F_ab, F_ba, F_i, F_tot) per item
    bands = torch.arange(18, dtype=torch.float64).view(3, 2, 3)              # [item][dir][band]
    for t, b, nv in ((time, bands, 4), (time, None, 1), (None, bands, 3)):
        meta = S.block_meta(t, b)
        assert tuple(meta.shape) == (3, 2, 2, nv) and meta.dtype == torch.float64 and meta.device.type == "cpu"
        assert torch.isnan(meta[:, 0, 0]).all() and torch.isnan(meta[:, 1, 1]).all()
        col = 0
        if t is not None:                                                    # the time value first ...
            assert torch.equal(meta[:, 1, 0, 0], t[:, 0]) and torch.equal(meta[:, 0, 1, 0], t[:, 1])
            col = 1
        if b is not None:                                                    # ... then the bands
            assert torch.equal(meta[:, 1, 0, col:], b[:, 0]) and torch.equal(meta[:, 0, 1, col:], b[:, 1])
    # the tested mask of the drivers is the off-diagonal: the diagonal is never tested
    assert np.array_equal(sg.tested_mask(2, "phase", 0), [[False, True], [True, False]])
    # and back: the leaves of a result dict, index 0 = A -> B
    meta = S.block_meta(time, bands)
    res = {k: meta.view(3, 2, 2, 4) for k in ("observed",) + S.STATS}
    leaves = S.block_leaves(res, ("time", "bands"))
    assert torch.equal(leaves["time"]["p"], time[:, :2]) and torch.equal(leaves["bands"]["observed"], bands)
    assert set(S.block_leaves(res, ("time",))) == {"time"}
    only = S.block_leaves({k: S.block_meta(None, bands) for k in ("observed",) + S.STATS}, ("bands",))
    assert set(only) == {"bands"} and torch.equal(only["bands"]["null_std"], bands)


def test_argument_checks():
    assert sg.block_want(("spectral", "time")) == (True, True) and sg.block_want("time") == (False, True)
    assert sg.block_want(["spectral"]) == (True, False)
    for bad in ((), ("time", "time"), ("bands",), "both", ("spectral", "x")):
        with pytest.raises(ValueError, match="want"):
            sg.block_want(bad)
    bands = ([0, 4], [4, 8])
    assert sg.block_values(("bands", "time"), bands) == ("time", "bands") and sg.block_values("time", None) == ("time",)
    for bad in ((), ("spectral",), ("time", "time")):
        with pytest.raises(ValueError, match="values"):
            sg.block_values(bad, bands)
    for b in (None, ([], []), ([0], [1, 2])):
        with pytest.raises(ValueError, match="bands"):
            sg.block_values(("time", "bands"), b)
    ok = dict(null="shift", n_surrogates=9, m=6, T=1000, n=200, split=2)
    assert sg.block_significance_args(**ok, bands=bands) == (9, 2, 200, ("time", "bands"))
    assert sg.block_significance_args(**dict(ok, null="phase", T=200), values=("time",)) == (9, 2, 200, ("time",))
    for over, msg in ((dict(null="trial"), "null"), (dict(n_surrogates=0), "n_surrogates"), (dict(n_surrogates=2.0), "integer"),
                      (dict(split=0), "split"), (dict(split=6), "split"), (dict(split=None), "split"), (dict(T=399), "min_shift"),
                      (dict(min_shift=-1), "min_shift"), (dict(check="mask"), "check"), (dict(values=("bands",), bands=None), "bands")):
        with pytest.raises(ValueError, match=msg):
            sg.block_significance_args(**{**dict(ok, bands=bands), **over})
    assert sg.block_pseudo_dyad_args(4, 6, None, None, 3, ("time",)) == (None, 3, ("time",))
    assert sg.block_pseudo_dyad_args(4, 6, 5, 1, 3, bands=bands) == (5, 3, ("time", "bands"))
    for args, msg in (((1, 6, None, None, 3), "at least 2 dyads"), ((4, 6, 5, None, 3), "seed"), ((4, 6, 0, 1, 3), "n_surrogates"),
                      ((4, 6, None, None, 6), "split"), ((4, 6, None, None, 3, ("bands",)), "bands")):
        with pytest.raises(ValueError, match=msg):
            sg.block_pseudo_dyad_args(*args)
    with pytest.raises(ValueError, match="check"):
        sg.block_pseudo_dyad_args(4, 6, None, None, 3, ("time",), None, False)
    # what was there stays as it was
    assert sg.MEASURES == ("ffdtf", "ddtf", "gpdc") and sg.NULLS == ("shift", "phase")


def test_the_restatement_finds_the_planted_coupling():
    """The figures the GPU test of the planted coupling rests on, on the host: observed F_{A->B} against every pseudo-dyad
    and every shift-null value, and the p values that follow."""
    c = BR.PLANTED
    x = BR.planted_dyads()
    D = len(x)
    partners = sg.partner_derangements(None, None, D)
    args = (c["n"], c["p"], c["freqs"], c["fs"], c["lo"], c["hi"])
    dyad, group, gap = BR.restate_pseudo_dyads(x, c["starts"], *args, c["split"], partners)
    obs, null = dyad["observed"], dyad["null"]
    print(f"time: observed A->B >= {obs[..., 0, 0].min():.4g}, null <= {null[..., 0].max():.4g};  bands: observed A->B >= "
          f"{obs[..., 0, 1].min():.4g}, null <= {null[..., 1].max():.4g};  gap {gap:.3g}")
    assert obs.shape == (D, 2, 2, 2) and null.shape == (2 * (D - 1), D, 2, 2, 2)
    assert obs[..., 0, 0].min() >= 1.246 and null[..., 0].max() <= 0.165
    assert obs[..., 0, 1].min() >= 19.9 and null[..., 1].max() <= 2.51
    assert (dyad["p"][:, :, 0] == 1.0 / 9.0).all() and (dyad["p_fwe"][:, :, 0] == 1.0 / 9.0).all()
    assert (group["p"][:, 0] == 1.0 / 5.0).all() and (group["p_fwe"][:, 0] == 1.0 / 5.0).all()
    assert (dyad["n_valid"] == 2 * (D - 1)).all() and (group["n_valid"] == D - 1).all()
    # the total is the sum of its three parts, and every part is positive on these data
    t = dyad["observed_time"]
    assert np.allclose(t[..., 3], t[..., :3].sum(-1), rtol=0, atol=1e-12) and (t > 0).all()
    sh, _ = BR.restate_surrogates("shift", x, c["starts"], *args, 19, 7, c["split"])
    print(f"shift null: time null <= {sh['null'][..., 0].max():.4g}")
    assert sh["null"][..., 0].max() <= 0.173
    assert (sh["p"][:, 0] == 1.0 / 20.0).all() and (sh["p_fwe"][:, 0] == 1.0 / 20.0).all() and (sh["n_valid"] == 19).all()
