"""CPU-side checks of the FAD entry points: symbols in the header / ctypes table / library, argument refusals without a
device, the host-only components table on a dict rebuilt from the reference's outputs (tests/golden/g9_fad.npz), and
the univariate-input check of fad_decomposition before any device work."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAD_SYMBOLS = ("hmv_fad_workspace_bytes", "hmv_fad_f64", "hmv_fad_decompose_f64")


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    return _lib.load()


def test_fad_symbols_declared_bound_and_exported(lib):
    from hyperscanning_signal_analysis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hypermvar.h")).read()
    for s in FAD_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", hdr), s
        assert s in _lib.SIGNATURES
        assert hasattr(lib, s)
    assert lib.hmv_version() >= 130


def test_fad_argument_checks_without_gpu(lib):
    D = 8                                            # never dereferenced: every call below is refused first
    outs = [D] * 16 + [0]                            # 16 outputs, stream

    def fad(m=1, n=100, pmax=20, order=0, crit=0, x=D, outs=outs):
        return lib.hmv_fad_f64(x, 0, 100, D, D, 1, m, n, pmax, order, crit, 250.0, 1e-8, 1, *outs)

    assert lib.hmv_fad_workspace_bytes(100, 20) == 0
    assert lib.hmv_fad_workspace_bytes(100, 33) < 0 and lib.hmv_fad_workspace_bytes(-1, 8) < 0
    assert fad(m=0) == -1 and fad(m=65) == -1
    assert b"channel count" in lib.hmv_last_error()
    assert fad(pmax=0) == -2 and fad(pmax=33) == -2
    assert fad(n=20) == -3 and fad(n=5, pmax=8) == -3
    assert fad(x=0) == -4
    assert fad(outs=[D] * 15 + [0, 0]) == -4         # info
    assert fad(crit=3) == -5 and fad(crit=-1) == -5
    assert b"criterion" in lib.hmv_last_error()
    assert fad(order=21) == -6 and fad(order=-1) == -6
    dec = [D] * 12 + [0]
    assert lib.hmv_fad_decompose_f64(D, 1, 0, 250.0, 1e-8, 1, *dec) == -2
    assert lib.hmv_fad_decompose_f64(D, 1, 33, 250.0, 1e-8, 1, *dec) == -2
    assert lib.hmv_fad_decompose_f64(0, 1, 8, 250.0, 1e-8, 1, *dec) == -4
    assert lib.hmv_fad_decompose_f64(D, 1, 8, 250.0, 1e-8, 1, *([D] * 11 + [0, 0])) == -4


def golden_dict(g, c):
    pc = {k: g[f"{c}__pc_{k}"] for k in ("pole_index", "poles", "C", "alpha", "freq_hz", "omega_rad_s", "beta",
                                          "bandwidth_hz", "phi", "B")}
    return {"model_order": int(g[f"{c}__model_order"]), "paired_components": pc}


def test_components_table_columns_rounding_and_errors(golden):
    from hyperscanning_signal_analysis_amd.mtmvar import fad_components_table
    g = golden("g9_fad.npz")
    d = golden_dict(g, "ar6_p8")
    pc = d["paired_components"]
    k = len(pc["freq_hz"])
    t = fad_components_table(d, output="ndarray")
    assert t.shape == (k, 11) and t.dtype == np.float64
    np.testing.assert_array_equal(t[:, 0], np.arange(1, k + 1))
    np.testing.assert_array_equal(t[:, 1], pc["freq_hz"])
    np.testing.assert_array_equal(t[:, 2], pc["omega_rad_s"])
    np.testing.assert_array_equal(t[:, 3], pc["beta"])
    np.testing.assert_array_equal(t[:, 4], pc["bandwidth_hz"])
    np.testing.assert_array_equal(t[:, 5], pc["B"])
    np.testing.assert_array_equal(t[:, 6], pc["phi"])
    np.testing.assert_array_equal(t[:, 7:9], np.c_[pc["poles"].real, pc["poles"].imag])
    np.testing.assert_array_equal(t[:, 9:11], np.c_[pc["C"].real, pc["C"].imag])
    np.testing.assert_array_equal(fad_components_table(d, output="ndarray", decimals=3), np.round(t, 3))
    assert fad_components_table({"paired_components": {k: v[:0] for k, v in pc.items()}}, "ndarray").shape == (0, 11)
    with pytest.raises(ValueError, match="paired_components"):
        fad_components_table({"model_order": 3})
    with pytest.raises(ValueError, match="output must be"):
        fad_components_table(d, output="csv")


def test_components_table_dataframe(golden):
    pd = pytest.importorskip("pandas")
    from hyperscanning_signal_analysis_amd.mtmvar import fad_components_table
    g = golden("g9_fad.npz")
    d = golden_dict(g, "unpaired")
    df = fad_components_table(d, decimals=4)
    assert isinstance(df, pd.DataFrame)
    assert list(df.columns) == ['component', 'freq_hz', 'omega_rad_s', 'beta_s_1', 'bandwidth_hz', 'B', 'phi_rad',
                                'pole_real', 'pole_imag', 'residue_real', 'residue_imag']
    assert df["component"].dtype.kind == "i" and list(df["component"]) == list(range(1, len(df) + 1))
    np.testing.assert_array_equal(df["freq_hz"].to_numpy(), np.round(d["paired_components"]["freq_hz"], 4))


def test_fad_decomposition_refuses_multirow_input_before_device_work(monkeypatch):
    from hyperscanning_signal_analysis_amd import mtmvar

    def no_device():
        raise AssertionError("device touched")
    monkeypatch.setattr(mtmvar, "default_engine", no_device)
    with pytest.raises(ValueError, match="univariate signal"):
        mtmvar.fad_decomposition(np.zeros((2, 100)), 250.0)
    with pytest.raises(ValueError, match="univariate signal"):
        mtmvar.fad_decomposition(np.zeros((100, 1)), 250.0)
    with pytest.raises(ValueError, match="Invalid criterion"):
        mtmvar.fad_decomposition(np.zeros(100), 250.0, crit_type="BIC")
    assert {"fad_decomposition", "fad_decomposition_batch", "fad_components_table"} <= set(mtmvar.__all__)
    from hyperscanning_signal_analysis_amd import sliding
    assert "sliding_fad" in sliding.__all__
