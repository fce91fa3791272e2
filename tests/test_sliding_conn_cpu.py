"""CPU-side checks of the sliding-window dDTF / GPDC entries (hmv_sliding_ddtf_f64, hmv_sliding_gpdc_f64): workspace
sizing, refusal of bad arguments before anything touches a GPU, and escan_batch.run's refusal of an unknown measure."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


def test_version_and_workspace_sizes(lib):
    assert lib.hmv_version() >= 140
    for ws in (lib.hmv_sliding_ddtf_workspace_bytes, lib.hmv_sliding_gpdc_workspace_bytes):
        assert ws(1, 64, 8, 256, 0) > 0 and ws(7, 64, 8, 256, 0) > ws(1, 64, 8, 256, 0)
        assert ws(1, 64, 8, 256, 5) > ws(1, 64, 8, 256, 0)          # the band form keeps the chunk's full array
        for bad in ((0, 8, 4, 16, 0), (1, 65, 4, 16, 0), (1, 0, 4, 16, 0), (1, 8, 0, 16, 0), (1, 8, 33, 16, 0),
                    (1, 8, 4, 0, 0), (1, 8, 4, 16, -1)):
            assert ws(*bad) == -1, bad
    # dDTF: K1 / K2 / K3 scratch plus the per-window factors (p + 1 and 2 p + 1 matrices); GPDC launches no K3
    dd, gp = lib.hmv_sliding_ddtf_workspace_bytes(1, 64, 8, 256, 0), lib.hmv_sliding_gpdc_workspace_bytes(1, 64, 8, 256, 0)
    assert dd >= lib.hmv_sliding_workspace_bytes(1, 64, 8, 256) + 26 * 64 * 64 * 8
    assert gp < lib.hmv_sliding_workspace_bytes(1, 64, 8, 256) - 256 * 64 * 64 * 8


def _call(lib, which, m=8, n=100, p=4, F=16, chunk=4, out=1, n_items=1):
    """Every pointer a fake non-zero address: the argument checks must refuse before any of them is read."""
    P = 0x1000
    head = (P, 0, 100, P, P, n_items, m, n, p, P, F, 100.0, out, 0, 0, 0, 0, 0, P)
    tail = (0, 0, 0, 100, 0, 0)
    if which == "ddtf":
        return lib.hmv_sliding_ddtf_f64(*head, P, P, 1 << 40, chunk, 0.25, 0, *tail)
    return lib.hmv_sliding_gpdc_f64(*head, P, 1 << 40, chunk, 0, *tail)


@pytest.mark.parametrize("which", ["ddtf", "gpdc"])
def test_argument_checks_without_gpu(lib, which):
    name = f"hmv_sliding_{which}_f64".encode()
    cases = [(dict(m=65), -1, b"channel count"), (dict(p=33), -2, b"model order"), (dict(n=4, p=4), -3, b"window shorter"),
             (dict(F=0), -4, b"null pointer"), (dict(chunk=0), -4, b"null pointer"), (dict(out=0), -4, b"null pointer")]
    for kw, code, text in cases:
        assert _call(lib, which, **kw) == code, kw
        err = lib.hmv_last_error()
        assert text in err and err.startswith(name), (kw, err)
    assert _call(lib, which, n_items=0, out=0) == 0                         # empty batch: nothing to do
    # bands asked for without the bin tables
    P = 0x1000
    head = (P, 0, 100, P, P, 1, 8, 100, 4, P, 16, 100.0, P, 0, 0, 3, 0, 0, P)
    if which == "ddtf":
        rc = lib.hmv_sliding_ddtf_f64(*head, P, P, 1 << 40, 4, 0.25, 0, 0, 0, 0, 100, 0, 0)
    else:
        rc = lib.hmv_sliding_gpdc_f64(*head, P, 1 << 40, 4, 0, 0, 0, 0, 100, 0, 0)
    assert rc == -4 and b"band bins" in lib.hmv_last_error()


def test_escan_rejects_unknown_measure(tmp_path):
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    missing = tmp_path / "no_such_root"
    for bad in (("ffdtf", "pdc"), ("ddtf",), ("ffdtf", "ddtf", "ddtf")):
        with pytest.raises(ValueError, match="measures"):
            EB.run(missing, tmp_path / "out", measures=bad, verbose=False)
    assert not (tmp_path / "out").exists()                                  # refused before anything is read or made
    assert EB.MEASURES == ("ffdtf", "ddtf", "gpdc")
