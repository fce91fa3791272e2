"""HMV_TUNE_K3_SPLIT (include/hypermvar.h): the tuning index of the two-part K2 -> K3 hand-over, its range and its default.
No GPU: argument checks of the C ABI only."""
import os

import pytest

from hyperscanning_signal_analysis_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_split_index_range_and_default(lib):
    key = _lib.TUNE_K3_SPLIT
    assert key == 6
    if "HYPERMVAR_K3_SPLIT" not in os.environ:
        assert lib.hmv_get_tuning(key) == 0                             # 0: the automatic rule
    try:
        for v in (-1, 1, 512, 1 << 20):
            assert lib.hmv_set_tuning(key, v) == 0 and lib.hmv_get_tuning(key) == v
        for v in (-2, (1 << 20) + 1):
            assert lib.hmv_set_tuning(key, v) < 0 and b"out of range" in lib.hmv_last_error()
            assert lib.hmv_get_tuning(key) == 1 << 20                   # a refused value changes nothing
    finally:
        assert lib.hmv_set_tuning(key, 0) == 0
    assert lib.hmv_set_tuning(key + 1, 0) < 0 and lib.hmv_get_tuning(key + 1) == -1


def test_the_other_indices_keep_their_lower_bound(lib):
    for key in (_lib.TUNE_NORM_LAG, _lib.TUNE_LAG_GROUP, _lib.TUNE_K3_FORM, _lib.TUNE_YW_FORM, _lib.TUNE_K3_LDS_PAD):
        before = lib.hmv_get_tuning(key)
        assert lib.hmv_set_tuning(key, -1) < 0 and lib.hmv_get_tuning(key) == before
