"""The K2 -> K3 hand-over of the fused ffDTF call in two parts (HMV_TUNE_K3_SPLIT): K2 solves the chunk's first c0 windows
on the main stream and the rest on the second stream while K3 already inverts the first c0; K3 comes as two launches that
share one normalisation protocol.  Nothing is computed differently, so every comparison here is bit for bit against the
same call with the split forced off (-1), into NaN-poisoned outputs and scratch.  All @pytest.mark.gpu.

Batch: 40 windows of n = 200 at hop 100, p = 2, normalisation lag forced to 8.  Items 3 and 38 are the exactly rank-deficient
fixture (tests/golden/g6_errors.npz, xs: singular), item 39 the cond-2e9 nearly collinear one (nc1: trips K2's conditioning
guard and goes through the LDL^T re-solve), built the way tests/test_gpu_k2_fused_tiles.py builds them.  Split points 8 (= lag),
9, 24, 38 and 39: a singular window in the first part at every one of them, the guarded window in the remainder at every one,
and a singular window in the remainder too except at 39, where the remainder is the guarded window alone.
Shapes: m = 64 (hand-scheduled K3 body), m = 20 (tf_inv_kernel<2>) at 32 frequencies, and m = 20 at 16 frequencies, where a
K3 workgroup owns the output rows f and f + 16.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

N, HOP, P, FS, ITEMS, LAG = 200, 100, 2, 500.0, 40, 8
SINGULAR, GUARDED = (3, 38), 39
SHAPES = [(64, 32), (20, 32), (20, 16)]
OFF = -1


def bits(t):
    return t.contiguous().view(torch.int64)


class Batch:
    """The recordings and window tables of one channel count, on the device."""

    def __init__(self, eng, golden, m, items=ITEMS, exceptional=True):
        g = golden("g6_errors.npz")
        n_grid = min(items, ITEMS)
        T = N + (n_grid - 1) * HOP
        x = np.stack([synthetic_var_dyad(11 + k + m, m=m, p=P, T=T, burn=300) for k in range(3)])
        x[1, :4, :N] = g["nc1_x"][:, :N]
        x[2, :4, :N] = g["xs"][:, :N]
        rec = [0] * items
        start = [HOP * (w % n_grid) for w in range(items)]
        if exceptional:
            for k in SINGULAR:
                rec[k], start[k] = 2, 0
            rec[GUARDED], start[GUARDED] = 1, 0
        self.eng, self.m, self.items = eng, m, items
        self.x = eng.to_device(x)
        self.rec = torch.tensor(rec, dtype=torch.int64, device=eng.device)
        self.start = torch.tensor(start, dtype=torch.int64, device=eng.device)

    def run(self, F, split, chunk=None, aux="own", flags=0, want_model=False, bands=None):
        """One hmv_sliding_ffdtf(_bands)_f64 call into poisoned buffers -> (out, info_yw, info_tf, ar, V)."""
        eng, lib, m, items = self.eng, self.eng.lib, self.m, self.items
        chunk = items if chunk is None else chunk
        mp = eng.pad(m)
        freqs = eng.to_device(2.0 * np.arange(1, F + 1))
        nb = 0 if bands is None else len(bands[0])
        nbytes = int((lib.hmv_sliding_bands_workspace_bytes if nb else lib.hmv_sliding_workspace_bytes)(chunk, m, P, F))
        assert nbytes > 0
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=eng.device)
        out = torch.full((items, m, m, nb or F), float("nan"), dtype=torch.float64, device=eng.device)
        info_yw = torch.full((items,), -77, dtype=torch.int32, device=eng.device)
        info_tf = torch.full((items * F,), -77, dtype=torch.int32, device=eng.device)
        ar = torch.full((items, mp, mp, P), float("nan"), dtype=torch.float64, device=eng.device) if want_model else None
        V = torch.full((items, mp, mp), float("nan"), dtype=torch.float64, device=eng.device) if want_model else None
        stream = eng.stream()
        aux = {"own": eng.aux_stream().cuda_stream, "none": 0, "same": stream}[aux]
        front = (self.x.data_ptr(), self.x.stride(0), self.x.stride(1), self.rec.data_ptr(), self.start.data_ptr(), items, m, N, P,
                 freqs.data_ptr(), F, FS, out.data_ptr())
        back = (ar.data_ptr() if want_model else 0, V.data_ptr() if want_model else 0, info_yw.data_ptr(), info_tf.data_ptr(),
                ws.data_ptr(), nbytes, chunk, eng.pivot_tau, flags, 0, 0, 0, 0, 0, 0, stream, aux)
        assert lib.hmv_set_tuning(_lib.TUNE_NORM_LAG, LAG) == 0 and lib.hmv_set_tuning(_lib.TUNE_K3_SPLIT, split) == 0
        try:
            with torch.cuda.device(eng.device):
                if nb:
                    lo = torch.tensor(bands[0], dtype=torch.int32, device=eng.device)
                    hi = torch.tensor(bands[1], dtype=torch.int32, device=eng.device)
                    rc = lib.hmv_sliding_ffdtf_bands_f64(*front, lo.data_ptr(), hi.data_ptr(), nb, *back)
                else:
                    rc = lib.hmv_sliding_ffdtf_f64(*front, *back)
            torch.cuda.synchronize()
        finally:
            assert lib.hmv_set_tuning(_lib.TUNE_NORM_LAG, 0) == 0 and lib.hmv_set_tuning(_lib.TUNE_K3_SPLIT, 0) == 0
        assert rc == 0, lib.hmv_last_error()
        return out, info_yw, info_tf.view(items, F), ar, V


_cache = {}


def batch_and_reference(golden, m, F):
    """The batch of m channels and its unsplit result at F frequencies: computed once, shared, never written to."""
    eng = default_engine()
    if ("batch", m) not in _cache:
        _cache["batch", m] = Batch(eng, golden, m)
    b = _cache["batch", m]
    if ("ref", m, F) not in _cache:
        _cache["ref", m, F] = b.run(F, OFF)
    return b, _cache["ref", m, F]


def assert_same(got, ref):
    """Outputs and both info arrays equal bit for bit; no poison left in any window that K2 and K3 report as good."""
    out, info_yw, info_tf = got[:3]
    assert torch.equal(info_yw, ref[1]) and torch.equal(info_tf, ref[2])
    good = (info_yw == 0) & (info_tf == 0).all(dim=1)
    assert not bool(torch.isnan(out[good]).any())
    assert torch.equal(bits(out), bits(ref[0]))


@pytest.mark.parametrize("m,F", SHAPES)
def test_the_batch_is_what_it_is_meant_to_be(m, F, golden):
    b, (out, info_yw, info_tf, _, _) = batch_and_reference(golden, m, F)
    assert all(int(info_yw[k]) != 0 for k in SINGULAR) and int(info_yw[GUARDED]) == 0
    ordinary = [k for k in range(ITEMS) if k not in SINGULAR]
    assert int(info_yw[ordinary].abs().sum()) == 0 and int(info_tf[ordinary].abs().sum()) == 0
    assert not bool(torch.isnan(out[ordinary]).any())
    # the guarded window went through the LDL^T re-solve (its model is that form's), an ordinary one did not
    ar = b.run(F, OFF, want_model=True)[3]
    ldlt = b.run(F, OFF, want_model=True, flags=_lib.FLAG_YW_ONE_LAUNCH)[3]
    assert torch.equal(bits(ar[GUARDED]), bits(ldlt[GUARDED]))
    assert any(not torch.equal(bits(ar[k]), bits(ldlt[k])) for k in ordinary if k != GUARDED)


@pytest.mark.parametrize("c0", [8, 9, 24, 38, 39])
@pytest.mark.parametrize("m,F", SHAPES)
def test_split_hand_over_equals_one_launch(m, F, c0, golden):
    b, ref = batch_and_reference(golden, m, F)
    assert_same(b.run(F, c0), ref)


@pytest.mark.parametrize("m,F", SHAPES)
def test_first_part_shorter_than_the_lag_falls_back_to_one_launch(m, F, golden):
    b, ref = batch_and_reference(golden, m, F)
    assert_same(b.run(F, LAG - 3), ref)


@pytest.mark.parametrize("m,F", SHAPES)
def test_two_chunks_in_one_call(m, F, golden):
    """Chunks of 24 and 16 windows, both split after 12: the events are reused and the counters zeroed per chunk."""
    b, _ = batch_and_reference(golden, m, F)
    assert_same(b.run(F, 12, chunk=24), b.run(F, OFF, chunk=24))


@pytest.mark.parametrize("aux", ["none", "same"])
def test_no_second_stream_no_split(aux, golden):
    b, ref = batch_and_reference(golden, 20, 32)
    assert_same(b.run(32, 24, aux=aux), ref)


def test_model_asked_for_no_split(golden):
    b, ref = batch_and_reference(golden, 20, 32)
    got, want = b.run(32, 24, want_model=True), b.run(32, OFF, want_model=True)
    assert_same(got, ref)
    good = [k for k in range(ITEMS) if k not in SINGULAR]
    assert not bool(torch.isnan(got[3][good]).any()) and not bool(torch.isnan(got[4][good]).any())
    assert torch.equal(bits(got[3]), bits(want[3])) and torch.equal(bits(got[4]), bits(want[4]))


@pytest.mark.parametrize("m,F", SHAPES)
def test_fused_equals_unfused_normalisation_with_the_split_on(m, F, golden):
    b, ref = batch_and_reference(golden, m, F)
    assert_same(b.run(F, 24, flags=_lib.FLAG_UNFUSED_NORM), ref)


def test_band_sums_with_the_split_on(golden):
    b, _ = batch_and_reference(golden, 20, 32)
    bands = ([0, 10], [10, 32])
    assert_same(b.run(32, 24, bands=bands), b.run(32, OFF, bands=bands))


@pytest.mark.parametrize("rounds,over", [(1, 5), (2, 7)])
def test_automatic_split_point(rounds, over, golden):
    """Chunks of CUs * k + r windows, CUs read from the device: whatever the rule decides, the result is the unsplit one."""
    eng = default_engine()
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    b = Batch(eng, golden, 20, items=cus * rounds + over, exceptional=False)
    assert_same(b.run(16, 0), b.run(16, OFF))
