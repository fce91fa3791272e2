"""The front of the fused ffDTF step cut in two (csrc/capi.hip, sliding_front): where a chunk's K2 -> K3 hand-over is split
after c0 windows and its K1 can be cut there too, the second stream forks behind K1 of the first part and runs the rest of
K1, its lagcomb and K2's second part beside the first part's lagcomb and K2.  Only the order of the launches changes, so
every comparison here is bit for bit against the same call with HMV_TUNE_K3_SPLIT at HMV_K3_SPLIT_NO_FRONT (the sequence
without the K1 cut, split by the rule of tests/test_gpu_k3_split.py), into NaN-poisoned outputs and scratch.
All @pytest.mark.gpu.

Regular grid: 40 windows of k hops of 500 samples (enough for 64 channels at p = 8), first window at sample 4, 32
frequencies, normalisation lag forced to 8; k = 2 and 4 (1 and 3 hop blocks shared between the two parts of K1), p = 8 and
3, m = 64 (hand-scheduled K3 body) and 20.
The samples of windows 3 and 38 are zero in every channel, so both are singular (one in each part at the split points up
to 38; at 39 the second part is window 39 alone).
Single windows (no grid, the direct form of K1): the batch of tests/test_gpu_k3_split.py at p = 3 -- items 3 and 38 the
exactly rank-deficient fixture, item 39 the nearly collinear one that goes through the LDL^T re-solve in the second part.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import _lib
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.synthetic import synthetic_var_dyad

HOP, FIRST, FS, ITEMS, LAG, F = 500, 4, 500.0, 40, 8, 32
SINGULAR, GUARDED = (3, 38), 39
SHAPES = [(m, p, k) for m in (64, 20) for p in (8, 3) for k in (2, 4)]      # all of them at the split points
SOME = [(64, 8, 2), (64, 3, 4), (20, 8, 4), (20, 3, 2)]                     # each value of each size, at the other cases
SPLITS = [8, 9, 24, 38, 39]
BANDS = ([0, 10], [10, 32])


def bits(t):
    return t.contiguous().view(torch.int64)


def never():
    return _lib.K3_SPLIT_NO_FRONT


class Batch:
    """Recordings and window tables on the device.  k > 0: `recs` recordings of `nwin` windows of k hops each on the regular
    grid, item = rec * nwin + w; k = 0: 40 single windows of 200 samples with the exceptional items, no grid."""

    def __init__(self, eng, golden, m, p, k, recs=1, nwin=ITEMS):
        self.eng, self.m, self.p, self.k = eng, m, p, k
        self.n = HOP * k if k else 200
        self.nwin = nwin
        if k:
            self.T = FIRST + self.n + (nwin - 1) * HOP
            x = np.stack([synthetic_var_dyad(17 + r + m + p, m=m, p=p, T=self.T, burn=300) for r in range(recs)])
            if nwin == ITEMS:
                for w in SINGULAR:
                    x[:, :, FIRST + w * HOP:FIRST + w * HOP + self.n] = 0.0
            rec = [r for r in range(recs) for _ in range(nwin)]
            start = [FIRST + w * HOP for _ in range(recs) for w in range(nwin)]
        else:
            g = golden("g6_errors.npz")
            self.T = self.n + (ITEMS - 1) * 100
            x = np.stack([synthetic_var_dyad(11 + r + m, m=m, p=p, T=self.T, burn=300) for r in range(3)])
            x[1, :4, :self.n] = g["nc1_x"][:, :self.n]
            x[2, :4, :self.n] = g["xs"][:, :self.n]
            rec, start = [0] * ITEMS, [100 * w for w in range(ITEMS)]
            for w in SINGULAR:
                rec[w], start[w] = 2, 0
            rec[GUARDED], start[GUARDED] = 1, 0
        self.items = len(rec)
        self.x = eng.to_device(x)
        self.rec = torch.tensor(rec, dtype=torch.int64, device=eng.device)
        self.start = torch.tensor(start, dtype=torch.int64, device=eng.device)

    def run(self, split, chunk=None, aux="own", flags=0, bands=None, want_model=False, F=F):
        """One hmv_sliding_ffdtf(_bands)_f64 call into poisoned buffers -> (out, info_yw, info_tf, ar)."""
        eng, lib, m, p, items = self.eng, self.eng.lib, self.m, self.p, self.items
        chunk = items if chunk is None else chunk
        mp = eng.pad(m)
        freqs = eng.to_device(2.0 * np.arange(1, F + 1))
        nb = 0 if bands is None else len(bands[0])
        nbytes = int((lib.hmv_sliding_bands_workspace_bytes if nb else lib.hmv_sliding_workspace_bytes)(chunk, m, p, F))
        assert nbytes > 0
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=eng.device)
        out = torch.full((items, m, m, nb or F), float("nan"), dtype=torch.float64, device=eng.device)
        info_yw = torch.full((items,), -77, dtype=torch.int32, device=eng.device)
        info_tf = torch.full((items * F,), -77, dtype=torch.int32, device=eng.device)
        ar = torch.full((items, mp, mp, p), float("nan"), dtype=torch.float64, device=eng.device) if want_model else None
        V = torch.full((items, mp, mp), float("nan"), dtype=torch.float64, device=eng.device) if want_model else None
        stream = eng.stream()
        aux = {"own": eng.aux_stream().cuda_stream, "none": 0, "same": stream}[aux]
        grid = (HOP, FIRST, self.nwin, self.T) if self.k else (0, 0, 0, 0)
        front = (self.x.data_ptr(), self.x.stride(0), self.x.stride(1), self.rec.data_ptr(), self.start.data_ptr(), items, m,
                 self.n, p, freqs.data_ptr(), F, FS, out.data_ptr())
        back = (ar.data_ptr() if want_model else 0, V.data_ptr() if want_model else 0, info_yw.data_ptr(), info_tf.data_ptr(),
                ws.data_ptr(), nbytes, chunk, eng.pivot_tau, flags, *grid, 0, 0, stream, aux)
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
        return out, info_yw, info_tf.view(items, F), ar


_cache = {}


def batch_and_reference(golden, m, p, k):
    """The batch of one shape and its result with the K1 cut off: computed once, shared, never written to."""
    if (m, p, k) not in _cache:
        b = Batch(default_engine(), golden, m, p, k)
        _cache[m, p, k] = (b, b.run(never()))
    return _cache[m, p, k]


def assert_same(got, ref):
    """Outputs and both info arrays equal bit for bit; no poison left in any window that K2 and K3 report as good."""
    out, info_yw, info_tf = got[:3]
    assert torch.equal(info_yw, ref[1]) and torch.equal(info_tf, ref[2])
    good = (info_yw == 0) & (info_tf == 0).all(dim=1)
    assert bool(good.any()) and not bool(torch.isnan(out[good]).any())
    assert torch.equal(bits(out), bits(ref[0]))


@pytest.mark.parametrize("m,p,k", SOME)
def test_the_grid_batch_is_what_it_is_meant_to_be(m, p, k, golden):
    _, (out, info_yw, info_tf, _) = batch_and_reference(golden, m, p, k)
    assert all(int(info_yw[w]) != 0 for w in SINGULAR)
    assert int((info_yw == 0).sum()) >= ITEMS // 2                    # (windows that are mostly zeros may fail as well)
    assert not bool(torch.isnan(out[info_yw == 0]).any())


def test_the_single_window_batch_is_what_it_is_meant_to_be(golden):
    b, (out, info_yw, info_tf, _) = batch_and_reference(golden, 20, 3, 0)
    assert all(int(info_yw[w]) != 0 for w in SINGULAR) and int(info_yw[GUARDED]) == 0
    ordinary = [w for w in range(ITEMS) if w not in SINGULAR]
    assert int(info_yw[ordinary].abs().sum()) == 0 and int(info_tf[ordinary].abs().sum()) == 0
    # the guarded window went through the LDL^T re-solve (its model is that form's), an ordinary one did not
    ar = b.run(never(), want_model=True)[3]
    ldlt = b.run(never(), want_model=True, flags=_lib.FLAG_YW_ONE_LAUNCH)[3]
    assert torch.equal(bits(ar[GUARDED]), bits(ldlt[GUARDED]))
    assert any(not torch.equal(bits(ar[w]), bits(ldlt[w])) for w in ordinary if w != GUARDED)


@pytest.mark.parametrize("c0", SPLITS)
@pytest.mark.parametrize("m,p,k", SHAPES)
def test_cut_front_equals_the_sequence_without_the_cut(m, p, k, c0, golden):
    b, ref = batch_and_reference(golden, m, p, k)
    assert_same(b.run(c0), ref)


@pytest.mark.parametrize("c0", SPLITS)
@pytest.mark.parametrize("m", [64, 20])
def test_single_windows_singular_and_guarded(m, c0, golden):
    """No grid: K1's two parts are item ranges of the direct form; the guarded window is re-solved on the second stream."""
    b, ref = batch_and_reference(golden, m, 3, 0)
    assert_same(b.run(c0), ref)


@pytest.mark.parametrize("m,p,k", SOME)
def test_split_without_the_cut_and_no_split_at_all(m, p, k, golden):
    b, ref = batch_and_reference(golden, m, p, k)
    assert_same(b.run(never() + 24), ref)
    assert_same(b.run(-1), ref)


@pytest.mark.parametrize("m,p,k", SOME)
def test_first_part_shorter_than_the_lag_runs_the_sequence_without_the_cut(m, p, k, golden):
    b, ref = batch_and_reference(golden, m, p, k)
    assert_same(b.run(LAG - 3), ref)


@pytest.mark.parametrize("m,p,k", SOME)
def test_direct_form_on_a_declared_grid(m, p, k, golden):
    b, _ = batch_and_reference(golden, m, p, k)
    assert_same(b.run(24, flags=_lib.FLAG_DIRECT_LAGCOV), b.run(never(), flags=_lib.FLAG_DIRECT_LAGCOV))


@pytest.mark.parametrize("m,p,k", SOME)
def test_band_sums(m, p, k, golden):
    b, _ = batch_and_reference(golden, m, p, k)
    assert_same(b.run(24, bands=BANDS), b.run(never(), bands=BANDS))


@pytest.mark.parametrize("m,p,k", SOME)
def test_unfused_normalisation(m, p, k, golden):
    b, ref = batch_and_reference(golden, m, p, k)
    assert_same(b.run(24, flags=_lib.FLAG_UNFUSED_NORM), ref)


@pytest.mark.parametrize("m,p,k", SOME)
def test_two_chunks_in_one_call(m, p, k, golden):
    """Chunks of 24 and 16 windows, both cut after 12: the second chunk's grid starts at window 24, the events are reused."""
    b, _ = batch_and_reference(golden, m, p, k)
    assert_same(b.run(12, chunk=24), b.run(never(), chunk=24))


@pytest.mark.parametrize("m,p,k", SOME)
def test_chunk_that_spans_two_recordings(m, p, k, golden):
    """Two recordings of 30 windows in chunks of 40: the first chunk spans both recordings and keeps K1 in one piece, the
    second (20 windows of the second recording) is cut after 12."""
    b = Batch(default_engine(), golden, m, p, k, recs=2, nwin=30)
    assert_same(b.run(12, chunk=40), b.run(never(), chunk=40))


@pytest.mark.parametrize("aux", ["none", "same"])
@pytest.mark.parametrize("k", [2, 0])
def test_no_second_stream_no_cut(aux, k, golden):
    b, ref = batch_and_reference(golden, 20, 3, k)
    assert_same(b.run(24, aux=aux), ref)


@pytest.mark.parametrize("rounds,over", [(1, 5), (2, 7)])
def test_automatic_rule(rounds, over, golden):
    """Chunks of CUs * rounds + over windows of one recording, CUs read from the device, at the forced lag of 8: the rule
    cuts both after the first CUs windows (given K2 holds three windows per compute unit, as it does at these sizes)."""
    eng = default_engine()
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    b = Batch(eng, golden, 20, 3, 2, nwin=cus * rounds + over)
    assert_same(b.run(0, F=16), b.run(never(), F=16))
