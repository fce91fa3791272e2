"""The single driver of the fused sliding-window calls (`Engine._sliding_call`): the four points on which the five earlier
drivers disagreed now follow the newer ones on every route, the two block Granger routes (second half of the file)
included.  The batch is ordinary windows with the exactly rank deficient window `xs` of g6_errors.npz among them, as in
tests/test_gpu_auto_order.py.  All @pytest.mark.gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd.engine import default_engine
    from hyperscanning_signal_analysis_amd.synthetic import mixed_order_recording

P, FS = 3, 64.0
FREQS = np.linspace(1.0, 30.0, 16)
BAD = [False, False, True, False, False]


@pytest.fixture(scope="module")
def case(golden):
    g = golden("g6_errors.npz")
    eng = default_engine()
    m, n = g["xs"].shape
    good = mixed_order_recording(100, m, [1, 2, 3, 5], n)
    batch = np.stack([good[:, :n], good[:, n:2 * n], g["xs"], good[:, 2 * n:3 * n], good[:, 3 * n:4 * n]])
    W = len(batch)
    rec = torch.arange(W, dtype=torch.int64, device=eng.device)
    st = torch.zeros(W, dtype=torch.int64, device=eng.device)
    keep = torch.as_tensor([k for k in range(W) if not BAD[k]], device=eng.device)
    return eng, eng.to_device(batch), rec, st, n, m, keep


def test_empty_batch_of_sliding_ffdtf_has_the_shape_and_the_tuple_of_a_full_one(case):
    eng, xd, rec, st, n, m, keep = case
    lo, hi = np.array([0, 4, 9]), np.array([4, 9, 16])
    none = (xd, rec[:0], st[:0], n, P, FREQS, FS)
    red = eng.sliding_ffdtf(*none, bands=(lo, hi))
    assert isinstance(red, torch.Tensor) and tuple(red.shape) == (0, m, m, 3)
    out, bad = eng.sliding_ffdtf(*none, check="mask")
    assert tuple(out.shape) == (0, m, m, len(FREQS)) and tuple(bad.shape) == (0,) and bad.dtype == torch.bool
    red, bad = eng.sliding_ffdtf(*none, bands=(lo, hi), check="mask")       # what stream_dyads unpacks
    assert tuple(red.shape) == (0, m, m, 3) and tuple(bad.shape) == (0,)
    assert tuple(eng.sliding_ffdtf(*none).shape) == (0, m, m, len(FREQS))


def test_fixed_order_spectra_know_every_form_of_check(case):
    eng, xd, rec, st, n, m, keep = case
    ref_ff, ref_S = eng.sliding_ffdtf_spectra(xd, rec[keep], st[keep], n, P, FREQS, FS)
    ff, S = eng.sliding_ffdtf_spectra(xd, rec, st, n, P, FREQS, FS, check="nan")
    assert bool(torch.isnan(ff[2]).all()) and bool(torch.isnan(torch.view_as_real(S[2])).all())
    assert torch.equal(ff[keep], ref_ff) and torch.equal(S[keep], ref_S)
    ff, S, bad = eng.sliding_ffdtf_spectra(xd, rec, st, n, P, FREQS, FS, check="mask")
    assert bad.cpu().tolist() == BAD and S.is_complex()
    assert torch.equal(ff[keep], ref_ff) and torch.equal(S[keep], ref_S)
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix") as ei:
        eng.sliding_ffdtf_spectra(xd, rec, st, n, P, FREQS, FS)
    assert list(ei.value.items) == [2]
    # the automatic order already did both
    ffa, Sa, bada = eng.sliding_ffdtf_spectra(xd, rec, st, n, None, FREQS, FS, check="mask", max_model_order=6)
    assert bada.cpu().tolist() == BAD


@pytest.mark.parametrize("measure", ["ffdtf", "ddtf", "gpdc"])
def test_mask_and_return_ar_together_give_both(case, measure):
    eng, xd, rec, st, n, m, keep = case
    fn = getattr(eng, "sliding_" + measure)
    mp = eng.pad(m)
    out, bad, ar, V, infos = fn(xd, rec, st, n, P, FREQS, FS, check="mask", return_ar=True)
    assert bad.cpu().tolist() == BAD
    assert tuple(ar.shape) == (len(BAD), mp, mp, P) and tuple(V.shape) == (len(BAD), mp, mp)
    ref, ref_ar, ref_V, ref_infos = fn(xd, rec, st, n, P, FREQS, FS, check=False, return_ar=True)
    assert torch.equal(out[keep], ref[keep]) and torch.equal(ar[keep], ref_ar[keep]) and torch.equal(V[keep], ref_V[keep])
    if measure == "gpdc":
        assert torch.equal(infos, ref_infos) and int(infos[2]) != 0
    else:
        assert torch.equal(infos[0], ref_infos[0]) and torch.equal(infos[1], ref_infos[1])
        assert int(infos[0][2]) != 0 or bool((infos[1].view(len(BAD), -1)[2] != 0).any())
    # the order of the automatic route and of the ensembles: (out, bad, ar, V, infos)
    auto = fn(xd, rec, st, n, None, FREQS, FS, check="mask", return_ar=True, max_model_order=6)
    assert len(auto) == 5 and auto[1].dtype == torch.bool


def test_sizes_the_library_refuses_are_a_value_error_on_every_route(case):
    eng, xd, rec, st, n, m, keep = case
    lo, hi = np.array([0, 4]), np.array([4, 16])
    for call in (lambda: eng.sliding_ffdtf(xd, rec, st, n, 33, FREQS, FS),
                 lambda: eng.sliding_ffdtf(xd, rec, st, n, 33, np.linspace(1.0, 30.0, 32), FS, bands=(lo, hi)),
                 lambda: eng.sliding_ffdtf_spectra(xd, rec, st, n, 33, FREQS, FS),
                 lambda: eng.sliding_ddtf(xd, rec, st, n, 33, FREQS, FS),
                 lambda: eng.sliding_gpdc(xd, rec, st, n, 33, FREQS, FS, bands=(lo, hi))):
        with pytest.raises(ValueError, match=r"bad sizes \(m=4, p=33, F=\d+, chunk=5\)"):
            call()


# ------------------------------------------------------------------ the block Granger routes of the same driver
SPLIT = 2
BLOCK_ENTRIES = ["sliding_block_granger", "sliding_block_granger_pairs"]


def _block(case, entry, items=slice(None), freqs=FREQS, p=P, **kw):
    """One of the two block entries on the windows `items` of the batch (the pairs entry with rec_b = rec_a)."""
    eng, xd, rec, st, n, m, keep = case
    if entry == "sliding_block_granger":
        return eng.sliding_block_granger(xd, rec[items], st[items], n, p, freqs, FS, split=SPLIT, **kw)
    return eng.sliding_block_granger_pairs(xd, rec[items], rec[items], st[items], n, p, freqs, FS, split=SPLIT, **kw)


@pytest.mark.parametrize("entry", BLOCK_ENTRIES)
def test_empty_batch_of_the_block_routes_has_the_shape_and_the_tuple_of_a_full_one(case, entry):
    eng, xd, rec, st, n, m, keep = case
    lo, hi = np.array([0, 4, 9]), np.array([4, 9, 16])
    none = slice(0, 0)
    spectral, time = _block(case, entry, none)
    assert tuple(spectral.shape) == (0, 2, len(FREQS)) and tuple(time.shape) == (0, 4)
    spectral, time = _block(case, entry, none, bands=(lo, hi))
    assert tuple(spectral.shape) == (0, 2, 3) and tuple(time.shape) == (0, 4)
    spectral, time, bad = _block(case, entry, none, bands=(lo, hi), check="mask")
    assert tuple(spectral.shape) == (0, 2, 3) and tuple(time.shape) == (0, 4)
    assert tuple(bad.shape) == (0,) and bad.dtype == torch.bool
    mp = eng.pad(m)
    spectral, time, bad, ar, V, infos = _block(case, entry, none, check="mask", return_ar=True)
    assert tuple(ar.shape) == (0, mp, mp, P) and tuple(V.shape) == (0, mp, mp) and len(infos) == 3
    if entry == "sliding_block_granger_pairs":
        spectral, time = _block(case, entry, none, freqs=None, want=("time",))
        assert spectral is None and tuple(time.shape) == (0, 4)
        spectral, time, bad = _block(case, entry, none, want=("spectral",), check="mask")
        assert time is None and tuple(spectral.shape) == (0, 2, len(FREQS)) and tuple(bad.shape) == (0,)
        spectral, time, (red, info_red) = _block(case, entry, none, return_red=True)
        assert tuple(red.shape) == (0, 2) and tuple(info_red.shape) == (0, 2) and info_red.dtype == torch.int32


@pytest.mark.parametrize("entry", BLOCK_ENTRIES)
def test_mask_and_return_ar_together_give_both_on_the_block_routes(case, entry):
    eng, xd, rec, st, n, m, keep = case
    mp, W, F = eng.pad(m), len(BAD), len(FREQS)
    spectral, time, bad, ar, V, infos = _block(case, entry, check="mask", return_ar=True)
    assert bad.cpu().tolist() == BAD
    assert tuple(spectral.shape) == (W, 2, F) and tuple(time.shape) == (W, 4)
    assert tuple(ar.shape) == (W, mp, mp, P) and tuple(V.shape) == (W, mp, mp)
    info_yw, info_red, info_gc = infos
    assert tuple(info_yw.shape) == (W,) and tuple(info_red.shape) == (W, 2) and tuple(info_gc.shape) == (W * F,)
    assert all(i.dtype == torch.int32 for i in infos)
    assert int(info_yw[2]) != 0 or bool(info_red[2].any()) or bool(info_gc.view(W, F)[2].any())
    ref_sp, ref_tm, ref_ar, ref_V, ref_infos = _block(case, entry, check=False, return_ar=True)
    assert torch.equal(spectral[keep], ref_sp[keep]) and torch.equal(time[keep], ref_tm[keep])
    assert torch.equal(ar[keep], ref_ar[keep]) and torch.equal(V[keep], ref_V[keep])
    assert all(torch.equal(a, b) for a, b in zip(infos, ref_infos))
    assert bool(torch.isfinite(spectral[keep]).all()) and bool(torch.isfinite(time[keep]).all())


@pytest.mark.parametrize("entry", BLOCK_ENTRIES)
def test_nan_fills_the_failed_window_of_both_block_outputs_and_nothing_else(case, entry):
    eng, xd, rec, st, n, m, keep = case
    ref_sp, ref_tm, ref_ar, ref_V, ref_infos = _block(case, entry, check=False, return_ar=True)
    r = _block(case, entry, check="nan", return_ar=True)
    assert len(r) == 5                                              # no mask: (spectral, time, ar, V, infos)
    spectral, time, ar, V, infos = r
    assert bool(torch.isnan(spectral[2]).all()) and bool(torch.isnan(time[2]).all())
    assert torch.equal(spectral[keep], ref_sp[keep]) and torch.equal(time[keep], ref_tm[keep])
    assert torch.equal(ar[keep], ref_ar[keep]) and torch.equal(V[keep], ref_V[keep])
    assert all(torch.equal(a, b) for a, b in zip(infos, ref_infos))
    lo, hi = np.array([0, 4]), np.array([4, 16])
    spectral, time = _block(case, entry, check="nan", bands=(lo, hi))
    assert bool(torch.isnan(spectral[2]).all()) and bool(torch.isnan(time[2]).all())
    assert torch.equal(spectral[keep], eng.band_sums(ref_sp, lo, hi)[keep]) and torch.equal(time[keep], ref_tm[keep])
    if entry == "sliding_block_granger_pairs":
        _, ref_time, (ref_red, ref_info_red) = _block(case, entry, freqs=None, want=("time",), return_red=True, check=False)
        sp, time, (red, info_red) = _block(case, entry, freqs=None, want=("time",), return_red=True, check="nan")
        assert sp is None and bool(torch.isnan(time[2]).all()) and torch.equal(time[keep], ref_time[keep])
        assert torch.equal(red[keep], ref_red[keep]) and bool(torch.isfinite(red[keep]).all())     # red is not filled
        assert torch.equal(info_red, ref_info_red)
        sp, time = _block(case, entry, want=("spectral",), check="nan")
        assert time is None and bool(torch.isnan(sp[2]).all()) and torch.equal(sp[keep], ref_sp[keep])


@pytest.mark.parametrize("entry", BLOCK_ENTRIES)
def test_check_true_names_the_failed_window_on_the_block_routes(case, entry):
    from hyperscanning_signal_analysis_amd.engine import SingularMatrixError
    with pytest.raises(SingularMatrixError, match="Singular matrix") as ei:
        _block(case, entry)
    assert list(ei.value.items) == [2]
    if entry == "sliding_block_granger_pairs":
        assert (f"(channels < {SPLIT} of recording 2 with channels >= {SPLIT} of recording 2, window at sample 0)"
                in str(ei.value.args[1]))
        assert list(ei.value.rec_a) == [2] and list(ei.value.rec_b) == [2] and list(ei.value.starts) == [0]
    else:
        assert "recording" not in str(ei.value.args[1])


def test_sizes_the_library_refuses_are_a_value_error_on_the_block_routes(case):
    """The "bad sizes" refusal of the block routes names split (and n, for pairs).  An order above 32 does not get that
    far on these two entries: `no_block_auto_order` refuses it first, as a ValueError of its own."""
    eng, xd, rec, st, n, m, keep = case
    for entry in BLOCK_ENTRIES:
        with pytest.raises(ValueError, match=r"p must be an integer in 1\.\.32, got 33"):
            _block(case, entry, p=33)
    with pytest.raises(ValueError, match=r"sliding_block_granger: bad sizes \(m=4, p=3, split=2, F=\d+, chunk=0\)"):
        _block(case, "sliding_block_granger", chunk=0)
    with pytest.raises(ValueError, match=rf"sliding_block_granger_pairs: bad sizes \(m=4, n={n}, p=3, split=2, F=\d+, chunk=0\)"):
        _block(case, "sliding_block_granger_pairs", chunk=0)
    with pytest.raises(ValueError, match=r"sliding_block_granger_pairs: bad sizes \(m=4, n=\d+, p=3, split=2, F=0, chunk=0\)"):
        _block(case, "sliding_block_granger_pairs", freqs=None, want=("time",), chunk=0)
