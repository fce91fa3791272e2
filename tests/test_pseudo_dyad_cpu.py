"""CPU side of the pseudo-dyad (shuffled-partner) test: the documented partner draws, the refusals of the two C entries
without a launch, the ValueErrors of the Python entry points before any GPU is touched, and the host logic of
`escan_batch.run_pseudo_dyads` with an injected reader and a stub engine."""
import json
import os
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


# ----------------------------------------------------------------------------------------------------- partner draws
def test_seeded_partners_follow_the_documented_draws():
    D, S = 5, 60
    got = sg.partner_derangements(np.random.default_rng(3), S, D)
    assert got.shape == (S, D) and got.dtype == np.int64
    rng = np.random.default_rng(3)                             # the documented order: one permutation per surrogate, drawn
    redraws = 0                                                # again while it has a fixed point
    for s in range(S):
        pi = rng.permutation(D)
        while np.any(pi == np.arange(D)):
            pi = rng.permutation(D)
            redraws += 1
        assert np.array_equal(got[s], pi), s
    assert redraws > 0                                         # most permutations of 5 have a fixed point
    assert (got != np.arange(D)).all() and (np.sort(got, axis=1) == np.arange(D)).all()
    assert np.array_equal(got, sg.partner_derangements(np.random.default_rng(3), S, D))
    assert not np.array_equal(got, sg.partner_derangements(np.random.default_rng(4), S, D))


def test_exhaustive_partners_are_the_cyclic_offsets():
    for D in (2, 3, 4, 7):
        pi = sg.partner_derangements(None, None, D)
        assert pi.shape == (D - 1, D) and pi.dtype == np.int64
        for k in range(1, D):
            assert np.array_equal(pi[k - 1], (np.arange(D) + k) % D)
        pairs = sorted((d, int(pi[s, d])) for s in range(D - 1) for d in range(D))
        assert pairs == [(d, j) for d in range(D) for j in range(D) if j != d]          # every ordered pair exactly once
        for d in range(D):          # every other dyad is d's partner once on each side
            assert sorted(pi[:, d]) == sorted(int(np.argsort(pi[s])[d]) for s in range(D - 1)) == [j for j in range(D) if j != d]
    assert np.array_equal(sg.partner_derangements(None, None, 2), [[1, 0]])
    assert (sg.partner_derangements(np.random.default_rng(0), 9, 2) == [1, 0]).all()    # two dyads: the swap, every time


def test_partner_refusals():
    rng = np.random.default_rng(0)
    for D in (1, 0):
        with pytest.raises(ValueError, match="at least 2 dyads"):
            sg.partner_derangements(rng, None, D)
        with pytest.raises(ValueError, match="at least 2 dyads"):
            sg.partner_derangements(rng, 3, D)
    for S, msg in ((0, "n_surrogates must be >= 1"), (-2, "n_surrogates must be >= 1"), (2.5, "integer"), (True, "integer")):
        with pytest.raises(ValueError, match=msg):
            sg.partner_derangements(rng, S, 4)
    with pytest.raises(ValueError, match="random generator"):
        sg.partner_derangements(None, 3, 4)
    assert sg.pseudo_dyad_args("gpdc", 3, 8, None, None) == (None, 4)
    assert sg.pseudo_dyad_args("ffdtf", 2, 7, 10, 1, split=3, check="nan") == (10, 3)
    # the two existing families of nulls are as they were
    assert sg.NULLS == ("shift", "phase") and sg.ENSEMBLE_NULLS == ("trial",)


# ------------------------------------------------------------------------------------------------------- C refusals
def _k1(lib, m=8, n=100, p=5, x=P, rec_a=P, rec_b=P, start=P, R=P, n_items=6, split=4, Rb=0, ba=0, bb=0):
    return lib.hmv_lagcov_pairs_f64(x, 1000, 1000, 1000, rec_a, rec_b, start, n_items, m, n, p, split, R, Rb, ba, bb, 0, 0)


def _sl(lib, measure=0, m=8, n=100, p=5, F=4, out=P, nb=0, n_items=6, ws=1 << 40, rec_a=P, rec_b=P, start=P, split=4, Rb=0,
        ba=0, bb=0):
    return lib.hmv_sliding_pairs_f64(measure, P, 1000, 1000, 1000, rec_a, rec_b, start, n_items, m, n, p, P, F, 100.0, out, 0, 0,
                                     nb, 0, 0, 0, P, P, P, ws, 2, 1.0, 0, split, Rb, ba, bb, 0, 0)


def test_entries_refuse_bad_arguments(lib):
    """Before any launch, with the code numbers of the ensemble-split entries for the same faults."""
    for call, name in ((_k1, b"hmv_lagcov_pairs_f64"), (_sl, b"hmv_sliding_pairs_f64")):
        for kw, code, msg in [(dict(m=65), -1, b"channel count"), (dict(m=0), -1, b"channel count"),
                              (dict(p=33), -2, b"model order"), (dict(p=0), -2, b"model order"), (dict(n=5), -3, b"shorter"),
                              (dict(rec_a=0), -4, b"null pointer"), (dict(start=0), -4, b"null pointer"),
                              (dict(rec_b=0), -4, b"rec_b"), (dict(Rb=P), -4, b"go together"),
                              (dict(ba=P), -4, b"go together"), (dict(bb=P), -4, b"go together"),
                              (dict(Rb=P, ba=P), -4, b"go together"), (dict(Rb=P, bb=P), -4, b"go together"),
                              (dict(ba=P, bb=P), -4, b"go together"),
                              (dict(split=0), -5, b"split must be in 1..m-1"), (dict(split=8), -5, b"split must be in 1..m-1"),
                              (dict(split=-2), -5, b"split must be in 1..m-1")]:
            assert call(lib, **kw) == code, (call.__name__, kw)
            err = lib.hmv_last_error()
            assert msg in err and name in err, (kw, err)
    assert _k1(lib, n_items=0) == 0 and _sl(lib, n_items=0) == 0              # empty batches: nothing to do
    assert _k1(lib, R=0) == -4 and _sl(lib, out=0) == -4 and _sl(lib, measure=3) == -4 and _sl(lib, nb=-1) == -4
    assert _sl(lib, ws=64) == -7 and b"hmv_sliding_pairs_f64: workspace too small" in lib.hmv_last_error()
    # the workspace is the ensemble entry's without a grid; bad sizes give -1
    for meas in (0, 1, 2):
        for nb in (-1, 0, 3):
            want = lib.hmv_sliding_ensemble_workspace_bytes(meas, 7, 8, 100, 5, 4, nb, 0, 0)
            assert lib.hmv_pairs_workspace_bytes(meas, 7, 8, 100, 5, 4, nb) == want
            assert (want > 0) == (nb >= 0 or meas == 0)        # n_bands = -1: the ffDTF with spectra only
    for bad in ((0, 7, 65, 100, 5, 4, 0), (0, 7, 8, 5, 5, 4, 0), (0, 0, 8, 100, 5, 4, 0), (3, 7, 8, 100, 5, 4, 0),
                (0, 7, 8, 100, 33, 4, 0)):
        assert lib.hmv_pairs_workspace_bytes(*bad) == -1, bad


# ------------------------------------------------------------------------------------------- ValueErrors before the GPU
def test_python_entries_refuse_bad_arguments_before_the_gpu():
    """The front-end refuses before `default_engine()`, which raises RuntimeError where there is no GPU; the engine method
    refuses before it looks at the device of x (an engine that was never initialised stands in for one)."""
    import torch
    from hyperscanning_signal_analysis_amd.engine import Engine
    from hyperscanning_signal_analysis_amd.sliding import sliding_pseudo_dyad_significance
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 6, 400))
    freqs = np.arange(1.0, 9.0)
    bands = ([0, 4], [4, 8])
    eng = object.__new__(Engine)
    starts = torch.tensor([0, 100], dtype=torch.int64)

    def front(x=x, p=3, bands=bands, **kw):
        return sliding_pseudo_dyad_significance(x, 200, 2, p, freqs, 100.0, bands, **dict(dict(measure="ffdtf"), **kw))

    def engine(x=x, p=3, bands=bands, **kw):
        return eng.pseudo_dyad_significance(torch.as_tensor(x), starts, 200, p, freqs, 100.0, bands,
                                            **dict(dict(measure="ffdtf"), **kw))
    for call in (front, engine):
        for kw, msg in [(dict(x=x[:1]), "at least 2 dyads"), (dict(p=None), "automatic model order"),
                        (dict(bands=([], [])), "at least one band"), (dict(x=x[:, :5]), "explicit split"),
                        (dict(n_surrogates=4), "need a seed"), (dict(n_surrogates=0, seed=1), "n_surrogates must be >= 1"),
                        (dict(n_surrogates=-3, seed=1), "n_surrogates must be >= 1"),
                        (dict(n_surrogates=2.5, seed=1), "integer"), (dict(split=0), "split must be in"),
                        (dict(split=6), "split must be in"), (dict(split=True), "integer"), (dict(measure="coh"), "measure must be"),
                        (dict(check="mask"), "check must be")]:
            with pytest.raises(ValueError, match=msg):
                call(**kw)
    with pytest.raises(ValueError, match="at least one band"):
        front(bands=None)
    with pytest.raises(ValueError, match="shape"):
        front(x=x[0])


# -------------------------------------------------------------------------------------------- run_pseudo_dyads, host logic
FS = 100.0
CHANS = ["Fp1", "Fp2", "M1", "Cz"]


def _tree(tmp_path, lengths, no_caregiver=(), no_event=()):
    """<root>/EEG/<dyad>/<role>/<dyad>_EEG_<code>_movies.nc, one JSON file per member: the event `Peppa` starts at 1 s and
    lasts lengths[dyad] seconds."""
    root = tmp_path / "tree"
    for d, (dyad, dur) in enumerate(lengths.items()):
        for r, (code, role) in enumerate((("ch", "child"), ("cg", "caregiver"))):
            if code == "cg" and dyad in no_caregiver:
                continue
            path = root / "EEG" / dyad / role / f"{dyad}_EEG_{code}_movies.nc"
            path.parent.mkdir(parents=True, exist_ok=True)
            name = "Brave" if dyad in no_event else "Peppa"
            path.write_text(json.dumps({"seed": 10 * d + r, "events": [{"name": name, "start_rel_s": 1.0, "duration_s": dur}]}))
    return root


def _reader(path):
    spec = json.loads(open(path).read())
    n = int(12 * FS)
    x = np.random.default_rng(spec["seed"]).standard_normal((n, len(CHANS)))
    return {"data_tc": x, "time": np.arange(n) / FS, "channels": CHANS,
            "attrs": {"sampling_freq": FS, "task_events_structure": spec["events"]}}


class StubEngine:
    """Records what `run_pseudo_dyads` hands to the engine; returns arrays of the right shapes."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def to_device(self, a):
        import torch
        return torch.as_tensor(np.ascontiguousarray(a))

    def pseudo_dyad_significance(self, x, item_start, n, p, freqs, fs, bands, *, measure, split, n_surrogates, seed, check):
        import torch
        self.calls.append(dict(x=x.numpy().copy(), starts=item_start.numpy().copy(), n=n, p=p, fs=fs, measure=measure,
                               split=split, n_surrogates=n_surrogates, seed=seed, check=check, nb=len(bands[0])))
        D, m, _ = x.shape
        W, nb = len(item_start), len(bands[0])
        z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
        d = {k: z(D, W, m, m, nb) for k in ("observed", "p", "p_fwe", "null_mean", "null_std")}
        d["n_valid"] = torch.zeros(D, W, dtype=torch.int32)
        d["group"] = dict({k: z(W, m, m, nb) for k in ("observed", "p", "p_fwe", "null_mean", "null_std")},
                          n_valid=torch.zeros(W, dtype=torch.int32))
        d["partners"] = torch.as_tensor(sg.partner_derangements(None, None, D))
        return d


def test_run_pseudo_dyads_host_logic(tmp_path, capsys):
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    lengths = {"W_01": 6.0, "W_02": 5.7, "W_03": 6.0, "W_04": 4.0, "W_05": 6.0, "W_06": 6.0}
    root = _tree(tmp_path, lengths, no_caregiver=("W_05",), no_event=("W_06",))
    eng = StubEngine()
    res = EB.run_pseudo_dyads(root, tmp_path / "out", "movies", "Peppa", window_s=2.0, overlap=0.5, model_order=4,
                              freqs=np.arange(1.0, 41.0), measures=("ffdtf", "ddtf"), reader=_reader, engine=eng)
    log = capsys.readouterr().out
    assert res["dyads"] == ["W_01", "W_02", "W_03"]
    assert "[SKIP] W_05 movies/Peppa: missing caregiver file" in log and "[SKIP] W_06 movies/Peppa: no event 'Peppa'" in log
    assert "[SKIP] W_04 movies/Peppa: 401 samples < 0.9 of the longest segment (601)" in log
    assert sorted(d for d, _ in res["skipped"]) == ["W_04", "W_05", "W_06"]
    # cropped to the shortest of the dyads that stay (W_02: 5.7 s, inclusive cut), the child's 3 channels first
    assert [c["measure"] for c in eng.calls] == ["ffdtf", "ddtf"]
    c = eng.calls[0]
    assert c["x"].shape == (3, 6, 571) and c["split"] == 3 and c["n"] == 200 and c["p"] == 4 and c["check"] == "nan"
    assert c["n_surrogates"] is None and c["seed"] is None and c["starts"].tolist() == [0, 100, 200, 300]
    found = EB.discover_dyads(root)
    for k, dy in enumerate(res["dyads"]):
        recs = {r: _reader(found[dy]["movies"][r]) for r in ("ch", "cg")}
        block, names, fs = EB.segment_block(recs["ch"], recs["cg"], 1.0, lengths[dy])
        assert np.array_equal(c["x"][k], block[:, :571]) and fs == FS
    z = np.load(res["path"], allow_pickle=False)
    assert res["path"].name == "pseudo_dyads_movies_Peppa.npz"
    assert list(z["dyads"]) == res["dyads"] and list(z["channels"]) == names and np.array_equal(z["starts"], c["starts"])
    nb = c["nb"]
    for meas in ("ffdtf", "ddtf"):
        for k in ("bands", "p", "p_fwe", "null_mean", "null_std"):
            assert z[f"{meas}_{k}"].shape == (3, 4, 6, 6, nb) and z[f"group_{meas}_{k}"].shape == (4, 6, 6, nb)
        assert z[f"{meas}_n_valid"].shape == (3, 4) and z[f"group_{meas}_n_valid"].shape == (4,)
    assert z["partners"].tolist() == [[1, 2, 0], [2, 0, 1]]
    meta = json.loads(str(z["meta"]))
    assert meta["samples"] == 571 and meta["split"] == 3 and meta["dyads"] == res["dyads"] and meta["n_surrogates"] is None
    # a lower threshold keeps the short dyad and everybody is cropped to it; seeded draws are passed on
    eng2 = StubEngine()
    res2 = EB.run_pseudo_dyads(root, tmp_path / "out2", "movies", "Peppa", model_order=4, freqs=np.arange(1.0, 41.0),
                               min_common_fraction=0.5, n_surrogates=7, seed=5, reader=_reader, engine=eng2, verbose=False)
    assert res2["dyads"] == ["W_01", "W_02", "W_03", "W_04"] and eng2.calls[0]["x"].shape == (4, 6, 401)
    assert eng2.calls[0]["n_surrogates"] == 7 and eng2.calls[0]["seed"] == 5
    # fewer than 2 dyads left; arguments refused before any file is read
    one = _tree(tmp_path / "one", {"W_01": 6.0, "W_02": 6.0}, no_caregiver=("W_02",))
    with pytest.raises(ValueError, match="at least 2 dyads"):
        EB.run_pseudo_dyads(one, tmp_path / "out3", "movies", "Peppa", reader=_reader, engine=StubEngine(), verbose=False)
    with pytest.raises(ValueError, match="at least 2 dyads"):
        EB.run_pseudo_dyads(root, tmp_path / "out3", "movies", "Nemo", reader=_reader, engine=StubEngine(), verbose=False)

    def no_reader(path):
        raise AssertionError("refused before any file is read")
    for kw, msg in [(dict(n_surrogates=3), "need a seed"), (dict(model_order=None), "automatic model order"),
                    (dict(measures=("ffdtf", "coh")), "measures must list"), (dict(min_common_fraction=0.0), "min_common_fraction")]:
        with pytest.raises(ValueError, match=msg):
            EB.run_pseudo_dyads(root, tmp_path / "out3", "movies", "Peppa", reader=no_reader, engine=StubEngine(), **kw)


def test_run_pseudo_dyads_reports_an_unreadable_dyad_as_failed(tmp_path, capsys):
    """An error inside the reader is not a `[SKIP]`: the dyad is listed under "failed" with the error, as in `run`, the others
    go on, and where fewer than 2 remain the refusal names what failed."""
    from hyperscanning_signal_analysis_amd import escan_batch as EB
    root = _tree(tmp_path, {"W_01": 6.0, "W_02": 6.0, "W_03": 6.0})

    def reader(path):
        if "W_02" in str(path):
            raise KeyError("data_tc")
        return _reader(path)
    res = EB.run_pseudo_dyads(root, tmp_path / "out", "movies", "Peppa", model_order=4, freqs=np.arange(1.0, 41.0),
                              reader=reader, engine=StubEngine())
    log = capsys.readouterr().out
    assert res["dyads"] == ["W_01", "W_03"] and res["skipped"] == [] and res["failed"] == [("W_02", "KeyError: 'data_tc'")]
    assert "[FAILED] W_02 movies/Peppa: KeyError: 'data_tc'" in log and "[SKIP]" not in log
    meta = json.loads(str(np.load(res["path"], allow_pickle=False)["meta"]))
    assert meta["failed"] == [["W_02", "KeyError: 'data_tc'"]] and meta["skipped"] == []
    two = _tree(tmp_path / "two", {"W_01": 6.0, "W_02": 6.0})
    with pytest.raises(ValueError, match=r"at least 2 dyads .* found 1 \(1 failed: W_02: KeyError"):
        EB.run_pseudo_dyads(two, tmp_path / "out2", "movies", "Peppa", reader=reader, engine=StubEngine(), verbose=False)
