"""`escan_batch.run` as a driver, without a GPU: a recording stub engine stands in for the real one, so what is pinned is the
Python around the engine -- which calls are made with which arguments in which order, what is printed and logged, and every
member of every file written -- in tests/golden/escan_run_calls.json (recorded on the CPU from the commit before `run` was
cut into stages, by `record` below; the convention of tests/test_gpu_block_routes.py).

The stub returns tensors of the right shapes filled with the running call number, so a tensor saved under the wrong key is
seen, and marks window 1 as failed in every call, so the NaN-fill of every saved array is pinned.  It raises for one segment
length, so `failed_segments` is exercised.  Beside it, the two shared host pieces on their own: `prepare_dyad` against
`segment_block`, and the segment geometry against hand-written values."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from hyperscanning_signal_analysis_amd import escan_batch as EB
from tests.test_gpu_escan_batch import _reader, _write

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "escan_run_calls.json")
FREQS = np.arange(1.0, 32.0)
FILTER = dict(low_cutoff_hz=1.0, high_cutoff_hz=45.0)
MOVIES = [("Peppa", 1.0, 11.0), ("Brave", 14.0, 9.5), ("Short", 25.0, 1.0)]      # the last one is shorter than a window
TALK = [("talk_1", 0.5, 12.0)]
FAILING = (1217, 609)          # samples of `Brave` (9.5 s at 128 Hz, inclusive cut), as recorded and decimated by 2
OPTION_SETS = (
    dict(model_order=3),
    dict(model_order=3, save_full=True, measures=("ffdtf", "ddtf", "gpdc"), validation_lags=5, block_granger=True,
         phase_sync=("plv", "imcoh"), pivoted_fallback=True),
    dict(model_order=None, max_model_order=4, crit_type="HQ", measures=("ffdtf", "gpdc"), validation_lags=5),
    dict(model_order=3, significance=dict(null="shift", n_surrogates=4, seed=1), measures=("ffdtf", "ddtf")),
    dict(model_order=3, decimate=2, block_granger=True, phase_sync=("plv",)),
)


def make_tree(root, dyads=("W_003",), movies=MOVIES, extras=True):
    """Complete dyads with a movies and a talk file; with `extras` one dyad without a caregiver file and one unreadable."""
    for d, dy in enumerate(dyads):
        for r, (code, role) in enumerate((("ch", "child"), ("cg", "caregiver"))):
            _write(root / "EEG" / dy / role / f"{dy}_EEG_{code}_passive_movies.nc", 10 * d + r, 30.0, movies, r == 0)
            _write(root / "EEG" / dy / role / f"{dy}_EEG_{code}_talk.nc", 100 + 10 * d + r, 16.0, TALK, r == 1)
    if extras:
        _write(root / "EEG" / "W_020" / "child" / "W_020_EEG_ch_talk.nc", 7, 16.0, TALK, True)
        for role, code, text in (("child", "ch", b"not a file the reader understands"), ("caregiver", "cg", b"neither")):
            bad = root / "EEG" / "W_030" / role / f"W_030_EEG_{code}_talk.nc"
            bad.parent.mkdir(parents=True)
            bad.write_bytes(text)
    return root


def _desc(v):
    """An argument as the call log keeps it: scalars as they are, tensors and arrays as their shapes."""
    if isinstance(v, (torch.Tensor, np.ndarray)):
        return {"shape": list(v.shape)}
    if isinstance(v, (tuple, list)):
        return [_desc(u) for u in v]
    if isinstance(v, (bool, str)) or v is None:
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    return type(v).__name__


class StubEngine:
    """Records what `run` hands to the engine; every tensor it returns is filled with the number of the call."""
    device = "cpu"
    MP = 16

    def __init__(self, pivoted_yw=False, failing=FAILING):
        self.calls, self.pivoted_yw, self.failing = [], pivoted_yw, failing

    def _log(self, name, *args, **kw):
        self.calls.append({"method": name, "args": [_desc(a) for a in args], "kw": {k: _desc(kw[k]) for k in sorted(kw)}})
        return len(self.calls)

    @staticmethod
    def _full(c, *shape, dtype=torch.float64):
        return torch.full(shape, c, dtype=dtype)

    @staticmethod
    def _bad(n_items):
        bad = torch.zeros(n_items, dtype=torch.bool)
        bad[1:2] = True
        return bad

    def to_device(self, a):
        self._log("to_device", a)
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)

    def decimate(self, x, q, design="decimate"):
        c = self._log("decimate", x, q, design)
        return self._full(c, *x.shape[:-1], -(-x.shape[-1] // int(q)))

    def _measure(self, name, x, rec, st, n, p, freqs, fs, **kw):
        c = self._log(name, x, rec, st, n, p, freqs, fs, **kw)
        if name == "sliding_ffdtf" and x.shape[2] in self.failing:
            raise RuntimeError(f"stub engine: no fit for a segment of {x.shape[2]} samples")
        N, m = len(rec), x.shape[1]
        r = (self._full(c, N, m, m, len(kw["bands"][0]) if "bands" in kw else len(freqs)), self._bad(N))
        if kw.get("return_orders") and p is None:
            pmax = kw["max_model_order"]
            r += ((1 + (torch.arange(N) + c) % pmax).to(torch.int32), self._full(c, N, pmax))
        return r

    def sliding_ffdtf(self, *a, **kw):
        return self._measure("sliding_ffdtf", *a, **kw)

    def sliding_ddtf(self, *a, **kw):
        return self._measure("sliding_ddtf", *a, **kw)

    def sliding_gpdc(self, *a, **kw):
        return self._measure("sliding_gpdc", *a, **kw)

    def band_sums(self, ff, lo, hi):
        c = self._log("band_sums", ff, lo, hi)
        return self._full(c, *ff.shape[:-1], len(lo))

    def lagcov(self, x, rec, st, n, p):
        c = self._log("lagcov", x, rec, st, n, p)
        return self._full(c, len(rec), p + 1, self.MP, self.MP)

    def yw_solve(self, R, m, **kw):
        c = self._log("yw_solve", R, m, **kw)
        N, p = R.shape[0], R.shape[1] - 1
        return self._full(c, N, self.MP, self.MP, p), self._full(c, N, self.MP, self.MP), None, self._bad(N).to(torch.int32)

    def yw_solve_auto(self, R, m, n, crit_type="AIC"):
        c = self._log("yw_solve_auto", R, m, n, crit_type)
        N, pmax = R.shape[0], R.shape[1] - 1
        return (self._full(c, N, self.MP, self.MP, pmax), self._full(c, N, self.MP, self.MP),
                (1 + (torch.arange(N) + c) % pmax).to(torch.int32), self._full(c, N, pmax), self._bad(N).to(torch.int32))

    def model_validation(self, x, rec, st, n, ar, max_lag, **kw):
        c = self._log("model_validation", x, rec, st, n, ar, max_lag, **kw)
        N = len(rec)
        return {"q": self._full(c, N, 3), "acf_count": self._full(c, N, dtype=torch.int32),
                "info": torch.zeros(N, dtype=torch.int32)}

    def sliding_block_granger(self, x, rec, st, n, p, freqs, fs, **kw):
        c = self._log("sliding_block_granger", x, rec, st, n, p, freqs, fs, **kw)
        N = len(rec)
        return self._full(c, N, 2, len(kw["bands"][0])), self._full(c + 0.5, N, 4), self._bad(N)

    def sliding_phase_sync(self, x, rec, st, n, fs, bands_hz, **kw):
        c = self._log("sliding_phase_sync", x, rec, st, n, fs, bands_hz, **kw)
        N, m = len(rec), x.shape[1]
        out = {q: self._full(c + 0.25 * k, N, len(bands_hz), m, m) for k, q in enumerate(kw["measures"])}
        out["info"] = torch.zeros(N, len(bands_hz), dtype=torch.int32)
        return out

    def sliding_significance(self, x, rec, st, n, p, freqs, fs, bands, **kw):
        c = self._log("sliding_significance", x, rec, st, n, p, freqs, fs, bands, **kw)
        N, m, nb = len(rec), x.shape[1], len(bands[0])
        out = {k_: self._full(c + 0.125 * j, N, m, m, nb)
               for j, k_ in enumerate(("observed", "p", "p_fwe", "null_mean", "null_std"))}
        out["n_valid"] = self._full(c, N, dtype=torch.int32)
        return out

    def window_routes(self, x, rec, st, n, p):
        c = self._log("window_routes", x, rec, st, n, p)
        return ((torch.arange(len(rec)) + c) % 3).to(torch.int32), torch.zeros(len(rec), dtype=torch.int32)


def npz_record(path):
    """A written file as the golden files keep it: [name, dtype, shape, SHA-256 of the bytes] of every member in the file's
    order, and `meta` (whose bytes hold the time of writing) as its JSON text without `created`, key order included."""
    members, meta = [], None
    with np.load(path, allow_pickle=False) as z:
        for name in z.files:
            a = z[name]
            if name == "meta":
                meta = json.loads(str(a))
                del meta["created"]
                members.append([name, a.dtype.str, list(a.shape), None])
            else:
                members.append([name, a.dtype.str, list(a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()])
    return {"members": members, "meta": json.dumps(meta)}


def _one_run(tree, out, capsys, tmp_path, **kw):
    eng = StubEngine()
    capsys.readouterr()
    timing = {}
    res = EB.run(tree, out, freqs=FREQS, with_psd=False, reader=_reader, engine=eng, timing=timing, **FILTER, **kw)
    assert res["timing"] == timing
    return {"calls": eng.calls,
            "printed": capsys.readouterr().out.replace(str(tmp_path), "<tmp>").splitlines(),
            "done": res["done"], "skipped": res["skipped"], "failed": [list(f) for f in res["failed"]],
            "timing_keys": list(timing), "dyad_timing_keys": [list(d) for d in timing["dyads"]],
            "save_s": [d["save_s"] for d in timing["dyads"]], "segments": [d["segments"] for d in timing["dyads"]],
            "logs": {p.name: p.read_text() for p in sorted(out.glob("batch*.log"))},
            "files": {p.name: npz_record(p) for p in sorted(out.glob("*.npz"))},
            "other_files": sorted(p.name for p in out.iterdir() if p.suffix not in (".npz", ".log"))}


def record(tmp_path, capsys, monkeypatch, which):
    """What tests/golden/escan_run_calls.json holds under str(which): the runs of one option set (set 5: set 0 a second time
    into the same directory, then two ranks into another)."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    tree = make_tree(tmp_path / "tree")
    if which < 5:
        return [_one_run(tree, tmp_path / "out", capsys, tmp_path, **OPTION_SETS[which])]
    _one_run(tree, tmp_path / "out", capsys, tmp_path, **OPTION_SETS[0])
    return [_one_run(tree, tmp_path / "out", capsys, tmp_path, **OPTION_SETS[0]),
            _one_run(tree, tmp_path / "ranks", capsys, tmp_path, world=2, rank=0, **OPTION_SETS[0]),
            _one_run(tree, tmp_path / "ranks", capsys, tmp_path, world=2, rank=1, **OPTION_SETS[0])]


@pytest.mark.parametrize("which", range(6))
def test_run_drives_the_engine_and_writes_what_it_did_before(tmp_path, capsys, monkeypatch, which):
    with open(GOLDEN) as fh:
        want = json.load(fh)[str(which)]
    got = json.loads(json.dumps(record(tmp_path, capsys, monkeypatch, which)))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [c["method"] for c in g["calls"]] == [c["method"] for c in w["calls"]]
        for k, (cg, cw) in enumerate(zip(g["calls"], w["calls"])):
            assert cg == cw, f"call {k} ({cw['method']})"
        assert g["printed"] == w["printed"]
        for key in sorted(set(w) | set(g)):
            assert g.get(key) == w.get(key), key


def test_the_recorded_runs_cover_what_they_are_meant_to():
    """Independent of the code under test: the golden file itself holds a failed segment, a short one, the NaN-filled window,
    a skipped and a failed dyad, the skip-if-exists run and both ranks."""
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert sorted(want) == [str(k) for k in range(6)] and [len(want[str(k)]) for k in range(6)] == [1, 1, 1, 1, 1, 3]
    for k in range(5):
        run = want[str(k)][0]
        meta = json.loads(run["files"]["W_003_ffdtf.npz"]["meta"])
        assert [s["event"] for s in meta["segments"]] == ["Peppa", "talk_1"]
        assert [f["segment"] for f in meta["failed_segments"]] == ["passive_movies/Brave"]
        assert all(s["singular_windows"] == 1 for s in meta["segments"])
        assert any("passive_movies/Short" in line and "< one window" in line for line in run["printed"])
        assert run["done"] == ["W_003"] and run["skipped"] == ["W_020"] and [f[0] for f in run["failed"]] == ["W_030"]
        assert run["save_s"] == [0.0] and run["other_files"] == []
    again, rank0, rank1 = want["5"]
    assert again["done"] == [] and again["calls"] == [] and sorted(again["skipped"]) == ["W_003", "W_020"]
    assert rank0["done"] == ["W_003"] and rank1["done"] == [] and sorted(rank1["logs"]) == ["batch_rank0.log", "batch_rank1.log"]
    methods = {c["method"] for k in range(5) for c in want[str(k)][0]["calls"]}
    assert methods == {"to_device", "decimate", "sliding_ffdtf", "sliding_ddtf", "sliding_gpdc", "band_sums", "lagcov",
                       "yw_solve", "yw_solve_auto", "model_validation", "sliding_block_granger", "sliding_phase_sync",
                       "sliding_significance", "window_routes"}


@pytest.mark.parametrize("subset", [None, ["F3", "O2", "XX", "Fp1"]])
def test_prepare_dyad_builds_the_blocks_of_segment_block(tmp_path, subset):
    tree = make_tree(tmp_path / "tree", extras=False)
    files = EB.discover_dyads(tree)["W_003"]
    prep = EB.prepare_dyad("W_003", files, _reader, channel_subset=subset, **FILTER)
    assert [s["event"] for s in prep["segments"]] == [e[0] for e in MOVIES] + ["talk_1"]
    for seg in prep["segments"]:
        recs = {r: _reader(files[seg["task"]][r]) for r in ("ch", "cg")}
        block, names, fs = EB.segment_block(recs["ch"], recs["cg"], seg["start_s"], seg["duration_s"], channel_subset=subset,
                                            **FILTER)
        assert np.array_equal(seg["block"], block) and seg["block"].dtype == block.dtype
        assert seg["names"] == names and seg["fs"] == fs
    assert EB.child_channels(prep["segments"][0]["names"]) == (8 if subset is None else 3)
    with pytest.raises(ValueError, match="None of the requested channels"):
        EB.prepare_dyad("W_003", files, _reader, channel_subset=["XX"], **FILTER)


def _settings(**kw):
    return EB.resolve_settings(engine=StubEngine(), **kw)[0]


def test_segment_geometry_against_hand_written_values():
    cfg = _settings(model_order=3, freqs=FREQS)
    g = EB.segment_geometry(cfg, 128.0, 1409, 16)
    assert (g.fs, g.T, g.W, g.hop) == (128.0, 1409, 256, 128) and g.pos.tolist() == list(range(0, 1153, 128))
    assert g.freqs is not None and np.array_equal(g.freqs, FREQS) and g.grid == (128, 0, 10)
    # delta 1..3 Hz, theta 4..7, alpha 8..12, beta 13..29, gamma 30..31 on the grid 1, 2, .., 31 Hz
    assert g.lo.tolist() == [0, 3, 7, 12, 29] and g.hi.tolist() == [3, 7, 12, 29, 31]
    short = EB.segment_geometry(cfg, 128.0, 255, 16)
    assert (short.fs, short.T, short.W) == (128.0, 255, 256) and short.pos is None
    assert EB.segment_geometry(cfg, 128.0, 256, 16).pos.tolist() == [0] and EB.segment_geometry(cfg, 128.0, 256, 16).grid is None
    # no frequencies given: 0.5 Hz steps up to the Nyquist rate, 128 Hz at the most
    assert np.array_equal(EB.segment_geometry(cfg._replace(freqs=None), 100.0, 1000, 16).freqs, np.arange(1, 101) * 0.5)
    assert EB.segment_geometry(cfg._replace(freqs=None), 500.0, 1000, 16).freqs[-1] == 128.0
    # 75 % overlap
    assert EB.segment_geometry(cfg._replace(overlap=0.75), 128.0, 1409, 16).hop == 64
    # decimated by 2: 64 Hz, ceil(1409 / 2) samples, windows of 128
    dec = _settings(model_order=3, freqs=FREQS, decimate=2)
    g = EB.segment_geometry(dec, 128.0, 1409, 16)
    assert (g.fs, g.T, g.W, g.hop) == (64.0, 705, 128, 64) and g.pos.tolist() == list(range(0, 577, 64)) and g.grid == (64, 0, 10)
    assert g.hi.tolist() == [3, 7, 12, 29, 31]
    short = EB.segment_geometry(dec, 128.0, 255, 16)
    assert (short.fs, short.T, short.W) == (64.0, 128, 128) and short.pos.tolist() == [0]
    assert EB.segment_geometry(dec, 128.0, 254, 16).pos is None
    with pytest.raises(EB.DecimateConfigError, match="not below the Nyquist rate 32 Hz"):
        EB.segment_geometry(dec._replace(freqs=np.arange(1.0, 33.0)), 128.0, 1409, 16)
    with pytest.raises(EB.DecimateConfigError, match="16 channels x order 8 = 128 unknowns"):
        EB.segment_geometry(_settings(model_order=8, freqs=FREQS, decimate=2), 128.0, 1409, 16)
    # the automatic order counts with max_model_order
    auto = _settings(model_order=None, max_model_order=8, freqs=FREQS, decimate=2)
    with pytest.raises(EB.DecimateConfigError, match="16 channels x order 8 = 128 unknowns"):
        EB.segment_geometry(auto, 128.0, 1409, 16)
