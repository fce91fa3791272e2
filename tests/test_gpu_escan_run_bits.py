"""What `escan_batch.run` writes with the real engine, pinned bit for bit in tests/golden/escan_run_bits.json (recorded on the
MI355X from the commit before `run` was cut into stages, by `record` below, twice with equal results; the convention of
tests/test_gpu_block_routes.py): per option set the members of the dyad's file in their order, each with dtype, shape and
SHA-256 of its bytes, and `meta` without `created`.

One dyad of the miniature tree of tests/test_gpu_escan_batch.py (16 channels at 128 Hz, windows of 256 samples, segments of
at most 12 s, order 3) through the option sets of tests/test_escan_run_cpu.py, the second of them also with the PSD on its
stream.  The blocks that `prepare_dyad` built are hashed too and compared first, so that a change of the host libraries'
filtering is not taken for a change of the driver.  All @pytest.mark.gpu."""
import hashlib
import json
import os

import pytest
import torch

from tests.test_escan_run_cpu import FILTER, FREQS, MOVIES, OPTION_SETS, make_tree, npz_record
from tests.test_gpu_escan_batch import _reader

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hyperscanning_signal_analysis_amd import escan_batch as EB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "escan_run_bits.json")
DYAD = "W_003"
SETS = {str(k): kw for k, kw in enumerate(OPTION_SETS)}
SETS["1+psd"] = dict(OPTION_SETS[1], with_psd=True, psd_fmin=2.0, psd_fmax=30.0)
NOT_REPRODUCIBLE = {}          # member name -> why its bytes differ between two runs of the same commit (none did)


def make_bits_tree(root):
    return make_tree(root, dyads=(DYAD,), movies=MOVIES[:2], extras=False)


def input_hashes(tree):
    """SHA-256 of every block `prepare_dyad` builds for the dyad: what the engine is given."""
    prep = EB.prepare_dyad(DYAD, EB.discover_dyads(tree)[DYAD], _reader, **FILTER)
    return {f"{s['task']}/{s['event']}": hashlib.sha256(s["block"].tobytes()).hexdigest() for s in prep["segments"]}


def record_set(tree, out, name):
    """What tests/golden/escan_run_bits.json holds under sets/<name>."""
    res = EB.run(tree, out, freqs=FREQS, reader=_reader, verbose=False, **FILTER, **SETS[name])
    assert res["done"] == [DYAD] and not res["failed"] and not res["skipped"], res
    return npz_record(out / f"{DYAD}_ffdtf.npz")


def record(root):
    """The whole golden file, from a fresh tree under `root`."""
    tree = make_bits_tree(root / "tree")
    return {"inputs": input_hashes(tree), "sets": {name: record_set(tree, root / f"out_{name}", name) for name in SETS}}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_bits_tree(tmp_path_factory.mktemp("escan_bits") / "tree")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", list(SETS))
def test_written_bytes(tree, recorded, tmp_path, name):
    assert input_hashes(tree) == recorded["inputs"], \
        "the host libraries (NumPy / SciPy) no longer reproduce the recorded input blocks: not a change of the driver"
    got, want = record_set(tree, tmp_path / "out", name), recorded["sets"][name]
    assert [m[0] for m in got["members"]] == [m[0] for m in want["members"]]
    meta = json.loads(got["meta"])
    assert [s["event"] for s in meta["segments"]] == ["Peppa", "Brave", "talk_1"] and not meta["failed_segments"]
    moved = [g[0] for g, w in zip(got["members"], want["members"])
             if g[:3] != w[:3] or (g[3] != w[3] and g[0].rsplit("/", 1)[-1] not in NOT_REPRODUCIBLE)]
    assert not moved, f"bits moved: {moved}"
    assert got["meta"] == want["meta"]
