"""Which refusal wins when several arguments of a phase entry are wrong at once: hmv_phase_sync_c128,
hmv_phase_sync_pairs_c128 and hmv_phase_lag_c128 through the library handle, with fake non-null aligned pointers (every call
is refused, or is an empty batch, before a pointer is read or anything is launched; no GPU).

Per entry: every single fault of the refusal tables of tests/test_phase_sync_cpu.py, tests/test_phase_sync_significance_cpu.py
and tests/test_phase_lag_cpu.py, every ordered pair of two faults with different codes (the second fault's arguments over the
first's), and the empty batch with every single fault.  The expected codes are tests/golden/phase_refusal_order.json, recorded
from the library of the commit before the three entries came to share their checks: HYPERMVAR_RECORD_PHASE_REFUSALS=1 makes
the test write the file instead of reading it."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "phase_refusal_order.json")
P = 4096                                                         # a non-null, 16-byte aligned "device pointer"

COMMON = (
    (dict(m=0), -1), (dict(m=65, rec_stride=65000), -1),
    (dict(n=0), -2), (dict(n=1001), -2),
    (dict(T=0, ld=0), -3), (dict(n_rec=-1), -3), (dict(n_items=-1), -3),
    (dict(n_items=1 << 31), -10),
    (dict(ld=999), -5), (dict(rec_stride=7999), -6), (dict(ld=1 << 58, rec_stride=(1 << 63) - 1, m=64), -6),
    (dict(z=None), -4), (dict(item_start=None), -4), (dict(info=None), -4),
    (dict(z=P + 8), -8))
MODE = ((dict(mode=2), -7), (dict(mode=-1), -7))

# entry -> (the arguments in the order of the prototype with a good value each, the single faults with their codes)
ENTRIES = {
    "hmv_phase_sync_c128": (
        dict(z=P, rec_stride=8000, ld=1000, T=1000, n_rec=2, m=8, item_rec=P, item_start=P, n_items=5, n=100, mode=0,
             coherency=P, mag=P, lagged=P, info=P),
        COMMON + MODE + ((dict(item_rec=None), -4), (dict(coherency=None, mag=None, lagged=None), -9))),
    "hmv_phase_sync_pairs_c128": (
        dict(z=P, rec_stride=8000, ld=1000, T=1000, n_rec=2, m=8, split=4, rec_a=P, rec_b=P, item_start=P, shift_b=P,
             n_items=5, n=100, mode=0, values=P, val_stride=4, col_mag=0, col_lagged=1, info=P),
        COMMON + MODE + (
            (dict(rec_a=None), -4), (dict(rec_b=None), -4), (dict(values=None), -4),
            (dict(split=0), -11), (dict(split=8), -11), (dict(split=-3), -11), (dict(m=1, split=1), -11),
            (dict(val_stride=0), -12), (dict(col_mag=4), -12), (dict(col_lagged=-2), -12),
            (dict(col_mag=-1, col_lagged=-1), -12), (dict(col_mag=2, col_lagged=2), -12))),
    "hmv_phase_lag_c128": (
        dict(z=P, rec_stride=8000, ld=1000, T=1000, n_rec=2, m=8, split=0, item_rec=P, item_start=P, n_items=5, n=100,
             pli=P, wpli=P, dwpli=P, info=P),
        COMMON + ((dict(item_rec=None), -4), (dict(pli=None, wpli=None, dwpli=None), -9),
                  (dict(split=-1), -11), (dict(split=8), -11), (dict(m=1, split=1), -11))),
}


def label(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def cases(entry):
    """[(label, the arguments that differ from the good call)]: singles, ordered pairs of different codes, empty batches."""
    faults = ENTRIES[entry][1]
    out = [(label(kw), kw) for kw, _ in faults]
    out += [(f"{label(a)} | {label(b)}", dict(a, **b)) for a, ca in faults for b, cb in faults if ca != cb]
    out += [(f"{label(kw)} | empty", dict(kw, n_items=0)) for kw, _ in faults if "n_items" not in kw]
    return out


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_refusal_precedence(lib, entry):
    good, faults = ENTRIES[entry]
    got = {}
    for name, kw in cases(entry):
        rc = getattr(lib, entry)(*dict(good, **kw).values(), None)
        assert rc == 0 or lib.hmv_last_error().startswith(entry.encode() + b": "), (name, lib.hmv_last_error())
        got[name] = rc
    for kw, code in faults:                                      # a single fault gives its own code
        assert got[label(kw)] == code, kw
    if os.environ.get("HYPERMVAR_RECORD_PHASE_REFUSALS"):
        recorded = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        recorded[entry] = got
        with open(GOLDEN, "w") as fh:
            json.dump(recorded, fh, indent=0, sort_keys=True)
            fh.write("\n")
    with open(GOLDEN) as fh:
        want = json.load(fh)[entry]
    assert sorted(got) == sorted(want)
    moved = {name: (rc, want[name]) for name, rc in got.items() if rc != want[name]}
    assert not moved, f"{entry}: refusals that changed (got, recorded): {moved}"
