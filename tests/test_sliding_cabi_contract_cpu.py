"""The C ABI of the fused sliding-window entries as a table: what every entry refuses, in which order, with which code and
text, and what every workspace sizer of the family returns.  Both tables were recorded from the commit before the C driver
became a plan and four stages (tests/golden/sliding_cabi_contract.json, by `refusals` and `sizes` below) and are compared
byte for byte.  No GPU: every recorded call is refused before anything is launched, or is an empty batch.

(a) Refusals.  The twelve `hmv_sliding_*_f64` entries and `hmv_yw_solve_auto_f64`, called with fake non-null pointers (as
tests/test_auto_order_cpu.py does).  `VALID` is one acceptable argument set per entry; `PERTURBATIONS` are single changes
to it, each applied to every entry that has the arguments it names and refuses the result; then every pair of an entry's
perturbations (the second wins where both set one argument), which pins the order of the checks; then the empty batches
(n_items = 0), which return 0 whatever the pointers.  Recorded per call: (return code, hmv_last_error()).
A perturbation applies to an entry that has every argument it names.  One kind is accepted by the entries it applies to and
is left out for them by hand (`ACCEPTED`), because an accepted call would launch: a flag of an LDL^T form or of the pivoted
LU at the eleven entries whose order is fixed -- only the automatic order (hmv_sliding_auto_f64, hmv_yw_solve_auto_f64)
refuses those.  Arguments an entry treats as optional (ar_out, V_out, crit_out, scale, the bases, the events, the streams) are
null in `VALID` and have no perturbation.
A second guard at run time: the test asserts that every recorded single and pair has a negative code in the golden file
before it makes the call.

(b) Sizes.  Every `hmv_*workspace_bytes` of the family over m x p x F x chunk x n_bands (`GRID`), -1 results included."""
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hyperscanning_signal_analysis_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sliding_cabi_contract.json")

P = 0x1000          # a fake non-zero device address: the checks must refuse before any pointer is read

# ---- the argument lists, in ABI order (include/hypermvar.h); `p` is pmax where the order is automatic
_ITEMS = "x rec_stride ld item_rec item_start n_items m n p"
_SPEC = "freqs F fs"
_BANDS = "out bin_lo bin_hi n_bands"
_GRID = "grid_hop grid_first grid_nwin grid_T"
_ENS = ("measure x rec_stride ld T trial_rec trial_start group_ptr n_groups item_group item_offset n_items m n p " + _SPEC + " " +
        _BANDS + " S_out ar_out V_out info_yw info_tf workspace workspace_bytes chunk pivot_tau flags")
ENTRIES = {
    "hmv_sliding_ffdtf_f64": f"{_ITEMS} {_SPEC} out ar_out V_out info_yw info_tf workspace workspace_bytes chunk pivot_tau flags "
                             f"{_GRID} ev_k3_start ev_k3_stop stream aux_stream",
    "hmv_sliding_ffdtf_bands_f64": f"{_ITEMS} {_SPEC} {_BANDS} ar_out V_out info_yw info_tf workspace workspace_bytes chunk "
                                   f"pivot_tau flags {_GRID} ev_k3_start ev_k3_stop stream aux_stream",
    "hmv_sliding_ffdtf_spectra_f64": f"{_ITEMS} {_SPEC} out S_out ar_out V_out info_yw info_tf workspace workspace_bytes chunk "
                                     f"pivot_tau flags {_GRID} stream aux_stream",
    "hmv_sliding_ddtf_f64": f"{_ITEMS} {_SPEC} {_BANDS} ar_out V_out info_yw info_tf workspace workspace_bytes chunk pivot_tau "
                            f"flags {_GRID} stream aux_stream",
    "hmv_sliding_gpdc_f64": f"{_ITEMS} {_SPEC} {_BANDS} ar_out V_out info_yw workspace workspace_bytes chunk flags {_GRID} "
                            f"stream aux_stream",
    "hmv_sliding_block_gc_f64": f"{_ITEMS} split {_SPEC} {_BANDS} time ar_out V_out info_yw info_red info_gc workspace "
                                f"workspace_bytes chunk flags {_GRID} stream",
    "hmv_sliding_block_gc_pairs_f64": f"x rec_stride ld T rec_a rec_b item_start n_items m n p split {_SPEC} {_BANDS} time ar_out "
                                      f"V_out info_yw info_red info_gc workspace workspace_bytes chunk flags R_base base_a base_b "
                                      f"want red_out red_base info_red_base stream",
    "hmv_sliding_auto_f64": f"measure {_ITEMS} crit {_SPEC} {_BANDS} S_out ar_out V_out order_out crit_out info_yw info_tf workspace "
                            f"workspace_bytes chunk pivot_tau flags {_GRID} stream aux_stream",
    "hmv_sliding_ensemble_f64": f"{_ENS} grid_hop grid_nwin stream aux_stream",
    "hmv_sliding_ensemble_split_f64": f"{_ENS} trial_rec_b trial_start_b split R_base item_base stream aux_stream",
    "hmv_sliding_pairs_f64": f"measure x rec_stride ld T rec_a rec_b item_start n_items m n p {_SPEC} {_BANDS} S_out ar_out V_out "
                             f"info_yw info_tf workspace workspace_bytes chunk pivot_tau flags split R_base base_a base_b stream "
                             f"aux_stream",
    "hmv_sliding_mix_f64": f"measure Rt n_trials n_win W scale n_mix m n p {_SPEC} {_BANDS} S_out ar_out V_out info_yw info_tf "
                           f"workspace workspace_bytes chunk pivot_tau flags stream aux_stream",
    "hmv_yw_solve_auto_f64": "R n_items m p n crit yw_ws ar V order_out crit_out vq_logdet info flags stream",
}
# one acceptable argument set; optional pointers are null
VALID = dict(
    x=P, rec_stride=1000, ld=1000, T=1000, item_rec=P, item_start=P, rec_a=P, rec_b=P, n_items=2, m=8, n=100, p=5, split=3,
    freqs=P, F=4, fs=100.0, out=P, bin_lo=0, bin_hi=0, n_bands=0, S_out=0, time=P, ar_out=0, V_out=0, info_yw=P, info_tf=P,
    info_red=P, info_gc=P, workspace=P, workspace_bytes=1 << 40, chunk=2, pivot_tau=1.0, flags=0, grid_hop=0, grid_first=0,
    grid_nwin=0, grid_T=0, ev_k3_start=0, ev_k3_stop=0, stream=0, aux_stream=0, measure=0, crit=0, order_out=P, crit_out=0,
    trial_rec=P, trial_start=P, group_ptr=P, n_groups=1, item_group=P, item_offset=P, trial_rec_b=P, trial_start_b=P, R_base=0,
    item_base=0, base_a=0, base_b=0, want=3, red_out=0, red_base=0, info_red_base=0, Rt=P, n_trials=3, n_win=2, W=P, scale=0,
    n_mix=2, R=P, yw_ws=P, ar=P, V=P, vq_logdet=0, info=P)
# what differs from VALID per entry: the band form has its bands, the spectra form its S_out
OWN = {"hmv_sliding_ffdtf_bands_f64": dict(bin_lo=P, bin_hi=P, n_bands=2), "hmv_sliding_ffdtf_spectra_f64": dict(S_out=P)}
_POINTERS = [k for k, v in VALID.items() if v == P]
PERTURBATIONS = {
    "m=0": dict(m=0), "m=65": dict(m=65), "p=0": dict(p=0), "p=33": dict(p=33), "n<=p": dict(n=5), "chunk=0": dict(chunk=0),
    "workspace=16B": dict(workspace_bytes=16), "F=0": dict(F=0),
    **{f"{k}=NULL": {k: 0} for k in _POINTERS},
    "n_bands=-1": dict(n_bands=-1), "bands without bins": dict(n_bands=2, bin_lo=0, bin_hi=0),
    "S_out with bands": dict(S_out=P, n_bands=2, bin_lo=P, bin_hi=P), "S_out with dDTF": dict(S_out=P, measure=1),
    "S_out with GPDC": dict(S_out=P, measure=2), "measure=3": dict(measure=3), "measure=-1": dict(measure=-1),
    "crit=-1": dict(crit=-1), "crit=3": dict(crit=3), "flags=YW_TILED": dict(flags=2), "flags=YW_ONE_LAUNCH": dict(flags=4),
    "flags=YW_PIVOTED": dict(flags=16), "grid without windows": dict(grid_hop=10, grid_nwin=0),
    "grid past the recording": dict(grid_hop=50, grid_nwin=2, grid_T=60),
    "ensemble grid past the recording": dict(grid_hop=50, grid_nwin=2, T=60),
    "split=0": dict(split=0), "split=m": dict(split=8), "want=0": dict(want=0), "want=4": dict(want=4),
    "R_base alone": dict(R_base=P), "red_base without info_red_base": dict(red_base=P),
    "red_base without R_base": dict(red_base=P, info_red_base=P), "n_groups=0": dict(n_groups=0),
    "n_trials=0": dict(n_trials=0), "n_win=0": dict(n_win=0), "n_mix=0": dict(n_mix=0), "Rt misaligned": dict(Rt=P + 8),
}
# (entry, perturbation) pairs that the entry accepts -- see the module docstring; `accepted(lib)` finds no others
ACCEPTED = {(entry, "flags=" + flag) for entry, spec in ENTRIES.items() if "crit" not in spec.split()
            for flag in ("YW_TILED", "YW_ONE_LAUNCH", "YW_PIVOTED")}
GRID = dict(m=(1, 6, 16, 19, 33, 64), p=(1, 3, 32), F=(1, 16, 32, 256), chunk=(1, 2, 7, 599), n_bands=(-1, 0, 3))


@pytest.fixture(scope="module")
def lib():
    from hyperscanning_signal_analysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True)
    return _lib.load()


def _call(lib, entry, changes):
    args = dict(VALID, **OWN.get(entry, {}))
    args.update(changes)
    rc = getattr(lib, entry)(*(args[name] for name in ENTRIES[entry].split()))
    return int(rc), lib.hmv_last_error().decode()


def perturbations_of(entry):
    """The single perturbations of one entry: those whose arguments it has, that change something, that it refuses."""
    names = set(ENTRIES[entry].split())
    base = dict(VALID, **OWN.get(entry, {}))
    return [k for k, ch in PERTURBATIONS.items()
            if set(ch) <= names and any(base[a] != v for a, v in ch.items()) and (entry, k) not in ACCEPTED]


def _changes(*keys):
    merged = {}
    for k in keys:
        merged.update(PERTURBATIONS[k])
    return merged


def accepted(lib):
    """Recorder's helper (CPU only, where a launch is an error code and nothing more): what `ACCEPTED` must list."""
    return sorted((e, k) for e in ENTRIES for k in perturbations_of(e) if _call(lib, e, _changes(k))[0] >= 0)


def refusals(lib, known=None):
    """Table (a): per entry its perturbations, then (code, text) of every single one and of every pair of them, in the
    order of `itertools.combinations`, then of the empty batch.  known: the golden table -- a call it does not list as
    refused is not made."""
    table = {}
    for entry in ENTRIES:
        singles = perturbations_of(entry)
        calls = [(k,) for k in singles] + list(itertools.combinations(singles, 2))
        if known is not None:
            assert known[entry]["perturbations"] == singles and len(known[entry]["rows"]) == len(calls), entry
            assert all(row[0] < 0 for row in known[entry]["rows"]), entry
        table[entry] = {"perturbations": singles, "rows": [list(_call(lib, entry, _changes(*keys))) for keys in calls]}
        if "n_items" in ENTRIES[entry].split():
            # (a sliding entry looks at no output pointer of an empty batch; hmv_yw_solve_auto_f64 still wants its own)
            empty = dict(n_items=0, out=0, order_out=0, S_out=0, time=0, info_gc=0, info_red=0) if "x" in ENTRIES[entry].split() \
                else dict(n_items=0)
            table[entry]["empty"] = list(_call(lib, entry, {a: v for a, v in empty.items() if a in ENTRIES[entry].split()}))
    return table


def pack(table):
    """The refusal table with every text written once: {"messages": [...], "entries": the table with indices for texts}."""
    texts = sorted({row[1] for e in table.values() for row in e["rows"] + [e.get("empty", [0, ""])]})
    index = {t: i for i, t in enumerate(texts)}
    entries = {name: dict(e, rows=[[rc, index[t]] for rc, t in e["rows"]],
                          **({"empty": [e["empty"][0], index[e["empty"][1]]]} if "empty" in e else {}))
               for name, e in table.items()}
    return {"messages": texts, "entries": entries}


def unpack(packed):
    texts = packed["messages"]
    return {name: dict(e, rows=[[rc, texts[i]] for rc, i in e["rows"]],
                       **({"empty": [e["empty"][0], texts[e["empty"][1]]]} if "empty" in e else {}))
            for name, e in packed["entries"].items()}


def sizes(lib):
    """Table (b): {sizer: [bytes over the grid, m slowest]}; a sizer without n_bands is not repeated over it, and where a sizer
    has more arguments (measure, the ensemble's grid, want), they vary fastest."""
    measures, n = (0, 1, 2), 120
    out = {}

    def over(name, fn, *more, bands=GRID["n_bands"]):
        f = getattr(lib, name)
        out[name] = [int(f(*fn(m, p, F, c, nb, *extra))) for m in GRID["m"] for p in GRID["p"] for F in GRID["F"]
                     for c in GRID["chunk"] for nb in bands for extra in itertools.product(*more)]
    split = lambda m: max(1, m // 2)  # noqa: E731
    over("hmv_tf_ffdtf_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, F), bands=(0,))
    over("hmv_tf_ffdtf_bands_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, F), bands=(0,))
    over("hmv_sliding_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, F), bands=(0,))
    over("hmv_sliding_bands_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, F), bands=(0,))
    over("hmv_sliding_spectra_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, F), bands=(0,))
    over("hmv_sliding_ddtf_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, F, nb))
    over("hmv_sliding_gpdc_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, F, nb))
    over("hmv_sliding_auto_workspace_bytes", lambda m, p, F, c, nb, meas: (meas, c, m, p, F, nb), measures)
    over("hmv_sliding_ensemble_workspace_bytes", lambda m, p, F, c, nb, meas, g: (meas, c, m, n, p, F, nb, *g), measures,
         ((0, 0), (30, 4)))
    over("hmv_pairs_workspace_bytes", lambda m, p, F, c, nb, meas: (meas, c, m, n, p, F, nb), measures)
    over("hmv_mix_workspace_bytes", lambda m, p, F, c, nb, meas: (meas, c, m, p, F, nb), measures)
    over("hmv_block_gc_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, split(m), F), bands=(0,))
    over("hmv_block_gc_sliding_workspace_bytes", lambda m, p, F, c, nb: (c, m, p, split(m), F, nb))
    over("hmv_block_gc_pairs_workspace_bytes", lambda m, p, F, c, nb, want: (c, m, n, p, split(m), F, nb, want), (1, 2, 3))
    return out


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def dumps(lib, known=None):
    """The golden file's text."""
    return json.dumps({"refusals": pack(refusals(lib, known)), "sizes": sizes(lib)}, sort_keys=True, separators=(",", ":")) + "\n"


def test_every_refusal_is_the_recorded_one(lib):
    want = unpack(_golden()["refusals"])
    got = refusals(lib, known=want)
    assert list(got) == list(ENTRIES) and sorted(got) == sorted(want)
    for entry, w in want.items():
        singles = w["perturbations"]
        names = [(k,) for k in singles] + list(itertools.combinations(singles, 2))
        moved = [(" + ".join(k), g, r) for k, g, r in zip(names, got[entry]["rows"], w["rows"]) if g != r]
        assert not moved, (entry, len(moved), moved[:5])
        assert got[entry].get("empty") == w.get("empty"), entry
        assert all(rc < 0 and text.startswith(entry + ": ") for rc, text in w["rows"]), entry
        assert w.get("empty", [0])[0] == 0, entry
    assert len(want) == 13 and sum(len(w["rows"]) for w in want.values()) > 3000


def test_every_workspace_size_is_the_recorded_one(lib):
    want = _golden()["sizes"]
    got = sizes(lib)
    assert sorted(got) == sorted(want) and len(want) == 14
    for name in want:
        assert got[name] == want[name], name
        assert any(v > 0 for v in want[name]), name
    assert -1 in want["hmv_sliding_auto_workspace_bytes"] and -1 in want["hmv_sliding_ddtf_workspace_bytes"]


def test_the_tables_are_the_golden_file_byte_for_byte(lib):
    with open(GOLDEN) as fh:
        assert fh.read() == dumps(lib, known=unpack(_golden()["refusals"]))
