#!/usr/bin/env python3
"""Static instruction mix of the K2 kernels per basic block, from a device-only cross-compile (no GPU needed).
The source is compiled with the Makefile's flags and -S, each kernel's text is split at its labels, and the mnemonics of
every block that holds matrix instructions are classified: MFMA, other vector ALU (and how many of those are f64),
barriers, global accesses, LDS writes and reads.  The last column is other-VALU per 256 MFMAs, i.e. per 64^3 product.
    python tools/dbg/k2_inst_count.py [yw_lwr|yw_auto|yw_solve|yw_lwr2] [name filter] [extra compiler flags...]"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "hyperscanning_signal_analysis_amd", "csrc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-mllvm", "-simplifycfg-sink-common=false",
         "-mllvm", "-simplifycfg-hoist-common=false", "--cuda-device-only", "-S"]


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("global_") or op.startswith("flat_"):
        return "global"
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return "ds_write"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    unit = sys.argv[1] if len(sys.argv) > 1 else "yw_lwr"
    flt = sys.argv[2] if len(sys.argv) > 2 else "ILi4E"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + sys.argv[3:] +
                       [os.path.join(CSRC, unit + ".hip"), "-o", out], check=True, stderr=subprocess.DEVNULL)
        lines = open(out).read().split("\n")
    kernel, block, blocks = None, None, collections.OrderedDict()
    for line in lines:
        t = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m and kernel is None and flt in m.group(1) and "kernel" in m.group(1):
            kernel, block = m.group(1), "entry"
            continue
        if kernel is None:
            continue
        if t.startswith(".Lfunc_end"):
            kernel = None
            continue
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            block = m.group(1)
            continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        op = t.split()[0]
        c = blocks.setdefault((kernel, block), collections.Counter())
        c[classify(op)] += 1
        if op.startswith("v_") and not op.startswith("v_mfma") and op.endswith("_f64"):
            c["valu_f64"] += 1
    cols = ("mfma", "valu", "valu_f64", "barrier", "global", "ds_write", "ds_read", "scratch", "salu")
    last, tot = None, None
    for (k, b), c in list(blocks.items()) + [((None, None), None)]:
        if k != last:
            if tot is not None:
                print(f"  {'whole kernel':12s} " + " ".join(f"{tot[x]:7d}" for x in cols) +
                      f"  {256.0 * tot['valu'] / max(tot['mfma'], 1):8.1f}")
            if k is None:
                break
            print(k)
            print(f"  {'block':12s} " + " ".join(f"{x:>7s}" for x in cols) + "  valu/256mfma")
            last, tot = k, collections.Counter()
        tot.update(c)
        if c["mfma"] >= 64:
            print(f"  {b:12s} " + " ".join(f"{c[x]:7d}" for x in cols) + f"  {256.0 * c['valu'] / c['mfma']:8.1f}")


if __name__ == "__main__":
    main()
