#!/usr/bin/env python3
"""ISA guard for the write-bound kernels: the prediction stores of the classed kernels must stay fire-and-forget.

On gfx9-class hardware loads and stores share ONE in-order counter (vmcnt), so a single `s_waitcnt vmcnt(..)` that the
compiler places in the emit path - e.g. because a rarely taken branch left a vector load pending at a join - makes every
observation step wait for all earlier prediction stores.  That cost the C3 headline 15 % once this round (0.83 -> 0.98 ms)
without changing one line of the hot loop's source.  This script has the Makefile compile pmx_classed.hip to assembly and
checks, for every exact and loose prediction instantiation of pmx_analytical_classed, that no basic block holding a
16-byte prediction store also holds a vmcnt wait.
usage: tools/isa_guard.py [path/to/pmx_classed.s]   (default: pharmsol_amd/csrc/build/pmx_classed.s, made when absent/stale)"""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = "pharmsol_amd/csrc/build/pmx_classed.s"


def assembly(path=None):
    if path:
        return open(path).read()
    subprocess.run(["make", "-s", "-C", ROOT, OUT], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(os.path.join(ROOT, OUT)).read()


def check(text):
    """-> (n kernels checked, [violations])"""
    bad, n = [], 0
    name, block, blocks = None, None, {}
    def finish():
        nonlocal n
        if name is None:
            return
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout
        m = re.search(r"pmx_analytical_classed<(\d+), (\w+), (\w+), (\w+), (\w+), (\w+)>", dem)
        if not m or m.group(2) != "false" or m.group(4) != "false" or m.group(6) != "false":
            return  # prediction mode, no lag class, no covariate rebuild: the write-bound instantiations
        n += 1
        for b, (waits, stores) in blocks.items():
            if waits and stores:
                bad.append(f"{m.group(0)}: block {b} holds {stores} prediction store(s) and {waits} vmcnt wait(s)")
    for line in text.split("\n"):
        m = re.match(r"^(_ZN3pmx\S*pmx_analytical_classed\S*):", line)
        if m:
            finish()
            name, block, blocks = m.group(1), "entry", {}
            continue
        if name is None:
            continue
        t = line.strip()
        if t.startswith("s_endpgm"):
            finish()
            name = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            block = m.group(1)
        d = blocks.setdefault(block, [0, 0])
        if t.startswith("s_waitcnt") and "vmcnt" in t:
            d[0] += 1
        if t.startswith("global_store_dwordx4"):
            d[1] += 1
    finish()
    return n, bad


if __name__ == "__main__":
    n, bad = check(assembly(sys.argv[1] if len(sys.argv) > 1 else None))
    print(f"{n} write-bound classed instantiations checked")
    for b in bad:
        print("VIOLATION", b)
    sys.exit(1 if bad or n == 0 else 0)
