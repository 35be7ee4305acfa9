#!/bin/bash
# Count VALU instructions per kernel (whole function; compare before/after a change).
# usage: tools/isa_count.sh [unit ...]   (kernel units such as pmx_classed; default: all.  The gfx950 assembly is the
# Makefile's: pharmsol_amd/csrc/build/<unit>.s)
b=pharmsol_amd/csrc/build
if [ $# -eq 0 ]; then make -s asm || exit 1; set -- $b/pmx_*.s; else set -- "${@/#/$b/}"; set -- "${@/%/.s}"; make -s "$@" || exit 1; fi
python3 - "$@" <<'PY'
import re, subprocess, sys
name, rows = None, {}
for line in (l for p in sys.argv[1:] for l in open(p)):
    m = re.match(r"^(_Z\S+):", line)
    if m:
        name = m.group(1); rows[name] = [0, 0, 0, 0]; continue
    if name is None: continue
    t = line.strip()
    if t.startswith("s_endpgm"): name = None; continue
    if t.startswith("v_mov_b64") or t.startswith("v_mov_b32"): rows[name][1] += 1
    if re.match(r"v_(fma|fmac|mul|add)_f64", t): rows[name][2] += 1
    if t.startswith("v_"): rows[name][0] += 1
    if t.startswith("s_"): rows[name][3] += 1
names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
print(f"{'kernel':48s} {'VALU':>6s} {'v_mov':>6s} {'f64 arith':>9s} {'SALU':>6s}")
for full, (k, v) in zip(names, rows.items()):
    mm = re.search(r"(pmx_\w+<[^>]*>)", full)
    if mm: print(f"{mm.group(1):48s} {v[0]:6d} {v[1]:6d} {v[2]:9d} {v[3]:6d}")
PY
