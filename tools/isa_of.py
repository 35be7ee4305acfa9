#!/usr/bin/env python3
"""Print the gfx950 ISA of ONE kernel (comment-free), from the Makefile's assembly of the unit that holds it, e.g.
   tools/isa_of.py 'pmx_analytical_stepsILi4ELb0E'"""
import re, subprocess, sys
pat = sys.argv[1]
UNITS = (("pmx_analytical_classed_ll", "pmx_classed_ll"), ("pmx_analytical_classed", "pmx_classed"), ("pmx_analytical_grid", "pmx_grid"),
         ("pmx_analytical_dyn3", "pmx_dyn3"), ("pmx_analytical_steps", "pmx_steps"), ("pmx_analytical_pair", "pmx_pair"),
         ("pmx_ode_", "pmx_ode_builtin"), ("pmx_", "pmx_util"))
path = "pharmsol_amd/csrc/build/" + next(u for k, u in UNITS if k in pat) + ".s"
subprocess.run(["make", "-s", path], check=True)
txt = open(path).read()
m = re.search(r"^(\S*" + re.escape(pat) + r"\S*):[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M)
name = m.group(1)
for l in m.group(2).split("\n"):
    if l.strip() and not l.strip().startswith(";") and not l.strip().startswith(".p2align"):
        print(l.split(";")[0].rstrip() if not l.startswith(".LBB") else l)
for key in ("num_vgpr", "numbered_sgpr", "private_seg_size"):
    mm = re.search(r"\.set " + re.escape(name) + r"\." + key + r", (\d+)", txt)
    print(";", key, mm.group(1) if mm else "?")
