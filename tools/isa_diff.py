#!/usr/bin/env python3
"""Compare the instruction streams of two builds of the kernel units' assembly (`make asm`), kernel by kernel.
usage: tools/isa_diff.py DIR_A DIR_B      (two directories of .s files, e.g. a parent checkout's csrc/build and this one's)
An instruction stream = the lines of a function that do not begin with `;`, `.` or `//` (comments, directives, labels),
trailing `;` comments cut; a branch target is named by the position of the instruction it points at, not by its label
(block numbers move with the compiler's bookkeeping, not with the code).  Per function: instructions in A and in B,
differing lines (0 = identical), and VGPR / SGPR / scratch / occupancy / LDS (the numbers tools/kernel_resources.py
prints; `a -> b` where the two builds differ; `-` for a function that is no kernel)."""
import difflib, os, re, subprocess, sys

RES = (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
       ("occ", r"; Occupancy: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"))


def resolve(body, at):
    """branch targets by the position they point at"""
    return [re.sub(r"\.LBB\d+_\d+", lambda t: "@%d" % at.get(t.group(0), -1), l) for l in body]


def functions(path):
    """symbol -> (instruction lines, resource numbers) for every function of one .s file (a function runs from its label
    to the `.Lfunc_end` label the compiler closes every function with; what follows the last one is data)"""
    out, name, body, info, at = {}, None, [], None, {}
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and name is None:
            name, body, at = m.group(1), [], {}
            continue
        if name is not None and info is None:
            if line.startswith(".Lfunc_end"):
                info = {}
                out[name] = (resolve(body, at), info)
                continue
            s = line.strip()
            lab = re.match(r"^(\.LBB\d+_\d+):", s)
            if lab:
                at[lab.group(1)] = len(body)
            if s and not s.startswith((";", ".", "//")):
                body.append(s.split(";")[0].rstrip())
        elif info is not None:  # behind the function: its resource comment block, up to the next section of text
            for key, pat in RES:
                mm = re.match(pat, line)
                if mm:
                    info[key] = int(mm.group(1))
            if line.startswith("\t.section\t.text") or line.startswith("\t.text"):
                name, info = None, None
    return out


def demangle(names):
    if not names:
        return {}
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        res = []
    if len(res) != len(names):  # no c++filt: the mangled names
        res = list(names)
    short = {}
    for n, d in zip(names, res):
        d = d.replace("pmx::(anonymous namespace)::", "").replace("pmx::", "")
        d = re.sub(r"^void ", "", d)
        short[n] = re.sub(r"\(.*$", "", d)[:72]
    return short


def main(a, b):
    units = sorted(f for f in os.listdir(a) if f.endswith(".s") and os.path.exists(os.path.join(b, f)))
    total = changed = 0
    for u in units:
        fa, fb = functions(os.path.join(a, u)), functions(os.path.join(b, u))
        names = demangle(sorted(set(fa) | set(fb)))
        print(f"== {u}: {len(fa)} functions in A, {len(fb)} in B")
        print(f"{'function':72s} {'insn A':>7s} {'insn B':>7s} {'differ':>7s}  resources (vgpr sgpr scratch occ lds)")
        for n in sorted(names, key=names.get):
            (ia, ra), (ib, rb) = fa.get(n, ([], {})), fb.get(n, ([], {}))
            nd = 0 if ia == ib else sum(1 for l in difflib.unified_diff(ia, ib, n=0, lineterm="")
                                        if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            fmt = lambda r: " ".join(str(r.get(k, "-")) for k, _ in RES)
            res = fmt(ra) if ra == rb else f"{fmt(ra)} -> {fmt(rb)}"
            print(f"{names[n]:72s} {len(ia):7d} {len(ib):7d} {nd:7d}  {res}")
            total += 1
            changed += nd != 0
    print(f"{total} functions, {changed} with a different instruction stream")
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
