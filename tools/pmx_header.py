"""Parse include/pmx.h: the one reader of the header behind the generated bindings (gen_rust_binding.py ->
bindings/rust/pmx_sys.rs, gen_python_binding.py -> pharmsol_amd/_pmx_h.py).  A tool, never on the product's import path."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "pmx.h")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def parse_header(path=HDR):
    raw = open(path).read()
    text = strip_comments(raw)
    defines = {}
    for m in re.finditer(r"^\s*#define\s+(PMX_\w+)\s+(-?\d+)\s*$", text, flags=re.M):
        defines[m.group(1)] = int(m.group(2))
    consts = []  # (name, value) in header order
    for m in re.finditer(r"#define\s+(PMX_\w+)\s+(-?\d+)", text):
        consts.append((m.group(1), int(m.group(2))))
    enum_types = []
    for m in re.finditer(r"(typedef\s+)?enum\s*(\w+)?\s*\{([^}]*)\}\s*(\w+)?\s*;", text):
        if m.group(4):
            enum_types.append(m.group(4))
        nxt = 0
        for item in m.group(3).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                name, val = [s.strip() for s in item.split("=")]
                nxt = int(val, 0) if re.fullmatch(r"-?(0x)?[0-9a-fA-F]+", val) else defines.get(val, dict(consts).get(val))
            else:
                name = item
            consts.append((name, nxt))
            nxt += 1
    structs = []  # (name, [(field, ctype, ptr_depth, is_const, array_len)])
    opaque = []
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;", text):
        opaque.append(m.group(2))
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            mm = re.match(r"(const\s+)?(\w+)\s*(.*)$", decl)
            is_const, ctype, rest = bool(mm.group(1)), mm.group(2), mm.group(3)
            for d in rest.split(","):
                d = d.strip()
                depth = d.count("*")
                d = d.replace("*", "").strip()
                arr = None
                am = re.match(r"(\w+)\s*\[(\w+)\]$", d)
                if am:
                    d, n = am.group(1), am.group(2)
                    arr = int(n) if n.isdigit() else defines[n]
                fields.append((d, ctype, depth, is_const, arr))
        structs.append((m.group(3), fields))
    funcs = []  # (name, return type text, [(param, ctype, ptr_depth, is_const)])
    for m in re.finditer(r"^\s*((?:const\s+)?\w+\s*\**)\s*(pmx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M | re.S):
        ret, name, args = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        params = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                am = re.match(r"(const\s+)?(\w+)\s*(\*\s*\*|\*)?\s*(\w+)$", a)
                assert am, (name, a)
                params.append((am.group(4), am.group(2), (am.group(3) or "").count("*"), bool(am.group(1))))
        funcs.append((name, ret, params))
    return consts, enum_types, structs, opaque, funcs


def unique_consts(consts):
    """(name, value) once per name, in header order."""
    seen, out = set(), []
    for name, val in consts:
        if name not in seen and name != "PMX_H":
            seen.add(name)
            out.append((name, val))
    return out


def return_type(ret):
    """(ctype, ptr_depth, is_const) of a function's return type text."""
    rm = re.match(r"(const\s+)?(\w+)\s*(\**)$", ret)
    return rm.group(2), len(rm.group(3)), bool(rm.group(1))


def emit(out, text, tool):
    """Write `text` to `out`; with --check on the command line, fail instead if the committed file is stale."""
    rel = os.path.relpath(out, ROOT)
    if "--check" in sys.argv:
        ok = os.path.exists(out) and open(out).read() == text
        print(rel, "is", "up to date" if ok else f"STALE: run tools/{tool}")
        sys.exit(0 if ok else 1)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write(text)
    print("wrote", out)
