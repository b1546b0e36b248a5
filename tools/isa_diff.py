#!/usr/bin/env python3
"""
Did a refactor change code generation?  Compiles every unit (*.hip) of pygmu2_amd/csrc of a git revision and of the
working tree to gfx950 device assembly (no GPU needed) and compares every kernel, by name, wherever it lives on either side:

    python tools/isa_diff.py REV          # a markdown table, one row per kernel; exit status 1 if anything differs

Two things are compared per kernel:
    instructions   the labels and instruction lines of its body, comments stripped and LLVM's local labels renamed:
                   .LBB<f>_<b>, .Ltmp<f>, .Lfunc_begin<f>, .Lfunc_end<f> and .LJTI<f>_<t> carry the index <f> of the
                   function in its translation unit, so a kernel that moves gets other label names around the same code
    descriptor     the lines of its .amdhsa_kernel ... .end_amdhsa_kernel block: registers, LDS, scratch and the other
                   fields its occupancy follows from
A kernel that is missing on one side, or that two units of one side both define, fails the comparison as well.  Device
functions that were not inlined are compared like kernels (they have no descriptor).

The flags are build.py's (the library's own), the compiler call is isa_count.assembly's.
"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOCAL_LABEL = re.compile(r"\.L(BB|tmp|func_begin|func_end|JTI)\d+")


def normalise(line: str) -> str:
    """One line of assembly without its comment, its indentation and the function index of its local labels."""
    return LOCAL_LABEL.sub(r".L\1#", line.split(";")[0].strip())


def kernels(asm: str):
    """{function name: {"insts": [normalised lines of the body], "desc": [descriptor lines] or None}}"""
    out, cur, in_desc = {}, None, False
    types = set(re.findall(r"^\s*\.type\s+([\w$.]+),@function", asm, re.M))
    for raw in asm.splitlines():
        s = normalise(raw)
        if not s:
            continue
        if cur is None:
            if s.endswith(":") and s[:-1] in types:
                cur = out[s[:-1]] = {"insts": [], "desc": None}
            continue
        if s.startswith(".amdhsa_kernel"):
            cur["desc"], in_desc = [], True
        elif s.startswith(".end_amdhsa_kernel"):
            in_desc = False
        elif in_desc:
            cur["desc"].append(s)
        elif s.startswith(".Lfunc_end"):
            cur = None
        else:
            cur["insts"].append(s)           # instructions, labels, and directives (.p2align) between them
    return out


def pair(base: dict, tree: dict):
    """base, tree: {unit name: assembly text}.  Returns (rows, ok); a row is (function, unit in base, unit in tree,
    instructions, descriptor) with the last two one of "same", "DIFFERENT", "missing", "duplicate", or "-" (no
    descriptor on either side: a device function)."""
    sides, dup = [], set()
    for units in (base, tree):
        found = {}
        for unit, asm in units.items():
            for name, k in kernels(asm).items():
                if name in found:
                    dup.add(name)
                    found[name] = (found[name][0] + "+" + unit, k)
                else:
                    found[name] = (unit, k)
        sides.append(found)
    rows, ok = [], True
    for name in sorted(set(sides[0]) | set(sides[1])):
        b, t = sides[0].get(name), sides[1].get(name)
        if name in dup:
            insts = desc = "duplicate"
        elif b is None or t is None:
            insts = desc = "missing"
        else:
            insts = "same" if b[1]["insts"] == t[1]["insts"] else "DIFFERENT"
            if b[1]["desc"] is None and t[1]["desc"] is None:
                desc = "-"
            else:
                desc = "same" if b[1]["desc"] == t[1]["desc"] else "DIFFERENT"
        ok = ok and insts == "same" and desc in ("same", "-")
        rows.append((name, b[0] if b else "-", t[0] if t else "-", insts, desc))
    return rows, ok


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
    import isa_count
    from pygmu2_amd import build
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-w"]
    with tempfile.TemporaryDirectory() as tmp:
        archive = subprocess.run(["git", "-C", ROOT, "archive", rev, "pygmu2_amd/csrc", "include"], check=True,
                                 stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=archive, check=True)
        base_csrc = os.path.join(tmp, "pygmu2_amd", "csrc")
        trees = (("base", base_csrc, os.path.join(tmp, "include")), ("tree", build.CSRC, os.path.join(ROOT, "include")))
        jobs = [(side, u, csrc, inc) for side, csrc, inc in trees for u in sorted(os.listdir(csrc)) if u.endswith(".hip")]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            texts = list(pool.map(lambda j: isa_count.assembly(j[1], flags=flags, csrc=j[2], include=j[3]), jobs))
    sides = {"base": {}, "tree": {}}
    for (side, unit, _, _), text in zip(jobs, texts):
        sides[side][unit] = text
    rows, ok = pair(sides["base"], sides["tree"])
    print(f"| function | unit at {rev} | unit in this tree | instructions | descriptor |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| `" + r[0] + "` | " + " | ".join(r[1:]) + " |")
    n_kernels = sum(1 for r in rows if r[4] != "-")
    moved = sum(1 for r in rows if r[1] != r[2])
    print(f"\n{len(rows)} functions ({n_kernels} kernels), {moved} in another unit than at {rev}: "
          + ("all instruction streams and descriptors equal" if ok else "NOT all equal"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
