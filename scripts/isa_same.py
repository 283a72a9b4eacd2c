#!/usr/bin/env python3
"""Are two `make asm` outputs the same kernels?

    isa_same.py PARENT.s BRANCH.s [--rename OLD=NEW ...]

The gate of a refactor that must not change code generation: every kernel
(`.amdhsa_kernel` symbol) of PARENT.s must exist in BRANCH.s, and no other,
with an equal instruction stream and equal resources.  A kernel's stream is
the text between its label and its `.Lfunc_end`, with comments, assembler
directives and blank lines dropped and the compiler's local labels
(`.LBB3_17`, ...) numbered by first appearance inside the kernel, so that the
position of a kernel in the file does not matter and the branch structure
still does.  Resources are the metadata's `.vgpr_count`, `.sgpr_count`,
`.private_segment_fixed_size` (scratch) and `.group_segment_fixed_size` (LDS).

--rename OLD=NEW: a regular expression and its replacement (`re.sub`), applied
to PARENT.s's text first, for a kernel renamed on purpose, e.g.
    --rename '17trace3_hit_kernelILi(\\d)EE=13trace3_kernelILi\\1ELi3EE'

Text only: the script knows nothing about particular instructions.  Prints
one markdown table row per kernel; exit status 1 on any difference.
"""
import argparse
import re
import shutil
import subprocess
import sys

RESOURCES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
             "group_segment_fixed_size")
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]+[0-9][0-9_]*")


def kernel_streams(text):
    """{symbol: [instruction and label lines]} of every .amdhsa_kernel."""
    lines = text.split("\n")
    symbols = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    starts = {}
    for i, l in enumerate(lines):
        if l and not l[0].isspace() and ":" in l:
            starts.setdefault(l.split(":", 1)[0], i)
    out = {}
    for sym in symbols:
        body, names = [], {}
        for l in lines[starts[sym] + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";", 1)[0].strip()
            if not l or (l.startswith(".") and not l.endswith(":")):
                continue  # blank, comment or directive (a local label ends in ':')
            l = LOCAL_LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), l)
            body.append(" ".join(l.split()))
        else:
            raise SystemExit("no .Lfunc_end after " + sym)
        out[sym] = body
    return out


def kernel_resources(text):
    """{symbol: {field: value}} from the amdhsa.kernels metadata."""
    out, cur = {}, None
    meta = text.split("amdhsa.kernels:", 1)[1]
    for l in meta.split("\n"):
        if l.startswith("  - "):
            cur = {}
        m = re.match(r"(?:  - |    )\.(\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                out[m.group(2)] = cur
    return out


def pretty(symbols):
    """Demangled names without parameter lists, where c++filt is at hand."""
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {s: s for s in symbols}
    names = subprocess.run([tool], input="\n".join(symbols), capture_output=True,
                           text=True, check=True).stdout.split("\n")
    def short(n):
        n = n.replace("(anonymous namespace)::", "")
        return (n[5:] if n.startswith("void ") else n).split("(", 1)[0]
    return {s: short(n) for s, n in zip(symbols, names)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    a_text = open(args.parent).read()
    b_text = open(args.branch).read()
    for r in args.rename:
        old, new = r.split("=", 1)
        a_text = re.sub(old, new, a_text)
    a, b = kernel_streams(a_text), kernel_streams(b_text)
    ar, br = kernel_resources(a_text), kernel_resources(b_text)
    names = pretty(sorted(set(a) | set(b)))
    differing = 0
    print("| kernel | instructions | vgpr | sgpr | scratch | lds | verdict |")
    print("|---|---|---|---|---|---|---|")
    for sym in sorted(set(a) | set(b), key=lambda s: names[s]):
        if sym not in a or sym not in b:
            verdict = "only in " + ("parent" if sym in a else "branch")
            res, n = (ar if sym in a else br)[sym], len((a if sym in a else b)[sym])
            cells = [str(n)] + [res[k] for k in RESOURCES]
        else:
            same_isa = a[sym] == b[sym]
            n = str(len(a[sym])) if same_isa else "%d -> %d" % (len(a[sym]), len(b[sym]))
            cells = [n] + [ar[sym][k] if ar[sym][k] == br[sym][k]
                           else "%s -> %s" % (ar[sym][k], br[sym][k]) for k in RESOURCES]
            same_res = all(ar[sym][k] == br[sym][k] for k in RESOURCES)
            verdict = "same" if same_isa and same_res else \
                "DIFFERS" + ("" if same_isa else " (instructions)") + ("" if same_res else " (resources)")
        differing += verdict != "same"
        print("| `%s` | %s | %s |" % (names[sym], " | ".join(cells), verdict))
    print()
    print("%d kernels in parent, %d in branch, %d differing" % (len(a), len(b), differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
