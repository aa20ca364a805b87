#!/usr/bin/env python3
"""tools/isa_diff.py — did the device code change?   python tools/isa_diff.py A B

A and B are two output directories of `make -C surfacenet_amd/csrc asm ASM_DIR=...` (say a parent build and a working build). Every
*-gfx950.s present in both is cut at its function labels (`name:   ; @name`; what precedes the first label and the module's metadata block
are two pieces of their own), lines containing __hip_cuid_ (a per-compilation id) are dropped, so are the assembler comments (`; ...`: they carry
the compiler's names of IR blocks, which are numbered through the whole unit and move when an unrelated `if constexpr` goes; the register and
scratch figures they also carry stay compared through the .amdhsa_ directives and the metadata), the number of the function inside its unit is
taken out of the local labels (.LBB<n>_k, .Lfunc_end<n>: it moves when a kernel joins or leaves the unit), what follows the last function is a
piece of its own, a bare `.text` that ends a piece is dropped (it depends on what comes next), and the pieces are compared as text, kernel
by kernel. Prints every kernel whose text differs, demangled, with both line counts. Exit status 1 if a kernel differs, if the two sides do
not hold the same kernels, or if a unit is missing on one side; 0 otherwise. It compares text only and knows nothing about instructions."""
import os
import re
import subprocess
import sys

LABEL = re.compile(r"^(\S+):\s*; @(\S+)\s*$")
INTRO = re.compile(r"^\s*\.(section\s+\.text|protected|globl|weak|hidden|p2align|type)\b")      # a function's directives in front of its label
FUNC_NO = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")
HEAD, META, TAIL = "(module header)", "(module metadata)", "(module trailer)"


def pieces(path):
    out, name = {HEAD: []}, HEAD
    for line in open(path, errors="replace"):
        if "__hip_cuid_" in line:
            continue
        m = LABEL.match(line)
        if m and m.group(1) == m.group(2):
            prev, name = out[name], m.group(1)
            if name in out:
                sys.exit("%s: label %s appears twice" % (path, name))
            out[name] = []
            while prev and INTRO.match(prev[-1]):
                out[name].insert(0, prev.pop())
        elif line.strip() == ".amdgpu_metadata":
            name = META
            out[name] = []
        elif line.strip().startswith(".p2alignl") and name not in (HEAD, META):
            name = TAIL
            out[name] = []
        code = FUNC_NO.sub(r".\1", line.split(";", 1)[0].rstrip())
        if code:
            out[name].append(code)
    for text in out.values():
        while text and text[-1].strip() == ".text":
            text.pop()
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True)
    dem = r.stdout.split("\n")[:len(names)] if r.returncode == 0 else names
    return dict(zip(names, dem))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a_dir, b_dir = sys.argv[1:]
    units = [sorted(f for f in os.listdir(d) if f.endswith("-gfx950.s")) for d in (a_dir, b_dir)]
    bad = False
    for side, other, d in ((0, 1, a_dir), (1, 0, b_dir)):
        for f in units[side]:
            if f not in units[other]:
                print("unit %s: only in %s" % (f, d))
                bad = True
    both = [f for f in units[0] if f in units[1]]
    if not both:
        sys.exit("no *-gfx950.s common to %s and %s" % (a_dir, b_dir))
    total = changed = 0
    for f in both:
        pa, pb = pieces(os.path.join(a_dir, f)), pieces(os.path.join(b_dir, f))
        names = [n for n in pa if n in pb]
        odd = [n for n in list(pa) + list(pb) if (n in pa) != (n in pb)]
        diff = [n for n in names if pa[n] != pb[n]]
        dem = demangle([n for n in odd + diff if n not in (HEAD, META, TAIL)])
        for n in odd:
            print("%s: only in %s: %s" % (f, a_dir if n in pa else b_dir, dem.get(n, n)))
        for n in diff:
            print("%s: DIFFERS (%d | %d lines): %s" % (f, len(pa[n]), len(pb[n]), dem.get(n, n)))
        nk = len([n for n in names if n not in (HEAD, META, TAIL)])
        print("%-50s %4d kernels compared, %d changed" % (f, nk, len(diff)))
        total += nk
        changed += len(diff)
        bad = bad or bool(odd) or bool(diff)
    print("%d units, %d kernels compared, %d changed%s" % (len(both), total, changed, "" if not bad else "  -> DIFFERENT"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
