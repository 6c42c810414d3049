"""Compare two device assemblies of the engine, function by function: python tools/device_code_diff.py A.s B.s

`make -C unige-tasi-path-planners_amd device-asm [DEFS="-D..."] ASM=A.s` writes one.  A refactor that must not move the kernels is held to this:
the same function names on both sides and every body the same text.  Text only -- the comparison knows nothing about instructions.  The one line of
a device assembly that follows the SOURCE text rather than the code, the module's __hip_cuid_<hash> symbol, is ignored; so is the number a
local label carries for its function's POSITION in the module (.LBB46_2, .Lfunc_end46, .LJTI46_0 -> .LBB#_2 ...): a kernel added in front of
another moves that number and nothing else of the other's body.
Prints the counts, the names present on one side only and the names whose bodies differ; --show N prints the first N differing lines of each.
Exit status 0: no difference."""
import argparse
import difflib
import re
import sys

CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
ORDINAL = re.compile(r"(?<![A-Za-z0-9_])((?:\.L)?(?:BB|JTI|func_begin|func_end))\d+")      # (also the "Header=BB46_3" of a comment)


def functions(path):
    """{name: [body lines]} for every function of a device assembly (a .type NAME,@function line ... its .Lfunc_end label), and the other lines"""
    funcs, rest, name = {}, [], None
    for line in open(path):
        line = ORDINAL.sub(r"\1#", CUID.sub("__hip_cuid_", line.rstrip("\n")))
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
            funcs[name] = []
            continue
        if name is None:
            rest.append(line)
            continue
        funcs[name].append(line)
        if re.match(r"\s*\.size\s+" + re.escape(name) + r",", line):
            name = None
    return funcs, rest


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--show", type=int, default=0, help="print the first N differing lines of every differing body")
    args = ap.parse_args()
    fa, ra = functions(args.a)
    fb, rb = functions(args.b)
    print("functions: %d in %s, %d in %s" % (len(fa), args.a, len(fb), args.b))
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    for side, names in ((args.a, only_a), (args.b, only_b)):
        for n in names:
            print("only in %s: %s" % (side, n))
    differ = [n for n in sorted(set(fa) & set(fb)) if fa[n] != fb[n]]
    for n in differ:
        print("body differs: %s (%d / %d lines)" % (n, len(fa[n]), len(fb[n])))
        if args.show:
            for l in list(difflib.unified_diff(fa[n], fb[n], lineterm="", n=0))[2:2 + args.show]:
                print("    " + l)
    outside = sum(1 for t in difflib.ndiff(ra, rb) if t[:1] in "+-") if ra != rb else 0
    print("bodies identical: %d of %d; differing: %d; lines outside functions that differ: %d" % (
        len(set(fa) & set(fb)) - len(differ), len(set(fa) & set(fb)), len(differ), outside))
    return 1 if (only_a or only_b or differ or outside) else 0


if __name__ == "__main__":
    sys.exit(main())
