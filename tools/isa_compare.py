#!/usr/bin/env python3
"""Are the kernels of two builds of rnnt_loss.hip the same machine code?  (No GPU needed.)

    python tools/isa_compare.py OLD.s [NEW.s]      # NEW.s: compiled from the tree when omitted

Both files are device-only gfx950 assembly (tools/ab_isa_count.compile_asm).  Every kernel is compared by name, by
instruction text and by its .amdhsa_* descriptor (registers, LDS, scratch).  Comments are dropped and the function
ordinal is taken out of local labels (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>): it follows emission order, which a change
of the host code may permute.  Exits non-zero on any difference."""
import os
import re
import sys
import tempfile

from ab_isa_count import compile_asm


def kernels(path):
    """{symbol: (body lines, descriptor lines)} of every kernel in an assembly file."""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)^\s*\.end_amdhsa_kernel" % re.escape(name), text, re.M | re.S).group(1)
        clean = []
        for ln in body.split("\n"):
            ln = re.sub(r"\.(LBB|Lfunc_end|Ltmp|Lfunc_begin)\d+", r".\1", ln.split(";")[0].strip())
            if ln:
                clean.append(ln)
        out[name] = (clean, [ln.split(";")[0].strip() for ln in desc.split("\n") if ln.strip()])
    return out


def main():
    old = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(tempfile.mkdtemp(), "rnnt_loss.s")
    if len(sys.argv) <= 2:
        compile_asm(new)
    a, b = kernels(old), kernels(new)
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print("only in %s: %s" % ("old" if k in a else "new", k))
    for k in sorted(set(a) & set(b)):
        if a[k][0] != b[k][0]:
            bad.append(k)
            print("text differs: %s (%d vs %d lines)" % (k, len(a[k][0]), len(b[k][0])))
        if a[k][1] != b[k][1]:
            bad.append(k)
            print("descriptor differs: %s" % k)
    print("%d kernels old, %d new: %s" % (len(a), len(b), "DIFFERENT" if bad else "identical"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
