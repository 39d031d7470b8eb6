#!/usr/bin/env python3
"""Instruction census of the loops of rnnt_alpha_beta_kernel<1>, from the gfx950 ISA.

Compiles pika_amd/csrc/rnnt_loss.hip to assembly (device only, no GPU needed), finds every loop
of the one-wave alpha/beta kernel (a backward branch and its target label) and prints, per loop:
instructions, diagonals (one v_exp_f32 per diagonal), instructions / branches / exec-mask writes per
diagonal, and the vmcnt waits.

By default only the two bulk loops are printed: the spans of exactly 32 diagonals (two 16-diagonal
groups per trip) with at most two exec-mask writes and two branches per group, all of them at the
group's end around the lane-masked offsets store.  A backward branch of the masked code is not always a loop
of its own (the structurizer's flow blocks jump back too), so the spans --all prints beyond these
mix head, bulk and tail and are not per-diagonal costs.

    python tools/ab_isa_count.py [--asm FILE] [--all]   # FILE: an existing .s instead of compiling
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN12_GLOBAL__N_122rnnt_alpha_beta_kernelILi1EE"


def compile_asm(out):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "pika_amd", "csrc"), "--cuda-device-only", "-S",
           os.path.join(ROOT, "pika_amd", "csrc", "rnnt_loss.hip"), "-o", out]
    subprocess.run(cmd, check=True)


def kernel_lines(path):
    lines, on = [], False
    for ln in open(path):
        if ln.startswith(KERNEL) and ln.rstrip().endswith(":") or (ln.startswith(KERNEL) and ": ;" in ln):
            on = True
            continue
        if on:
            if ln.lstrip().startswith(".Lfunc_end"):
                break
            lines.append(ln.rstrip("\n"))
    return lines


def is_insn(ln):
    s = ln.strip()
    return bool(s) and not s.startswith((";", ".")) and not s.endswith(":")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--all", action="store_true", help="every backward-branch span, not only the bulk loops")
    args = ap.parse_args()
    path = args.asm
    if not path:
        path = os.path.join(tempfile.mkdtemp(), "rnnt_loss.s")
        compile_asm(path)
    lines = kernel_lines(path)
    if not lines:
        sys.exit("kernel %s not found in %s" % (KERNEL, path))
    labels = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            labels[m.group(1)] = i
    print("     %-10s %6s %5s %9s %9s %9s  %s" % ("loop", "insns", "diag", "insn/diag", "br/diag",
                                               "exec/diag", "vmcnt waits"))
    seen, nbulk = set(), 0
    for i, ln in enumerate(lines):
        m = re.match(r"\s*s_cbranch_\w+\s+(\.LBB\w+)|\s*s_branch\s+(\.LBB\w+)", ln)
        if not m:
            continue
        tgt = m.group(1) or m.group(2)
        if tgt not in labels or labels[tgt] > i:
            continue
        body = [l.strip() for l in lines[labels[tgt]:i + 1] if is_insn(l)]
        n = len(body)
        diag = sum(1 for l in body if l.startswith("v_exp_f32"))
        br = sum(1 for l in body if l.startswith(("s_cbranch", "s_branch")))
        ex = sum(1 for l in body if re.search(r"\bexec\b", l) and not l.startswith("s_cbranch"))
        waits = [re.search(r"vmcnt\((\d+)\)", l).group(1) for l in body
                 if l.startswith("s_waitcnt") and "vmcnt" in l]
        bulk = diag == 32 and ex <= 4 and br <= 4
        if bulk:
            if tgt in seen:
                continue
            seen.add(tgt)
            nbulk += 1
        elif not args.all:
            continue
        per = lambda k: "%.1f" % (k / diag) if diag else "-"
        print("BULK " if bulk else "     ", end="")
        print("%-10s %6d %5d %9s %9s %9s  %s" % (tgt, n, diag, per(n), per(br), per(ex),
                                                 " ".join(waits)))
    if nbulk != 2:
        sys.exit("expected 2 bulk loops (alpha, beta), found %d" % nbulk)


if __name__ == "__main__":
    main()
