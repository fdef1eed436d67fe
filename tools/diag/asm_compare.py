#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds of one .hip file, kernel by kernel:

    python tools/diag/asm_compare.py parent.s new.s [--changed SUBSTRING]

(each .s from `hipcc <the flags of __graft_entry__.build()> --cuda-device-only -S`).  For every kernel symbol: is the body the same text
(comments and blank lines dropped)?  For the symbols whose name contains SUBSTRING (the ones a change is meant to touch): instruction
count by kind, before and after (with everything else untouched, the difference IS the region that was changed), and the histogram of
the v_*_f64 opcodes: the arithmetic ones must not move (unchanged arithmetic = unchanged contraction = the same bits); the comparisons
(v_cmp_*: the non-finite tests of the copy-out, one per trip) are listed.  Exit status 1 when a symbol outside SUBSTRING differs or an
arithmetic histogram moved."""
import argparse
import collections
import re
import sys


def kernels(path):
    """{symbol: [instruction lines]} for every .amdhsa_kernel symbol of the file"""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        code = line.split(";")[0].strip()
        if code:
            cur.append(code)
    return out


def is_instruction(line):
    return not line.endswith(":") and not line.startswith(".")


def summary(body):
    ins = [ln for ln in body if is_instruction(ln)]
    hist = collections.Counter(ln.split()[0] for ln in ins if re.match(r"v_\w*f64", ln.split()[0]))
    kinds = collections.Counter()
    for ln in ins:
        op = ln.split()[0]
        kinds["global_store" if op.startswith("global_store") else "global_load" if op.startswith("global_load") else "ds_read" if op.startswith("ds_read") or op.startswith("ds_load")
              else "branch" if op.startswith("s_cbranch") or op == "s_branch" else "s_waitcnt" if op == "s_waitcnt" else "valu" if op.startswith("v_") else "salu / other"] += 1
    return len(ins), hist, kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--changed", default="Lb1EE", help="substring of the symbols the change is meant to touch")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.new)
    bad = 0
    same = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("ONLY IN ONE BUILD:", name)
            bad += 1
        elif a.changed in name and "knot_kernel" in name:
            continue
        elif old[name] == new[name]:
            same += 1
        else:
            print("DIFFERS:", name)
            bad += 1
    print("%d kernel symbols outside *%s* have identical bodies, %d differ" % (same, a.changed, bad))
    for name in sorted(n for n in new if a.changed in n and "knot_kernel" in n and n in old):
        (n0, h0, k0), (n1, h1, k1) = summary(old[name]), summary(new[name])
        print(name)
        print("  instructions %d -> %d (%+d): %s" % (n0, n1, n1 - n0, ", ".join("%s %d -> %d" % (k, k0[k], k1[k]) for k in sorted(set(k0) | set(k1)))))
        arith0 = {op: c for op, c in h0.items() if not op.startswith("v_cmp")}
        arith1 = {op: c for op, c in h1.items() if not op.startswith("v_cmp")}
        print("  v_*_f64 arithmetic opcodes: %d kinds, %d instructions; histogram %s" % (len(arith1), sum(arith1.values()), "IDENTICAL" if arith0 == arith1 else "MOVED"))
        for op in sorted(set(h0) | set(h1)):
            if h0[op] != h1[op]:
                print("    %s %d -> %d" % (op, h0[op], h1[op]))
        if arith0 != arith1:
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
