#!/usr/bin/env python
"""Which kernels of two builds are the same machine code?  Compares two device assembly listings
(hipcc with the Makefile's HIPFLAGS and KARG_PRELOAD plus --offload-device-only -S) kernel by
kernel, the method of profiles/r08_isa_equal.txt:

  per kernel, the text from its label to .Lfunc_end (code and .amdhsa_kernel descriptor), ';'
  comments dropped, mangled names, __hip_cuid_* and .LBB / .Lfunc numbers replaced by
  placeholders; kernels paired by demangled name; SHA-1 of both normalised bodies compared.

    python tools/isa_equal.py parent.s new.s [--expect-changed REGEX] > profiles/rNN_isa_equal.txt

Exit status 1 when a kernel outside --expect-changed differs, appears or disappears.
"""
from __future__ import annotations

import argparse
import hashlib
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read().splitlines()
    names = [m.group(1) for ln in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    want = set(names)
    out, cur, body = {}, None, []
    for ln in text:
        m = re.match(r"(\S+):", ln)
        if cur is None and m and m.group(1) in want:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"\.Lfunc_end\d+:", ln):
                out[cur] = body
                cur = None
                continue
            ln = ln.split(";")[0].rstrip()
            if not ln.strip():
                continue
            ln = re.sub(r"_Z[\w$.]+", "@SYM", ln)
            ln = re.sub(r"__hip_cuid_\w+", "@CUID", ln)
            ln = re.sub(r"\.L(BB|func_\w+?|tmp|_amdgpu\w*?)(\d+)(_\d+)?", r".L\1#", ln)
            body.append(ln)
    return out


def demangle(names):
    got = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    short = [re.sub(r"rt::\(anonymous namespace\)::|rt::|\(.*$", "", g) for g in got]
    return dict(zip(names, short)) if len(short) == len(names) else {n: n for n in names}


def summarise(body):
    insts = sum(1 for ln in body if ln.startswith("\t") and not ln.lstrip().startswith("."))
    return insts, hashlib.sha1("\n".join(body).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--expect-changed", default=None, help="regex on the demangled name: kernels meant to differ")
    a = ap.parse_args()
    A, B = kernels(a.parent), kernels(a.new)
    dn = demangle(sorted(set(A) | set(B)))
    exp = re.compile(a.expect_changed) if a.expect_changed else None
    same, changed, bad = [], [], []
    for k in sorted(set(A) | set(B), key=lambda n: dn[n]):
        sa, sb = (summarise(A[k]) if k in A else None), (summarise(B[k]) if k in B else None)
        row = (f"{dn[k]} | {sa[0] if sa else '-'} -> {sb[0] if sb else '-'} | {sa[1] if sa else 'absent'} | "
               f"{sb[1] if sb else 'absent'}")
        if sa and sb and sa[1] == sb[1]:
            same.append(row)
        elif exp and exp.search(dn[k]):
            changed.append(row)
        else:
            bad.append(row)
    print(f"{len(A)} -> {len(B)} kernels: {len(same)} identical, {len(changed)} changed as intended, {len(bad)} unexpected")
    print("Columns: kernel | instruction lines parent -> new | SHA-1 parent | SHA-1 new")
    for title, rows in (("unexpected", bad), ("changed as intended", changed), ("identical", same)):
        print(f"\n== {title}: {len(rows)} ==")
        print("\n".join(rows))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
