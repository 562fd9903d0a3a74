#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assembly listings of the same source file (hipcc -S --cuda-device-only with the
Makefile's flags): name, instruction count before and after, and whether the instruction streams are the same once local labels
are renumbered in order of appearance.  With -Rpass-analysis=kernel-resource-usage logs it adds, for every kernel whose stream
differs, the compiler's resource lines (VGPRs, scratch, occupancy, LDS) before and after.

usage: tools/isa_diff.py before.s after.s [--rpass before.log after.log] [--rename OLD=NEW ...]
       (--rename pairs a kernel of `before` with a differently named one of `after`; names are demangled, without arguments)"""
import argparse
import re
import subprocess


def kernels(path):
    """{demangled name: [instructions]} for every kernel (symbols with an .amdhsa_kernel descriptor) of the listing."""
    text = open(path).read()
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        body = re.search(rf"^{re.escape(sym)}:.*?^\.Lfunc_end\d+:", text, re.M | re.S).group(0)
        labels, ins = {}, []
        for line in body.splitlines()[1:]:
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.endswith(":"):
                continue
            line = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), line)
            if not line.endswith(":"):
                ins.append(line)
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        out[re.sub(r"^void ", "", name).split("(")[0]] = ins
    return out


def resources(path):
    """{demangled name: 'VGPRs .. Occupancy .. LDS ..'} from a kernel-resource-usage log."""
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: (?:.*: )?(?:Function Name: (\S+)|\s*(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+))", line)
        if m and m.group(1):
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"^void ", "", name).split("(")[0]
            out[name] = []
        elif m and name:
            out[name].append(f"{m.group(2).split(' [')[0]} {m.group(3)}")
    return {k: ", ".join(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rpass", nargs=2)
    ap.add_argument("--rename", action="append", default=[])
    args = ap.parse_args()
    rename = dict(r.split("=", 1) for r in args.rename)
    a, b = kernels(args.before), kernels(args.after)
    ra, rb = (resources(args.rpass[0]), resources(args.rpass[1])) if args.rpass else ({}, {})
    for name, ins in a.items():
        new = rename.get(name, name)
        if new not in b:
            print(f"{name}: {len(ins)} -> (gone)")
            continue
        same = ins == b[new]
        print(f"{name}{' -> ' + new if new != name else ''}: {len(ins)} -> {len(b[new])} {'same' if same else 'DIFFERENT'}")
        if not same and args.rpass:
            print(f"    before: {ra.get(name)}\n    after:  {rb.get(new)}")
    for name in b.keys() - {rename.get(n, n) for n in a}:
        print(f"{name}: (new) -> {len(b[name])}")


if __name__ == "__main__":
    main()
