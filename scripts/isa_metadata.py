#!/usr/bin/env python3
"""Per-kernel resource figures from the assembly `hipcc --cuda-device-only -S` writes: VGPR, AGPR, SGPR and spill counts, private
and LDS bytes.  One file: prints the table.  Two files: prints every kernel whose figures differ (exit 1 if any does) -- the check
that a change to a shared header left the existing kernels as they were (DESIGN.md sections 11 and 12).

    hipcc <the Makefile's FLAGS> -Wno-unused-command-line-argument --cuda-device-only -S -o new.s gsim_scan.hip
    scripts/isa_metadata.py old.s new.s
"""
import re
import sys

KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size"]


def kernels(path):
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")]
    out = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS)
    return out


def main():
    a = kernels(sys.argv[1])
    if len(sys.argv) == 2:
        print("kernel " + " ".join(k.lstrip(".") for k in KEYS))
        for n, v in sorted(a.items()):
            print(n, *v)
        return 0
    b = kernels(sys.argv[2])
    bad = [n for n in sorted(set(a) | set(b)) if a.get(n) != b.get(n)]
    for n in bad:
        print(n, a.get(n), b.get(n))
    print("%d kernels, %d differ" % (len(set(a) | set(b)), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
