#!/usr/bin/env python3
"""Per-symbol ISA comparison of attention kernel files between two trees.

    hipcc -S --cuda-device-only -O3 --offload-arch=gfx950 <file>.hip -o <dir>/<file>.s      in both trees, then
    tools/attention_isa_compare.py <parent dir> <this dir> [--files a,b,...] [--twin-suffix _seg_kernel] [--twin-of-suffix _kernel]

--files names the files to compare, without .hip (default: the three flash files attention, attention_bf16, attention_dh).

Per kernel symbol: the instruction lines with comments stripped and block labels renumbered, plus next_free_vgpr, next_free_sgpr,
accum_offset, LDS and scratch sizes of the kernel descriptor.  Symbols of the second tree that the first does not have are listed
beside their twin (the symbol without the suffix's middle part, e.g. attention_bf16_seg_kernel<..> beside attention_bf16_kernel<..>;
--twin-of-suffix names what the suffix becomes: `--twin-suffix _seg_bias_kernel --twin-of-suffix _seg_kernel` lists the weighted forms
of DESIGN.md 4w beside their segmented twins).
Exit status 1 if any symbol of the first tree is missing from or differs in the second.
"""
import re
import subprocess
import sys
from pathlib import Path

FILES = ("attention", "attention_bf16", "attention_dh")
FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    text = Path(path).read_text()
    desc = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        desc[m.group(1)] = tuple(re.search(r"\.amdhsa_" + f + r" (\S+)", m.group(2)).group(1) for f in FIELDS)
    out = {}
    for name in desc:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        labels, lines = {}, []
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith("."):
                lab = re.match(r"(\.LBB\d+_\d+):", ln)
                if lab:
                    labels.setdefault(lab.group(1), f"L{len(labels)}")
                    lines.append(labels[lab.group(1)] + ":")
                continue
            lines.append(ln)
        body = "\n".join(lines)
        for lab in re.findall(r"\.LBB\d+_\d+", body):
            labels.setdefault(lab, f"L{len(labels)}")
        body = re.sub(r"\.LBB\d+_\d+", lambda x: labels[x.group(0)], body)
        out[name] = (desc[name], body)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines())) if r.returncode == 0 else {n: n for n in names}


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    suffix = sys.argv[sys.argv.index("--twin-suffix") + 1] if "--twin-suffix" in sys.argv else "_seg_kernel"
    twin_suffix = sys.argv[sys.argv.index("--twin-of-suffix") + 1] if "--twin-of-suffix" in sys.argv else "_kernel"
    files = sys.argv[sys.argv.index("--files") + 1].split(",") if "--files" in sys.argv else FILES
    bad = same = 0
    for f in files:
        a, b = kernels(f"{a_dir}/{f}.s"), kernels(f"{b_dir}/{f}.s")
        pretty = demangle(sorted(set(a) | set(b)))
        print(f"== {f}.hip: {len(a)} symbols before, {len(b)} after")
        for name in sorted(a):
            if name not in b:
                bad += 1
                print(f"MISSING   {pretty[name]}")
            elif a[name] != b[name]:
                bad += 1
                print(f"DIFFERS   {pretty[name]}  descriptor {a[name][0]} -> {b[name][0]}, "
                      f"{a[name][1].count(chr(10)) + 1} -> {b[name][1].count(chr(10)) + 1} lines")
            else:
                same += 1
        def short(n):                                                             # attention_bf16_seg_kernel<true, 2>
            m = re.search(r"(\w+<[^>]*>)", pretty[n]) or re.search(r"(\w+)\(", pretty[n])      # (or the name of a kernel that is no template)
            return m.group(1) if m else pretty[n]
        by_short = {short(n): n for n in b}
        for name in sorted(set(b) - set(a), key=short):
            twin = by_short.get(short(name).replace(suffix, twin_suffix))
            d = dict(zip(FIELDS, b[name][0]))
            t = dict(zip(FIELDS, b[twin][0])) if twin else {}
            print(f"NEW       {short(name)}: " + ", ".join(f"{k} {d[k]} (twin {t.get(k, '?')})" for k in FIELDS) +
                  f", {b[name][1].count(chr(10)) + 1} lines (twin {b[twin][1].count(chr(10)) + 1 if twin else '?'})")
    print(f"== {same} existing symbols identical, {bad} missing or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
