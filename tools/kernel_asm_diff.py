"""Did a change to a .hip file move the gfx950 instruction stream?  Compares two builds of ONE source file, kernel by kernel.  No GPU.

  python tools/kernel_asm_diff.py OLD NEW [--rename 'old_kernel<false>=new_kernel<false, true>' ...]

OLD / NEW: two object files of the build (f2-nerf_amd/build/field.o of two trees) or two outputs of hipcc --cuda-device-only -S.
Per kernel it prints "identical" -- the same instructions with the same operands in the same order -- or both instruction counts,
the opcodes whose counts differ and both sides' resource metadata.  What is not compared: comments, directives, the numbers of
block labels, kernel names, and the pc-relative literals behind s_getpc_b64 (they move with every other function of the file).
Exit status 1 when any kernel differs or exists on one side only."""
import argparse
import collections
import re
import sys

import yaml

import kernel_resources as kr

RES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count",
       ".sgpr_spill_count")


def parse(path):
    """{kernel<template args>: (instructions, metadata)} of an object file or an assembly listing"""
    if path.endswith(".o"):
        meta = kr.code_object_metadata(path)
        text, comment = kr.code_object_dump(path, "llvm-objdump", "-d"), "//"
        label = re.compile(r"^[0-9a-f]+ <(\w+)>:")
    else:
        text, comment = open(path).read(), ";"
        start = text.index("---", text.index(".amdgpu_metadata"))
        meta = yaml.safe_load(text[start:text.index("\n...", start)])["amdhsa.kernels"]
        label = re.compile(r"^(\w+):")
    by_symbol = {k[".name"]: k for k in meta}
    code, cur, pcrel = {}, None, 0
    for line in text.splitlines():
        m = label.match(line)
        if m:
            cur = code.setdefault(m.group(1), []) if m.group(1) in by_symbol else None
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.startswith("\t") and not line.startswith("\t."):
            ins = re.sub(r"\.LBB\d+_\d+", ".LBB", " ".join(line.split(comment)[0].split()))
            if not ins:
                continue
            if pcrel and ins.startswith("s_add"):  # s_add_u32 / s_addc_u32 lo, hi of an address behind s_getpc_b64
                ins = ins.rsplit(",", 1)[0] + ", <pcrel>"
            pcrel = 2 if ins.startswith("s_getpc_b64") else max(0, pcrel - 1)
            cur.append(ins)
    for ins in code.values():  # (the padding behind the last s_endpgm)
        while ins and ins[-1] != "s_endpgm":
            ins.pop()
    names = kr.demangle(list(code))
    return {kr.short(n): (code[s], by_symbol[s]) for s, n in zip(code, names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    rename = dict(r.split("=", 1) for r in a.rename)
    old = {rename.get(k, k): (k, v) for k, v in parse(a.old).items()}
    new = parse(a.new)
    n_diff = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%-60s only in %s" % (name, "NEW" if name in new else "OLD"))
            n_diff += 1
            continue
        was, ((ci, mi), (cj, mj)) = old[name][0], (old[name][1], new[name])
        title = name if was == name else "%s -> %s" % (was, name)
        if ci == cj:
            print("%-60s identical (%d instructions)" % (title, len(ci)))
            continue
        n_diff += 1
        hi, hj = collections.Counter(i.split()[0] for i in ci), collections.Counter(i.split()[0] for i in cj)
        print("%-60s DIFFERS: %d -> %d instructions" % (title, len(ci), len(cj)))
        print("    opcodes: " + (", ".join("%s %d -> %d" % (op, hi[op], hj[op]) for op in sorted(set(hi) | set(hj)) if hi[op] != hj[op])
                                 or "same histogram (operands or order differ)"))
        for side, m in (("old", mi), ("new", mj)):
            print("    %s: " % side + " ".join("%s=%s" % (k[1:], m.get(k, 0)) for k in RES))
    print("# %d kernels compared, %d differ" % (len(set(old) | set(new)), n_diff))
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
