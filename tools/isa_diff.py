#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of csrc/, kernel by kernel.

    isa_diff.py OLD_CSRC_DIR NEW_CSRC_DIR [--rename OLD=NEW ...] [--arch gfx950] [--show N]

For every *.o of either directory the gfx950 code object is taken out of the fat binary (llvm-objcopy + clang-offload-bundler, the recipe of
tests/test_cabi_cpu.py), disassembled per function symbol and demangled.  A kernel is SAME when
  * its instruction list equals the old one's -- addresses, encodings and branch-target comments stripped, the alignment padding behind the last
    instruction ignored, and the literal of an `s_getpc_b64` / `s_add_u32` / `s_addc_u32` sequence (a PC-relative offset to a global, which moves
    when anything in front of it changes size) masked; and
  * its descriptor fields (.vgpr_count, .sgpr_count, .agpr_count, .group_segment_fixed_size, .private_segment_fixed_size,
    .max_flat_workgroup_size of the code object's metadata note) are equal.
--rename: a Python regular expression and its replacement, applied to the OLD build's demangled names before the two sides are matched -- for a
template argument list that shrank, e.g.  --rename 'feat_prenet_split_kernel<(\\d), (\\d), 1>=feat_prenet_split_kernel<\\1, \\2>'.
One line per kernel: SAME / DIFF / ONLY-OLD / ONLY-NEW; the exit status is 0 only when every line reads SAME.  Needs two builds, so it is a tool
and not a test."""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".max_flat_workgroup_size")


def code_object(llvm, obj, arch, tmp):
    base = os.path.basename(obj)[:-2]
    fat, co = os.path.join(tmp, base + ".bin"), os.path.join(tmp, base + ".co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None  # a host-only translation unit
    r = subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--input=" + fat,
                        "--output=" + co, "--unbundle"], capture_output=True, text=True)
    return co if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) else None


def functions(llvm, co):
    """{mangled symbol: [instruction text]} of the code object's .text"""
    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ins = " ".join(line.split("//")[0].split())
        if ins and ins != "...":
            cur.append(ins)
    for name, ins in out.items():
        while ins and ins[-1].startswith("s_nop"):
            ins.pop()
        pc = 0  # instructions left of a PC-relative address computation: s_getpc_b64, then the add of the offset's low and high half
        for i, text in enumerate(ins):
            if text.startswith("s_getpc_b64"):
                pc = 2
            elif pc and text.startswith(("s_add_u32", "s_addc_u32")):
                ins[i] = re.sub(r", (0x[0-9a-fA-F]+|-?\d+)$", ", <pcrel>", text)
                pc -= 1
            else:
                pc = 0
    return out


def descriptors(llvm, co):
    """{mangled kernel name: {field: value}} from the metadata note"""
    notes = subprocess.run([os.path.join(llvm, "llvm-readobj"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"^  ([- ]) (\.[a-z_]+):\s*(\S*)$", line)  # the keys of an entry of amdhsa.kernels (its argument list is indented further)
        if not m:
            continue
        if m.group(1) == "-":  # first key of the next entry
            cur = {}
        if m.group(2) == ".name":
            out[m.group(3)] = cur
        elif m.group(2) in FIELDS:
            cur[m.group(2)] = m.group(3)
    return out


def demangle(names):
    names = list(names)
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def build_table(llvm, csrc, arch, tmp):
    """{(translation unit, demangled name): (instructions, descriptor fields or None)}"""
    table = {}
    for obj in sorted(glob.glob(os.path.join(csrc, "*.o"))):
        sub = os.path.join(tmp, "x")
        os.makedirs(sub, exist_ok=True)
        co = code_object(llvm, obj, arch, sub)
        if co is None:
            continue
        fn, kd = functions(llvm, co), descriptors(llvm, co)
        pretty = demangle(fn)
        for sym, ins in fn.items():
            table[(os.path.basename(obj)[:-2], pretty[sym])] = (ins, kd.get(sym))
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--llvm", default="/opt/rocm/lib/llvm/bin")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N lines of a DIFF kernel's instruction diff")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old, new = build_table(a.llvm, a.old, a.arch, t_old), build_table(a.llvm, a.new, a.arch, t_new)
    renamed = {}
    for (tu, name), v in old.items():
        for pat, rep in renames:
            name = re.sub(pat, rep, name)
        if (tu, name) in renamed:
            sys.exit("isa_diff: the renames map two old kernels of %s onto %s" % (tu, name))
        renamed[(tu, name)] = v
    counts = {"SAME": 0, "DIFF": 0, "ONLY-OLD": 0, "ONLY-NEW": 0}
    for key in sorted(set(renamed) | set(new)):
        why = ""
        if key not in new:
            verdict = "ONLY-OLD"
        elif key not in renamed:
            verdict = "ONLY-NEW"
        else:
            (oi, od), (ni, nd) = renamed[key], new[key]
            parts = []
            if oi != ni:
                parts.append("code (%d -> %d instructions)" % (len(oi), len(ni)))
            if od != nd:
                parts.append("descriptor " + " ".join("%s %s -> %s" % (f, (od or {}).get(f), (nd or {}).get(f)) for f in FIELDS
                                                       if (od or {}).get(f) != (nd or {}).get(f)))
            verdict, why = ("DIFF", "  " + "; ".join(parts)) if parts else ("SAME", "")
            if oi != ni and a.show:
                why += "\n" + "\n".join(list(difflib.unified_diff(oi, ni, "old", "new", lineterm="", n=2))[:a.show])
        counts[verdict] += 1
        print("%-8s %s: %s%s" % (verdict, key[0], key[1], why))
    kernels = sum(1 for v in new.values() if v[1] is not None)
    print("%d symbols (%d kernels with a descriptor): %s" % (len(set(renamed) | set(new)), kernels, ", ".join("%d %s" % (n, k) for k, n in counts.items())))
    return 0 if counts["SAME"] == sum(counts.values()) and counts["SAME"] else 1


if __name__ == "__main__":
    sys.exit(main())
