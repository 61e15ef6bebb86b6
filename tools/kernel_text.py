#!/usr/bin/env python3
"""kernel_text.py -- did a change move an instruction?  Compares the gfx950 assembly of every kernel of two builds, no GPU needed.

    python tools/kernel_text.py dump DIR          # csrc/*.hip and pjd_plan.cpp of THIS tree -> DIR/<unit>.s (hipcc -S, the product's flags)
    python tools/kernel_text.py compare OLD NEW   # two such directories, e.g. of a `git worktree` of the parent and of this tree

Kernels are matched by SYMBOL, whichever unit holds them, so a kernel that moved to another file still meets its old self.  A kernel's
text runs from its label to .Lfunc_end, descriptor (.amdhsa_kernel: registers, LDS, scratch) included; comments are stripped, and the
function's index within its unit (.LBB<n>_, .Lfunc_end<n>) is dropped, since it changes with the kernel's position and nothing else.
For a kernel that differs the figures a reviewer asks for are printed for both sides: VGPRs, SGPRs, occupancy, scratch, vector loads,
vector stores, LDS instructions, all instructions, LDS bytes -- and whether registers, occupancy, scratch, LDS bytes and the multiset of
instruction mnemonics are equal: a kernel that --may-differ names may differ in its text alone, not in any of these.  Units that hold
no kernel named by --moved (default: the resize kernels) must be equal as whole files but for their __hip_cuid lines.  Exit status 1
where such a unit differs, or a kernel that --may-differ does not name, or one that it names and that lost one of those equalities.
"""
import argparse
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pim-jpeg-decoder_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]
# what a kernel that --may-differ names must keep: its registers, occupancy, scratch, LDS bytes and the multiset of its mnemonics
SAME_FIGURES = ("NumVgprs", "TotalNumSgprs", "Occupancy", "ScratchSize", "lds_bytes", "mnemonics")


def dump(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    units = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip") or f == "pjd_plan.cpp")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    procs = [(u, subprocess.Popen([hipcc] + FLAGS + ["-x", "hip", "-o", os.path.join(out_dir, os.path.splitext(u)[0] + ".s"), os.path.join(CSRC, u)],
                                  stderr=subprocess.PIPE, text=True)) for u in units]
    for u, p in procs:
        err = p.communicate()[1]
        if p.returncode:
            sys.exit(f"{u}: {err}")
    print(f"{len(units)} units -> {out_dir}")


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)


def kernels(path):
    """{symbol: (text lines, figures)} of one .s file, and the file's lines without __hip_cuid."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\t\.amdhsa_kernel (\S+)", l)] if m]
    out = {}
    for name in names:
        start = lines.index(next(l for l in lines if l.startswith(name + ":")))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        text = [c for c in map(clean, lines[start:end + 1]) if c]
        code = [c.split()[0] for c in text[1:text.index("\t.section\t.rodata,\"a\",@progbits")] if c.startswith("\t") and not c.startswith("\t.")]
        fig = {"insts": len(code),
               "vload": sum(c.startswith(("global_load", "buffer_load", "flat_load")) for c in code),
               "vstore": sum(c.startswith(("global_store", "buffer_store", "flat_store")) for c in code),
               "lds": sum(c.startswith("ds_") for c in code),
               "mnemonics": collections.Counter(code),
               "lds_bytes": next(int(c.split()[1]) for c in text if c.lstrip().startswith(".amdhsa_group_segment_fixed_size"))}
        for l in lines[end:end + 60]:
            m = re.match(r"; (NumVgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", l)
            if m and m.group(1) not in fig:
                fig[m.group(1)] = int(m.group(2))
        out[name] = (text, fig)
    return out, [l for l in lines if "__hip_cuid" not in l]


def load(d):
    ks, units = {}, {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".s"):
            k, rest = kernels(os.path.join(d, f))
            units[f] = (set(k), rest)
            ks.update(k)
    return ks, units


def compare(old_dir, new_dir, moved, may_differ):
    old, old_units = load(old_dir)
    new, new_units = load(new_dir)
    bad = 0
    for sym in sorted(set(old) | set(new)):
        short = subprocess.run(["c++filt", "-p", sym], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "") or sym
        if sym not in old or sym not in new:
            print(f"ONLY IN {'OLD' if sym in old else 'NEW'}  {short}")
            bad += 1
        elif old[sym][0] == new[sym][0]:
            print(f"identical    {short}")
        else:
            print(f"DIFFERENT    {short}")
            for side, k in (("old", old[sym]), ("new", new[sym])):
                f = k[1]
                print(f"    {side}: vgpr {f['NumVgprs']} sgpr {f['TotalNumSgprs']} occupancy {f['Occupancy']} scratch {f['ScratchSize']} "
                      f"vload {f['vload']} vstore {f['vstore']} lds {f['lds']} insts {f['insts']} lds bytes {f['lds_bytes']}")
            same = {k: old[sym][1][k] == new[sym][1][k] for k in SAME_FIGURES}
            print("    " + ", ".join(f"{k} {'equal' if v else 'NOT EQUAL'}" for k, v in same.items()))
            bad += not (may_differ and re.search(may_differ, sym) and all(same.values()))
    for f in sorted(set(old_units) | set(new_units)):
        a, b = old_units.get(f), new_units.get(f)
        if any(re.search(moved, s) for u in (a, b) if u for s in u[0]):
            continue                                   # holds moved kernels: compared per kernel above
        if a is None or b is None or a[1] != b[1]:
            print(f"UNIT DIFFERS beyond __hip_cuid: {f}")
            bad += 1
        else:
            print(f"unit equal but for __hip_cuid: {f}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("dump").add_argument("dir")
    c = sub.add_parser("compare")
    c.add_argument("old")
    c.add_argument("new")
    c.add_argument("--moved", default="pjd_k_resize", help="regex: kernels that changed units; the units that hold them are not compared whole")
    c.add_argument("--may-differ", default="", help="regex: kernels whose text may differ where registers, occupancy, scratch, LDS bytes and mnemonics are equal")
    a = ap.parse_args()
    sys.exit(dump(a.dir) if a.cmd == "dump" else compare(a.old, a.new, a.moved, a.may_differ))
