#!/usr/bin/env python3
"""Compare the device code of every kernel two source trees have in common, instruction by instruction.

    python tools/isa_compare.py OLD_TREE NEW_TREE [FILE ...]     (e.g. OLD_TREE = a `git worktree` of the parent commit;
                                                                  FILE: some of FILES below, default all)

Each tree's kernel sources are compiled with hipcc -S under the flags of mixdq_amd/build.py.  A kernel of the old tree
is matched to the new kernel of the same name, or to the one whose template argument list gained a trailing default
(`, false` / `, 0`: how MIXDQ_FLAG_A4 entered quantize_one / quantize_pack8 and the kernels around them).  Bodies are
compared with the symbol's own name, basic-block numbers and assembler comments normalised away, and so is each
kernel's .amdhsa_kernel descriptor block (registers, LDS, scratch, ...).  Prints a line per source file and every
kernel whose code or descriptor differs; exit status 0 = every old kernel is unchanged AND each file has as many
kernels as before (a refactor of the launch code must not add or drop an instantiation).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["quantize", "fused_norm", "attention", "igemm", "igemm_aq", "igemm_ln", "iconv", "sampler", "vae", "image",
         "sampler_rescale", "control"]             # (every unit of build.py, whichever object directory it goes to)


def assemble(tree, out, files):
    sys.path.insert(0, ROOT)
    from mixdq_amd import build as B
    procs = []
    for f in files:
        src = os.path.join(tree, "mixdq_amd", "csrc", f + ".hip")
        cmd = [B._hipcc()] + B.FLAGS + B.EXTRA.get(f + ".hip", []) + ["--cuda-device-only", "-S", "-o",
                                                                        os.path.join(out, f + ".s"), src]
        procs.append(subprocess.Popen(cmd, stderr=subprocess.DEVNULL))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit(f"hipcc failed in {tree}")


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S):
        name, body = m.group(1), m.group(2).replace(m.group(1), "SELF")
        lines = (l.split(";")[0].strip() for l in body.split("\n"))
        out[name] = "\n".join(re.sub(r"\.?L?BB\d+_\d+", "BB", l) for l in lines
                              if l and not l.startswith((".Ltmp", ".loc", ".cfi")))
    # the kernel descriptors: every .amdhsa_ directive of the kernel, joined to its code (where the assembler
    # writes the block behind the function's end label; in front of it, the block is part of the body already)
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", txt, re.M | re.S):
        if m.group(1) in out and ".amdhsa_kernel " not in out[m.group(1)]:
            desc = [" ".join(l.split(";")[0].split()) for l in m.group(2).split("\n")]
            out[m.group(1)] += "\n" + "\n".join(l for l in desc if l)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def main():
    old_tree, new_tree, files = sys.argv[1], sys.argv[2], sys.argv[3:] or FILES
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "old")), os.makedirs(os.path.join(d, "new"))
        assemble(old_tree, os.path.join(d, "old"), files)
        assemble(new_tree, os.path.join(d, "new"), files)
        for f in files:
            a, b = kernels(os.path.join(d, "old", f + ".s")), kernels(os.path.join(d, "new", f + ".s"))
            bd = dict(zip(demangle(list(b)), b))
            same = diff = 0
            for dn, mn in zip(demangle(list(a)), a):
                i = dn.rfind(">(")
                cands = [bd.get(dn)] + ([bd.get(dn[:i] + x + dn[i:]) for x in (", false", ", 0")] if i > 0 else [])
                mn2 = next((c for c in cands if c), None)
                if mn2 is not None and a[mn] == b[mn2]:
                    same += 1
                else:
                    diff += 1
                    print("  changed or missing:", dn[:200])
            print(f"{f}: {len(a)} kernels before, {len(b)} after; {same} unchanged, {diff} changed or missing")
            if len(a) != len(b):
                print(f"  kernel count changed: {len(a)} -> {len(b)}")
            bad += diff + (len(a) != len(b))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
