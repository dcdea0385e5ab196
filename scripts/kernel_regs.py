#!/usr/bin/env python3
"""Registers, scratch, occupancy and code identity of every kernel in two sets of gfx950 assembly files (profiles/bf16_planes.md).

    hipcc <the flags of csrc/build.sh> --cuda-device-only -S fgmm_tab.hip -o OLD/fgmm_tab.s      (per .hip file, old and new tree)
    python scripts/kernel_regs.py OLD NEW [--all]

For every kernel of OLD: its VGPRs, SGPRs, scratch bytes, LDS bytes and occupancy in both sets, and whether its instructions are the
SAME TEXT (labels renumbered: inserting instantiations shifts the function numbers in .LBB<n>_<m>).  A kernel with matrix instructions
gets a second verdict for the span from its first to its last v_mfma - the K loop of the parameter head (profiles/head_frame_refactor.md):
"same mfma span" says that a change around the loop left the loop's own schedule alone; "same mfma span, masked" that the spans are
equal once block labels and register numbers are masked - the same opcodes and waits in the same order, other registers
(profiles/mfma32_tile_refactor.md).  Kernels only NEW has are summarised per template.  Needs no GPU."""
import hashlib
import re
import subprocess
import sys
from pathlib import Path


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


LABEL = re.compile(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?")
MASK = re.compile(rb"\.LBB_\d+|\b[vsa](\d+|\[\d+:\d+\])")  # block labels and register numbers, for the span's third verdict
FIELDS = {"next_free_vgpr": "vgpr", "next_free_sgpr": "sgpr", "private_segment_fixed_size": "scratch", "group_segment_fixed_size": "lds"}


def kernels(d):
    """name -> dict(vgpr, sgpr, scratch, lds, occ, sha, span, masked) for every kernel of the directory's .s files (one pass over the
    lines); span: the hash of the lines from the first to the last v_mfma, None without one; masked: the same with MASK applied"""
    res, sha, span, masked, occ = {}, {}, {}, {}, {}
    for f in sorted(Path(d).glob("*.s")):
        cur = text = last = desc = pending = None
        with open(f) as fh:
            for line in fh:
                t = line.strip()
                if desc is not None:  # inside a kernel descriptor (it lies between the code and the function's end label)
                    if t.startswith(".end_amdhsa_kernel"):
                        desc = None
                    elif t.startswith(".amdhsa_"):
                        k, _, v = t[len(".amdhsa_"):].partition(" ")
                        if k in FIELDS:
                            res[desc][FIELDS[k]] = int(v)
                elif t.startswith(".amdhsa_kernel "):
                    desc = t.split()[1]
                    res[desc] = {}
                elif cur is not None:
                    if t.startswith(".Lfunc_end"):
                        mf = [i for i, ln in enumerate(text) if ln.startswith(b"v_mfma")]
                        span[cur] = hashlib.sha1(b"".join(text[mf[0]:mf[-1] + 1])).hexdigest()[:12] if mf else None
                        masked[cur] = hashlib.sha1(MASK.sub(b"#", b"".join(text[mf[0]:mf[-1] + 1]))).hexdigest()[:12] if mf else None
                        sha[cur], last, cur = hashlib.sha1(b"".join(text)).hexdigest()[:12], cur, None
                    elif t and not t.startswith((";", ".loc", ".file", ".cfi")):
                        text.append(LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), t.split(";")[0].rstrip()).encode() + b"\n")
                elif t.startswith(".type") and t.endswith(",@function"):
                    pending = t.split()[1].split(",")[0]
                elif pending and line.startswith(pending + ":"):
                    cur, text, pending = pending, [], None
                elif t.startswith("; Occupancy:") and last:
                    occ[last] = int(t.split()[-1])
                    last = None
    for name, r in res.items():
        r["sha"], r["span"], r["masked"], r["occ"] = sha.get(name, "?"), span.get(name), masked.get(name), occ.get(name)
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show_all = "--all" in sys.argv
    old, new = kernels(args[0]), kernels(args[1])
    dm = demangle(sorted(set(old) | set(new)))
    keys = ("vgpr", "sgpr", "scratch", "lds", "occ")
    differ, regs_differ, n_mfma, span_differ, masked_differ = [], 0, 0, 0, 0
    for name in sorted(old):
        if name not in new:
            differ.append((name, "missing in NEW"))
            continue
        o, n = old[name], new[name]
        same_regs = all(o.get(k) == n.get(k) for k in keys)
        if not same_regs or o["sha"] != n["sha"]:
            differ.append((name, f"old {[o.get(k) for k in keys]} {o['sha']}  new {[n.get(k) for k in keys]} {n['sha']}"))
        regs_differ += not same_regs
        if o["span"]:
            n_mfma += 1
            span_differ += o["span"] != n["span"]
            masked_differ += o["masked"] != n["masked"]
        if show_all:
            verdict = "same mfma span" if o["span"] == n["span"] else "same mfma span, masked" if o["masked"] == n["masked"] else "MFMA SPAN DIFFERS"
            print(f"{dm[name][:150]:150s} " + " ".join(f"{k}={o.get(k)}" for k in keys) + (" same text" if o["sha"] == n["sha"] else " TEXT DIFFERS")
                  + (f" {verdict}" if o["span"] else ""))
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW; of OLD's: {len(old) - len(differ)} with the same instructions, registers, scratch, LDS and occupancy; "
          f"{len(differ)} that differ, {regs_differ} of them in {list(keys)}; {n_mfma} with matrix instructions, {span_differ} whose first-to-last v_mfma span differs, "
          f"{masked_differ} of them with labels and register numbers masked too")
    for name, why in differ:
        print("  DIFFERS", dm[name], why)
    # the kernels only NEW has: each bfloat16 instantiation (DF16b in the mangled name) beside its float16 sibling (DF16_)
    fam = {}
    for name in sorted(set(new) - set(old)):
        sib = name.replace("DF16b", "DF16_")
        g = re.match(r"_ZN4fgmm\d+(\w+?_kernel)I", name)
        st = fam.setdefault(g.group(1) if g else name, dict(n=0, equal=0, diffs=[]))
        st["n"] += 1
        if sib == name or sib not in new:
            st["diffs"].append(f"{name}: no float16 sibling")
            continue
        a, b = new[name], new[sib]
        if all(a.get(k) == b.get(k) for k in keys):
            st["equal"] += 1
        else:
            st["diffs"].append(f"{name}: bf16 {[a.get(k) for k in keys]}  f16 {[b.get(k) for k in keys]}")
    for g, st in sorted(fam.items()):
        print(f"  new: {g:22s} {st['n']:3d} bfloat16 kernels, {st['equal']:3d} with their float16 sibling's [vgpr, sgpr, scratch, occ]")
        for dline in st["diffs"]:
            print("       ", dline)


if __name__ == "__main__":
    main()
