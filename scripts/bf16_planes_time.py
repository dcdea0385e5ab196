#!/usr/bin/env python3
"""bf16_planes_time.py - the kernels that read parameter planes on bfloat16, float16 and float32 planes in the same run
(profiles/bf16_planes.md).  Two workloads of bench.py's synthetic generator (tests/synth.make_latent, not real images' latents):

  elic    one 4K ELIC image: the channel groups 16 / 16 / 32 / 64 / 192 x two halves, hw = 136 x 120 (ten items, 5.2 M latents)
  kodak   twelve Kodak images: 24 halves of [1, 192, 32, 24] (3.5 M latents)

and six calls, one per kernel family: compress_batch (symtab_kernel), estimate_bits_batch (rate_kernel), quantize_rdo_batch
(rdoq_kernel), rd_curve_batch at 16 lambdas (rdcurve_kernel), decompress_batch (tab_kernel) and decompress_batch of checkpointed
streams with gpu_decode = 1 (segdec_kernel).  Every repetition runs the three plane types one after the other, so that a drift of the
clock or a neighbour on the host meets all three alike.

  python scripts/bf16_planes_time.py --reps 20                      call times: device events around each call (the compress and
                                                                    decompress calls include the host coder: read the KERNEL rows)
  rocprofv3 --kernel-trace --stats --mangled-kernels --output-format csv -d DIR -- python scripts/bf16_planes_time.py --reps 20
  python scripts/bf16_planes_time.py --summarise DIR [DIR ...]      kernel times per family and plane type from the traces' statistics

FGMM_LIB=<another build's libflashgmm_amd.so> runs a build of the parent commit (no bfloat16 there: --types f32,f16).  Prints JSON."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = ("symtab_kernel", "rate_kernel", "rdoq_kernel", "rdcurve_kernel", "tab_kernel", "segdec_kernel", "cdftab_count_kernel", "cdftab_fill_kernel")
LAMBDAS16 = [0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 16.0]


PT = re.compile(r"(?<=E)(DF16b|DF16_|f)(?=Lb[01]E|E)")  # the plane type among a mangled name's template arguments


def summarise(dirs):
    """per instantiation that ran (mangled names: run rocprofv3 with --mangled-kernels; the demangler of some toolchains garbles the
    bfloat16 forms), the plane type replaced by PT: launches and mean / min / max duration in microseconds for each plane type"""
    acc = {}
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                name = r["Name"]
                fam = next((k for k in FAMILIES if f"{len(k)}{k}I" in name), None)
                m = PT.search(name) if fam else None
                if m is None:
                    continue
                args = name[name.index(fam) + len(fam):].split("EEv")[0]
                key = f"{fam}<{PT.sub('PT', args + 'E')[1:-1]}>"
                pt = {"DF16b": "bf16", "DF16_": "f16", "f": "f32"}[m.group(1)]
                a = acc.setdefault(key, {}).setdefault(pt, {"launches": 0, "total_ns": 0.0, "min_us": float("inf"), "max_us": 0.0})
                a["launches"] += int(r["Calls"])
                a["total_ns"] += float(r["TotalDurationNs"])
                a["min_us"], a["max_us"] = min(a["min_us"], float(r["MinNs"]) / 1e3), max(a["max_us"], float(r["MaxNs"]) / 1e3)
    out = {}
    for key, pts in sorted(acc.items()):
        out[key] = {pt: {"launches": a["launches"], "mean_us": round(a["total_ns"] / a["launches"] / 1e3, 2), "min_us": round(a["min_us"], 2),
                         "max_us": round(a["max_us"], 2)} for pt, a in sorted(pts.items())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--types", default="f32,f16,bf16")
    ap.add_argument("--workloads", default="elic,kodak")
    ap.add_argument("--summarise", nargs="+")
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise), indent=1))
        return
    import numpy as np
    import torch

    from flashgmm_amd import GaussianMixtureConditional, _lib
    from tests import bf16_planes as B
    from tests import synth as T

    dev = torch.device("cuda:0")
    types = a.types.split(",")

    def planes(sg, mu, pi, pt):
        if pt == "f32":
            return [torch.from_numpy(x).to(dev) for x in (sg, mu, pi)]
        if pt == "f16":
            return [torch.from_numpy(x).to(dev) for x in T.to_float16_planes(sg, mu, pi)]
        return [torch.from_numpy(b.view(np.int16)).to(dev).view(torch.bfloat16) for b in B.planes_bits(sg, mu, pi, False)]

    def workload(name):
        shapes = [(g, 136, 120) for g in (16, 16, 32, 64, 192) for _ in range(2)] if name == "elic" else [(192, 32, 24)] * 24
        ys, prm = [], {pt: ([], [], []) for pt in types}
        for k, (M, h, w) in enumerate(shapes):
            y, sg, mu, pi = T.make_latent(k, M=M, h=h, w=w)
            ys.append(torch.from_numpy(y).to(dev))
            for pt in types:
                for col, t in zip(prm[pt], planes(sg, mu, pi, pt)):
                    col.append(t)
        return ys, prm

    plain = GaussianMixtureConditional(K=4, mode="polya")
    ck = GaussianMixtureConditional(K=4, mode="polya", checkpoint_stride=4096)
    out = {"lib": _lib.LIB_PATH if os.environ.get("FGMM_LIB") else "in-tree", "reps": a.reps, "types": types}
    for wl in a.workloads.split(","):
        ys, prm = workload(wl)
        enc = {pt: plain.compress_batch(ys, *prm[pt]) for pt in types}
        enc_ck = {pt: ck.compress_batch(ys, *prm[pt]) for pt in types}

        def dec(gmc, e, pt):
            return gmc.decompress_batch([r[0][0] for r in e[pt]], [r[0][1] for r in e[pt]], [r[0][2] for r in e[pt]], *prm[pt])

        calls = {
            "compress (symtab_kernel)": lambda pt: plain.compress_batch(ys, *prm[pt]),
            "estimate (rate_kernel)": lambda pt: plain.estimate_bits_batch(ys, *prm[pt]),
            "rdoq (rdoq_kernel)": lambda pt: plain.quantize_rdo_batch(ys, *prm[pt], 0.1),
            "curve (rdcurve_kernel)": lambda pt: plain.rd_curve_batch(ys, *prm[pt], LAMBDAS16),
            "decompress (tab_kernel)": lambda pt: dec(plain, enc, pt),
            "decompress checkpointed, gpu_decode=1 (segdec_kernel)": lambda pt: dec(ck, enc_ck, pt),
        }
        res = {"latents": int(sum(y.numel() for y in ys)), "items": len(ys)}
        for what, fn in calls.items():
            _lib.set_option(0, "gpu_decode", 1 if "segdec" in what else 0)
            ms = {pt: [] for pt in types}
            for rep in range(a.warmup + a.reps):
                for pt in types:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(pt)
                    e1.record()
                    e1.synchronize()
                    if rep >= a.warmup:
                        ms[pt].append(e0.elapsed_time(e1))
            res[what] = {pt: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for pt, v in ms.items()}
        _lib.set_option(0, "gpu_decode", 0)
        out[wl] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
