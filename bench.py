#!/usr/bin/env python3
"""bench.py — the path's headline metric on MI355X (BASELINE.json: encode+decode Mpixels/s, Kodak, K=4 N=192).

    python bench.py --gpus N --steps K --warmup W          (N > 1: this process starts the N ranks itself)

Workload (config.workload = "kodak24"): BASELINE.json configs[1] — 24 Kodak-sized images (768x512 ->
y [1,192,32,48] -> two checkerboard halves [1,192,32,24] each), mixture parameters [1,768,32,24] x3 per half,
synthetic and seeded (no Kodak files / checkpoint exist offline), resident in HBM before the
timed region.  One STEP = one pass of the hot path over that batch, scheduled AS THE CODEC CAN schedule it:
    encode  GaussianMixtureConditional.compress of all 48 halves in ONE native call — the encoder holds round(y) of the
            anchors, which is all the non-anchor parameters depend on (checkerboard.py:282-288)
    decode  GaussianMixtureConditional.decompress in TWO calls, the 24 anchor halves, then the 24 non-anchor halves: the
            non-anchor parameters need the decoded anchors (checkerboard.py:316-324)
(--workload elic4k: 5 channel groups x 2 halves; encode one call — every group's context is round(.) of data the
encoder holds — decode ten sequential calls, channel_groups.py:147-154.)  The all-at-once schedule of round 1 (every
stream of the batch in one decode call) is timed beside it and reported as `upper_bound`.
value = pixels of all images of all ranks / wall time (Mpixels/s).  N > 1: one process per GPU, each rank codes its own
24 images (weak scaling); the only exchange is one RCCL all-gather of the per-stream byte lengths per step.

A plain run sets up, warms up, times the --steps steps, checks the last step's result (decode == round(y)), writes that step's
outputs with --dump-outputs DIR, and prints one JSON line from rank 0: the driver's contract (`ms_per_step` = milliseconds of
one timed step) and two figures taken from the timed steps themselves:
  roofline         the symtab (encode-side GMM-CDF) kernel: algorithmic bytes (56 B/coded symbol) over its
                   launch duration measured here with HIP events on the stream it runs on, against 8 TB/s HBM
  roofline_decode  the decode-side table kernel against both of its rooflines (VALU issue, HBM), edges per latent
  ranks            per-rank step times and the all-gather's share (N > 1)
Everything else is measured with --full only (implied by --diag and --baseline-extras), which also writes the whole result to
bench_detail.json and stderr:
  cpu_baseline     the REAL reference extension (oracle/_ref, built from /root/reference in the build container; kind
                   "reference"), or this repo's C restatement (kind "port"), timed on this box's host cores on the same
                   images: one core (`value`), and every core this process may use, one stream per process (`all_cores`)
  latency_ms       one image (two bitstreams), encode + decode, as the codec schedules it and all at once
  upper_bound      the step with every stream in one decode call
  reference_md5    the first four bitstreams against the reference's md5s (tests/golden/ka1.json)
  modes            BASELINE configs[2] in the same run (N = 1): the A&S and logistic approximations on the same batch, a few steps each,
                   the first four bitstreams checked against the reference's md5s (tests/golden/ka1.json: fixtures made from the
                   compiled reference)
  elic4k           BASELINE configs[4] in the same run (N = 1): sixteen 4K images in flight, fp16 parameter planes, a few steps
  checkpointed     the step on checkpointed bitstreams (segments decoded on the GPU), every rank, max over ranks
  head_fused       the parameter head's last layer fused with the encode-side CDF kernel (N = 1)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from scripts import bench_diag as D  # noqa: E402  (host-side forensics: off the default run's path except two counter reads)
from scripts.bench_diag import _plain_children  # noqa: E402  (helper processes start without a profiler's preload)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
HBM_COPY_GBS = 6290.0  # ... what a float4 copy kernel reaches on the chip (same guide): reported beside the spec fraction, never instead of it
# VALU issue peak of the chip as scripts/valu_peak.hip measures it (profiles/r02_valu_peak.txt): a wave64 fp32 instruction
# issues once per 4 cycles per SIMD: 256 CUs x 4 SIMDs x 64 lanes / 4 cycles x 2.4 GHz
VALU_PEAK_LANE_SLOTS = 256 * 4 * 64 / 4 * 2.4e9
# issue slots of the table kernel's evaluation loop per edge (ISA of tab_kernel<mode, clamped, f32>, the loop body of
# phase 2 handles one PAIR of edges: plain VALU instructions count 1, packed ones 1.16, rsq / rcp 2)
TAB_SLOTS_PER_EDGE = {"polya": (134 + 107 * 1.16 + 4) / 2, "as": (150 + 140 * 1.16 + 4) / 2, "logistic": (230 + 110 * 1.16 + 4) / 2}

ELIC_GROUPS = (16, 16, 32, 64, 192)  # elic_gmm.py:92-96
ELIC_IMAGES = 16  # 4K images in flight per GPU (4.6 GB resident with fp16 parameter planes)
ELIC_DISTINCT = 4  # ... of the default line's ELIC sub-leg: four generated from their seeds, each resident four times (seven seconds of numpy per image)


def workload_shapes(workload: str):
    """-> (stream shapes of one image in coding order, pixels per image)"""
    if workload == "kodak24":
        return [(192, 32, 24)] * 2, 768 * 512
    return [(g, 136, 120) for g in ELIC_GROUPS for _ in range(2)], 3840 * 2160


def stream_seed(rank: int, image: int, stream: int, streams_per_image: int) -> int:
    return 1000 * rank + image * streams_per_image + stream


def _make_stream(args):
    seed, M, h, w, f16 = args
    from tests import synth as T

    y, sg, mu, pi = T.make_latent(seed, M=M, h=h, w=w)  # sigma pre-clamped as KA-1
    if f16:
        sg, mu, pi = T.to_float16_planes(sg, mu, pi)
    return y, sg, mu, pi


def make_workload(rank: int, images: int, dev, workload: str = "kodak24", f16: bool = False, keep_host_images: int = 1 << 30, distinct=None):
    """-> (host arrays per stream, device tensors per stream, pixels per image).
    kodak24: 2 streams per image, [1,192,32,24]; elic4k: 10 streams per image (5 channel groups x 2 halves of a
    3840x2160 image padded to 2176 rows -> y [1,320,136,240], SURVEY.md §8 sizes).  Large workloads (ELIC: seven seconds of
    numpy per image) are generated by a pool of processes, stream by stream from their seeds - the same arrays either way.
    `distinct` < images: only the first `distinct` images are generated; image i >= distinct is a device-side COPY (its own HBM) of
    image i mod distinct - the same work per image for every kernel, copy and host decoder, a quarter of the numpy (the ELIC sub-leg)."""
    host, devt = [], []
    shapes, pix = workload_shapes(workload)
    n_gen = images if not distinct else min(images, distinct)
    jobs = [(stream_seed(rank, i, j, len(shapes)), M, h, w, f16) for i in range(n_gen) for j, (M, h, w) in enumerate(shapes)]
    n_elem = sum(M * h * w for _, M, h, w, _ in jobs)
    procs = min(len(os.sched_getaffinity(0)), 8, len(jobs)) if n_elem > 8_000_000 else 1
    if procs > 1:
        import multiprocessing as mp

        with _plain_children():
            pool = mp.get_context("spawn").Pool(procs)
        with pool:
            it = pool.imap(_make_stream, jobs, chunksize=1)
            for k in range(len(jobs)):
                st = it.next(timeout=300)  # (a helper that never answers must not hang the run: TimeoutError ends this leg)
                host.append(st if k < keep_host_images * len(shapes) else None)  # (host copies feed the CPU baseline only)
                devt.append([torch.from_numpy(a).to(dev) for a in st])
    else:
        for k, jb in enumerate(jobs):
            st = _make_stream(jb)
            host.append(st if k < keep_host_images * len(shapes) else None)
            devt.append([torch.from_numpy(a).to(dev) for a in st])
    for i in range(n_gen, images):
        for j in range(len(shapes)):
            host.append(None)
            devt.append([t.clone() for t in devt[(i % n_gen) * len(shapes) + j]])
    return host, devt, pix


def load_latents_dir(path: str, dev, f16: bool, images=None):
    """--latents-dir: REAL latents instead of the synthetic ones - what it takes to repeat the reference's own measurement
    (eval_ckbd.py:113-143: real images through a trained checkpoint) when someone supplies both: every `*.pt` file of the directory
    is one image, a list of its bitstreams in coding order, each a dict {"y": [1, M, h, w], "scales" / "means" / "weights":
    [1, 4 M, h, w]} (float tensors as the latent codec hands them to GaussianMixtureConditional.compress,
    latent_codecs/gaussian_mixture_conditional.py:134; INTEGRATION.md shows the three lines that save them), optionally
    {"pixels": H * W} as a last element.  -> (host arrays per stream, device tensors per stream, pixels per image, streams per image)"""
    files = sorted(f for f in os.listdir(path) if f.endswith(".pt"))
    if images:
        files = files[:images]
    if not files:
        raise SystemExit(f"--latents-dir {path}: no *.pt files")
    host, devt, pix, spi = [], [], None, None
    for f in files:
        img = torch.load(os.path.join(path, f), map_location="cpu")
        streams = [e for e in img if isinstance(e, dict) and "y" in e]
        meta = [e for e in img if isinstance(e, dict) and "pixels" in e]
        if spi is None:
            spi = len(streams)
        if len(streams) != spi:
            raise SystemExit(f"{f}: {len(streams)} bitstreams, the first image had {spi}")
        if meta:
            pix = int(meta[0]["pixels"])
        for e in streams:
            y = e["y"].float().contiguous()
            prm = [e[k].to(torch.float16 if f16 else torch.float32).contiguous() for k in ("scales", "means", "weights")]
            if y.dim() != 4 or y.shape[0] != 1 or any(p.shape != (1, 4 * y.shape[1], y.shape[2], y.shape[3]) for p in prm):
                raise SystemExit(f"{f}: expected y [1, M, h, w] and parameters [1, 4 M, h, w]")
            host.append((y.numpy(), *(p.numpy() for p in prm)))
            devt.append([y.to(dev), *(p.to(dev) for p in prm)])
    return host, devt, pix, spi


# ---------------------------------------------------------------------------------------------------------------------
# CPU baseline: the reference's own coder (or the C restatement) on host cores of this box — test infrastructure, used
# here only as the reported baseline
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_coder():
    """-> (kind, prepare(host stream) -> state, code(state) -> (decoded symbols, expected symbols, the encoder's bytes))"""
    from tests import synth as T
    from oracle import oracle as O

    kind = "port"
    ans = None
    if O.ref_available():
        try:
            os.environ.pop("APPROX_MODE", None)
            ans = O.ref_ans()
            kind = "reference"
        except Exception as e:  # pragma: no cover - e.g. ISA mismatch on an unexpected host
            print(f"[bench] reference extension unusable here ({e}); falling back to the C restatement", file=sys.stderr)

    def prepare(stream):
        y, sg, mu, pi = stream
        sym, s, m, w, abs_max, zb, yq = T.to_coder_inputs(y, *(a.astype(np.float32) for a in (sg, mu, pi)))
        if kind == "reference":  # the reference is handed (n,4) views with strides (1,n) (entropy_models.py:810-828)
            return (torch.from_numpy(sym), *(torch.from_numpy(np.ascontiguousarray(a.T)).T for a in (s, m, w)), abs_max, sym)
        return (sym, s, m, w, abs_max, sym)

    def code(st):
        sym, s, m, w, am, want = st
        if kind == "reference":
            b = ans.RansEncoder().encode_with_indexes_gmm(sym, s, m, w, am + 1)
            return ans.RansDecoder().decode_with_indexes_gmm(b, s, m, w, am + 1).numpy(), want, b
        b = O.encode_gmm(0, sym, s, m, w)
        return O.decode_gmm(0, b, s, m, w, am + 1), want, b

    return kind, prepare, code


def _all_cores_worker(args):
    """one process of the all-cores baseline: its share of the streams, regenerated from their seeds; passes until the
    budget is spent -> (streams coded, wall clock start, wall clock end)"""
    seeds, shapes, f16, budget_s = args
    from tests import synth as T

    torch.set_num_threads(1)
    kind, prepare, code = _cpu_coder()
    states = []
    for seed, (M, h, w) in zip(seeds, shapes):
        y, sg, mu, pi = T.make_latent(seed, M=M, h=h, w=w)
        if f16:
            sg, mu, pi = T.to_float16_planes(sg, mu, pi)
        states.append(prepare((y, sg, mu, pi)))
    code(states[0])  # warm-up
    done = 0
    t0 = time.time()
    while done == 0 or time.time() - t0 < budget_s:
        for st in states:
            code(st)
            done += 1
    return done, t0, time.time()


def _scalar_worker(args):
    """the reference's USE_SIMD=0 path (rans_interface.cpp:119-130 latches the switch once per process: its own process).
    -> (kind, symbols coded per pass, best seconds per pass, passes)"""
    seeds, shapes, f16, budget_s = args
    os.environ["USE_SIMD"] = "0"
    from tests import synth as T

    torch.set_num_threads(1)
    kind, prepare, code = _cpu_coder()
    states = []
    for seed, (M, h, w) in zip(seeds, shapes):
        y, sg, mu, pi = T.make_latent(seed, M=M, h=h, w=w)
        if f16:
            sg, mu, pi = T.to_float16_planes(sg, mu, pi)
        states.append(prepare((y, sg, mu, pi)))
    best, passes, t_start = None, 0, time.perf_counter()
    while passes < 3 and (passes < 1 or time.perf_counter() - t_start < budget_s):
        t0 = time.perf_counter()
        for st in states:
            got, want, _ = code(st)
            assert np.array_equal(got, want)  # the scalar path round-trips its own streams (they are not the SIMD path's)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        passes += 1
    return kind, sum(len(st[-1]) for st in states), best, passes


def _mode_md5_worker(args):
    """the reference's ENCODER under another approximation mode (APPROX_MODE is latched once per process,
    rans_interface.cpp:99-115: its own process) on streams regenerated from their seeds -> (kind, [md5 of each bitstream])"""
    mode_id, seeds, shapes, f16 = args
    os.environ["APPROX_MODE"] = str(mode_id)
    import hashlib

    from tests import synth as T
    from oracle import oracle as O

    torch.set_num_threads(1)
    ans = O.ref_ans() if O.ref_available() else None
    out = []
    for seed, (M, h, w) in zip(seeds, shapes):
        y, sg, mu, pi = T.make_latent(seed, M=M, h=h, w=w)
        if f16:
            sg, mu, pi = T.to_float16_planes(sg, mu, pi)
        sym, s, m, wt, am, zb, yq = T.to_coder_inputs(y, *(a.astype(np.float32) for a in (sg, mu, pi)))
        if ans is not None:
            b = ans.RansEncoder().encode_with_indexes_gmm(torch.from_numpy(sym), *(torch.from_numpy(np.ascontiguousarray(a.T)).T for a in (s, m, wt)), am + 1)
        else:
            b = O.encode_gmm(mode_id, sym, s, m, wt)
        out.append(hashlib.md5(b).hexdigest())
    return ("reference" if ans is not None else "port"), out


def reference_bytes_of_modes(modes: dict, rank: int, shapes, streams_per_image: int, f16: bool):
    """{mode name: [bytes of every bitstream of the HIP path]} -> {mode name: reference_bytes_equal}: the reference's encoder run on
    the same streams in one helper process per mode (in parallel), md5 against md5"""
    import hashlib
    import multiprocessing as mp

    from flashgmm_amd import _lib

    names = list(modes)
    n = len(modes[names[0]])
    seeds = [stream_seed(rank, k // streams_per_image, k % streams_per_image, streams_per_image) for k in range(n)]
    shp = [shapes[k % streams_per_image] for k in range(n)]
    with _plain_children():
        pool = mp.get_context("spawn").Pool(len(names))
    with pool:
        res = pool.map(_mode_md5_worker, [(_lib.mode_id(nm), seeds, shp, f16) for nm in names])
    out = {}
    for nm, (kind, md5s) in zip(names, res):
        eq = sum(hashlib.md5(bytes(b)).hexdigest() == h for b, h in zip(modes[nm], md5s))
        out[nm] = {"streams": n, "equal": eq, "kind": kind}
    return out


def cpu_baseline(host, shapes, pix_per_image: int, streams_per_image: int, rank: int, f16: bool, budget_s: float = 3.5, hip_bytes=None,
                 from_seeds: bool = True, extras: bool = False):
    """Time the reference's own coder on this box: ONE core on the same images (bounded sample), then every core this
    process may use, one stream at a time per process (the reference is single-threaded and holds the GIL), then its
    USE_SIMD=0 path on a smaller sample (those two and the C restatement's own time only with `extras`: --baseline-extras).  `hip_bytes`: the HIP path's bitstreams of the same streams - the reference encoder's
    bytes are compared with them, stream by stream (`reference_bytes_equal`: checker use of the baseline)."""
    kind, prepare, code = _cpu_coder()
    host = host[: next((k for k, st in enumerate(host) if st is None), len(host))]  # (legs that kept the first image(s) only)
    # a bounded sample of the same workload: whole images, up to about 8 M latents (all 24 Kodak images; one 4K image)
    n_sample, n_sym_acc = 0, 0
    while n_sample < len(host) // streams_per_image and (n_sample == 0 or n_sym_acc < 7_000_000):
        n_sym_acc += sum(int(np.prod(st[0].shape)) for st in host[n_sample * streams_per_image:(n_sample + 1) * streams_per_image])
        n_sample += 1
    host = host[: n_sample * streams_per_image]
    prepared = [prepare(s) for s in host]
    torch.set_num_threads(1)
    best = None
    passes = 0
    t_start = time.perf_counter()
    ref_bytes = []
    while passes < 5 and (passes < 2 or time.perf_counter() - t_start < budget_s):  # (whole passes: 1.0 s each on kodak24)
        t0 = time.perf_counter()
        for st in prepared:
            got, want, b = code(st)
            if passes == 0:
                ref_bytes.append(b)
        dt = time.perf_counter() - t0
        assert np.array_equal(got, want)
        best = dt if best is None else min(best, dt)
        passes += 1
    n_img = len(prepared) // streams_per_image
    n_sym = sum(len(p[-1]) for p in prepared)
    out = {
        "value": round(n_img * pix_per_image / best / 1e6, 3),
        "unit": "Mpixels/s",
        "cores": 1,
        "kind": kind,
        "sample": f"{n_img} image(s) x {streams_per_image} streams ({n_sym} symbols), encode+decode, best of {passes} passes, "
                  f"{best * 1e3:.0f} ms/pass = {best / n_sym * 1e9:.0f} ns/symbol",
        "ms_per_image": round(best / n_img * 1e3, 2),
    }
    if hip_bytes is not None:
        eq = sum(bytes(h) == bytes(r) for h, r in zip(hip_bytes, ref_bytes))
        out["reference_bytes_equal"] = {"streams": len(ref_bytes), "equal": eq, "kind": kind}
        if eq != len(ref_bytes):
            print(f"[bench] PARITY FAILURE: {len(ref_bytes) - eq} of {len(ref_bytes)} bitstreams differ from the {kind} encoder's bytes", file=sys.stderr)
    if not extras:
        return out
    # how this repo's C restatement (what `kind: "port"` runs would time) compares with the reference extension on this host:
    # the first image, both coders, so that a line from a checkout without oracle/_ref stays comparable
    if kind == "reference":
        try:
            from tests import synth as T
            from oracle import oracle as O

            t_port = t_ref = None
            for _ in range(2):
                t0 = time.perf_counter()
                for st in host[:streams_per_image]:
                    sym, s, m, w, am, zb, yq = T.to_coder_inputs(st[0], *(x.astype(np.float32) for x in st[1:]))
                    b = O.encode_gmm(0, sym, s, m, w)
                    assert np.array_equal(O.decode_gmm(0, b, s, m, w, am + 1), sym)
                dtp = time.perf_counter() - t0
                # (to_coder_inputs is part of the loop above and not of the reference's: taken out below)
                t0 = time.perf_counter()
                for st in host[:streams_per_image]:
                    T.to_coder_inputs(st[0], *(x.astype(np.float32) for x in st[1:]))
                dtp -= time.perf_counter() - t0
                t0 = time.perf_counter()
                for st in prepared[:streams_per_image]:
                    code(st)
                dtr = time.perf_counter() - t0
                t_port, t_ref = (dtp if t_port is None else min(t_port, dtp)), (dtr if t_ref is None else min(t_ref, dtr))
            out["port_over_reference"] = {"time_ratio": round(t_port / t_ref, 2), "port_ms_per_image": round(t_port * 1e3, 1),
                                          "reference_ms_per_image": round(t_ref * 1e3, 1),
                                          "note": "oracle/fgmm_oracle.c (scalar C restatement, what kind=port times) over the reference extension's SIMD path, first image, best of 2"}
        except Exception as e:  # pragma: no cover
            out["port_over_reference"] = {"time_ratio": None, "error": str(e)[:200]}
    if not from_seeds:  # (real latents: the helper processes of the two legs below regenerate synthetic streams from their seeds)
        return out
    # all cores: processes, not threads; each regenerates its share of the streams from their seeds
    try:
        import multiprocessing as mp

        cores = max(1, min(len(os.sched_getaffinity(0)), 16, len(host)))
        n_streams = len(host)
        seeds = [stream_seed(rank, k // streams_per_image, k % streams_per_image, streams_per_image) for k in range(n_streams)]
        shp = [shapes[k % streams_per_image] for k in range(n_streams)]
        jobs = [(seeds[c::cores], shp[c::cores], f16, 6.0) for c in range(cores)]
        with _plain_children():
            pool = mp.get_context("spawn").Pool(cores)
        with pool:
            res = pool.map(_all_cores_worker, jobs)
        streams_done = sum(r[0] for r in res)
        wall = max(r[2] for r in res) - min(r[1] for r in res)
        out["all_cores"] = {"value": round(streams_done / streams_per_image * pix_per_image / wall / 1e6, 2), "unit": "Mpixels/s",
                            "cores": cores, "sample": f"{cores} processes, one stream at a time each, {streams_done} streams in {wall:.1f} s"}
    except Exception as e:  # pragma: no cover
        out["all_cores"] = {"value": None, "error": str(e)[:200]}
    # SURVEY.md section 8(a')/(d): the USE_SIMD=0 line beside the SIMD baseline - a different codec (its streams differ from
    # the SIMD path's), timed for orientation only, on a quarter of the sample (it is ~2.5x slower)
    try:
        import multiprocessing as mp

        if kind == "reference":
            n_sc = max(1, n_img // 4) * streams_per_image
            seeds = [stream_seed(rank, k // streams_per_image, k % streams_per_image, streams_per_image) for k in range(n_sc)]
            shp = [shapes[k % streams_per_image] for k in range(n_sc)]
            with _plain_children():
                pool = mp.get_context("spawn").Pool(1)
            with pool:
                k2, sym2, best2, passes2 = pool.map(_scalar_worker, [(seeds, shp, f16, 8.0)])[0]
            out["scalar"] = {"value": round(n_sc / streams_per_image * pix_per_image / best2 / 1e6, 3), "unit": "Mpixels/s", "cores": 1,
                             "kind": k2, "env": "USE_SIMD=0",
                             "sample": f"{n_sc // streams_per_image} image(s) ({sym2} symbols), encode+decode, best of {passes2} passes, "
                                       f"{best2 / sym2 * 1e9:.0f} ns/symbol; not a parity target: a different bitstream"}
    except Exception as e:  # pragma: no cover
        out["scalar"] = {"value": None, "error": str(e)[:200]}
    return out


def pmc_traffic(workload: str, mode: str, f16: bool, images: int):
    """roofline.traffic: HBM bytes per symtab launch from rocprofv3 PMC passes (scripts/collect_pmc.sh, committed under
    profiles/), gfx950-corrected as MI355X_MICROARCH.md prescribes.  PMC collection needs the profiler, so bench.py
    reports the LATEST COMMITTED measurement of this same workload (same mode, parameter dtype and image count) with the
    file it came from — a recorded value, not this run's — or null when there is none."""
    best = src = None
    for f in sorted(__import__("glob").glob(os.path.join(ROOT, "profiles", "r*_pmc_symtab*.json"))):
        try:
            d = json.load(open(f))
            same = d.get("workload") == workload and d.get("mode") == mode and d.get("param_dtype", "f32") == ("f16" if f16 else "f32")
            if same and d.get("images_per_gpu", 24 if workload == "kodak24" else 1) == images:
                best, src = d["symtab"]["hbm_bytes_corrected"], os.path.relpath(f, ROOT)
        except Exception:
            pass
    return best, src


def tab_kernel_alone():
    """roofline_decode.alone: the decode-side table kernel measured ALONE under rocprofv3 (scripts/profile_tab_alone.sh: one Kodak
    stage in one launch, kernel-trace statistics + the SQ instruction counters in a pass of their own) - the latest committed
    profiles/r*_tab_kernel_alone.json, a recorded measurement like roofline.traffic: in a bench step the launches share the GPU
    with the table copies, and under --kernel-trace the step's 22 small launches are inflated 2.5x."""
    for f in sorted(__import__("glob").glob(os.path.join(ROOT, "profiles", "r*_tab_kernel_alone.json")), reverse=True):
        try:
            d = json.load(open(f))
            return {"launch_ms": d["valu"]["launch_ms"], "latents_per_launch": d["latents_per_launch"], "edges_per_latent": d["edges_per_latent"],
                    "valu_frac": d["valu"]["valu_frac"], "valu_wave_insts_per_latent": d["valu"]["valu_wave_insts_per_latent"],
                    "source": os.path.relpath(f, ROOT), "stats": os.path.relpath(f, ROOT).replace(".json", "_stats.csv")}
        except Exception:
            pass
    return None


def symtab_valu_roof(workload: str, mode: str, f16: bool, n_coded: int, launch_ms: float):
    """The encode-side kernel against its OTHER roof, VALU issue: wave-level VALU instructions per coded symbol as the SQ counters
    give them (recorded: profiles/r*_pmc_valu_symtab.json, scripts/pmc_valu.sh) x coded symbols x the measured average issue cost of
    this kernel's instruction mix (cycles per wave64 instruction: plain 4.5, packed fp32 5.2, rcp / rsq 9 - scripts/valu_peak.hip)
    / (1024 SIMDs x 2.4 GHz) / the launch duration measured in THIS run.  -> dict, or None when no count is recorded for the
    configuration."""
    best = src = None
    for f in sorted(__import__("glob").glob(os.path.join(ROOT, "profiles", "r*_pmc_valu_symtab.json"))):
        try:
            d = json.load(open(f))
            e = d.get(workload)
            if e and e.get("mode") == mode and e.get("param_dtype") == ("f16" if f16 else "f32"):
                best, src = (e["valu_wave_insts_per_symbol"], d["cycles_per_wave_instruction"]["average"]), os.path.relpath(f, ROOT)
        except Exception:
            pass
    if best is None or launch_ms <= 0:
        return None
    per_sym, cyc = best
    issue_ms = per_sym * n_coded * cyc / (256 * 4 * 2.4e9) * 1e3
    return {"valu_frac": round(issue_ms / launch_ms, 4), "valu_issue_ms_at_peak": round(issue_ms, 4), "valu_wave_insts_per_symbol": per_sym,
            "cycles_per_wave_instruction": cyc, "counts_source": src,
            "note": "instruction counts recorded (PMC passes of their own), launch time measured in this run"}


def _die_with_parent():
    """runs in a rank between fork and exec: SIGTERM when the launcher dies (even of SIGKILL: prctl PR_SET_PDEATHSIG), so a
    killed launcher cannot leave ranks holding the GPUs"""
    try:
        import ctypes
        import signal

        ctypes.CDLL("libc.so.6", use_errno=True).prctl(1, int(signal.SIGTERM), 0, 0, 0)  # PR_SET_PDEATHSIG = 1
    except Exception:
        pass


def launch_ranks(a, argv):
    """`python bench.py --gpus N` with N > 1 and no torch.distributed.run around it: start N fresh child processes, one
    per GPU (RANK / LOCAL_RANK / WORLD_SIZE / LOCAL_WORLD_SIZE / MASTER_* in their environment), BEFORE anything in this
    process touches the GPU, and SUPERVISE them: rank 0's stdout is read by a thread, every child is polled; the first rank
    that exits non-zero (or the overall timeout, or SIGTERM / SIGINT to this process) ends the others within seconds —
    SIGTERM to each child's process group, SIGKILL after a grace period — and the launcher exits non-zero.  A rank that
    dies at start-up can therefore not leave rank 0 waiting in the rendezvous until the collective's own timeout.
    Children are started as children (never exec'ed over this process)."""
    import signal
    import socket
    import subprocess
    import threading

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), FGMM_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, start_new_session=True,
                                      preexec_fn=_die_with_parent, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out0 = []
    reader = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
    reader.start()

    def stop_all(grace_s: float = 3.0):
        for sig, wait_s in ((signal.SIGTERM, grace_s), (signal.SIGKILL, 5.0)):
            for p in procs:
                if p.poll() is None:
                    try:
                        os.killpg(p.pid, sig)  # the child leads its own session: its helpers go with it
                    except (ProcessLookupError, PermissionError):
                        pass
            t_end = time.monotonic() + wait_s
            while time.monotonic() < t_end and any(p.poll() is None for p in procs):
                time.sleep(0.02)

    interrupted = []

    def on_signal(signum, _frame):
        interrupted.append(signum)

    old_handlers = {sg: signal.signal(sg, on_signal) for sg in (signal.SIGTERM, signal.SIGINT)}
    deadline = time.monotonic() + a.launch_timeout
    failed = None
    try:
        while True:
            rcs = [p.poll() for p in procs]
            bad = [(r, rc) for r, rc in enumerate(rcs) if rc not in (None, 0)]
            if bad:
                failed = f"rank {bad[0][0]} exited with code {bad[0][1]}"
                break
            if all(rc == 0 for rc in rcs):
                break
            if interrupted:
                failed = f"interrupted by signal {interrupted[0]}"
                break
            if time.monotonic() > deadline:
                failed = f"no result within --launch-timeout {a.launch_timeout:.0f} s"
                break
            time.sleep(0.05)
    except BaseException as e:  # anything unexpected in the supervision loop: the ranks must not outlive it
        failed = failed or f"launcher error: {type(e).__name__}: {e}"
        raise
    finally:
        # each rank leads its own session (a terminal's Ctrl-C does not reach it): whatever ended the loop, no rank is left behind
        if failed or any(p.poll() is None for p in procs):
            stop_all()
        for sg, h in old_handlers.items():
            signal.signal(sg, h)
    reader.join(timeout=5.0)
    rcs = [p.poll() for p in procs]
    if failed:
        print(f"bench.py: {failed}; the other ranks were stopped (exit codes {rcs})", file=sys.stderr)
        raise SystemExit(1)
    sys.stdout.write((out0[0] if out0 else b"").decode())
    sys.stdout.flush()


def plan_l3(local_rank: int, ranks_on_node: int):
    """flashgmm_amd.parallel.plan_l3 (an L3 domain of its own for the calling thread, the host workers of every rank elsewhere) with the
    bench's switch: FGMM_BENCH_L3=0 leaves workers and calling thread wherever the scheduler puts them (FGMM_WORKER_CPUS=inherit).
    timed() keeps the calling thread on its domain for the timed region only (helper processes must inherit the wide mask)."""
    from flashgmm_amd import parallel as P_

    if os.environ.get("FGMM_BENCH_L3", "1") == "0":
        os.environ.setdefault("FGMM_WORKER_CPUS", "inherit")
        return None, "off (FGMM_BENCH_L3=0): workers and calling thread wherever the scheduler puts them"
    return P_.plan_l3(local_rank, ranks_on_node)


_REAL_STDOUT = None
LINE_LIMIT = 4096  # the driver keeps ~8 KB of stdout: the ONE line it parses stays under half of that, asserted (BENCH_r05 was 22 KB: unparsed)


def step_stats(step_s, cpu_s=None, throttled=None):
    """per-step wall times of a timed region; cpu_ms = CPU time of all threads of the process per step (time.process_time between
    steps); nr_throttled = the cgroup CPU controller's throttling count over the region, every visible level summed (two reads)"""
    ms = np.asarray(step_s) * 1e3
    out = {"min": round(float(ms.min()), 3), "median": round(float(np.median(ms)), 3), "p90": round(float(np.percentile(ms, 90)), 3),
           "max": round(float(ms.max()), 3), "all": [round(float(v), 2) for v in ms]}
    if cpu_s is not None:
        out["cpu_ms"] = [round(float(v) * 1e3, 1) for v in cpu_s]
    if throttled is not None:
        out["nr_throttled"] = int(throttled)
    return out


def _pick(d, *keys):
    """the named keys of a dict that has them (None / absent ones dropped)"""
    return {k: d[k] for k in keys if isinstance(d, dict) and d.get(k) is not None}


def _eq(d):
    """reference_bytes_equal without its notes"""
    return _pick(d, "streams", "equal", "kind", "error") if isinstance(d, dict) else None


def summary_line(full: dict, detail_path=None) -> dict:
    """The ONE line of stdout: the driver's contract + `roofline` + `cpu_baseline` + one number per extra leg.  Everything else
    (per-step arrays, phases, notes, the diagnostic legs) is `full`, which goes to bench_detail.json and stderr."""
    g = full.get
    out = {k: g(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                             "dtype", "data")}
    sm = g("step_ms") or {}
    out["step_ms"] = _pick(sm, "min", "median", "p90", "max")
    if sm.get("cpu_ms"):
        out["step_ms"]["cpu_ms_median"] = round(float(np.median(sm["cpu_ms"])), 1)
    if sm.get("nr_throttled") is not None:
        out["step_ms"]["nr_throttled"] = sm["nr_throttled"]
    if isinstance(sm.get("phases_ms"), dict) and "between_calls" in sm["phases_ms"]:
        out["step_ms"]["between_calls"] = sm["phases_ms"]["between_calls"]
    out["config"] = _pick(g("config") or {}, "workload", "schedule", "images_per_gpu", "K", "approx_mode", "param_dtype", "coded_symbols_per_gpu",
                          "host_threads_per_gpu", "binding", "checkpoint_stride", "streams_per_gpu", "one_device_rehearsal")
    rf = g("roofline")
    if isinstance(rf, dict):
        out["roofline"] = _pick(rf, "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic_source", "launch_ms", "bytes_per_launch")
        out["roofline"]["traffic"] = rf.get("traffic")  # (null when no PMC measurement of this configuration is on file)
        if isinstance(rf.get("valu"), dict):
            out["roofline"]["valu"] = _pick(rf["valu"], "valu_frac")
    rd = g("roofline_decode")
    if isinstance(rd, dict):
        out["roofline_decode"] = _pick(rd, "kernel", "bound", "ms_per_step", "valu_frac", "hbm_frac")
        if isinstance(rd.get("alone"), dict):
            out["roofline_decode"]["alone"] = _pick(rd["alone"], "launch_ms", "valu_frac", "source")
    cb = g("cpu_baseline")
    if isinstance(cb, dict):
        out["cpu_baseline"] = _pick(cb, "value", "unit", "cores", "kind", "sample", "ms_per_image", "throughput_speedup")
        out["cpu_baseline"]["reference_bytes_equal"] = _eq(cb.get("reference_bytes_equal"))
    lt = g("latency_ms")
    if isinstance(lt, dict):
        out["latency_ms"] = _pick(lt, "as_codec", "reference_cpu", "speedup_plain", "speedup_checkpointed")
    for k in ("checkpointed", "upper_bound", "as_codec", "one_host_thread"):
        if isinstance(g(k), dict):
            out[k] = _pick(g(k), "value")
    if isinstance(g("modes"), dict):
        out["modes"] = {m: {"value": e.get("value"), "symtab": _pick(e.get("symtab") or {}, "frac"), "reference_bytes_equal": _eq(e.get("reference_bytes_equal"))}
                        for m, e in g("modes").items()}
    el = g("elic4k")
    if isinstance(el, dict):
        out["elic4k"] = {"value": el.get("value"), "symtab": _pick(el.get("symtab") or {}, "frac"),
                         "reference_bytes_equal": _eq(el.get("reference_bytes_equal")),
                         "cpu_baseline": _pick(el.get("cpu_baseline") or {}, "value"), **_pick(el, "error")}
        if isinstance(el.get("checkpointed"), dict):
            out["elic4k"]["checkpointed"] = _pick(el["checkpointed"], "value")
    if isinstance(g("head_fused"), dict):
        out["head_fused"] = _pick(g("head_fused"), "value", "mfma_frac", "mfma_frac_back_to_back", "head_ms", "unfused_ms", "bytes_equal_unfused", "error")
        if isinstance(g("head_fused").get("bf16x6"), dict):
            out["head_fused"]["bf16x6"] = _pick(g("head_fused")["bf16x6"], "fused_kernel_ms", "head_params_ms_back_to_back", "bytes_equal_unfused", "error")
    rk = g("ranks") or {}
    out["ranks"] = _pick(rk, "backend", "rccl_ranks", "ms_per_step", "host_threads_per_gpu", "result_checked_ranks")
    if isinstance(rk.get("allgather_ms"), dict):
        out["ranks"]["allgather_ms"] = _pick(rk["allgather_ms"], "issue", "exposed")
    elif rk.get("allgather_ms") is not None:
        out["ranks"]["allgather_ms"] = rk["allgather_ms"]
    if "host_cpu_budget" in rk:
        out["ranks"]["host_cpu_budget"] = rk["host_cpu_budget"]
    if isinstance(g("reference_md5"), dict):
        out["reference_md5_equal"] = g("reference_md5").get("md5_equal_reference")
    if g("host_throttled"):
        out["host_throttled"] = True
    if g("bench_s") is not None:
        out["bench_s"] = g("bench_s")
    if detail_path:
        out["detail"] = detail_path
    return out


def emit(full: dict, detail: bool = True) -> None:
    """Rank 0's output: the whole result to bench_detail.json (FGMM_BENCH_DETAIL names another path; "" = none) and to stderr, the
    summary - ONE line under LINE_LIMIT bytes - to stdout."""
    detail_path = os.environ.get("FGMM_BENCH_DETAIL", "bench_detail.json") if detail else None
    blob = json.dumps(full)
    if detail_path:
        try:
            with open(detail_path, "w") as f:
                f.write(blob + "\n")
        except OSError as e:
            print(f"[bench] could not write {detail_path}: {e}", file=sys.stderr)
            detail_path = None
    if detail:
        print("[bench detail] " + blob, file=sys.stderr)
    line = json.dumps(summary_line(full, detail_path))
    assert len(line) < LINE_LIMIT, f"bench.py's stdout line is {len(line)} bytes: the driver's window is ~8 KB, the limit here {LINE_LIMIT}"
    out = _REAL_STDOUT or sys.stdout
    out.write(line + "\n")
    out.flush()


def dryrun(a, world, rank):
    """FGMM_BENCH_DRYRUN=1 (tests/test_bench_launcher_cpu.py): everything of an N-rank run EXCEPT the GPU work — process
    group (gloo), the per-step all-gather of stream lengths, barriers, max-over-ranks timing, rank 0's one JSON line.
    The line says so ("data": "dryrun-no-gpu", value 0): it is never a measurement."""
    import torch.distributed as dist
    from flashgmm_amd import _lib
    from flashgmm_amd import parallel as P

    if os.environ.get("FGMM_BENCH_DRYRUN_FAIL_RANK") == str(rank):  # test hook: this rank dies before the rendezvous
        raise SystemExit(3)
    if os.environ.get("FGMM_BENCH_DRYRUN_HANG_RANK") == str(rank):  # test hook: this rank never reaches the rendezvous
        time.sleep(3600)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    n_streams = 2 * (a.images or 24)
    threads = _lib.lib().fgmm_host_thread_budget(_lib.ranks_on_node())  # what this rank's context would get
    t_gather = []

    ex = P.LengthExchange(n_streams) if world > 1 else None

    def step():
        lens = [1000 + 7 * rank + i for i in range(n_streams)]  # stand-in for the coder's output lengths
        t0 = time.perf_counter()
        g = None
        if ex is not None:
            ex.start(lens)  # (in flight while the decode calls would run)
            g = ex.wait()
        t_gather.append(time.perf_counter() - t0)
        return g

    for _ in range(max(a.warmup, 1)):
        g = step()
    if world > 1:
        assert g.shape == (world, n_streams) and g[rank].tolist() == [1000 + 7 * rank + i for i in range(n_streams)]
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    per_rank, per_rank_threads = [dt], [threads]
    if world > 1:
        tt = torch.tensor([dt, float(threads)], dtype=torch.float64)
        gathered = [torch.empty_like(tt) for _ in range(world)]
        dist.all_gather(gathered, tt)
        per_rank = [float(t[0]) for t in gathered]
        per_rank_threads = [int(t[1]) for t in gathered]
        dt = max(per_rank)
    if rank == 0:
        emit({"metric": "dryrun", "value": 0.0, "unit": "Mpixels/s", "n_gpus": world, "steps": a.steps,
              "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True,
              "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "dryrun-no-gpu",
              "config": {"workload": a.workload, "streams_per_gpu": n_streams, "checkpoint_stride": a.checkpoint_stride,
                         "one_device_rehearsal": bool(os.environ.get("FGMM_BENCH_ONE_DEVICE"))},
              "ranks": {"backend": "gloo" if world > 1 else None, "rccl_ranks": 0,
                        "ms_per_step": [round(t / a.steps * 1e3, 3) for t in per_rank],
                        "host_threads_per_gpu": per_rank_threads, "host_cpu_budget": _lib.host_cpu_budget(),
                        "allgather_ms": round(float(np.mean(t_gather[-a.steps:])) * 1e3, 4)}}, detail=False)
    if world > 1:
        dist.destroy_process_group()


class Env:
    """what every leg of a run shares: the rank's place in the job, its device, the process group"""

    def __init__(self, rank, world, local_rank, dev, dist, coll_dev, backend, l3_cpus=None):
        self.rank, self.world, self.local_rank, self.dev, self.dist, self.coll_dev, self.backend = rank, world, local_rank, dev, dist, coll_dev, backend
        self.l3_cpus = l3_cpus  # plan_l3(): where timed() keeps the calling thread (the workers are elsewhere)
        self.diag = False  # --diag

    def max_over_ranks(self, v: float) -> float:
        if not self.dist:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=self.coll_dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())


class Leg:
    """One workload resident in HBM and the schedules that are timed over it.  Streams in coding order: image-major,
    stage-minor; stage s of the decode schedule = stream s of every image."""

    def __init__(self, env: Env, workload: str, images: int, mode: str, f16: bool, keep_host_images: int = 1 << 30, share=None, latents_dir=None,
                 pixels_per_image=None, distinct=None):
        from flashgmm_amd import GaussianMixtureConditional

        self.env, self.workload, self.images, self.mode, self.f16 = env, workload, images, mode, f16
        self.shapes1, _ = workload_shapes(workload)
        self.spi = len(self.shapes1)  # streams per image = stages of the codec's decode schedule
        self.real = False
        if share is None and latents_dir:
            self.host, devt, pix, self.spi = load_latents_dir(latents_dir, env.dev, f16, images)
            self.images = images = len(devt) // self.spi
            self.pix_per_image = pix or pixels_per_image or workload_shapes(workload)[1]
            self.shapes1 = [tuple(t[0].shape[1:]) for t in devt[: self.spi]]
            self.real = True
        if share is None and self.real:
            self.n_streams = len(devt)
            self.hw_of = [t[0].shape[2] * t[0].shape[3] for t in devt]
            self.shapes = sorted({tuple(t[0].shape) for t in devt})
            self.stacked = len(self.shapes) == 1
            if self.stacked:
                self.ys, self.ss, self.ms, self.ws = (torch.cat([t[k] for t in devt]) for k in range(4))
            else:
                self.ys, self.ss, self.ms, self.ws = ([t[k] for t in devt] for k in range(4))
        elif share is None:
            self.host, devt, self.pix_per_image = make_workload(env.rank, images, env.dev, workload, f16, keep_host_images, distinct)
            self.n_streams = len(devt)
            self.hw_of = [t[0].shape[2] * t[0].shape[3] for t in devt]
            self.shapes = sorted({tuple(t[0].shape) for t in devt})
            self.stacked = len(self.shapes) == 1
            if self.stacked:  # items of one shape go in as ONE tensor each, [N, ., h, w]: what a network run on a batch produces
                self.ys, self.ss, self.ms, self.ws = (torch.cat([t[k] for t in devt]) for k in range(4))
            else:
                self.ys, self.ss, self.ms, self.ws = ([t[k] for t in devt] for k in range(4))
        else:  # the same tensors under another approximation mode
            for k in ("host", "pix_per_image", "n_streams", "hw_of", "shapes", "stacked", "ys", "ss", "ms", "ws", "real", "spi", "shapes1", "images"):
                setattr(self, k, getattr(share, k))
        spi, n = self.spi, self.n_streams
        self.stage_params = [(self.ss[s::spi], self.ms[s::spi], self.ws[s::spi]) for s in range(spi)]  # strided batch views / sub-lists
        self.stage_idx = [list(range(s, n, spi)) for s in range(spi)]
        self.bytes_per_symbol = 32 if f16 else 56
        self.gmc = GaussianMixtureConditional(K=4, mode=mode)
        self.k_sym, self.k_tab, self.k_qs, self.t_gather, self.edges, self.tab_bytes = [], [], [], [], [], []
        # the path's one exchange: per-stream bitstream lengths, ONE preallocated all_gather_into_tensor, issued
        # asynchronously after the encode call and waited for at the end of the step (the lengths only feed the container index)
        from flashgmm_amd import parallel as P_

        self.ex = P_.LengthExchange(self.n_streams, device=env.coll_dev, threaded=os.environ.get("FGMM_BENCH_EX_THREAD", "1") != "0") if env.dist else None
        self.last = {}

    def with_mode(self, mode: str):
        return Leg(self.env, self.workload, self.images, mode, self.f16, share=self)

    # ---- one step ----------------------------------------------------------------------------------------------------
    def decode_codec(self, res, record=False):
        """stage by stage; every image's stream of a stage in one call"""
        from flashgmm_amd import _lib

        lr = self.env.local_rank
        spi = self.spi
        outs = [None] * (spi if self.stacked else self.n_streams)
        tk = eg = tb = 0.0
        for s in range(spi):
            sp, mp_, wp = self.stage_params[s]
            if self.stacked:  # the batch's results are held stacked (CompressedBatch): a stage is a stride over them, in and out
                outs[s] = self.gmc.decompress_batch(res.strings[s::spi], res.abs_maxes[s::spi], res.zero_bitmaps[s::spi], sp, mp_, wp,
                                                    stacked_output=True)
            else:
                idx = self.stage_idx[s]
                o = self.gmc.decompress_batch([res[i][0][0] for i in idx], [res[i][0][1] for i in idx], [res[i][0][2] for i in idx], sp, mp_, wp)
                for i, t in zip(idx, o):
                    outs[i] = t
            if record:
                tk += _lib.kernel_ms(lr, 1)
                eg += _lib.ctx_stat(lr, 3)
                tb += _lib.ctx_stat(lr, 1)
        if record:
            self.k_tab.append(tk), self.edges.append(eg), self.tab_bytes.append(tb)
        return outs

    def decode_all(self, res, record=False):
        from flashgmm_amd import _lib

        lr = self.env.local_rank
        if self.stacked:
            outs = [self.gmc.decompress_batch(res.strings, res.abs_maxes, res.zero_bitmaps, self.ss, self.ms, self.ws, stacked_output=True)]
        else:
            outs = self.gmc.decompress_batch([r[0][0] for r in res], [r[0][1] for r in res], [r[0][2] for r in res], self.ss, self.ms, self.ws)
        if record:
            self.k_tab.append(_lib.kernel_ms(lr, 1)), self.edges.append(_lib.ctx_stat(lr, 3)), self.tab_bytes.append(_lib.ctx_stat(lr, 1))
        return outs

    def step(self, schedule, record=False):
        from flashgmm_amd import _lib

        res = self.gmc.compress_batch(self.ys, self.ss, self.ms, self.ws)
        if record:
            self.k_sym.append(_lib.kernel_ms(self.env.local_rank, 0))
            self.k_qs.append(_lib.kernel_ms(self.env.local_rank, 2))
        if self.ex is not None:  # issued now, in flight during the decode calls
            self.ex.start([len(b) for b in res.strings] if self.stacked else [len(r[0][0]) for r in res])
        outs = self.decode_codec(res, record) if schedule == "codec" else self.decode_all(res, record)
        if self.ex is not None:
            self.last["lengths"] = self.ex.wait(to_host=False)  # (read on the host when the containers are assembled: check_last)
            if record:
                self.t_gather.append((self.ex.issue_ms, self.ex.exposed_ms, self.ex.total_ms))
        return res, outs

    def timed(self, schedule, steps, record=False):
        """-> (wall time of the whole region, step_ms statistics).  The per-step clock reads sit between steps, after the step's
        own stream synchronisation (decompress returns with y_hat complete): they add nothing to the region.
        (main() keeps the interpreter's generational GC off for the whole run: a pass takes tens of ms with torch loaded and
        is not part of the path.)"""
        dist = self.env.dist if self.env.world > 1 else None  # (a barrier over one rank orders nothing - and an RCCL barrier right before
        #                                                       the timed steps idles the GPU long enough to cost the first two of them 1-3 ms)
        wide = None
        if self.env.l3_cpus:  # the calling thread on its own L3 domain for the region (plan_l3); the mask is opened again below
            try:
                wide = os.sched_getaffinity(0)
                os.sched_setaffinity(0, self.env.l3_cpus)
            except OSError:  # (the allowed CPUs have changed under us: go on without)
                wide, self.env.l3_cpus = None, None
        settled = D.settle_calling_thread()
        if settled is not None or wide is not None:
            self.step(schedule)  # (one more untimed step: the 5 ms of probing / a migration must not be the idle gap before the region)
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        probe = D.HostProbe() if self.env.diag else None  # (--diag: cgroup / pressure files between steps; default: two clocks)
        thr0 = D.throttle_count()
        marks = [(time.perf_counter(), time.process_time())]
        for _ in range(steps):
            self.last["res"], self.last["outs"] = self.step(schedule, record=record)
            marks.append((time.perf_counter(), time.process_time()))
            if probe is not None:
                probe.sample()
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        t1 = time.perf_counter()
        thr1 = D.throttle_count()
        if wide is not None:
            os.sched_setaffinity(0, wide)
        wall, cpu = np.diff([m[0] for m in marks]), np.diff([m[1] for m in marks])
        stats = step_stats(wall, cpu, None if thr0 is None or thr1 is None else thr1 - thr0)
        stats["calling_thread"] = settled
        stats["phases_ms"] = D.region_phases(self.env.local_rank, 1 + (self.spi if schedule == "codec" else 1), [x * 1e3 for x in wall])
        if probe is not None:
            probe.close()
            stats["host_probe"] = D.probe_stats(probe)
        return t1 - marks[0][0], stats

    def check_last(self):
        """correctness of what was timed: decode(encode(y)) == round(y) for every stream of this rank"""
        res, outs = self.last["res"], self.last["outs"]
        if self.ex is not None:  # what the exchange delivered for this rank's row: the last step's bitstream lengths
            mine = self.last["lengths"][self.env.rank].cpu().tolist()
            assert mine[: self.n_streams] == ([len(b) for b in res.strings] if self.stacked else [len(r[0][0]) for r in res]), "gathered stream lengths mismatch"
        if self.stacked:  # outs: one [N', 1, M, h, w] tensor per decode call (stage s = every spi-th stream from s; or all of them)
            assert torch.equal(res.y_q[:, 0], torch.round(self.ys)), "quantised latents mismatch"
            step = len(outs)
            for s, o in enumerate(outs):
                assert o.shape[0] == len(range(s, self.n_streams, step)) and torch.equal(o, res.y_q[s::step]), f"decode call {s} mismatch"
            return res
        for i in range(self.n_streams):
            assert torch.equal(outs[i], res[i][1]) and torch.equal(res[i][1], torch.round(self.ys[i])), f"stream {i} mismatch"
        return res

    def coded_symbols(self, res):
        return sum(int(r[0][2].sum()) * hw for r, hw in zip(res, self.hw_of))

    def symtab_roofline(self, res):
        n_coded = self.coded_symbols(res)
        sym_ms = float(np.mean(self.k_sym))
        achieved = n_coded * self.bytes_per_symbol / (sym_ms * 1e-3) / 1e9
        return n_coded, sym_ms, achieved

    def mpix(self, steps, dt):
        return self.env.world * self.images * self.pix_per_image * steps / dt / 1e6

    def checkpointed(self, schedule, stride, steps, total_bytes):
        """the whole step on CHECKPOINTED streams (GaussianMixtureConditional(checkpoint_stride=...): the reference's bitstreams +
        out-of-band notes of the coder state every `stride` symbols, 16 bytes each): the segments between notes are independent, so
        the decode runs ON THE GPU, one workgroup per segment (segdec_kernel; no decode-side tables, nothing but the bitstreams
        crosses PCIe), every segment verified against the next note.  Not the reference's interface alone - its decoder has no
        such notes.  Every rank runs it; the time is the slowest rank's."""
        from flashgmm_amd import GaussianMixtureConditional, _lib

        lr = self.env.local_rank
        plain, self.gmc = self.gmc, GaussianMixtureConditional(K=4, mode=self.mode, checkpoint_stride=stride)
        try:
            self.step(schedule)
            dt_ck, step_ms_ck = self.timed(schedule, steps)
            res_ck = self.check_last()
            on_gpu, back = _lib.ctx_stat(lr, 4), _lib.ctx_stat(lr, 5)
        finally:
            self.gmc = plain
        dt_ck = self.env.max_over_ranks(dt_ck)
        ck_bytes = int(sum(16 * len(r[0][0].ckpt) for r in res_ck))
        return {"schedule": schedule, "value": round(self.mpix(steps, dt_ck), 2), "unit": "Mpixels/s",
                "ms_per_step": round(dt_ck / steps * 1e3, 3), "steps": steps, "step_ms": step_ms_ck,
                "checkpoint_stride": stride, "checkpoint_bytes": ck_bytes,
                "checkpoint_bytes_over_bitstream_bytes": round(ck_bytes / max(total_bytes, 1), 4),
                "bitstreams_decoded_on_gpu_last_call": on_gpu, "bitstreams_handed_back_last_call": back,
                "note": "the same bitstreams + out-of-band checkpoints: decoded on the GPU, one workgroup per segment "
                        "(segdec_kernel), every segment verified against the next checkpoint"}


def head_leg(leg: Leg, device: int, reps: int = 8):
    """SURVEY.md section 8 f2 in the default line: the parameter head's last layer - Conv2d(640, 3*K*192, 1), ckbd_gmm.py:115-121 - FUSED
    with the encode-side CDF kernel (fgmm_head.hip: v_mfma_f32_32x32x2_f32, the table entry as the epilogue) on this batch's latents with
    a random head of that shape, against what a caller does today (torch's fp32 conv2d, three parameter tensors through HBM,
    symtab_kernel).  GPU milliseconds by events on the stream; `value` = matrix-product TFLOP/s of the fused kernel, table epilogue
    included; the bitstreams of the fused kernel against those of the un-fused path fed the head kernel's own parameter planes."""
    from flashgmm_amd import ParameterHead, _lib
    from tests.synth import make_head

    y = leg.ys
    N, M, h, w = y.shape
    conv, x, _ = make_head(5, M, 640, h, w, N, dev=y.device)
    head = ParameterHead(conv)
    gmc = leg.gmc
    flop = 2.0 * 12 * M * 640 * N * h * w

    def gpu_ms(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a_.record()
        r = fn()
        b_.record()
        torch.cuda.synchronize()
        return a_.elapsed_time(b_), r

    def torch_params():
        with torch.no_grad():
            return torch.nn.functional.conv2d(x, conv.weight, conv.bias).chunk(3, 1)

    t_conv, t_sym, t_fused = [], [], []
    for i in range(reps + 2):
        ms, prm = gpu_ms(torch_params)
        gmc.compress_batch(y, *prm, weights_are_logits=True)
        if i >= 2:
            t_conv.append(ms), t_sym.append(_lib.kernel_ms(device, 0))
    for i in range(reps + 2):
        fused = gmc.compress_head_batch(y, x, head)
        if i >= 2:
            t_fused.append(_lib.kernel_ms(device, 0))
    # the matrix product alone, launched back to back (six launches in one bracket): what the kernel takes when the GPU does not come
    # out of an idle gap - 0.12-0.14 ms of a lone launch is the chip waking up (profiles/r06_head_kernel.md)
    warm = []
    for _ in range(3):
        ms, _r = gpu_ms(lambda: [head.params(x) for _ in range(6)])
        warm.append(ms / 6)
    planes = head.params(x)
    plain = gmc.compress_batch(y, *planes, weights_are_logits=True)
    out = gmc.decompress_batch(fused.strings, fused.abs_maxes, fused.zero_bitmaps, *planes, weights_are_logits=True, stacked_output=True)
    # the OPTION: the same layer on the BF16 matrix cores with binary32 accuracy (FGMM_HEAD_BF16X6, fgmm_head16.hip) - the whole call's GPU
    # time (the features' split + the fused kernel), its bytes against its own un-fused path, its parameters against the exact form's
    bf = {}
    try:
        head16 = ParameterHead(conv, arithmetic="bf16x6")
        t16 = []
        for i in range(reps + 2):
            ms, fused16 = gpu_ms(lambda: gmc.compress_head_batch(y, x, head16))
            if i >= 2:
                t16.append((_lib.kernel_ms(device, 0), ms))
        p16 = head16.params(x)
        plain16 = gmc.compress_batch(y, *p16, weights_are_logits=True)
        warm16 = [gpu_ms(lambda: [head16.params(x) for _ in range(6)])[0] / 6 for _ in range(3)]
        scale = torch.nn.functional.conv2d(x.abs(), conv.weight.abs(), conv.bias.abs())
        bf = {"fused_kernel_ms": round(float(np.median([t[0] for t in t16])), 4),
              "head_params_ms_back_to_back": round(float(np.median(warm16)), 4),
              "equivalent_tflops_back_to_back": round(flop / float(np.median(warm16)) / 1e9, 1),
              "bytes_equal_unfused": [bytes(b) for b in fused16.strings] == [bytes(b) for b in plain16.strings],
              "max_error_over_sum_abs_wx_vs_exact_form": float(((torch.cat(p16, 1) - torch.cat(planes, 1)).abs() / scale).max()),
              "note": "three bf16 parts per operand, six v_mfma_f32_32x32x16_bf16 per product, binary32 accumulation; deterministic on gfx950, not the "
                      "fmaf chain of the default form; head_params_ms includes the split of the features (head16_split_kernel)"}
    except Exception as e:  # pragma: no cover
        bf = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
    k = float(np.median(t_fused))
    return {"value": round(flop / k / 1e9, 1), "unit": "TFLOP/s (f32 MFMA, table epilogue included)", "mfma_frac": round(flop / k / 1e9 / 157.3, 4),
            "mfma_peak_tflops": 157.3, "head_ms": round(k, 4), "unfused_ms": round(float(np.median(t_conv) + np.median(t_sym)), 4),
            "torch_conv_ms": round(float(np.median(t_conv)), 4), "symtab_ms": round(float(np.median(t_sym)), 4), "gemm_gflop": round(flop / 1e9, 1),
            "head_params_ms_back_to_back": round(float(np.median(warm)), 4), "mfma_frac_back_to_back": round(flop / float(np.median(warm)) / 1e9 / 157.3, 4),
            "bytes_equal_unfused": [bytes(b) for b in fused.strings] == [bytes(b) for b in plain.strings],
            "decode_equals_round_y": bool(torch.equal(out, fused.y_q)),
            "bf16x6": bf,
            "head": f"Conv2d(640, {12 * M}, 1), random weights; {N} bitstreams of [{M}, {h}, {w}]",
            "detail": "profiles/r06_head_kernel.md"}


def ka1_check(leg: Leg, res):
    """The first four bitstreams of rank 0 are SURVEY.md §8c's known-answer streams (seeds 0..3 = images 0 and 1 of the Kodak
    batch): their md5s against tests/golden/ka1.json — fixtures made from the reference compiled in the build container
    (tests/golden/make_golden.py).  -> dict, or None when the workload is not the one the fixtures were made for."""
    import hashlib

    if leg.workload != "kodak24" or leg.f16 or leg.env.rank != 0 or leg.n_streams < 2:
        return None
    try:
        ka = json.load(open(os.path.join(ROOT, "tests", "golden", "ka1.json")))[leg.mode]
    except (OSError, KeyError, ValueError):
        return None
    n = min(4, leg.n_streams)
    got = [hashlib.md5(bytes(res[i][0][0])).hexdigest() for i in range(n)]
    want = [ka[str(i)]["md5"] for i in range(n)]
    return {"streams": n, "md5_equal_reference": got == want, "md5": got, "source": "tests/golden/ka1.json"}


DUMP_MAX_ELEMS = 1 << 22  # --dump-outputs: a larger array is written as a seeded sample of this many elements (16 MB in float32)
DUMP_MAX_BYTES = 64 << 20


def _dump_sample(n: int):
    """fixed positions of an array of n > DUMP_MAX_ELEMS elements: one per equal slice of it, drawn by a seeded generator
    (the same positions in every run, and for every array of that length), ascending -> int64 array, or None (everything)"""
    if n <= DUMP_MAX_ELEMS:
        return None
    edges = np.arange(DUMP_MAX_ELEMS + 1, dtype=np.int64) * n // DUMP_MAX_ELEMS
    return edges[:-1] + np.random.default_rng(20240611).integers(0, edges[1:] - edges[:-1])


def dump_outputs(path: str, leg: Leg) -> dict:
    """--dump-outputs DIR: what the timed path handed its caller in the LAST timed step, as DIR/<name>.npy - streams in coding order
    (image-major, stage-minor), each array flattened stream after stream:
      y_hat              decompress: the decoded latents (float32)
      y_q                compress: round(y) as the encoder returns it (float32)
      bitstreams         compress: the bytes of every bitstream, concatenated (float32, 0..255)
      bitstream_lengths  compress: bytes per bitstream (float64)
      abs_max            compress: each bitstream's abs_max (float64)
      zero_bitmaps       compress: each bitstream's per-channel flags, concatenated (float32)
    An array of more than DUMP_MAX_ELEMS elements is written as the sample _dump_sample picks (the same positions in every run).
    -> {name: elements written}"""
    res, outs = leg.last["res"], leg.last["outs"]
    if leg.stacked:  # outs: one [N', 1, M, h, w] tensor per decode call, call s = every len(outs)-th stream from s
        strings, abs_max, zb, y_q = res.strings, res.abs_maxes, res.zero_bitmaps.reshape(-1), res.y_q.reshape(-1)
        y_hat = torch.empty_like(res.y_q)
        for s, o in enumerate(outs):
            y_hat[s::len(outs)] = o
        y_hat = y_hat.reshape(-1)
    else:
        strings, abs_max = [r[0][0] for r in res], [r[0][1] for r in res]
        zb = torch.cat([r[0][2].reshape(-1).cpu() for r in res])
        y_q = torch.cat([r[1].reshape(-1) for r in res])
        y_hat = torch.cat([o.reshape(-1) for o in outs])

    def sampled(t):
        idx = _dump_sample(t.numel())
        if idx is not None:
            t = t[torch.from_numpy(idx).to(t.device)]
        return t.to(torch.float32).cpu().numpy()

    blob = np.frombuffer(b"".join(bytes(b) for b in strings), np.uint8)
    idx = _dump_sample(blob.size)
    arrays = {"y_hat": sampled(y_hat), "y_q": sampled(y_q),
              "bitstreams": (blob if idx is None else blob[idx]).astype(np.float32),
              "bitstream_lengths": np.array([len(b) for b in strings], np.float64),
              "abs_max": np.array(abs_max, np.float64), "zero_bitmaps": sampled(zb)}
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_MAX_BYTES
    os.makedirs(path, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(path, name + ".npy"), arr)
    return {name: int(arr.size) for name, arr in arrays.items()}


def main(argv=None):
    t_bench0 = time.perf_counter()
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (>= 1); ms_per_step is their mean")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the extra legs and sub-legs, the CPU baseline, the comparisons with the reference, "
                         "the whole result to bench_detail.json and stderr (off: set up, warm up, time the steps, print the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last timed step to DIR/<name>.npy (rank 0; see dump_outputs)")
    ap.add_argument("--workload", default="kodak24", choices=["kodak24", "elic4k"])
    ap.add_argument("--images", type=int, default=None, help="images per GPU (default 24 for kodak24, 16 for elic4k)")
    ap.add_argument("--param-dtype", default=None, choices=["f32", "f16"], help="default f32 (kodak24) / f16 (elic4k)")
    ap.add_argument("--mode", default="polya", choices=["polya", "as", "logistic"])
    ap.add_argument("--schedule", default="codec", choices=["codec", "all-at-once"],
                    help="codec (default): decode stage by stage as the codec's dependencies demand; all-at-once: round 1's")
    ap.add_argument("--launch-timeout", type=float, default=float(os.environ.get("FGMM_BENCH_LAUNCH_TIMEOUT", "1500")),
                    help="self-launch (N > 1): seconds after which the ranks are stopped and the launch fails")

    def _stride(v):
        v = int(v)
        if v < 256 or v & (v - 1):
            raise argparse.ArgumentTypeError("a power of two >= 256 (what the segment decoders take)")
        return v

    ap.add_argument("--checkpoint-stride", type=_stride, default=1024,
                    help="stride of the `checkpointed` extra legs: symbols between the out-of-band notes of the coder state (16 B each)")
    ap.add_argument("--host-threads", type=int, default=0, help="host rANS workers per GPU (0: this rank's share of the CPU budget)")
    ap.add_argument("--diag", action="store_true",
                    help="host-side forensics (scripts/bench_diag.py), off by default: cgroup / pressure probes between the steps of every timed "
                         "region and the self-diagnosing `step_diag` leg - to bench_detail.json and stderr, never to the stdout line")
    ap.add_argument("--diag-steps", type=int, default=40, help="--diag: steps per pool size of the `step_diag` leg")
    ap.add_argument("--diag-pools", default="", help="step_diag: comma-separated host-worker counts that take turns in blocks of 20 steps (default: the "
                                                     "context's pool and - when that is a different number - as many workers as the quota has CPUs)")
    ap.add_argument("--latents-dir", default=None,
                    help="REAL latents instead of synthetic ones: a directory of *.pt files, one per image (see load_latents_dir; the line then "
                         "says data: real-latents).  The reference's own measurement (eval_ckbd.py:113-143) needs a trained checkpoint and the "
                         "Kodak PNGs, neither of which exists offline: this is the hook for whoever has them")
    ap.add_argument("--pixels-per-image", type=int, default=None, help="with --latents-dir, when the files carry no {'pixels': H*W} entry")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--baseline-extras", action="store_true",
                    help="cpu_baseline also times the reference on every core (one stream per process), its USE_SIMD=0 path and this repo's C "
                         "restatement beside it: ~20 s more; the default line carries the one-core number north_star names")
    ap.add_argument("--no-extras", action="store_true", help="skip upper_bound / latency / per-thread legs (profiling runs)")
    ap.add_argument("--no-sublegs", action="store_true",
                    help="skip the `modes` (configs[2]) and `elic4k` (configs[4]) legs of the default kodak24 line")
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    a.full = a.full or a.diag or a.baseline_extras  # (their legs are part of the full run)

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(a, argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {a.gpus}, or without a launcher")
    # stdout carries exactly ONE line (rank 0's JSON): whatever libraries print there (gloo / RCCL banners) goes to stderr
    global _REAL_STDOUT
    sys.stdout.flush()
    _REAL_STDOUT = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    one_device = bool(os.environ.get("FGMM_BENCH_ONE_DEVICE"))  # rehearsal of the N > 1 code path on a 1-GPU box: every rank on GPU 0, gloo
    if os.environ.get("FGMM_BENCH_DRYRUN"):  # no GPU: the launcher, the collective and the JSON contract only (CPU test)
        return dryrun(a, world, rank)
    if one_device:
        local_rank = 0
    from flashgmm_amd import parallel as P

    # first of all (the PCI address comes from sysfs): every thread this process creates from here on — the HIP runtime's
    # own, torch's, the host rANS workers — starts on the GPU's NUMA node
    numa = P.bind_to_gpu_numa_node(local_rank) if os.environ.get("FGMM_BENCH_BIND", "1") != "0" else "not bound (FGMM_BENCH_BIND=0)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if os.environ.get("FGMM_BENCH_BIND", "1") != "0":
        numa = P.confirm_numa_binding(local_rank, numa)  # the runtime's own address for the device: rebinds if sysfs said otherwise
    dist = None
    backend = None
    pg_note = None
    if world > 1 or os.environ.get("FGMM_BENCH_PG", "1") != "0":
        # N = 1 goes through the same collective: a process group of one rank over RCCL (`ranks.rccl_ranks` 1), so that the line of a
        # one-GPU run has made, on hardware, the exchange it will make at N > 1.  What it costs the step: 0.08 ms to issue + 0.02 ms
        # exposed (profiles/r05_n1_process_group.txt; the first build, which copied the lengths to the host on every step, cost
        # 0.7 ms).  FGMM_BENCH_PG=0 runs without a process group; if RCCL cannot be initialised the run goes on without (and says so).
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1 and "MASTER_PORT" not in os.environ:
            import socket

            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        try:
            if one_device:  # RCCL refuses two ranks on one GPU: rehearse with gloo
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            backend = dist.get_backend()
        except Exception as e:
            if world > 1:
                raise
            pg_note = f"no process group at N = 1 ({type(e).__name__}: {str(e)[:120]})"
            dist = None
    coll_dev = dev if backend == "nccl" else torch.device("cpu")
    env = Env(rank, world, local_rank, dev, dist, coll_dev, backend)
    env.diag = a.diag

    from flashgmm_amd import GaussianMixtureConditional, _lib, container as Cn

    if a.images is None:
        # elic4k: SIXTEEN 4K images in flight, decoded stage-major (stage s of every image in one call, as kodak24 does with
        # its 24 images): a call then has a bitstream for every host worker (with eight, half the workers idle: 458 against
        # 612 Mpixels/s, profiles/r04_elic_images_ab.txt); one image alone is a chain of ten single-bitstream calls - that
        # is the latency_ms leg
        a.images = 24 if a.workload == "kodak24" else ELIC_IMAGES
    f16 = (a.param_dtype or ("f32" if a.workload == "kodak24" else "f16")) == "f16"
    perf = D.PerfCounters() if a.diag else None  # (before the library creates its workers: the counters are inherited by new threads)
    env.l3_cpus, l3_note = plan_l3(local_rank, _lib.ranks_on_node())  # (before the library creates its workers)
    _lib.ctx(local_rank, a.host_threads)
    l3_note += f"; fgmm_ctx_worker_cpus: '{_lib.worker_cpus(local_rank)}'"
    _lib.set_profiling(local_rank, True)
    leg = Leg(env, a.workload, a.images, a.mode, f16, latents_dir=a.latents_dir, pixels_per_image=a.pixels_per_image)
    a.images = leg.images
    spi, n_streams, pix_per_image = leg.spi, leg.n_streams, leg.pix_per_image
    ys, ss, ms, ws = leg.ys, leg.ss, leg.ms, leg.ws

    # Warm-up and timed region run back to back: 150 ms of idling between them (the result check used to sit there) costs the
    # following steps 4 % (scripts/step_drift.py: the clocks have come down), so what is checked is the LAST TIMED step's
    # result, after the clock has stopped.
    import gc

    gc.collect()
    gc.freeze()
    gc.disable()  # for the whole run (what a step allocates is freed by reference counting)
    for _ in range(max(a.warmup, 1)):
        leg.step(a.schedule)
    dt, step_ms = leg.timed(a.schedule, a.steps, record=True)
    res = leg.check_last()
    dumped = dump_outputs(a.dump_outputs, leg) if a.dump_outputs and rank == 0 else None
    n_coded = leg.coded_symbols(res)
    total_bytes = sum(len(r[0][0]) for r in res)
    enc_table_bytes = _lib.ctx_stat(local_rank, 0)
    host_threads = _lib.lib().fgmm_ctx_threads(_lib.ctx(local_rank))
    per_rank, per_rank_threads, checked = [dt], [host_threads], 1
    if dist:
        tt = torch.tensor([dt, float(host_threads), 1.0], dtype=torch.float64, device=coll_dev)
        gathered = [torch.empty_like(tt) for _ in range(world)]
        dist.all_gather(gathered, tt)
        per_rank = [float(t[0].item()) for t in gathered]
        per_rank_threads = [int(t[1].item()) for t in gathered]
        checked = int(sum(t[2].item() for t in gathered))
        dt = max(per_rank)
    ka1 = ka1_check(leg, res) if a.full else None

    extras = {}
    if perf is not None and perf.ok and rank == 0:
        # --diag: where the host's cycles go, per coded symbol (user space, every thread of the process): the encode call alone, the
        # decode calls alone, 10 passes each over the last step's data
        def counted(fn, passes=10):
            fn()
            torch.cuda.synchronize()
            c0, t0 = perf.read(), time.perf_counter()
            for _ in range(passes):
                fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return D.PerfCounters.per_symbol(c0, perf.read(), n_coded * passes, dt) | {"ms_per_pass": round(dt / passes * 1e3, 3)}

        extras["perf"] = {"encode_only": counted(lambda: leg.gmc.compress_batch(ys, ss, ms, ws)),
                          "decode_only": counted(lambda: leg.decode_codec(res) if a.schedule == "codec" else leg.decode_all(res)),
                          "note": "perf_event_open, user space, all threads of the process (host workers, calling thread, the runtime's own), per coded "
                                  "symbol of the batch; cycles / instructions / last-level-cache references and misses"}
    payload_ms = None
    if world > 1 and a.full:
        # the containers themselves, once per run (the timed step exchanges the LENGTHS; a deployment that assembles every
        # image's container on every rank would pay this as well): rank r owns the images r, r + world, ...
        local = [Cn.pack([res[i * spi + s][0] for s in range(spi)], {"y": list(leg.shapes1[0])}) for i in range(a.images)]
        P.gather_containers(local, a.images * world, device=coll_dev)  # (the first use of a collective sets up its connections)
        dist.barrier()
        t0 = time.perf_counter()
        allc = P.gather_containers(local, a.images * world, device=coll_dev)
        payload_ms = env.max_over_ranks((time.perf_counter() - t0) * 1e3)
        assert len(allc) == a.images * world and allc[rank] == local[0]
    if a.full and not a.no_extras:
        other = "all-at-once" if a.schedule == "codec" else "codec"
        n_ub = max(3, min(a.steps, 10))
        leg.step(other)
        dt_o, step_ms_o = leg.timed(other, n_ub)
        dt_o = env.max_over_ranks(dt_o)
        extras["upper_bound" if other == "all-at-once" else "as_codec"] = {
            "schedule": other, "value": round(leg.mpix(n_ub, dt_o), 2), "unit": "Mpixels/s",
            "ms_per_step": round(dt_o / n_ub * 1e3, 3), "steps": n_ub, "step_ms": step_ms_o}
        # the whole step on checkpointed streams: EVERY rank (this is the decode path that needs neither decode tables on
        # the bus nor host decoders - the one that scales with GPUs, not with host cores)
        extras["checkpointed"] = leg.checkpointed(a.schedule, a.checkpoint_stride, max(3, min(a.steps, 10)), total_bytes)
        if rank == 0 and world == 1:
            # latency of ONE image (its spi streams): encode in one call, decode stage by stage / in one call
            gmc = leg.gmc

            def one_image(codec: bool):
                y1 = ys[:spi]
                p1 = [t[:spi] for t in (ss, ms, ws)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = gmc.compress_batch(y1, *p1)
                if codec:
                    for s in range(spi):
                        gmc.decompress_batch([r[s][0][0]], [r[s][0][1]], [r[s][0][2]], *[t[s:s + 1] for t in p1])
                else:
                    gmc.decompress_batch([x[0][0] for x in r], [x[0][1] for x in r], [x[0][2] for x in r], *p1)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            reps = 30 if a.workload == "kodak24" else 3
            _lib.set_profiling(local_rank, False)  # (no timing events around the kernels of these calls: nothing reads them; on again below)
            wide = None
            if env.l3_cpus:  # the calling thread on its own L3 domain, as in the timed regions (Leg.timed); opened again below
                try:
                    wide = os.sched_getaffinity(0)
                    os.sched_setaffinity(0, env.l3_cpus)
                except OSError:
                    wide = None
            for codec in (True, False):
                one_image(codec)
            extras["latency_ms"] = {"images": 1, "streams": spi,
                                    "as_codec": round(float(np.median([one_image(True) for _ in range(reps)])), 3),
                                    "all_at_once": round(float(np.median([one_image(False) for _ in range(reps)])), 3)}
            # the same image with checkpointed streams
            gmc_ck = GaussianMixtureConditional(K=4, mode=a.mode, checkpoint_stride=a.checkpoint_stride)
            gmc = gmc_ck
            r_ck = gmc_ck.compress_batch(ys[:spi], *[t[:spi] for t in (ss, ms, ws)])
            assert all(bytes(x[0][0]) == bytes(y_[0][0]) for x, y_ in zip(r_ck, res[:spi])), "checkpointed streams differ"
            for codec in (True, False):
                one_image(codec)
            extras["latency_ms"]["as_codec_checkpointed"] = round(float(np.median([one_image(True) for _ in range(reps)])), 3)
            extras["latency_ms"]["all_at_once_checkpointed"] = round(float(np.median([one_image(False) for _ in range(reps)])), 3)
            extras["latency_ms"]["checkpoint_bytes"] = int(sum(16 * len(x[0][0].ckpt) for x in r_ck))
            extras["latency_ms"]["checkpoint_stride"] = a.checkpoint_stride
            if a.workload == "kodak24" and a.checkpoint_stride != 256:
                # ... and with a note every 256 symbols: a single bitstream then has enough segments for the GPU decoder
                gmc = GaussianMixtureConditional(K=4, mode=a.mode, checkpoint_stride=256)
                r_256 = gmc.compress_batch(ys[:spi], *[t[:spi] for t in (ss, ms, ws)])
                one_image(True)
                extras["latency_ms"]["as_codec_checkpointed_stride_256"] = round(float(np.median([one_image(True) for _ in range(reps)])), 3)
                extras["latency_ms"]["checkpoint_bytes_stride_256"] = int(sum(16 * len(x[0][0].ckpt) for x in r_256))
            extras["latency_ms"]["calling_thread_on_its_l3_domain"] = wide is not None  # (as in the timed regions: plan_l3)
            if wide is not None:
                os.sched_setaffinity(0, wide)
            _lib.set_profiling(local_rank, True)
            if a.diag and a.diag_steps > 0:
                threads = _lib.lib().fgmm_ctx_threads(_lib.ctx(local_rank))
                if a.diag_pools:
                    cfgs = [x for x in a.diag_pools.split(",") if x]
                else:
                    by_quota = max(1, int(_lib.host_cpu_budget()["cpus"] // _lib.ranks_on_node()))
                    cfgs = [str(threads)] + ([str(by_quota)] if by_quota != threads else [])
                try:
                    extras["step_diag"] = D.step_diag(leg, a.schedule, a.diag_steps, cfgs)
                except Exception as e:  # pragma: no cover - a diagnostic must not cost the run its line
                    extras["step_diag"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
            # one host thread instead of the pool: what the GPU path is worth per host core
            threads = _lib.lib().fgmm_ctx_threads(_lib.ctx(local_rank))
            _lib.set_threads(local_rank, 1)
            leg.step(a.schedule)
            n1 = 3
            dt1, _ = leg.timed(a.schedule, n1)
            extras["one_host_thread"] = {"value": round(a.images * pix_per_image * n1 / dt1 / 1e6, 2), "unit": "Mpixels/s",
                                         "ms_per_step": round(dt1 / n1 * 1e3, 2), "host_threads": 1}
            _lib.set_threads(local_rank, threads)

    # ---- BASELINE configs[2] and configs[4] in the default line (N = 1): a few steps each, so that the driver's own run witnesses them
    sublegs = a.full and world == 1 and a.workload == "kodak24" and a.mode == "polya" and not f16 and not a.no_sublegs and not a.no_extras and not leg.real
    if sublegs:
        t_sub = time.perf_counter()
        modes = {}
        for m in ("as", "logistic"):
            lm = leg.with_mode(m)
            lm.step(a.schedule)
            n_m = 8  # (80 ms per mode: three steps were too few to stand a co-tenant's surge)
            dt_m, st_m = lm.timed(a.schedule, n_m, record=True)
            res_m = lm.check_last()
            nc_m, sym_ms_m, ach_m = lm.symtab_roofline(res_m)
            modes[m] = {"value": round(lm.mpix(n_m, dt_m), 2), "unit": "Mpixels/s", "steps": n_m, "ms_per_step": round(dt_m / n_m * 1e3, 3),
                        "step_ms": st_m["all"], "bitstream_bytes": sum(len(r[0][0]) for r in res_m),
                        "symtab": {"launch_ms": round(sym_ms_m, 4), "achieved": round(ach_m, 1), "unit": "GB/s", "frac": round(ach_m / HBM_PEAK_GBS, 4)},
                        "tab_kernels_ms_per_step": round(float(np.mean(lm.k_tab)), 4),
                        "reference_md5": ka1_check(lm, res_m)}
            modes[m]["_bytes"] = [bytes(r[0][0]) for r in res_m]
        if not a.no_cpu_baseline:  # the reference's encoder under each mode on ALL 48 streams, bytes against bytes
            try:
                rb = reference_bytes_of_modes({m: modes[m]["_bytes"] for m in modes}, rank, leg.shapes1, spi, f16)
                for m in modes:
                    modes[m]["reference_bytes_equal"] = rb[m]
            except Exception as e:  # pragma: no cover
                for m in modes:
                    modes[m]["reference_bytes_equal"] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
        for m in modes:
            del modes[m]["_bytes"]
        extras["modes"] = modes
        try:
            extras["head_fused"] = head_leg(leg, local_rank)
        except Exception as e:  # pragma: no cover - the headline must not die of a sub-leg
            extras["head_fused"] = {"value": None, "error": f"{type(e).__name__}: {str(e)[:300]}"}
        try:
            el = Leg(env, "elic4k", ELIC_IMAGES, "polya", True, keep_host_images=1, distinct=ELIC_DISTINCT)
            for _ in range(2):  # (the first steps grow the pinned receive area to this workload's 2.8 GB per stage)
                el.step("codec")
            dt_e, st_e = el.timed("codec", 3, record=True)
            res_e = el.check_last()
            nc_e, sym_ms_e, ach_e = el.symtab_roofline(res_e)
            tb_e = float(np.mean(el.tab_bytes))
            elic = {"config": {"workload": "elic4k", "images_per_gpu": ELIC_IMAGES, "distinct_images": ELIC_DISTINCT, "param_dtype": "f16", "schedule": "codec", "decode_calls_per_step": el.spi,
                               "coded_symbols_per_gpu": nc_e, "approx_mode": "polya"},
                    "value": round(el.mpix(3, dt_e), 2), "unit": "Mpixels/s", "steps": 3, "ms_per_step": round(dt_e / 3 * 1e3, 3), "step_ms": st_e["all"],
                    "symtab": {"launch_ms": round(sym_ms_e, 4), "achieved": round(ach_e, 1), "unit": "GB/s", "frac": round(ach_e / HBM_PEAK_GBS, 4),
                               "bytes_per_symbol": el.bytes_per_symbol, "loads": "16 B per lane and plane (8 positions per lane)",
                               "valu": symtab_valu_roof("elic4k", "polya", True, nc_e, sym_ms_e)},
                    "decode_table_bytes_per_latent": round(tb_e / max(1, nc_e), 2),
                    "checkpointed": el.checkpointed("codec", a.checkpoint_stride, 3, sum(len(r[0][0]) for r in res_e))}
            if not a.no_cpu_baseline:  # the reference's own coder on ONE of these images, one pass
                kind, prepare, code = _cpu_coder()
                prepared = [prepare(s) for s in el.host[:el.spi]]
                t0 = time.perf_counter()
                ref_b = []
                for st in prepared:
                    got, want, b = code(st)
                    ref_b.append(b)
                    assert np.array_equal(got, want)
                t_ref = time.perf_counter() - t0
                eq = sum(bytes(res_e[k][0][0]) == bytes(rb_) for k, rb_ in enumerate(ref_b))
                elic["reference_bytes_equal"] = {"streams": len(ref_b), "equal": eq, "kind": kind,
                                                 "note": "image 0: five channel groups x two halves, the 64- and 192-channel groups included"}
                elic["cpu_baseline"] = {"value": round(el.pix_per_image / t_ref / 1e6, 3), "unit": "Mpixels/s", "cores": 1, "kind": kind,
                                        "sample": f"1 image x {el.spi} streams ({sum(len(p[-1]) for p in prepared)} symbols), encode+decode, one pass, {t_ref * 1e3:.0f} ms"}
            del el
            torch.cuda.empty_cache()
            _lib.trim(local_rank)
            extras["elic4k"] = elic
        except Exception as e:  # pragma: no cover - the headline must not die of a sub-leg (e.g. out of memory on a shared card)
            extras["elic4k"] = {"value": None, "error": f"{type(e).__name__}: {str(e)[:300]}"}
        extras["sublegs_s"] = round(time.perf_counter() - t_sub, 1)

    if rank == 0:
        ms_per_step = dt / a.steps * 1e3
        value = world * a.images * pix_per_image * a.steps / dt / 1e6
        _, sym_ms, achieved = leg.symtab_roofline(res)
        tab_ms, n_edges, tbytes = float(np.mean(leg.k_tab)), float(np.mean(leg.edges)), float(np.mean(leg.tab_bytes))
        traffic, traffic_src = pmc_traffic(a.workload, a.mode, f16, a.images)
        tab_alg_bytes = n_coded * (12 * (2 if f16 else 4)) + tbytes  # parameters in, headers + block offsets + rows out
        slots = n_edges * TAB_SLOTS_PER_EDGE[a.mode]
        budget = _lib.host_cpu_budget()
        # host memory traffic of the plain path per rank: every table byte is written once by the DMA and read once by a host
        # worker (encode tables + decode tables), per second of stepping
        host_traffic = 2.0 * (enc_table_bytes + tbytes) / (ms_per_step * 1e-3) / 1e9
        note = (f"{host_threads} host rANS workers for this GPU: min(affinity {budget.get('affinity')}, cgroup quota "
                f"{budget.get('quota')}) / {_lib.ranks_on_node()} rank(s) on the node, times FGMM_WORKERS_PER_CPU (default 3, up to the rank's share of "
                f"the mask) where the quota, a limit on CPU time, is the smaller - the workers sleep most of a call; at most 48")
        if host_threads < 8:
            note += ("; FEWER THAN 8 WORKERS: the plain (table) path is host-bound by configuration here - its rate follows the "
                     "workers (one_host_thread x workers), the `checkpointed` leg does not need them")
            print(f"[bench] {note}", file=sys.stderr)
        out = {
            # BASELINE.json's metric, verbatim: `value` is its Mpixels/s half, the `roofline` object its GMM-CDF HBM half
            "metric": "encode+decode Mpixels/s (Kodak, K=4 N=192) + GMM-CDF HBM GB/s vs roofline" if a.workload == "kodak24"
            else "encode+decode Mpixels/s (ELIC 4K, K=4, fp16 params)",
            "value": round(value, 2),
            "unit": "Mpixels/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "step_ms": step_ms,  # rank 0's per-step wall times of the timed region + the cgroup's throttling meanwhile
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",  # the CDF arithmetic; parameter planes: config.param_dtype
            "data": "real-latents" if leg.real else "synthetic",
            "config": {"workload": a.workload, "schedule": a.schedule,
                       "decode_calls_per_step": spi if a.schedule == "codec" else 1, "images_per_gpu": a.images,
                       "streams_per_gpu": n_streams, "stream_shapes": leg.shapes, "stacked_input": leg.stacked, "K": 4, "approx_mode": a.mode,
                       "param_dtype": "f16" if f16 else "f32",
                       "coded_symbols_per_gpu": n_coded, "bitstream_bytes_per_gpu": total_bytes,
                       "host_threads_per_gpu": host_threads, "host_cpu_budget": budget,
                       "ranks_on_node": _lib.ranks_on_node(), "numa": numa, "l3": l3_note,
                       "host_mem_traffic_GBps_per_rank": round(host_traffic, 1), "cpu_budget_note": note,
                       "one_device_rehearsal": one_device,
                       "parallelism": f"images sharded over {world} GPU(s)"},
            "roofline": {"bound": "hbm", "kernel": "symtab_kernel (encode-side GMM-CDF)",
                         "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_note": "recorded PMC measurement of this workload (file in traffic_source), not collected in this run",
                         "launch_ms": round(sym_ms, 4), "bytes_per_launch": n_coded * leg.bytes_per_symbol,
                         "bytes_per_symbol": leg.bytes_per_symbol,
                         "frac_of_measured_copy_bandwidth": round(achieved / HBM_COPY_GBS, 4), "measured_copy_bandwidth": HBM_COPY_GBS,
                         # the same launch against the kernel's other roof (VALU issue): it is balanced between the two at fp32 planes
                         "valu": symtab_valu_roof(a.workload, a.mode, f16, n_coded, sym_ms)},
            # the decode-side table kernel against BOTH of its rooflines: VALU issue and HBM
            "roofline_decode": {"kernel": "tab_kernel (decode-side edge tables, all launches of a step)", "bound": "valu",
                                "ms_per_step": round(tab_ms, 4), "edges_evaluated": int(n_edges),
                                "mean_edges_per_latent": round(n_edges / max(n_coded, 1), 2),
                                "issue_slots_per_edge": round(TAB_SLOTS_PER_EDGE[a.mode], 1),
                                "valu_achieved_Tslots": round(slots / (tab_ms * 1e-3) / 1e12, 2),
                                "valu_peak_Tslots": round(VALU_PEAK_LANE_SLOTS / 1e12, 1),
                                "valu_frac": round(slots / (tab_ms * 1e-3) / VALU_PEAK_LANE_SLOTS, 4),
                                "hbm_bytes_algorithmic": int(tab_alg_bytes),
                                "hbm_achieved": round(tab_alg_bytes / (tab_ms * 1e-3) / 1e9, 1),
                                "hbm_frac": round(tab_alg_bytes / (tab_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                "note": "in situ: the launches share the GPU with the table copies; valu_frac counts the issue slots of the edge "
                                        "evaluation alone (what the reference's arithmetic needs) - `alone` counts every VALU instruction the kernel issues",
                                "alone": tab_kernel_alone() if a.workload == "kodak24" and a.mode == "polya" and not f16 else None},
            "kernels_ms": {"symtab": round(sym_ms, 4), "tab_kernels_all_launches": round(tab_ms, 4),
                           "quant_stats": round(float(np.mean(leg.k_qs)), 4)},
            # what crosses PCIe per step and rank (the decode-side tables are the longest leg of a step)
            "pcie": {"encode_tables_bytes": enc_table_bytes, "decode_tables_bytes": int(tbytes),
                     "decode_table_bytes_per_latent": round(tbytes / max(1, n_coded), 2), "bitstream_bytes": total_bytes},
            "ranks": {"backend": backend, "rccl_ranks": world if backend == "nccl" else 0,
                      "ms_per_step": [round(t / a.steps * 1e3, 3) for t in per_rank],
                      "host_threads_per_gpu": per_rank_threads, "result_checked_ranks": checked,
                      # the lengths' all-gather per step: issued after the encode call, waited for at the end of the step -
                      # `exposed` is what the step pays, `total` how long the collective was in flight (hidden behind the decode)
                      "allgather_ms": ({"issue": round(float(np.mean([t[0] for t in leg.t_gather])), 4), "exposed": round(float(np.mean([t[1] for t in leg.t_gather])), 4),
                                        "total_in_flight": round(float(np.mean([t[2] for t in leg.t_gather])), 3),
                                        "form": "one preallocated all_gather_into_tensor, async_op"} if leg.t_gather else None),
                      "process_group_note": pg_note,
                      "allgather_payload_ms": round(payload_ms, 4) if payload_ms is not None else None},
            "reference_md5": ka1,
        }
        if dumped is not None:
            out["outputs_dumped"] = {"dir": a.dump_outputs, "elements": dumped}
        out.update(extras)
        out["host_throttled"] = bool(step_ms.get("nr_throttled", 0))
        if out["host_throttled"]:
            print(f"[bench] THE CGROUP'S CPU CONTROLLER THROTTLED THIS PROCESS DURING THE TIMED REGION ({step_ms.get('cpu_throttled')}): `value` "
                  f"measures the quota, not the path - fewer host workers (--host-threads, FGMM_WORKERS_PER_CPU) or a larger quota", file=sys.stderr)
        if a.full and world == 1 and not a.no_cpu_baseline:
            cb = cpu_baseline(leg.host, leg.shapes1, pix_per_image, spi, rank, f16, hip_bytes=[bytes(r[0][0]) for r in res], from_seeds=not leg.real,
                              extras=a.baseline_extras)
            if "one_host_thread" in extras and cb.get("value"):
                cb["per_thread_speedup"] = round(extras["one_host_thread"]["value"] / cb["value"], 1)
            if cb.get("all_cores", {}).get("value"):
                cb["speedup_vs_all_cores"] = round(value / cb["all_cores"]["value"], 1)
            if cb.get("value"):
                # THROUGHPUT: the whole GPU path (24 images in flight, all host workers) over ONE reference thread coding image after
                # image.  north_star's >= 100x is worded on LATENCY: that ratio is latency_ms.speedup_plain (one image through the
                # reference's interface) and its floor is the sequential rANS decoder, see latency_ms.note
                cb["throughput_speedup"] = round(value / cb["value"], 1)
            if "latency_ms" in out:
                lt = out["latency_ms"]
                lt["reference_cpu"] = cb["ms_per_image"]
                # one image, the reference's coder on one core over this path: through the reference's interface alone
                # (plain streams), and with checkpointed streams (the same bytes + out-of-band notes: not the reference's format)
                lt["speedup_plain"] = round(cb["ms_per_image"] / lt["as_codec"], 1)
                ck_key = "as_codec_checkpointed_stride_256" if "as_codec_checkpointed_stride_256" in lt else "as_codec_checkpointed"
                lt["speedup_checkpointed"] = round(cb["ms_per_image"] / lt[ck_key], 1)
                lt["speedup_checkpointed_basis"] = ck_key
                lt["note"] = ("north_star's >= 100x is stated on one-image latency: speedup_plain is that number through the reference's own "
                              "interface (byte-identical single rANS streams), speedup_checkpointed needs out-of-band notes the reference's "
                              "format does not have.  100x is out of reach with byte-identical streams: a 129 k-symbol stream encodes "
                              "in 0.33 ms and decodes in 1.1-1.5 ms on one core (9-11 ns per symbol, a dependent chain), and the codec's two "
                              "halves decode one after the other: 0.5 + 2 x 1.5 ms against the reference's 42 ms is 12x at best")
            out["cpu_baseline"] = cb
        out["bench_s"] = round(time.perf_counter() - t_bench0, 1)  # this process, argument parsing to here (imports excluded)
        emit(out, detail=a.full)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
