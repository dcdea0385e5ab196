"""Runs the compiled reference (oracle/_ref: the unmodified `compressai.ans`, and `_fast_gmm_cdf<4>` through libref_probe) on
cases of tests/edge_corpus.py, in a child process of its own: the reference reads APPROX_MODE once per process
(rans_interface.cpp:99-117), so every mode is a fresh process.  The child never initialises a GPU.

    run(mode, cases, tmp_dir) -> {case name: {field: array}}

`cases` maps a name to a dict of numpy arrays with a "kind":
    "cdf"     v, s, m, w            -> c1, c2      (_fast_gmm_cdf<4> at v - 0.5, v + 0.5)
    "cdf_x"   x1, x2, s, m, w       -> c1, c2      (at arbitrary abscissae)
    "encode"  v, s, m, w            -> bytes       (RansEncoder.encode_with_indexes_gmm)
    "decode"  bytes, s, m, w, max_bs -> syms, past_end
    "pmf"     pmf                   -> cdf, error  (compressai._CXX.pmf_to_quantized_cdf, precision 16)

The reference's decoder has no end-of-stream check: on a short or corrupt stream it reads past the end of its buffer.  The
worker gives it the stream followed by zero words (the answer reported, `syms`), and again followed by other words: if the
answers differ - on the real rows or on one ordinary row appended after them (whose symbol is decided by the state the real
rows leave, before it reads anything itself) - its result depended on words past the end of the stream, and `past_end` is 1 (the reference has no answer there; a decoder with an end check must fail).
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"polya": 0, "as": 1, "logistic": 2}
_PAD_B = 0x5A5A5A5A  # no bypass marker (cf 0xFFFF) and no long nibble runs: a padded read never runs away


def _save(path, cases):
    flat = {}
    for name, c in cases.items():
        assert "/" not in name
        for k, v in c.items():
            flat[f"{name}/{k}"] = np.asarray(v)
    np.savez(path, **flat)


def _load(path):
    out = {}
    with np.load(path, allow_pickle=False) as z:
        for key in z.files:
            name, k = key.split("/", 1)
            out.setdefault(name, {})[k] = z[key]
    return out


def run(mode: str, cases: dict, tmp_dir, timeout: float = 600.0) -> dict:
    """evaluate `cases` with the reference in APPROX_MODE = mode, in a fresh child process"""
    tmp_dir = str(tmp_dir)
    src, dst = os.path.join(tmp_dir, f"ref_in_{mode}.npz"), os.path.join(tmp_dir, f"ref_out_{mode}.npz")
    _save(src, cases)
    env = dict(os.environ, APPROX_MODE=str(MODES[mode]), HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env.pop("USE_SIMD", None)  # the reference's default: the SIMD path
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, src, dst], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"reference worker ({mode}) exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return _load(dst)


def _child(mode: str, src: str, dst: str) -> None:
    sys.path.insert(0, ROOT)
    import torch

    from oracle import oracle as O

    ans, probe = O.ref_ans(), O.ref_probe()
    assert probe.ref_probe_mode() == MODES[mode] | 0x100, hex(probe.ref_probe_mode())  # this mode, the SIMD path
    cxx = None
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    ordinary = (np.full((1, 4), 1.0, np.float32), np.zeros((1, 4), np.float32), np.full((1, 4), 0.25, np.float32))

    def decode(enc: bytes, s, m, w, max_bs, pad_word):
        n = s.shape[0]
        s2, m2, w2 = (np.concatenate([a, o]) for a, o in zip((s, m, w), ordinary))
        pad = np.full(8 * (n + 1) + 64, pad_word, np.uint32).tobytes()
        return ans.RansDecoder().decode_with_indexes_gmm(enc + pad, t(s2), t(m2), t(w2), int(max_bs)).numpy()

    out = {}
    for name, c in _load(src).items():
        kind = str(c["kind"])
        if kind == "cdf":
            c1, c2 = O.ref_gmm_cdf(probe, c["v"], c["s"], c["m"], c["w"])
            out[name] = {"c1": c1, "c2": c2}
        elif kind == "cdf_x":
            c1, c2 = O.ref_gmm_cdf_x(probe, c["x1"], c["x2"], c["s"], c["m"], c["w"])
            out[name] = {"c1": c1, "c2": c2}
        elif kind == "encode":
            b = ans.RansEncoder().encode_with_indexes_gmm(t(c["v"].astype(np.int32)), t(c["s"]), t(c["m"]), t(c["w"]), 0)
            out[name] = {"bytes": np.frombuffer(b, np.uint8)}
        elif kind == "decode":
            enc, n = c["bytes"].tobytes(), c["s"].shape[0]
            a = decode(enc, c["s"], c["m"], c["w"], c["max_bs"], 0)
            b = decode(enc, c["s"], c["m"], c["w"], c["max_bs"], _PAD_B)
            out[name] = {"syms": a[:n], "past_end": np.int32(not np.array_equal(a, b))}
        elif kind == "pmf":
            if cxx is None:
                cxx = O.ref_cxx()
            try:
                cdf, err = np.asarray(cxx.pmf_to_quantized_cdf([float(p) for p in c["pmf"]], 16), np.int64), 0
            except (ValueError, RuntimeError):  # std::domain_error
                cdf, err = np.zeros(0, np.int64), 1
            out[name] = {"cdf": cdf, "error": np.int32(err)}
        else:
            raise ValueError(kind)
    _save(dst, out)


if __name__ == "__main__":
    _child(*sys.argv[1:4])
