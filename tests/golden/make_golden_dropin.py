#!/usr/bin/env python3
"""The drop-in fixture from the REAL reference (build container only; oracle/_ref built by oracle/Makefile).

    REF=<the reference's source tree> python tests/golden/make_golden_dropin.py

Writes tests/golden/g9_dropin.json for tests/test_reference_dropin_cpu.py: the reference's own Python `EntropyBottleneck`
(imported in place from $REF by tests/dropin_worker.py) is run once over the reference's compiled extensions, with every
call it makes into them recorded - `pmf_to_quantized_cdf` (update(): one per channel), `RansEncoder.encode_with_indexes`
(compress()) and `RansDecoder.decode_with_indexes` (decompress()), arguments and result - and once over this repo's drop-in
`ans` / `pmf_to_quantized_cdf`; both runs must agree before anything is written.  The fixture is data: the calls' plain
arguments and results (lists of numbers, bitstreams as hex) and what the Python layer returned; the test replays the calls
on the drop-in modules, so it needs neither the reference's Python nor its extensions."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(ROOT, "tests", "dropin_worker.py")


def run(*args):
    r = subprocess.run([sys.executable, WORKER, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout[r.stdout.index("{"):])


def main():
    ref_root = os.environ.get("REF", "")
    assert os.path.isdir(os.path.join(ref_root, "compressai")), "set REF to the reference's source tree (build container only)"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle", "ref", f"REF={ref_root}"])
    ref, got = run("ref", "--record"), run("fgmm")
    calls = ref.pop("calls")
    assert got == ref, "the drop-in modules under the reference's EntropyBottleneck differ from its own extensions"
    assert ref["z_hat_max"] == 500.0  # (the bypass of an out-of-table value was exercised)
    kinds = [c["call"] for c in calls]
    assert kinds.count("encode_with_indexes") == kinds.count("decode_with_indexes") == 2 and kinds.count("pmf_to_quantized_cdf") == 24
    out = {"note": "tests/golden/make_golden_dropin.py: the reference's EntropyBottleneck(24) (seed 7) over its own compiled extensions: "
                   "every call into them, and what update() / compress() / decompress() returned",
           "calls": calls, "result": ref}
    path = os.path.join(HERE, "g9_dropin.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
