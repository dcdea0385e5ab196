"""Helper of tests/golden/make_golden_dropin.py: run the REFERENCE'S OWN Python EntropyBottleneck (imported in place from
the reference's source tree, named by $REF as in oracle/Makefile - only present in the build container) on top of either the
reference's compiled extensions (oracle/_ref) or this repo's drop-in modules, and print what it produced.  With `--record`
every call the Python layer makes into the two compiled modules (pmf_to_quantized_cdf, RansEncoder.encode_with_indexes,
RansDecoder.decode_with_indexes) is printed as well, with its arguments and its result: tests/test_reference_dropin_cpu.py
replays them on the drop-in modules without the reference."""
import importlib.util
import json
import os
import sys
import sysconfig
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _recording(ans, cxx, calls):
    """proxies of the two modules that log (method, args, result) of every call the Python layer makes"""
    def rec(name, fn):
        def call(*args):
            out = fn(*args)
            calls.append({"call": name, "args": [a.hex() if isinstance(a, bytes) else a for a in args],
                          "result": out.hex() if isinstance(out, bytes) else list(out)})
            return out
        return call

    class Encoder:
        def __init__(self):
            self._e = ans.RansEncoder()
            self.encode_with_indexes = rec("encode_with_indexes", self._e.encode_with_indexes)

    class Decoder:
        def __init__(self):
            self._d = ans.RansDecoder()
            self.decode_with_indexes = rec("decode_with_indexes", self._d.decode_with_indexes)

    ans_p = types.ModuleType("compressai.ans")
    ans_p.RansEncoder, ans_p.RansDecoder = Encoder, Decoder
    cxx_p = types.ModuleType("compressai._CXX")
    cxx_p.pmf_to_quantized_cdf = rec("pmf_to_quantized_cdf", cxx.pmf_to_quantized_cdf)
    return ans_p, cxx_p


def main(backend: str, record: bool = False):
    import torch

    if backend == "ref":
        from oracle import oracle as O

        ans = O.ref_ans()
        cxx = O.ref_cxx()
    else:
        from flashgmm_amd import ans, ops

        cxx = types.ModuleType("compressai._CXX")
        cxx.pmf_to_quantized_cdf = ops.pmf_to_quantized_cdf
    calls = []
    if record:
        ans, cxx = _recording(ans, cxx, calls)
    pkg = types.ModuleType("compressai")
    pkg.__path__ = [os.path.join(os.environ["REF"], "compressai")]
    pkg.available_entropy_coders = lambda: ["ans"]
    pkg.get_entropy_coder = lambda: "ans"
    pkg.ans = ans
    sys.modules["compressai"] = pkg
    sys.modules["compressai.ans"] = ans
    sys.modules["compressai._CXX"] = cxx
    from compressai.entropy_models.entropy_models import EntropyBottleneck

    torch.manual_seed(7)
    eb = EntropyBottleneck(24)
    eb.update(force=True)
    z = torch.randn(2, 24, 8, 12) * 3
    z[0, 3, 2, 2] = 500.0   # far outside the table: bypass
    z[1, 5, 1, 1] = -321.0
    strings = eb.compress(z)
    z_hat = eb.decompress(strings, z.size()[2:])
    out = {"cdf": eb._quantized_cdf.tolist(), "strings": [s.hex() for s in strings],
           "z_hat_sum": float(z_hat.double().sum()), "z_hat_max": float(z_hat.max())}
    if record:
        out["calls"] = calls
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1], "--record" in sys.argv[2:])
