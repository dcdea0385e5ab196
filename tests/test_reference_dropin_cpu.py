"""CPU: the reference's own Python `EntropyBottleneck` must behave identically on this repo's drop-in `ans` /
`pmf_to_quantized_cdf` and on its own compiled extensions.  The Python layer is the same code either way, so what is checked is
every call it makes into the two modules: tests/golden/g9_dropin.json holds them as the reference's extensions answered them
(update(): `pmf_to_quantized_cdf` per channel; compress(): `RansEncoder.encode_with_indexes`, a bypassed out-of-table value
included; decompress(): `RansDecoder.decode_with_indexes` - made by tests/golden/make_golden_dropin.py, which also ran the
reference's Python over the drop-in modules end to end), and each is replayed here on the drop-in modules."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_entropy_bottleneck_on_dropin_modules_equals_reference():
    from flashgmm_amd import ans, ops

    g = json.load(open(os.path.join(HERE, "golden", "g9_dropin.json")))
    calls, ref = g["calls"], g["result"]
    seen = {}
    for c in calls:
        name, args, want = c["call"], c["args"], c["result"]
        seen[name] = seen.get(name, 0) + 1
        if name == "pmf_to_quantized_cdf":    # update(): pmf_to_quantized_cdf rows
            assert ops.pmf_to_quantized_cdf(*args) == want
        elif name == "encode_with_indexes":   # compress(): table rANS bytes, bypass included
            got = ans.RansEncoder().encode_with_indexes(*args)
            assert isinstance(got, bytes) and got.hex() == want
        else:                                 # decompress(): the symbols, the bypassed ones included
            assert name == "decode_with_indexes"
            got = ans.RansDecoder().decode_with_indexes(bytes.fromhex(args[0]), *args[1:])
            assert list(got) == want
    assert seen == {"pmf_to_quantized_cdf": 24, "encode_with_indexes": 2, "decode_with_indexes": 2}
    # the replayed calls are those of the recorded run: its quantised CDFs and its bitstreams
    assert [c["result"] for c in calls if c["call"] == "encode_with_indexes"] == ref["strings"]
    assert [c["result"] for c in calls if c["call"] == "pmf_to_quantized_cdf"] == [row[:len(c["result"])] for row, c in zip(
        ref["cdf"], [c for c in calls if c["call"] == "pmf_to_quantized_cdf"])]
    assert ref["z_hat_max"] == 500.0
