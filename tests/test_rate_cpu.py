"""CPU (-m "not gpu"): the coded size of an encode-side table without coding it - the host building blocks fgmm_symtab_bits and
fgmm_rate_stream_bytes (include/flashgmm_amd.h section 3b) against numpy float64 and against the lengths of the reference's
streams (the oracle's encoder, tests/golden)."""
import json
import os

import numpy as np
import pytest

from flashgmm_amd import _lib
from tests import synth as T
from tests import rate_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = ["polya", "as", "logistic"]


def _g3_cases():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.g3_cases()


def test_per_symbol_cost_exhaustive():
    """every range 1 .. 65535: within one unit (2^-24 bit) of float64, exact at the powers of two, strictly decreasing"""
    L = _lib.lib()
    r = np.arange(1, 65536, dtype=np.uint32)
    bits_q, nb, cost = R.host_bits(L, r << 16, costs=True)
    want = R.ONE * (16.0 - np.log2(r.astype(np.float64)))
    assert np.abs(cost.astype(np.float64) - want).max() <= 1.0
    pow2 = (r & (r - 1)) == 0
    assert pow2.sum() == 16 and np.array_equal(cost[pow2].astype(np.int64), (16 - np.log2(r[pow2]).astype(np.int64)) * R.ONE)
    assert np.all(np.diff(cost.astype(np.int64)) < 0)
    assert nb == 0 and bits_q == int(cost.astype(np.uint64).sum())
    assert cost[0] == 16 * R.ONE  # L[1] = 0


def test_bypass_cost(oracle):
    """16 (the {65535, 1} sentinel) + 4 (the count nibble) + 4 per nibble of the symbol's uint32 bit pattern.  Without `symbols` an entry
    is priced by what fgmm_rans_encode_symtab codes then: its low 16 bits SIGN-EXTENDED to an int32 - the symbol itself whenever
    abs(symbol) < 32768, else whatever that extension gives (32768 -> -32768, 2^31 - 1 -> -1: eight nibbles; -2^31 -> 0: none).

    The symbols are the issue's list.  Its expected figures for 32767 and 32768 read 32 bits; by its own formula, and by the coder, they
    are 36: 0x7FFF and 0x8000 are four nibbles, not three (rans_interface.cpp:529-533 shifts four times).  The last block below holds the
    figure to the coder itself: seven bypass symbols of each value, the length of the stream the reference's flush writes."""
    L = _lib.lib()
    sym = np.array(R.BYPASS_SYMBOLS, np.int64).astype(np.int32)
    packed = (sym.view(np.uint32) & 0xFFFF).astype(np.uint32)  # range 0: the low half carries the low 16 bits of the symbol
    bits_q, nb, cost = R.host_bits(L, packed, sym, costs=True)
    assert (cost.astype(np.int64) // R.ONE).tolist() == R.BYPASS_BITS and not np.any(cost % R.ONE)
    assert nb == len(sym) and bits_q == sum(R.BYPASS_BITS) * R.ONE
    assert [16 + 4 * (1 + R.nibbles(v)) for v in R.BYPASS_SYMBOLS] == R.BYPASS_BITS
    # symbols_or_null = NULL
    _, nb0, cost0 = R.host_bits(L, packed, None, costs=True)
    ext = [int(np.int16(np.uint16(p))) for p in packed]
    assert ext == [0, 1, 15, 16, 32767, -32768, -1, 0, -1]
    assert (cost0.astype(np.int64) // R.ONE).tolist() == [16 + 4 * (1 + R.nibbles(v)) for v in ext] == [20, 24, 24, 28, 36, 52, 52, 20, 52]
    assert nb0 == len(sym)
    # the encoder follows the same rule: the stream it writes without symbols is the stream of the extended ones
    from helpers import host_encode_symtab
    assert host_encode_symtab(L, packed, None) == host_encode_symtab(L, packed, np.array(ext, np.int32))
    # ... and the coder: seven of a kind (7 * cost is at least 4 bits from a multiple of 32 for every cost here)
    for v, want in zip(R.BYPASS_SYMBOLS, R.BYPASS_BITS):
        s7, p7 = np.full(7, v, np.int64).astype(np.int32), np.full(7, v & 0xFFFF, np.uint32)
        stream = oracle.rans_encode_symtab(p7, s7)
        assert stream == host_encode_symtab(L, p7, s7)
        assert 32 < 8 * len(stream) - 7 * want <= 64 and L.fgmm_rate_stream_bytes(7 * want * R.ONE) == len(stream), (v, want, len(stream))


def _streams(oracle):
    """(name, mode, table, symbols, true length) of every stream of item 3"""
    for shape in ((8, 4, 4), (32, 16, 8)):
        for seed in range(12):
            sym, s, m, w, *_ = T.to_coder_inputs(*T.make_latent(seed, *shape, clamp=False, zero_frac=0.2))
            for mode in MODES:
                yield f"synth{shape}/{seed}/{mode}", oracle.symtab(mode, sym, s, m, w), sym, len(oracle.encode_gmm(mode, sym, s, m, w))
    ka = json.load(open(os.path.join(GOLD, "ka1.json")))
    for seed in sorted(ka["polya"], key=int):
        sym, s, m, w, *_ = T.to_coder_inputs(*T.make_latent(int(seed), 192, 32, 24))
        for mode in MODES:
            assert len(sym) == ka[mode][seed]["n"]
            yield f"ka1/{seed}/{mode}", oracle.symtab(mode, sym, s, m, w), sym, ka[mode][seed]["len"]
    gold = json.load(open(os.path.join(GOLD, "g3_small.json")))["cases"]
    for name, (sym, s, m, w) in _g3_cases().items():
        for mode in MODES:
            yield f"g3/{name}/{mode}", oracle.symtab(mode, sym, s, m, w), sym, len(bytes.fromhex(gold[name][mode]["hex"]))


def test_stream_length_identity(oracle):
    """With B the summed cost, the flushed stream has 8 * len - B in (32, 64]; len is a multiple of 4, hence len = 4 * floor((B + 64) / 32).
    Lengths are the reference's: the oracle's encoder, tests/golden/ka1.json, tests/golden/g3_small.json (forced bypass)."""
    L = _lib.lib()
    n = skipped = n_bypass_seen = 0
    for name, packed, sym, true_len in _streams(oracle):
        bits_q, nb = R.host_bits(L, packed, sym)
        n_bypass_seen += nb
        assert nb == int(np.sum((packed >> 16) == 0)), name
        bits = bits_q / R.ONE
        b64 = R.float_bits(packed, sym)
        assert abs(bits - b64) <= len(packed) * 2.0 ** -24 + 1e-6, name  # half a unit per symbol at most, and float64's own sum
        assert 32 < 8 * true_len - bits <= 64, (name, true_len, bits)
        n += 1
        if R.left_out(b64):
            skipped += 1
            continue
        assert L.fgmm_rate_stream_bytes(bits_q) == true_len, (name, true_len, bits)
    assert n == 72 + 15 + 15 and n_bypass_seen > 0
    assert skipped * 10 <= n, f"{skipped} of {n} streams within 0.05 bit of a multiple of 32"


def test_empty_table():
    L = _lib.lib()
    assert R.host_bits(L, np.zeros(0, np.uint32)) == (0, 0)
    assert L.fgmm_rate_stream_bytes(0) == 8
    # the closed form itself, at its edges: 8 * len - B in (32, 64]
    for b, want in ((0, 8), (31, 8), (32, 12), (63, 12), (64, 16)):
        assert L.fgmm_rate_stream_bytes(b << R.Q) == want
        assert L.fgmm_rate_stream_bytes(((b + 1) << R.Q) - 1) == want
