"""Shared by tests/test_rate_cpu.py and tests/test_gpu_rate.py: the size estimate's reference side.

The float64 restatement of a table's cost (numpy, independent of the library's fixed-point table), the rule for the few streams
whose length the closed form may miss by 4 bytes, and thin wrappers over the library's host functions."""
from __future__ import annotations

import ctypes as C

import numpy as np

Q = 24
ONE = 1 << Q
BYPASS_SYMBOLS = [0, 1, 15, 16, 32767, 32768, -1, -2 ** 31, 2 ** 31 - 1]
BYPASS_BITS = [20, 24, 24, 28, 36, 36, 52, 52, 52]  # 16 + 4 * (1 + nibbles): 32767 = 0x7FFF and 32768 = 0x8000 are FOUR nibbles


def nibbles(v: int) -> int:
    """nibbles of the symbol's uint32 bit pattern up to its leading one (rans_interface.cpp:524-551): 0 for 0, 8 for a negative symbol"""
    return ((int(v) & 0xFFFFFFFF).bit_length() + 3) // 4


def float_bits(packed, symbols) -> float:
    """B = sum of the costs in float64, from the table alone: 16 - log2 r per coded entry, 16 + 4 (1 + nib) per bypass entry"""
    packed = np.asarray(packed, np.uint32)
    r = (packed >> 16).astype(np.float64)
    coded = r > 0
    b = float(np.sum(16.0 - np.log2(r[coded])))
    for v in np.asarray(symbols, np.int64)[~coded]:
        b += 16 + 4 * (1 + nibbles(v))
    return b


def left_out(b: float) -> bool:
    """The only streams whose predicted length need not be the true one: B within 0.05 bit of a multiple of 32 (the coder's state
    departs from the ideal x * 2^16 / r by up to a relative 2^-15 per symbol; 0.05 bit is far more than the streams here accumulate)"""
    m = b % 32.0
    return min(m, 32.0 - m) < 0.05


def host_bits(lib, packed, symbols=None, costs=False):
    """fgmm_symtab_bits -> (bits_q, n_bypass[, cost_q uint32[n]])"""
    packed = np.ascontiguousarray(packed, np.uint32)
    n = len(packed)
    sp = None
    if symbols is not None:
        symbols = np.ascontiguousarray(symbols, np.int32)
        assert len(symbols) == n
        sp = symbols.ctypes.data_as(C.c_void_p)
    cost = np.empty(n, np.uint32) if costs else None
    bits, nb = C.c_uint64(), C.c_int64()
    rc = lib.fgmm_symtab_bits(packed.ctypes.data_as(C.c_void_p), sp, n, cost.ctypes.data_as(C.c_void_p) if costs else None, C.byref(bits), C.byref(nb))
    assert rc == 0, rc
    return (bits.value, nb.value, cost) if costs else (bits.value, nb.value)
