// fgmm_rate_host.cpp — the coded size of an encode-side symbol table WITHOUT coding it: host side, integer only.
//
// rANS with 16-bit frequencies spends 16 - log2(range) bits on a coded symbol; the reference's bypass escape
// (rans_interface.cpp:513-552) spends 16 (the {65535, 1} sentinel) + 4 (the count nibble) + 4 per nibble of the symbol's
// uint32 bit pattern.  The encoder's state starts at 2^31, ends in [2^31, 2^63) and is flushed as 8 bytes, so a stream of
// B = sum(cost) bits is 8 * len - B in (32, 64] bits long and, len being a multiple of 4, len = 4 * floor((B + 64) / 32)
// (include/flashgmm_amd.h, section 3b).  Costs are fixed point, 2^-FGMM_RATE_Q bit, summed in uint64: no order, no rounding.
//
// The table L[r] = round(2^24 * log2 r) is built here once - by the integer square-and-compare recurrence, so that it does
// not depend on a libm - and is what BOTH sides price a range with: fgmm_symtab_bits below gathers from it, the context
// uploads it and the kernels of fgmm_rate.hip gather from the copy (fgmm_estimate.cpp).
#include <mutex>

#include "../../include/flashgmm_amd.h"
#include "fgmm_internal.h"

namespace fgmm {

namespace {
uint32_t g_rate_log2[65536];
std::once_flag g_rate_once;

// 2^40 * log2(r), truncated, r >= 1: the integer part is the position of r's leading bit; every fractional bit is one squaring
// of the mantissa m in [1, 2) (Q1.63) - m^2 >= 2 gives a 1 and halves it.  A truncated squaring lowers log2 m by less than
// 2^-62, and what squaring j loses weighs 2^-j in the result: 40 bits come out right to 2^-56.  Exact for powers of two.
uint64_t log2_q40(uint32_t r) {
  const int e = 31 - __builtin_clz(r);
  uint64_t m = (uint64_t)r << (63 - e);
  uint64_t frac = 0;
  for (int i = 0; i < 40; ++i) {
    const unsigned __int128 top = ((unsigned __int128)m * m) >> 63; // Q2.63
    const bool one = (uint64_t)(top >> 64) != 0;
    frac = (frac << 1) | (one ? 1u : 0u);
    m = one ? (uint64_t)(top >> 1) : (uint64_t)top;
  }
  return ((uint64_t)e << 40) | frac;
}
void init_rate_log2() {
  g_rate_log2[0] = 0; // (range 0 is the bypass escape: never looked up)
  for (uint32_t r = 1; r < 65536; ++r) g_rate_log2[r] = (uint32_t)((log2_q40(r) + (1ull << (39 - FGMM_RATE_Q))) >> (40 - FGMM_RATE_Q));
}
} // namespace

const uint32_t *rate_log2_table() {
  std::call_once(g_rate_once, init_rate_log2);
  return g_rate_log2;
}

} // namespace fgmm

extern "C" {

int fgmm_symtab_bits(const uint32_t *packed, const int32_t *symbols_or_null, int64_t n, uint32_t *cost_q_or_null, uint64_t *bits_q_out,
                     int64_t *n_bypass_out) {
  if (n < 0 || (n > 0 && !packed)) return FGMM_ERR_INVALID;
  const uint32_t *L = fgmm::rate_log2_table();
  uint64_t bits = 0;
  int64_t nb = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bool bypass = (packed[i] >> 16) == 0;
    const uint32_t c = fgmm::rate_cost_q(packed[i], symbols_or_null ? symbols_or_null[i] : fgmm::rate_entry_symbol(packed[i]), L);
    if (cost_q_or_null) cost_q_or_null[i] = c;
    bits += c;
    nb += bypass;
  }
  if (bits_q_out) *bits_q_out = bits;
  if (n_bypass_out) *n_bypass_out = nb;
  return FGMM_OK;
}

uint64_t fgmm_rate_stream_bytes(uint64_t bits_q) { return fgmm::rate_stream_bytes(bits_q); }

} // extern "C"
