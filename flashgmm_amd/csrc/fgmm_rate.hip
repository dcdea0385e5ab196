// fgmm_rate.hip — the coded size of a latent without coding it (include/flashgmm_amd.h section 3b), for CDNA4 / gfx950 (MI355X).
//
//   rate_kernel          (y | symbols, sigma, mu, pi) -> per-channel sums of the exact code length, optionally a per-latent map
//   symtab_bits_kernel   an encode-side table -> per-entry costs and their sum
//
// rate_kernel runs symtab_kernel's frame (fgmm_encframe.h: placement, loads, sym_entry on the same mixture), so the range it prices is the
// range the encoder codes, and ends in a reduction instead of the 4-byte store: cost = (16 << 24) - L[range] gathered from the 256 KB
// table of 2^24 * log2 r (L2-resident; coded ranges are mostly large, so few lines are touched), or the bypass escape's
// 16 + 4 * (1 + nibbles).  Costs are integers, summed in uint64: across the wave by shuffles, then ONE 64-bit atomic add per wave into
// the accumulator of the wave's channel (a wave never straddles a channel in either grid).  Integer sums do not depend on the order the
// atomics arrive in: the result is the same bits on every run.  A Kodak batch is 27 648 waves on 9 216 accumulators, three adds per address.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fgmm_encframe.h"

namespace fgmm {

#ifndef FGMM_RATE_WAVES
#define FGMM_RATE_WAVES 5 // min waves per SIMD the register allocator must leave room for, as symtab_kernel's (<= 96 VGPRs)
#endif
template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR>
__global__ __launch_bounds__(kBlock, FGMM_RATE_WAVES) void rate_kernel(const EncDesc *__restrict__ descs, const RateDesc *__restrict__ rdescs,
                                                      const uint32_t *__restrict__ L) {
  const EncDesc &d = descs[blockIdx.z];
  const RateDesc &r = rdescs[blockIdx.z];
  const int64_t hw = d.hw;
  int rank;
  int64_t p0;
  bool active;
  if (!enc_place<VEC, LINEAR>(hw, enc_n_coded(d), rank, p0, active)) return;
  const int c = enc_channel(d, rank);
  const bool from_y = d.sym == nullptr;
  unsigned long long cost = 0; // the lane's symbols (at most 4 * 52 bits)
  int nbypass = 0;             // the wave's, the same on every active lane (ballots)
  if (active) {
    float vq[VEC];
    int vi[VEC];
    enc_load_sym<VEC>(d, c, p0, vq, vi);
    EncPlanes<PT, VEC> P;
    P.load(d, c, p0);
    float bits[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float mu[4], sg[4], pi[4];
      P.get(e, d.logits, mu, sg, pi);
      int bp;
      const uint32_t ent = sym_entry<MODE, CLAMPED>(vq[e], vi[e], mu, sg, pi, bp);
      nbypass += __popcll(__ballot(bp));
      const uint32_t cq = entry_cost(ent, vq[e], vi[e], from_y, L);
      cost += cq;
      bits[e] = (float)cq * 0x1p-24f;
      if constexpr (VEC == 1) break; // (one position: no loop, see EncPlanes<PT, 1>)
    }
    if (r.bits_map) enc_st<float, VEC>(r.bits_map + (int64_t)c * hw + p0, bits);
  }
  // lanes past the end of a channel are the wave's last ones: lane 0 is active whenever any lane is, and holds the wave's bypass count
  cost = wave_sum64(cost);
  if ((threadIdx.x & 63) == 0 && cost) { // (every symbol costs something: 0 = a wave wholly past the end of its channel)
    add64(r.chan_bits + c, cost);
    if (nbypass) add64(r.chan_bypass + c, (unsigned long long)nbypass);
  }
}

// ---------------------------------------------------------------------------------------------------------
// symtab_bits_kernel: table -> cost (the host's fgmm_symtab_bits, entry by entry).  4 B/entry in (+ 4 with symbols), 4 out with
// the per-entry costs; a grid-stride loop, one atomic per wave into each of the two totals.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void symtab_bits_kernel(const uint32_t *__restrict__ packed, const int32_t *__restrict__ symbols,
                                                             int64_t n, const uint32_t *__restrict__ L, uint32_t *__restrict__ cost_q,
                                                             unsigned long long *__restrict__ bits_q, unsigned long long *__restrict__ n_bypass) {
  unsigned long long cost = 0, nb = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint32_t ent = packed[i];
    const uint32_t cq = rate_cost_q(ent, symbols ? symbols[i] : rate_entry_symbol(ent), L);
    if (cost_q) cost_q[i] = cq;
    cost += cq;
    nb += (ent >> 16) == 0;
  }
  cost = wave_sum64(cost);
  nb = wave_sum64(nb);
  if ((threadIdx.x & 63) == 0) {
    if (bits_q && cost) add64(bits_q, cost);
    if (n_bypass && nb) add64(n_bypass, nb);
  }
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
struct RateLaunch {
  const EncDesc *d;
  const RateDesc *r;
  const uint32_t *L;
  template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    hipLaunchKernelGGL((rate_kernel<MODE, VEC, CLAMPED, PT, LINEAR>), grid, dim3(kBlock), 0, s, d, r, L);
  }
};
int launch_rate(const EncDesc *d_descs, const RateDesc *d_rdescs, const uint32_t *d_log2, int count, int M_max, int64_t hw_max,
                int64_t n_max, bool linear, int mode, int vec, bool clamped, int planes, void *stream) {
  return enc_launch<false>(RateLaunch{d_descs, d_rdescs, d_log2}, count, M_max, hw_max, n_max, linear, mode, vec, clamped, planes, stream);
}

int launch_symtab_bits(const uint32_t *packed, const int32_t *symbols_or_null, int64_t n, const uint32_t *d_log2, uint32_t *cost_q_or_null,
                       unsigned long long *bits_q, unsigned long long *n_bypass, void *stream) {
  if (n <= 0) return 0;
  const dim3 grid((unsigned)std::min<int64_t>((n + kBlock - 1) / kBlock, 2048));
  hipLaunchKernelGGL(symtab_bits_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, packed, symbols_or_null, n, d_log2, cost_q_or_null, bits_q,
                     n_bypass);
  return (int)hipGetLastError();
}

} // namespace fgmm
