// fgmm_rate.hip — the coded size of a latent without coding it (include/flashgmm_amd.h section 3b), for CDNA4 / gfx950 (MI355X).
//
//   rate_kernel          (y | symbols, sigma, mu, pi) -> per-channel sums of the exact code length, optionally a per-latent map
//   symtab_bits_kernel   an encode-side table -> per-entry costs and their sum
//
// rate_kernel IS symtab_kernel (fgmm_kernels.hip) up to the table entry - the same EncDesc addressing, the same sym_entry and
// softmax4 on the same loads, so the range it prices is the range the encoder codes - and ends in a reduction instead of the
// 4-byte store: cost = (16 << 24) - L[range] gathered from the 256 KB table of 2^24 * log2 r (L2-resident; coded ranges are
// mostly large, so few lines are touched), or the bypass escape's 16 + 4 * (1 + nibbles).  Costs are integers, summed in uint64:
// across the wave by shuffles, then ONE 64-bit atomic add per wave into the accumulator of the wave's channel (a wave never
// straddles a channel in either grid).  Integer sums do not depend on the order the atomics arrive in: the result is the same
// bits on every run.  A Kodak batch is 27 648 waves on 9 216 accumulators, three adds per address.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fgmm_dev.h"

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
  const int n_nz = d.chan_list ? d.chan_list[d.M] : d.M; // wave-uniform scalar load
  int rank;    // compact (coded) channel of this wave: wave-uniform in both grids
  int64_t p0;  // position of the lane's first symbol within the channel
  bool active; // lanes past the end of a channel stay for the wave reduction
  if constexpr (LINEAR) { // every hw of the batch is a multiple of 64 * VEC: waves take 64 * VEC consecutive coded symbols (symtab_kernel)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t w0 = ((int64_t)blockIdx.x * kBlock + wave * 64) * VEC;
    if (w0 >= (int64_t)n_nz * hw) return;
    rank = __builtin_amdgcn_readfirstlane((int)(w0 / hw));
    p0 = (w0 - (int64_t)rank * hw) + (int64_t)(threadIdx.x & 63) * VEC;
    active = true;
  } else { // one block per (tile of kBlock * VEC positions, compact channel)
    rank = blockIdx.y;
    if (rank >= n_nz) return;
    if ((int64_t)blockIdx.x * kBlock * VEC >= hw) return;
    p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
    active = p0 < hw;
  }
  const int c = d.chan_list ? d.chan_list[rank] : rank;
  const bool from_y = d.sym == nullptr;
  unsigned long long cost = 0; // the lane's symbols (at most 4 * 52 bits)
  int nbypass = 0;             // the wave's, the same on every active lane (ballots)
  if (!active) {
  } else if constexpr (VEC > 1) {
    // planar, aligned (checked by the host): one VEC-wide load per plane per lane (16 B fp32 / 8 B fp16 at VEC = 4)
    typedef float fvec_t __attribute__((ext_vector_type(VEC)));
    typedef int ivec_t __attribute__((ext_vector_type(VEC)));
    const int64_t base = (int64_t)c * d.stride_c + p0;
    float vq[VEC];
    int vi[VEC];
    if (d.sym) {
      const ivec_t t = ldg<ivec_t>(d.sym + (int64_t)c * hw + p0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        vi[e] = t[e];
        vq[e] = (float)vi[e];
      }
    } else {
      const fvec_t t = ldg<fvec_t>(d.y + (int64_t)c * hw + p0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        vq[e] = __builtin_rintf(t[e]);
        vi[e] = (int)vq[e];
      }
    }
    float S[4][VEC], Mu[4][VEC], Pi[4][VEC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ldv<PT, VEC>(d.scales, base + k * d.stride_k, S[k]);
      ldv<PT, VEC>(d.means, base + k * d.stride_k, Mu[k]);
      ldv<PT, VEC>(d.weights, base + k * d.stride_k, Pi[k]);
    }
    fvec_t bits;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float mu[4], sg[4], pi[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        sg[k] = S[k][e];
        mu[k] = Mu[k][e];
        pi[k] = Pi[k][e];
      }
      if (d.logits) softmax4(pi);
      int bp;
      const uint32_t ent = sym_entry<MODE, CLAMPED>(vq[e], vi[e], mu, sg, pi, bp);
      nbypass += __popcll(__ballot(bp));
      const uint32_t cq = entry_cost(ent, vq[e], vi[e], from_y, L);
      cost += cq;
      bits[e] = (float)cq * 0x1p-24f;
    }
    if (r.bits_map) stg<fvec_t>(r.bits_map + (int64_t)c * hw + p0, bits);
  } else {
    const int64_t base = (int64_t)c * d.stride_c + p0 * d.stride_p;
    float vq;
    int vi;
    if (d.sym) {
      vi = ldg<int32_t>(d.sym + (int64_t)c * hw + p0);
      vq = (float)vi;
    } else {
      vq = __builtin_rintf(ldg<float>(d.y + (int64_t)c * hw + p0));
      vi = (int)vq;
    }
    float mu[4], sg[4], pi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sg[k] = ld1<PT>(d.scales, base + k * d.stride_k);
      mu[k] = ld1<PT>(d.means, base + k * d.stride_k);
      pi[k] = ld1<PT>(d.weights, base + k * d.stride_k);
    }
    if (d.logits) softmax4(pi);
    int bp;
    const uint32_t ent = sym_entry<MODE, CLAMPED>(vq, vi, mu, sg, pi, bp);
    nbypass = __popcll(__ballot(bp));
    const uint32_t cq = entry_cost(ent, vq, vi, from_y, L);
    cost = cq;
    if (r.bits_map) stg<float>(r.bits_map + (int64_t)c * hw + p0, (float)cq * 0x1p-24f);
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
template <int VEC, bool CLAMPED, typename PT, bool LINEAR>
static int launch_rate_v(const EncDesc *d, const RateDesc *r, const uint32_t *L, int count, int M_max, int64_t hw_max, int64_t n_max, int mode,
                         hipStream_t s) {
  const int64_t per_block = (int64_t)kBlock * VEC;
  const dim3 grid = LINEAR ? dim3((unsigned)((n_max + per_block - 1) / per_block), 1u, (unsigned)count)
                           : dim3((unsigned)((hw_max + per_block - 1) / per_block), (unsigned)M_max, (unsigned)count);
  switch (mode) {
  case MODE_AS: hipLaunchKernelGGL((rate_kernel<MODE_AS, VEC, CLAMPED, PT, LINEAR>), grid, dim3(kBlock), 0, s, d, r, L); break;
  case MODE_LOGISTIC: hipLaunchKernelGGL((rate_kernel<MODE_LOGISTIC, VEC, CLAMPED, PT, LINEAR>), grid, dim3(kBlock), 0, s, d, r, L); break;
  default: hipLaunchKernelGGL((rate_kernel<MODE_POLYA, VEC, CLAMPED, PT, LINEAR>), grid, dim3(kBlock), 0, s, d, r, L); break;
  }
  return (int)hipGetLastError();
}
template <typename PT, bool LINEAR>
static int launch_rate_t(const EncDesc *d, const RateDesc *r, const uint32_t *L, int count, int M_max, int64_t hw_max, int64_t n_max, int mode,
                         int vec, bool clamped, hipStream_t s) {
  if (vec >= 4) return clamped ? launch_rate_v<4, true, PT, LINEAR>(d, r, L, count, M_max, hw_max, n_max, mode, s)
                               : launch_rate_v<4, false, PT, LINEAR>(d, r, L, count, M_max, hw_max, n_max, mode, s);
  return clamped ? launch_rate_v<1, true, PT, LINEAR>(d, r, L, count, M_max, hw_max, n_max, mode, s)
                 : launch_rate_v<1, false, PT, LINEAR>(d, r, L, count, M_max, hw_max, n_max, mode, s);
}

int launch_rate(const EncDesc *d_descs, const RateDesc *d_rdescs, const uint32_t *d_log2, int count, int M_max, int64_t hw_max,
                int64_t n_max, bool linear, int mode, int vec, bool clamped, bool f16, void *stream) {
  if (count <= 0 || M_max <= 0 || hw_max <= 0) return 0;
  if (count > 65535 || M_max > 65535) return (int)hipErrorInvalidValue; // grid.z, grid.y
  if (linear && (n_max + kBlock - 1) / kBlock > 0x7FFFFFFFll) linear = false; // grid.x
  hipStream_t s = (hipStream_t)stream;
  if (linear)
    return f16 ? launch_rate_t<_Float16, true>(d_descs, d_rdescs, d_log2, count, M_max, hw_max, n_max, mode, vec, clamped, s)
               : launch_rate_t<float, true>(d_descs, d_rdescs, d_log2, count, M_max, hw_max, n_max, mode, vec, clamped, s);
  return f16 ? launch_rate_t<_Float16, false>(d_descs, d_rdescs, d_log2, count, M_max, hw_max, n_max, mode, vec, clamped, s)
             : launch_rate_t<float, false>(d_descs, d_rdescs, d_log2, count, M_max, hw_max, n_max, mode, vec, clamped, s);
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
