// fgmm_headframe.h — the frame the two parameter-head kernels share: head_kernel (fgmm_head.hip, exact binary32) and head16_kernel
// (fgmm_head16.hip, bf16x6).  Which (item, position tile, channel group) a block is, the compact-channel ranks of the fused form, the
// bias a row tile starts from, what happens to a latent's twelve parameters once they lie in the accumulators (a table entry, or twelve
// plane stores), the index decomposition of the two pack kernels, and the launchers' geometry and ladder over mode x clamped x VEC.
// A kernel adds its tiling, its staging and its K loop: the table entry one arithmetic writes is the entry the other writes because
// they run this text, not a copy of it.
#pragma once
#include "fgmm_mfma32.h"

namespace fgmm {

// placement.  Blocks are dealt to the 8 XCDs round robin: the blocks that share an x tile (the channel groups of one position tile) get
// consecutive logical slots L on ONE XCD, whose L2 then holds the tile.  PB: positions per block
// The early returns stay in the kernels, in their words: a helper that returns "nothing to do" beside a half-filled HeadPlace costs
// the loads through the descriptors their provenance, and the K loop its register assignment (profiles/head_frame_refactor.md).
__device__ __forceinline__ int head_slot() { // the block's logical slot L; L >= total: the grid's padding to a multiple of 8
  const int per_xcd = (int)gridDim.x >> 3;
  return ((int)blockIdx.x & 7) * per_xcd + ((int)blockIdx.x >> 3);
}
template <typename XT> struct HeadPlace {
  int item, pt, cg, M;
  int64_t hw, P0; // the item's positions; the block's first.  P0 >= hw or cg * kHeadCG >= M: a smaller item than the call's largest
  const XT *x;    // the item's features as the kernel reads them: float = the descriptor's x, uint16_t = its split copy xs
};
template <bool FUSED> __device__ __forceinline__ const void *head_xs(const EncDesc *edescs, const HeadDesc *hdescs, int item) {
  return FUSED ? edescs[item].xs : hdescs[item].xs;
}
template <bool FUSED, int PB, typename XT>
__device__ __forceinline__ HeadPlace<XT> head_place(const EncDesc *edescs, const HeadDesc *hdescs, const HeadW &w, int L, int pt_max, int cg_max) {
  HeadPlace<XT> b;
  b.item = L / (pt_max * cg_max);
  const int rem = L - b.item * (pt_max * cg_max);
  b.pt = rem / cg_max, b.cg = rem - b.pt * cg_max;
  if constexpr (sizeof(XT) == 4) {
    b.x = FUSED ? edescs[b.item].x : hdescs[b.item].x;
  } else {
    b.x = static_cast<const XT *>(head_xs<FUSED>(edescs, hdescs, b.item));
  }
  if constexpr (FUSED) {
    b.hw = edescs[b.item].hw, b.M = edescs[b.item].M;
  } else {
    b.hw = hdescs[b.item].hw, b.M = w.M;
  }
  b.P0 = (int64_t)b.pt * PB;
  return b;
}
// a bf16x6 call (w.oob), and a feature of the item is outside the bf16x6 domain: the item is the exact kernel's, launched second
template <bool FUSED>
__device__ __forceinline__ bool head_item_oob(const EncDesc *edescs, const HeadDesc *hdescs, const HeadW &w, int item, int64_t hw) {
  return w.oob && *head16_oob_word(head_xs<FUSED>(edescs, hdescs, item), w.c_in, hw);
}

// the fused form's prologue: s_rank[i] = compact (coded) channel of the block's channel i, -1 = no coded symbol - a prefix sum over
// quant_stats' census.  Every thread takes channels tid, tid + THREADS ...: one ballot per wave and chunk of THREADS channels, the
// sixteen ranks are popcounts below a channel.  false: sixteen channels that round to zero everywhere - nothing to code, nothing to
// multiply
template <int THREADS> __device__ __forceinline__ bool head_ranks(const EncDesc &d, int cg, int M, int *s_rank) {
  static_assert(THREADS % kHeadCG == 0, "the block's channels lie in one chunk");
  constexpr int kWaves = THREADS / 64;
  __shared__ unsigned long long s_nzmask[kWaves];
  __shared__ int s_below[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int below = 0; // coded channels in the chunks before the one that holds this block's channels (per wave; summed over the waves below)
  const int c_first = cg * kHeadCG;
  for (int base = 0; base <= c_first; base += THREADS) {
    const int c = base + tid;
    const unsigned long long m = __ballot(c < M && d.chan_nz[c] != 0);
    if (base + THREADS <= c_first) {
      below += __popcll(m);
      continue;
    }
    if (lane == 0) s_nzmask[wave] = m;
  }
  if (lane == 0) s_below[wave] = below;
  __syncthreads();
  if (tid < kHeadCG) {
    const int c = c_first + tid, off = c & (THREADS - 1);
    int r = -1;
    if (c < M && ((s_nzmask[off >> 6] >> (off & 63)) & 1ull)) {
      r = 0;
      for (int wv = 0; wv < kWaves; ++wv) r += s_below[wv];
      for (int wv = 0; wv < (off >> 6); ++wv) r += __popcll(s_nzmask[wv]);
      r += __popcll(s_nzmask[off >> 6] & ((1ull << (off & 63)) - 1ull));
    }
    s_rank[tid] = r;
  }
  __syncthreads();
  bool any = false;
#pragma unroll
  for (int i = 0; i < kHeadCG; ++i) any = any || s_rank[i] >= 0;
  return any;
}

// the accumulators of row tile `tile` of the block's 192 rows start at the bias (bp: the channel group's)
__device__ __forceinline__ void head_bias_tile(const float *bp, int tile, int h, f16_t &acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = bp[tile * 32 + mfma32_row(r, h)];
}

// epilogues.  A lane owns all twelve parameters of its latents: registers 4 j + k of the scales | means | logits tiles of a channel
// octet are parameter k of channel 2 j + (lane >> 5) of the octet, at the lane's position - no lane movement, no LDS.
// FUSED: where the table row of compact channel `rank` begins (the table lies in up to four segments of compact channels); -1, no
// coded symbol: null
__device__ __forceinline__ uint32_t *head_row(const EncDesc &d, int rank, int64_t hw) {
  uint32_t *row_out = nullptr;
  if (rank >= 0) {
    const int seg = (rank >= d.seg_b[0]) + (rank >= d.seg_b[1]) + (rank >= d.seg_b[2]);
    row_out = (seg ? d.packed_seg[seg] : d.packed) + (int64_t)(rank - seg * d.cps) * hw;
  }
  return row_out;
}
// ... and the entry of one latent y of a coded channel, from slot j of the channel octet's three tiles -> its bypass bit
template <int MODE, bool CLAMPED>
__device__ __forceinline__ int head_entry(uint32_t *entry, const f16_t &s_t, const f16_t &m_t, const f16_t &l_t, int j, float y) {
  float sg[4], mu[4], pi[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) sg[k] = s_t[4 * j + k], mu[k] = m_t[4 * j + k], pi[k] = l_t[4 * j + k];
  softmax4(pi);
  const float vq = __builtin_rintf(y);
  int bp = 0;
  stg<uint32_t>(entry, sym_entry<MODE, CLAMPED>(vq, (int)vq, mu, sg, pi, bp));
  return bp;
}
// bypass census: nbypass = the wave's ballots of head_entry's bits, summed; the host sums the item's slots - one atomic per wave that
// saw any (rare: 0.2 % of the symbols)
template <int WAVES> __device__ __forceinline__ void head_census(const EncDesc &d, int L, int nbypass) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0 && nbypass) atomicAdd(d.meta + ((L * WAVES + wave) % (int)d.meta_slots), (uint32_t)nbypass);
}
// un-fused: where parameter (t, k) of channel c at position p lies in the planes [3 * 4 * M, hw] (scales | means | logits, channel
// k * M + c).  One element, not a latent's twelve stores: loops in here are unrolled before the kernel's own, their invariants hoisted
// out of those, and the accumulators change registers through the K loop (profiles/head_frame_refactor.md)
__device__ __forceinline__ int64_t head_plane_at(int t, int k, int c, int M, int64_t hw, int64_t p) {
  return ((int64_t)t * 4 * M + (int64_t)k * M + c) * hw + p;
}

// the pack kernels: row r of channel group cg's 192 = row tile (g, t), g = which 8 of the 16 channels, t = scales | means | logits;
// row 4 * cl + k within it = parameter (t, k) of channel 8 g + cl.  -> c, that latent channel (may be >= M in the last group), and o,
// the output channel of the convolution: chunk t, component k, channel c.  (How an element index splits into K tile, row and column
// stays with the kernels: one function over both the weights' and the bias' index space compiles to other registers)
struct HeadPackRow { int c; int64_t o; };
__device__ __forceinline__ HeadPackRow head_pack_row(int r, int cg, int M) {
  const int tile = r >> 5, ri = r & 31;
  const int g = tile / 3, t = tile % 3, cl = ri >> 2, k = ri & 3;
  const int c = cg * kHeadCG + g * 8 + cl;
  return HeadPackRow{c, (int64_t)t * 4 * M + (int64_t)k * M + c};
}

// the launchers' geometry and ladder.  F::go<MODE, CLAMPED, VEC>(g) launches the kernel with its own arguments and returns the HIP
// status; a launcher whose kernel has no such parameter ignores it.  cg_max: channel groups of the largest M of the call
struct HeadGrid { unsigned blocks; int pt_max, cg_max, total; }; // blocks: total rounded up to 8, every XCD gets as many slots
template <int MODE, typename F> static int head_launch_m(const F &f, const HeadGrid &g, bool clamped, bool vec) {
  if (clamped) return vec ? f.template go<MODE, true, true>(g) : f.template go<MODE, true, false>(g);
  return vec ? f.template go<MODE, false, true>(g) : f.template go<MODE, false, false>(g);
}
template <int PB, typename F> static int head_launch(const F &f, int count, int cg_max, int64_t hw_max, int mode, bool clamped, bool vec) {
  const int pt_max = (int)((hw_max + PB - 1) / PB);
  const int64_t total = (int64_t)count * pt_max * cg_max;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const HeadGrid g{(unsigned)((total + 7) / 8 * 8), pt_max, cg_max, (int)total};
  switch (mode) {
  case 0: return head_launch_m<0>(f, g, clamped, vec);
  case 1: return head_launch_m<1>(f, g, clamped, vec);
  case 2: return head_launch_m<2>(f, g, clamped, vec);
  }
  return (int)hipErrorInvalidValue;
}

} // namespace fgmm
