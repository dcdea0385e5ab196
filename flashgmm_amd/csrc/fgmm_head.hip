// fgmm_head.hip — the parameter head's last layer on the matrix cores, fused with the encode-side CDF kernel.
//
// What it replaces: the final 1x1 convolution of `entropy_parameters`, nn.Conv2d(N*10//3, 3*K*N, 1) (compressai/models/ckbd_gmm.py:115-121),
// the chunk(3, 1) into scales | means | weights and the softmax over K (compressai/latent_codecs/gaussian_mixture_conditional.py:183-202),
// the sigma clamp (compressai/entropy_models/entropy_models.py:817) - and, in the FUSED form, symtab_kernel: the 3*K parameters of a
// latent never exist in HBM, they go from the MFMA accumulators straight into sym_entry() and only the packed 4-byte table entry is
// written (56 -> 8 B of HBM traffic per symbol beside the features the convolution reads anyway).
//
// Arithmetic: out[o][p] = bias[o] + sum_k W[o][k] * x[k][p] on v_mfma_f32_32x32x2_f32 - exact binary32, and bit for bit the chain
//     acc = bias[o];  for k = 0 .. c_in - 1:  acc = fmaf(W[o][k], x[k][p], acc)
// (one rounding per product, k ascending: lane half 0 of the instruction holds the even k of a pair, half 1 the odd one).  The order is
// the library's, not a BLAS's: encoder and decoder get the same parameters from the same weights on any ROCm / torch / MIOpen version,
// which the reference silently relies on.  The CPU checker under tests restates the chain with fmaf: the GPU tests compare
// bit for bit.
//
// Tiling (wave64, 256 threads = 4 waves, TWO blocks per CU - a wave holds 96 accumulator registers and at most 256 in all):
//   block  = 16 latent channels (their 3*K = 12 parameters each: 192 rows of W) x 128 positions
//   wave   = all 192 rows x 32 positions = 6 row tiles of 32x32 accumulators
//   K loop = mfma32_k_loop (fgmm_mfma32.h) over tiles of 32 input channels: W tile 192 x 32 from a PRE-PACKED copy of the weights
//            (one contiguous 24 KB read per block and tile), x tile 32 x 128
//   rows   : row tile (g, t), g = which 8 of the 16 channels, t = scales | means | logits; row 4 * cl + k within it = parameter
//            (t, k) of channel 8 g + cl.  The 32x32 accumulator map (row = mfma32_row(reg, lane >> 5), column = lane & 31)
//            then gives every lane, for ITS position, registers 4 j + k = parameter (t, k) of channel 8 g + 2 j + (lane >> 5): a lane
//            owns all twelve parameters of its latents - the epilogue needs no lane movement and no LDS.
//   blocks that share an x tile (the channel groups of one position tile) get consecutive slots on ONE XCD: its L2 holds the tile.
#include "fgmm_headframe.h"

namespace fgmm {
namespace {

constexpr int kCG = kHeadCG;          // latent channels per block
constexpr int kRows = 12 * kCG;       // rows of W per block (192)
constexpr int kBK = kHeadBK;          // input channels per LDS tile
constexpr int kPB = kMfma32PB;        // positions per block
constexpr int kALd = kMfma32ALd, kBLd = kMfma32BLd; // LDS row pitches
constexpr int kTiles = kRows / 32;    // 6 row tiles

// packed weights: [channel group][K tile][192 rows][32 columns]; column h * 16 + s of a tile = input channel tile * 32 + 2 s + h
__global__ __launch_bounds__(256) void head_pack_kernel(const float *__restrict__ w, const float *__restrict__ bias, int M, int c_in, int n_cg, int n_kt,
                                                        float *__restrict__ wp, float *__restrict__ bp) {
  const int64_t total = (int64_t)n_cg * n_kt * kRows * kBK;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total + (int64_t)n_cg * kRows; i += (int64_t)gridDim.x * 256) {
    const bool is_bias = i >= total;
    const int64_t e = is_bias ? i - total : i;
    const int q = is_bias ? 0 : (int)(e % kBK);
    const int r = (int)((is_bias ? e : e / kBK) % kRows);
    const int kt = is_bias ? 0 : (int)((e / (kBK * kRows)) % n_kt);
    const int cg = (int)(is_bias ? e / kRows : e / ((int64_t)kBK * kRows * n_kt));
    const auto [c, o] = head_pack_row(r, cg, M);
    if (is_bias) {
      bp[e] = (c < M && bias) ? bias[o] : 0.0f;
    } else {
      const int kin = kt * kBK + mfma32_pack_col(q);
      wp[e] = (c < M && kin < c_in) ? w[o * c_in + kin] : 0.0f;
    }
  }
}

// FUSED: the epilogue evaluates the table entry (EncDesc: y, channel census of quant_stats_kernel, the table's place); else it writes the
// three parameter tensors as planes [3 * 4 * M, hw] (scales | means | logits, channel k * M + c).
// VEC: every item's positions are a multiple of 4 and its features 16-byte aligned (checked by the host): the x tile is staged with
// 16-byte loads; else element by element (any shape, slowly).
template <int MODE, bool CLAMPED, bool FUSED, bool VEC>
__global__ __launch_bounds__(256, 2) void head_kernel(const EncDesc *__restrict__ edescs, const HeadDesc *__restrict__ hdescs, HeadW hw_, int pt_max,
                                                       int cg_max, int total) {
  __shared__ __attribute__((aligned(16))) float sA[kRows * kALd];
  __shared__ __attribute__((aligned(16))) float sB[kBK * kBLd];
  __shared__ int s_rank[kCG];
  const int L = head_slot();
  if (L >= total) return;
  const HeadPlace<float> b = head_place<FUSED, kPB, float>(edescs, hdescs, hw_, L, pt_max, cg_max);
  if (b.P0 >= b.hw || b.cg * kCG >= b.M) return;
  if (hw_.oob && !head_item_oob<FUSED>(edescs, hdescs, hw_, b.item, b.hw)) return; // a bf16x6 call: only the items outside its domain are this kernel's
  const int item = b.item, cg = b.cg, M = b.M;
  const int64_t hw = b.hw, P0 = b.P0;
  const float *x = b.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  if constexpr (FUSED)
    if (!head_ranks<256>(edescs[item], cg, M, s_rank)) return;
  // the lane's eight latents, fetched now: their latency lies under the K loop instead of in front of the epilogue
  float yv[8];
  if constexpr (FUSED) {
    const EncDesc &d = edescs[item];
    const int64_t p = P0 + wave * 32 + col;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = cg * kCG + (q >> 2) * 8 + 2 * (q & 3) + h;
      yv[q] = (s_rank[(q >> 2) * 8 + 2 * (q & 3) + h] >= 0 && p < hw) ? ldg<float>(d.y + (int64_t)c * hw + p) : 0.0f;
    }
  }
  // ---- accumulators start at the bias
  f16_t acc[kTiles];
  {
    const float *bp = hw_.bp + (int64_t)cg * kRows;
#pragma unroll
    for (int tl = 0; tl < kTiles; ++tl) head_bias_tile(bp, tl, h, acc[tl]);
  }
  // ---- K loop
  const int n_kt = hw_.n_kt, c_in = hw_.c_in;
  const float *wp = static_cast<const float *>(hw_.wp) + (int64_t)cg * n_kt * (kRows * kBK);
  // Staging, branch-free: a load that would fall outside the features (input channels past c_in in the last tile, positions past hw
  // in the last position tile) reads a valid address instead and is replaced by -0 when the tile is written (mfma32_store_tile); the
  // packed weights are +0 there: the padded channels leave the chain's bits as they are.
  float4_t ra[kTiles], rb[4];
  unsigned rb_ok = 0; // bit 4 j + e: element e of rb[j] lies inside the features
  auto load_tile = [&](int kt) {
    rb_ok = 0;
#pragma unroll
    for (int j = 0; j < kTiles; ++j) ra[j] = mfma32_load_a(wp + (int64_t)kt * (kRows * kBK), 256 * j);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = tid + 256 * j, kk = f >> 5, p4 = f & 31;
      const int kin = kt * kBK + kk;
      const int64_t p = P0 + 4 * p4;
      const bool k_ok = kin < c_in;
      const float *g = x + (int64_t)(k_ok ? kin : c_in - 1) * hw;
      float4_t v;
      if constexpr (VEC) {
        v = ldg<float4_t>(g + (p < hw ? p : 0));
        rb_ok |= (k_ok && p < hw ? 0xFu : 0u) << (4 * j); // (hw is a multiple of 4: the four positions are inside or outside together)
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = g[p + e < hw ? p + e : 0];
          rb_ok |= (k_ok && p + e < hw ? 1u : 0u) << (4 * j + e);
        }
      }
      rb[j] = v;
    }
  };
  mfma32_k_loop(acc, sA, sB, n_kt, wave, h, col, load_tile, [&]() { mfma32_store_tile(sA, sB, ra, rb, rb_ok, [](int) { return -0.0f; }); });
  // ---- epilogue: the lane's 8 latents (2 channel halves x 4 channels at its position), all twelve parameters in registers
  if constexpr (FUSED) {
    const EncDesc &d = edescs[item];
    int nbypass = 0;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rank = s_rank[g * 8 + 2 * j + h];
        uint32_t *row_out = head_row(d, rank, hw);
        const int64_t p = P0 + wave * 32 + col;
        int bp = 0;
        if (rank >= 0 && p < hw) bp = head_entry<MODE, CLAMPED>(row_out + p, acc[g * 3], acc[g * 3 + 1], acc[g * 3 + 2], j, yv[g * 4 + j]);
        nbypass += __popcll(__ballot(bp));
      }
    head_census<4>(d, L, nbypass);
  } else {
    float *out = hdescs[item].out;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = cg * kCG + g * 8 + 2 * j + h;
        const int64_t p = P0 + wave * 32 + col;
        if (c < M && p < hw) {
#pragma unroll
          for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) out[head_plane_at(t, k, c, M, hw, p)] = acc[g * 3 + t][4 * j + k];
        }
      }
  }
}

template <bool FUSED> struct Go { // F::go of head_launch (fgmm_headframe.h); the un-fused form has one mode
  const EncDesc *edescs;
  const HeadDesc *hdescs;
  const HeadW &w;
  hipStream_t st;
  template <int MODE, bool CLAMPED, bool VEC> int go(const HeadGrid &g) const {
    hipLaunchKernelGGL((head_kernel<FUSED ? MODE : 0, FUSED ? CLAMPED : true, FUSED, VEC>), dim3(g.blocks), dim3(256), 0, st, edescs, hdescs, w, g.pt_max, g.cg_max, g.total);
    return (int)hipGetLastError();
  }
};

} // namespace

int launch_head_pack(const float *w, const float *bias, int M, int c_in, float *wp, float *bp, void *stream) {
  const int n_cg = (M + kCG - 1) / kCG, n_kt = (c_in + kBK - 1) / kBK;
  const int64_t total = (int64_t)n_cg * n_kt * kRows * kBK + (int64_t)n_cg * kRows;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(head_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, bias, M, c_in, n_cg, n_kt, wp, bp);
  return (int)hipGetLastError();
}

int launch_head_params(const HeadDesc *d_descs, const HeadW &w, int count, int64_t hw_max, bool vec, void *stream) {
  return head_launch<kPB>(Go<false>{nullptr, d_descs, w, (hipStream_t)stream}, count, w.n_cg, hw_max, 0, true, vec);
}
int launch_head_symtab(const EncDesc *d_descs, const HeadW &w, int count, int M_max, int64_t hw_max, int mode, bool clamped, bool vec, void *stream) {
  return head_launch<kPB>(Go<true>{d_descs, nullptr, w, (hipStream_t)stream}, count, (M_max + kCG - 1) / kCG, hw_max, mode, clamped, vec);
}

} // namespace fgmm
