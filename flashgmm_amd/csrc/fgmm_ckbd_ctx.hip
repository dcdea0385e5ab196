// fgmm_ckbd_ctx.hip — the checkerboard context convolution on the matrix cores, in one fixed order (SURVEY.md §8 f rank 3; header
// section 5b).
//
// What it replaces: unembed(context_prediction(embed(y_hat_)))[1] of CheckerboardLatentCodec (compressai/latent_codecs/checkerboard.py:
// 281-284, 310-313) with context_prediction = CheckerboardMaskedConv2d(M, C_out, 5, padding=2): a full-size 5x5 convolution between two
// data movements, of which the mask keeps 12 taps and the codec half of the outputs.  Here: the compact anchors half in, the compact
// non-anchor context out, one launch, the 12 kept taps at the non-anchor positions only - a quarter of the multiply-adds.
//
// Arithmetic: a non-anchor at full-size (r, c) reads, for tap t = 0 .. 11 (fgmm_ckbd_geom.h: the kernel positions (i, j) with i + j odd,
// row-major), the full-size position (r + i - 2, c + j - 2): inside the image always an anchor (read from the anchors half at its
// compact place), outside +0.  Then, on v_mfma_f32_32x32x2_f32, bit for bit the chain
//     acc = bias[o] (+0 without);  for t ascending, for c = 0 .. M - 1 ascending:  acc = fmaf(W[o][c][tap t], x(t, c), acc)
// - head_kernel's chain (fgmm_head.hip) over c_in = 12 M gathered features, on the same tile (fgmm_mfma32.h), two blocks per CU,
//   block  = T row tiles of 32 output channels x 128 compact positions
//   K loop = mfma32_k_loop over tiles of 32 input channels of ONE tap: the gather offset of a position is constant over a tile.  Weights
//            from a PRE-PACKED copy [row tile][K tile][32 rows][32 columns], features by masked element loads of A[c][neighbour(q, t)].
//   T      = 6 (head_kernel's block: 192 rows) where that still gives every CU a block, else 2, else 1: ONE Kodak image is 6 position
//            tiles - at T = 6 and C_out = 384 twelve blocks on 256 CUs, each walking the whole K loop with six products per step; at
//            T = 1, 72 blocks with one.  An output's chain does not depend on T: the same bits from every instantiation.
// Padding (channels up to a K tile, positions up to 128, rows up to a row tile - and row tiles up to six): weights +0, features -0:
// +0 * -0 = -0 leaves every accumulator's bits alone, -0 included.  A tap outside the image is +0 and takes part in the chain as the
// definition says.
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"

namespace fgmm {
namespace {

constexpr int kBK = kCkbdCtxBK;     // input channels per LDS tile
constexpr int kTileW = kMfma32TileW; // floats of one packed tile: 32 rows x 32 columns
constexpr int kPB = kMfma32PB;      // compact positions per block
constexpr int kALd = kMfma32ALd, kBLd = kMfma32BLd; // LDS row pitches

// packs the 12 kept taps, and flags a dropped tap that is not +-0 (*bad = 1; zeroed by the host; null: not looked for).  M, c_out: the
// PACKED convolution's input and output channels.  TRANSPOSED (the data gradient's filters, section 5c): w is [M, c_out, 5, 5] - the
// forward's weight, whose outputs are this convolution's inputs - and W'[o][c][tap t] = w[c][o][tap 11 - t] (the 5x5 turned by 180 degrees)
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void ckbd_ctx_pack_kernel(const float *__restrict__ w, const float *__restrict__ bias, int M, int c_out, int n_rt, int mt,
                                                            float *__restrict__ wp, float *__restrict__ bp, uint32_t *__restrict__ bad) {
  const int n_kt = kCkbdCtxTaps * mt;
  const int64_t total = (int64_t)n_rt * n_kt * kTileW, n_bias = (int64_t)n_rt * 32, n_w = (int64_t)c_out * M * 25; // n_rt: a multiple of 6
  const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t i = first; i < total + n_bias; i += step) {
    if (i >= total) {
      const int64_t o = i - total;
      bp[o] = (o < c_out && bias) ? bias[o] : 0.0f;
      continue;
    }
    const int q = (int)(i % kBK), r = (int)((i / kBK) % 32);
    const int kt = (int)((i / kTileW) % n_kt), rt = (int)(i / ((int64_t)kTileW * n_kt));
    const int t = kt / mt, c = (kt - t * mt) * kBK + mfma32_pack_col(q);
    const int64_t o = (int64_t)rt * 32 + r;
    if (TRANSPOSED) wp[i] = (o < c_out && c < M) ? w[((int64_t)c * c_out + o) * 25 + ckbd_tap_flat(11 - t)] : 0.0f;
    else wp[i] = (o < c_out && c < M) ? w[(o * M + c) * 25 + ckbd_tap_flat(t)] : 0.0f;
  }
  if (!bad) return;
  bool any = false;
  for (int64_t i = first; i < n_w; i += step)
    if (((i % 25) & 1) == 0 && (__float_as_uint(w[i]) & 0x7FFFFFFFu) != 0u) any = true;
  if (any) *bad = 1u;
}

template <int T> // row tiles per block
__global__ __launch_bounds__(256, 2) void ckbd_ctx_kernel(CkbdCtxArgs a, int n_rg, int total) {
  constexpr int kTiles = T, kRows = 32 * T;
  __shared__ __attribute__((aligned(16))) float sA[kRows * kALd];
  __shared__ __attribute__((aligned(16))) float sB[kBK * kBLd];
  const int L = head_slot();
  if (L >= total) return;
  const int per_item = a.pt * n_rg;
  const int item = L / per_item, rem = L - item * per_item, pt = rem / n_rg, rg = rem - pt * n_rg;
  const int M = a.M, hgt = a.h, w2 = a.w2, wid = 2 * a.w2, hw = a.h * a.w2, P0 = pt * kPB;
  const float *x = a.anchors + (int64_t)item * M * hw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  // the thread's four positions of the feature tile (the same for its four channels: 256 is a multiple of the 32 position quads):
  // row and full-size column of the non-anchor at compact position q
  int pr[4], pc[4];
  unsigned p_ok = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = P0 + 4 * (tid & 31) + e;
    const CkbdAt at = ckbd_nonanchor(q, w2, a.odd);
    pr[e] = at.r, pc[e] = at.c;
    p_ok |= (q < hw ? 1u : 0u) << e;
  }
  // ---- accumulators start at the bias
  f16_t acc[kTiles];
  {
    const float *bp = a.bp + (int64_t)rg * kRows;
#pragma unroll
    for (int tl = 0; tl < kTiles; ++tl) head_bias_tile(bp, tl, h, acc[tl]);
  }
  // ---- K loop (mfma32_k_loop): tile kt = K tile kt - t * mt of tap t = kt / mt
  const int n_kt = a.n_kt, mt = a.mt;
  const float *wp = a.wp + (int64_t)rg * kTiles * n_kt * kTileW; // row tile rg * T + j, K tile kt: at ((rg * T + j) * n_kt + kt) * kTileW
  // Staging, branch-free: a load that would fall outside the anchors (channels past M in a tap's last tile, positions past hw, a tap
  // outside the image) reads a valid address instead and is replaced when the tile is written: by +0 where the tap of a real channel
  // lies outside the image (it takes part in the chain), by -0 for a padded channel (the packed weights are +0 there)
  float4_t ra[kTiles], rb[4];
  unsigned rb_ok = 0; // bit 4 j + e: element e of rb[j] is an anchor inside the image
  unsigned rb_ch = 0; // bit j: the channel of rb[j] is one of the M
  auto load_tile = [&](int kt) {
    rb_ok = 0, rb_ch = 0;
#pragma unroll
    for (int j = 0; j < kTiles; ++j) ra[j] = mfma32_load_a(wp + (int64_t)kt * kTileW, (int64_t)j * n_kt * (kTileW / 4));
    const int t = kt / mt, c0 = (kt - t * mt) * kBK;
    const CkbdTap tap = ckbd_tap(t);
    int off[4];
    unsigned in = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rr = pr[e] + tap.di, cc = pc[e] + tap.dj;
      const bool ok = ((p_ok >> e) & 1u) && ckbd_inside(rr, cc, hgt, wid);
      off[e] = ok ? ckbd_anchor_at(rr, cc, w2) : 0;
      in |= (ok ? 1u : 0u) << e;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + (tid >> 5) + 8 * j;
      const bool k_ok = c < M;
      const FGMM_GLOBAL float *g = (const FGMM_GLOBAL float *)(x + (int64_t)(k_ok ? c : M - 1) * hw);
      float4_t v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = g[off[e]];
      rb[j] = v;
      rb_ok |= (k_ok ? in : 0u) << (4 * j);
      rb_ch |= (k_ok ? 1u : 0u) << j;
    }
  };
  mfma32_k_loop(acc, sA, sB, n_kt, wave, h, col, load_tile,
                [&]() { mfma32_store_tile(sA, sB, ra, rb, rb_ok, [&](int j) { return (rb_ch >> j) & 1u ? 0.0f : -0.0f; }); });
  // ---- epilogue: register reg of row tile tl is output channel (rg * T + tl) * 32 + mfma32_row(reg, h) at the lane's position
  const int p = P0 + wave * 32 + col;
  if (p < hw) {
    float *out = a.out + (int64_t)item * a.c_out * hw + p;
#pragma unroll
    for (int tl = 0; tl < kTiles; ++tl)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
        if (o < a.c_out) stg<float>(out + (int64_t)o * hw, acc[tl][reg]);
      }
  }
}

} // namespace

int launch_ckbd_ctx_pack(const float *w, const float *bias, int M, int c_out, bool transposed, float *wp, float *bp, uint32_t *bad, void *stream) {
  if (transposed) std::swap(M, c_out); // the packed convolution's sizes
  const int n_rt = ckbd_ctx_row_tiles(c_out), mt = (M + kBK - 1) / kBK;
  const int64_t total = std::max<int64_t>((int64_t)ckbd_ctx_packed_floats(M, c_out), bad ? (int64_t)c_out * M * 25 : 0);
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
  if (transposed) hipLaunchKernelGGL(ckbd_ctx_pack_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, bias, M, c_out, n_rt, mt, wp, bp, bad);
  else hipLaunchKernelGGL(ckbd_ctx_pack_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, bias, M, c_out, n_rt, mt, wp, bp, bad);
  return (int)hipGetLastError();
}

template <int T> static int ckbd_ctx_go(const CkbdCtxArgs &a, int64_t n, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T;
  const int64_t total = n * a.pt * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8); // every XCD gets as many slots (head_slot)
  hipLaunchKernelGGL(ckbd_ctx_kernel<T>, dim3(blocks), dim3(256), 0, st, a, n_rg, (int)total);
  return (int)hipGetLastError();
}

// T: the most row tiles per block (6, 2, 1) at which the launch still has a block for every CU; 1 when none has
int ckbd_ctx_tiles(int64_t n, int64_t pt, int c_out) {
  return ckbd_row_tiles_go<6, 2, 1>(n * pt, c_out, [](auto T) { return (int)T; });
}
int launch_ckbd_ctx(const CkbdCtxArgs &args, int64_t n, void *stream) {
  return ckbd_row_tiles_go<6, 2, 1>(n * args.pt, args.c_out, [&](auto T) { return ckbd_ctx_go<T>(args, n, (hipStream_t)stream); });
}

} // namespace fgmm
