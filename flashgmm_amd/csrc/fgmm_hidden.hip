// fgmm_hidden.hip — the HIDDEN layers of the entropy-parameter network on the matrix cores, in one fixed order (header
// section 2c).
//
// What it replaces: entropy_parameters[:-1] of the checkerboard models - Conv2d(768, 640, 1) -> LeakyReLU -> Conv2d(640, 640, 1) ->
// LeakyReLU (compressai/models/ckbd_gmm.py:115-121; ELIC's parameter aggregation: the same with ReLU) - with the torch.cat in front of
// it: the layer reads its input as TWO sources, the context (xa, c_a channels) and the side parameters (xb, c_b channels), and the merged
// tensor never exists.  One launch per layer.
//
// Arithmetic: per item i and position p, on v_mfma_f32_32x32x2_f32, bit for bit the chain
//     acc = bias[o] (+0 without);  for k = 0 .. c_a - 1: acc = fmaf(W[o][k], xa[i][k][p], acc);
//                                  for k = 0 .. c_b - 1: acc = fmaf(W[o][c_a + k], xb[i][k][p], acc);   out[i][o][p] = act(acc)
// - head_kernel's chain (fgmm_head.hip) over cat(xa, xb), on the same tile and the same K loop (fgmm_mfma32.h).  An ABSENT first
// source (xa null: the anchors' context, which is zeros) drops its K tiles from the loop: its c_a columns are not part of the chain.
//   block  = T row tiles of 32 output channels x 128 positions, a wave: all T tiles x 32 positions (16 T accumulator registers)
//   K loop = mfma32_k_loop over source a's tiles, then source b's: each source's channels are padded to a multiple of 32 ON THEIR OWN
//            (packed weights +0, features -0: +0 * -0 = -0 leaves every accumulator's bits alone), so that a tile never straddles
//            the two and the source is ONE pointer select per tile in load_tile - the loop stays one basic block.  Weights from a
//            PRE-PACKED copy [row tile][source a's K tiles | source b's][32 rows][32 columns] (mfma32_pack_col's column order).
//   T      = 5, 2 or 1 (hidden_tiles_go, below): 5 divides the 20 row tiles of c_out = 640 - four blocks, no empty tile, 80 accumulator
//            registers a wave, two blocks a CU.  An output's chain does not depend on T: the same bits from every instantiation.
//   VEC    : hw % 4 == 0 and both sources 16-byte aligned (the host checks): the feature tile is staged with 16-byte loads; else element
//            by element (any shape).
//   epilogue: the activation in registers (the sequences of header section 2c), plane stores out[i][o][p] - what the next hidden
//            layer, or the head, reads as its features.
// No atomics, no workspace.
// A bf16x6 call (fgmm_hidden16.hip) launches this kernel after its own with the per-item domain words of its split copies (HiddenArgs::
// only, only_b): the blocks of an item inside the domain return at once, a flagged item gets the chain above.  Null - every other caller
// - means every item.
#include "fgmm_headframe.h"
#include "fgmm_hidden_act.h"

namespace fgmm {
namespace {

constexpr int kBK = kMfma32BK;       // input channels per LDS tile
constexpr int kTileW = kMfma32TileW; // floats of one packed tile: 32 rows x 32 columns
constexpr int kPB = kMfma32PB;       // positions per block
constexpr int kALd = kMfma32ALd, kBLd = kMfma32BLd; // LDS row pitches

// packed weights: [n_rt row tiles][kta + ktb K tiles][32 rows][32 columns], then the bias [n_rt][32].  K tile kt < kta: channels
// 32 kt ..+31 of source a; else channels 32 (kt - kta) ..+31 of source b - column c_a + that of W.  Padding (rows past c_out, a
// source's channels past its count): +0
__global__ __launch_bounds__(256) void hidden_pack_kernel(const float *__restrict__ w, const float *__restrict__ bias, int c_out, int c_a, int c_b, int n_rt,
                                                          int kta, int ktb, float *__restrict__ wp, float *__restrict__ bp) {
  const int n_kt = kta + ktb;
  const int64_t total = (int64_t)n_rt * n_kt * kTileW, n_bias = (int64_t)n_rt * 32;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total + n_bias; i += (int64_t)gridDim.x * 256) {
    if (i >= total) {
      const int64_t o = i - total;
      bp[o] = (o < c_out && bias) ? bias[o] : 0.0f;
      continue;
    }
    const int q = (int)(i % kBK), r = (int)((i / kBK) % 32);
    const int kt = (int)((i / kTileW) % n_kt), rt = (int)(i / ((int64_t)kTileW * n_kt));
    const bool src_a = kt < kta; // (row tile, source, K tile of the source)
    const int c = (src_a ? kt : kt - kta) * kBK + mfma32_pack_col(q);
    const int64_t o = (int64_t)rt * 32 + r;
    const bool in = o < c_out && c < (src_a ? c_a : c_b);
    wp[i] = in ? w[o * ((int64_t)c_a + c_b) + (src_a ? c : c_a + c)] : 0.0f;
  }
}

// (the library's activations, header section 2c: fgmm_hidden_act.h, shared with fgmm_hidden16.hip)

template <int T, bool VEC> // row tiles per block; 16-byte feature loads
__global__ __launch_bounds__(256, 2) void hidden_kernel(HiddenArgs a, int n_rg, int total) {
  constexpr int kTiles = T, kRows = 32 * T;
  __shared__ __attribute__((aligned(16))) float sA[kRows * kALd];
  __shared__ __attribute__((aligned(16))) float sB[kBK * kBLd];
  const int L = head_slot();
  if (L >= total) return;
  // the row groups of one position tile are consecutive slots of one XCD: its L2 holds the feature tile
  const int per_item = a.pt * n_rg;
  const int item = L / per_item, rem = L - item * per_item, pt = rem / n_rg, rg = rem - pt * n_rg;
  // a bf16x6 call (fgmm_hidden16.hip), and every present source of the item is inside its domain: hidden16_kernel has written it
  if (a.only && !(a.only[(int64_t)item * a.only_stride] | a.only_b[(int64_t)item * a.only_stride])) return;
  const int64_t hw = a.hw, P0 = (int64_t)pt * kPB;
  const int c_a = a.c_a, c_b = a.c_b, kta = a.kta;
  const float *xa = a.xa ? a.xa + (int64_t)item * c_a * hw : a.xb; // (absent: kta == 0 and no tile reads it)
  const float *xb = a.xb + (int64_t)item * c_b * hw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  // ---- accumulators start at the bias
  f16_t acc[kTiles];
  {
    const float *bp = a.bp + (int64_t)rg * kRows;
#pragma unroll
    for (int tl = 0; tl < kTiles; ++tl) head_bias_tile(bp, tl, h, acc[tl]);
  }
  // ---- K loop (mfma32_k_loop): tile kt < kta is source a's tile kt, else source b's tile kt - kta
  const int n_kt = a.n_kt;
  const int64_t rt_words = a.rt_words;                         // 16-byte words between the packed row tiles
  const float *wp = a.wp + (int64_t)rg * kTiles * rt_words * 4; // row tile rg * T + j, K tile kt: at wp + (j * rt_words + kt * 256) * 4
  // Staging, branch-free: a load that would fall outside a source (its channels past its count in its last tile, positions past hw in
  // the last position tile) reads a valid address instead and is replaced by -0 when the tile is written (mfma32_store_tile); the
  // packed weights are +0 there: the padding leaves the chain's bits as they are.
  float4_t ra[kTiles], rb[4];
  unsigned rb_ok = 0; // bit 4 j + e: element e of rb[j] lies inside the features
  auto load_tile = [&](int kt) {
    rb_ok = 0;
#pragma unroll
    for (int j = 0; j < kTiles; ++j) ra[j] = mfma32_load_a(wp + (int64_t)kt * kTileW, (int64_t)j * rt_words);
    const bool src_a = kt < kta;
    const float *x = src_a ? xa : xb; // the source switch: a select, not a branch
    const int c_src = src_a ? c_a : c_b, k0 = (src_a ? kt : kt - kta) * kBK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = tid + 256 * j, kk = f >> 5, p4 = f & 31;
      const int kin = k0 + kk;
      const int64_t p = P0 + 4 * p4;
      const bool k_ok = kin < c_src;
      const float *g = x + (int64_t)(k_ok ? kin : c_src - 1) * hw;
      float4_t v;
      if constexpr (VEC) {
        v = ldg<float4_t>(g + (p < hw ? p : 0));
        rb_ok |= (k_ok && p < hw ? 0xFu : 0u) << (4 * j); // (hw is a multiple of 4: the four positions are inside or outside together)
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = ((const FGMM_GLOBAL float *)g)[p + e < hw ? p + e : 0];
          rb_ok |= (k_ok && p + e < hw ? 1u : 0u) << (4 * j + e);
        }
      }
      rb[j] = v;
    }
  };
  mfma32_k_loop(acc, sA, sB, n_kt, wave, h, col, load_tile, [&]() { mfma32_store_tile(sA, sB, ra, rb, rb_ok, [](int) { return -0.0f; }); });
  // ---- epilogue: register reg of row tile tl is output channel (rg * T + tl) * 32 + mfma32_row(reg, h) at the lane's position
  const int64_t p = P0 + wave * 32 + col;
  if (p >= hw) return;
  float *out = a.out + (int64_t)item * a.c_out * hw + p;
  auto store = [&](auto act) {
#pragma unroll
    for (int tl = 0; tl < kTiles; ++tl)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
        if (o < a.c_out) stg<float>(out + (int64_t)o * hw, act(acc[tl][reg]));
      }
  };
  with_activation(a.act, a.slope, store);
}

template <int T> static int hidden_go(const HiddenArgs &a, int64_t n, bool vec, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T;
  const int64_t total = n * a.pt * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8); // every XCD gets as many slots (head_slot)
  if (vec) hipLaunchKernelGGL((hidden_kernel<T, true>), dim3(blocks), dim3(256), 0, st, a, n_rg, (int)total);
  else hipLaunchKernelGGL((hidden_kernel<T, false>), dim3(blocks), dim3(256), 0, st, a, n_rg, (int)total);
  return (int)hipGetLastError();
}

// The height rule (header section 2c): the first T of the ladder 5, 2, 1 at which the launch - `outer` = n * position tiles blocks per
// group of T row tiles - still has a block for every one of the device's `cus` compute units; 1 when none has.
template <int T, int... Ts, typename Go> static int hidden_tiles_go(int64_t outer, int c_out, int cus, const Go &go) {
  const int64_t n_rt = (c_out + 31) / 32;
  if constexpr (sizeof...(Ts) > 0)
    if (outer * ((n_rt + T - 1) / T) < cus) return hidden_tiles_go<Ts...>(outer, c_out, cus, go);
  return go(std::integral_constant<int, T>{});
}

} // namespace

int launch_hidden_pack(const float *w, const float *bias, int c_out, int c_a, int c_b, float *wp, float *bp, void *stream) {
  const int n_rt = hidden_row_tiles(c_out), kta = (c_a + kBK - 1) / kBK, ktb = (c_b + kBK - 1) / kBK;
  const int64_t total = (int64_t)hidden_packed_floats(c_out, c_a, c_b);
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(hidden_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, bias, c_out, c_a, c_b, n_rt, kta, ktb, wp, bp);
  return (int)hipGetLastError();
}

int hidden_device_cus(int device, int *cus) {
  return (int)hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device);
}
int hidden_tiles(int64_t n, int64_t pt, int c_out, int cus) {
  return hidden_tiles_go<5, 2, 1>(n * pt, c_out, cus, [](auto T) { return (int)T; });
}
int launch_hidden(const HiddenArgs &args, int64_t n, int cus, bool vec, void *stream) {
  return hidden_tiles_go<5, 2, 1>(n * args.pt, args.c_out, cus, [&](auto T) { return hidden_go<T>(args, n, vec, (hipStream_t)stream); });
}

} // namespace fgmm
