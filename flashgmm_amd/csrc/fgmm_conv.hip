// fgmm_conv.hip — dense 3x3 / 5x5 convolutions (stride 1, padding k / 2) on the matrix cores, in one fixed order (header section 5d).
//
// What it replaces: the convolutions MIOpen still computes from decoded values on the decode-side parameter path - the five 3x3 layers of
// the checkerboard GMM model's h_s (compressai/models/ckbd_gmm.py:97-107: conv3x3 and subpel_conv3x3 = Conv2d + PixelShuffle(2), LeakyReLU
// between them) and the three 5x5 layers of ELIC's channel context (models/elic_gmm.py:151-164).  One launch per layer: the convolution,
// the activation of section 2c (fgmm_hidden_act.h) and a plain or PixelShuffle(2) store.
//
// Arithmetic: per item i, output channel o and position (r, q), on v_mfma_f32_32x32x2_f32, bit for bit the chain
//     acc = bias[o] (+0 without);  for c = 0 .. c_in - 1 ascending, for t = a * k + b = 0 .. k * k - 1 ascending:
//         acc = fmaf(W[o][c][a][b], x[i][c][r + a - k/2][q + b - k/2] (inside the image, else +0), acc);      v = act(acc)
// - head_kernel's chain (fgmm_head.hip) over K = c_in k^2 gathered features in the order of W.reshape(c_out, c_in k^2): channel outer,
// tap inner, so that all k^2 taps of a channel read one small neighbourhood of one plane.
//   block   = T row tiles of 32 output channels x 128 positions, the positions an 8 x 16 PATCH of the image; wave wv owns patch rows
//             2 wv, 2 wv + 1: lane column col = lane & 31 is position (2 wv + (col >> 4), col & 15), lane half h = lane >> 5 the odd k of a pair.
//   K loop  = chunks of kConvCB = 8 input channels: KC = 8 k^2 = 72 | 200 K entries, 9 | 25 whole groups of four k-pairs (Mfma32Frag); no
//             pair straddles a chunk.  Per chunk the block stages, ONCE, (a) the T packed weight tiles [32 rows][KC] by 16-byte loads into
//             sA (row pitch KC + 4 floats: 12 mod 64 - the 16 rows of a quarter wave's 16-byte reads start 12 banks apart, all multiples
//             of 4 distinct mod 64) and (b) the patch plus its halo of the 8 channels, (8 + k - 1) x (16 + k - 1) elements a channel, into
//             sH: an element outside the image as +0 (it takes part in the chain), a channel past c_in as -0 (its packed weights are +0:
//             +0 * -0 = -0 leaves every accumulator's bits alone, -0 included).  Every input element crosses from global memory once per
//             block and chunk, not k^2 times.
//   B reads = the fragment of K entry kappa = c k^2 + a k + b of the chunk is ONE 4-byte LDS read at sH[lane base + off(kappa)], lane base
//             = pr PITCH + pc, off(kappa) = c PLANE + a PITCH + b - a constant of the instantiation (the loop over the groups is unrolled:
//             the two offsets of a k-pair are literals, the lane half selects one).
//   pitch   : PITCH = 24, PLANE = 264 (k = 3) | 312 (k = 5) floats, for 64 banks of 4 bytes.  A wave's read touches four runs of 16
//             consecutive floats: the two patch rows (PITCH apart) of lane half 0, and the same two moved by d = off(kappa + 1) -
//             off(kappa) for half 1.  d = 1 inside a tap row: runs [0, 16] and [24, 40] - 34 addresses, 34 banks (the overlapping lanes
//             read the SAME address: a broadcast).  d = PITCH - (k - 1) at the end of a tap row: runs [0, 15], [24 - (k - 1), 39] and
//             [48 - (k - 1), 63 - (k - 1)]: disjoint mod 64 for 20 <= PITCH <= 26 (and PITCH >= 16 + k - 1 holds the halo's row).  d =
//             PLANE - (k - 1) PITCH - (k - 1) at the end of a channel: PLANE = k PITCH mod 64 (and >= (8 + k - 1) PITCH) makes that
//             the second case again.  No read of the loop collides.
//   T       = 4, 2 or 1 (ckbd_row_tiles_go: the tallest at which every CU still gets a block, else 1).  An output's chain depends on
//             neither T, nor n, nor the item's place in the batch, nor its patch: the same bits from every instantiation.
//   loop    : one LDS buffer, two barriers per chunk (profiles/conv_stack.md); the next chunk's global loads are issued before this chunk's
//             first product, the fragments are read one group ahead of the products that use them, the products of a chunk are ONE
//             basic block fenced as mfma32_k_loop's (which does not fit: its B tile is [K][128]).
//   epilogue: the activation on the accumulators, then out[i][o][r][q] or - shuffle 2, PixelShuffle(2) by index arithmetic -
//             out[i][o >> 2][2 r + ((o >> 1) & 1)][2 q + (o & 1)].  Lanes outside the image and rows past c_out store nothing.
// No atomics, no workspace.
// A bf16x6 call (fgmm_conv16.hip) launches conv_kernel after its own with per-item domain words (ConvArgs::only): the blocks of an item
// inside the domain return at once, a flagged item gets the chain above.  Null - every other caller - means every item.
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"
#include "fgmm_hidden_act.h"

namespace fgmm {
namespace {

constexpr int kCB = kConvCB, kPR = kConvPR, kPC = kConvPC;

template <int K> struct ConvGeom {
  static constexpr int KK = K * K, KC = kCB * KK, NG = KC / 8; // taps; K entries and groups of four k-pairs per chunk
  static constexpr int HR = kPR + K - 1, HW = kPC + K - 1;     // the halo's rows and columns
  static constexpr int PITCH = 24, PLANE = K == 3 ? 264 : 312; // sH: floats between two rows, two channels (the head comment)
  static constexpr int ALD = KC + 4;                           // sA: floats between two rows
  static constexpr int HALO_N = kCB * HR * HW, HALO_J = (HALO_N + 255) / 256; // halo elements per chunk, per thread
  static constexpr int A_W = 8 * KC, A_J = (A_W + 255) / 256;  // 16-byte words of one packed tile, per thread
  static_assert(KC % 8 == 0 && NG % 2 == 1, "whole groups; the last group of a chunk is read into the first fragment");
  static_assert(HW <= PITCH && PITCH >= 20 && PITCH <= 26 && PLANE >= HR * PITCH && (PLANE - K * PITCH) % 64 == 0, "the bank argument");
  // K entry kappa of a chunk -> where its feature lies past the lane's own position
  __host__ __device__ static constexpr int off(int kappa) { return (kappa / KK) * PLANE + ((kappa % KK) / K) * PITCH + (kappa % KK) % K; }
};

// packed weights: [n_rt row tiles][n_ch chunks][32 rows][KC columns], then the bias [n_rt][32].  Column 8 g + 4 h + e of a row holds K
// entry kappa = 8 g + 2 e + h of the chunk - mfma32_pack_col's order within a group of four k-pairs: a lane's 16-byte read is its half's
// four.  kappa = c k^2 + t: channel CB ch + c, tap t.  Padding (rows past c_out, channels past c_in): +0.  TR (section 5e, stride 1): w is
// a ConvTranspose2d's [c_in, c_out, k, k], and tap t of the chain is its flipped tap k^2 - 1 - t = (k - 1 - a, k - 1 - b)
template <int K, bool TR>
__global__ __launch_bounds__(256) void conv_pack_kernel(const float *__restrict__ w, const float *__restrict__ bias, int c_out, int c_in, int n_rt, int n_ch,
                                                        float *__restrict__ wp, float *__restrict__ bp) {
  using G = ConvGeom<K>;
  const int64_t total = (int64_t)n_rt * n_ch * 32 * G::KC, n_bias = (int64_t)n_rt * 32;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total + n_bias; i += (int64_t)gridDim.x * 256) {
    if (i >= total) {
      const int64_t o = i - total;
      bp[o] = (o < c_out && bias) ? bias[o] : 0.0f;
      continue;
    }
    const int q = (int)(i % G::KC), r = (int)((i / G::KC) % 32);
    const int ch = (int)((i / (32 * G::KC)) % n_ch), rt = (int)(i / ((int64_t)32 * G::KC * n_ch));
    const int kappa = (q & ~7) + 2 * (q & 3) + ((q >> 2) & 1);
    const int c = ch * kCB + kappa / G::KK, t = kappa % G::KK;
    const int64_t o = (int64_t)rt * 32 + r;
    wp[i] = (o < c_out && c < c_in) ? (TR ? w[((int64_t)c * c_out + o) * G::KK + (G::KK - 1 - t)] : w[(o * c_in + c) * G::KK + t]) : 0.0f;
  }
}

// GRAD (header section 5f, the data gradient): 0 - the layer.  1 | 2 - x is gy, the gradient of a layer's stored output, and what is staged
// is gz: gy itself (1: FGMM_ACT_NONE, the saved output is never loaded) or grad_act(gy, saved output) (2), both read through the
// un-shuffle of the epilogue's store when g_shuffle is 2.  Everything past the staging is the layer's text
template <int K, int T, int GRAD = 0> // kernel size; row tiles per block
__global__ __launch_bounds__(256) void conv_kernel(ConvArgs a, int n_rg, int total) {
  using G = ConvGeom<K>;
  constexpr int kRows = 32 * T;
  __shared__ __attribute__((aligned(16))) float sA[kRows * G::ALD];
  __shared__ __attribute__((aligned(16))) float sH[kCB * G::PLANE];
  const int L = head_slot();
  if (L >= total) return;
  // the row groups of one patch are consecutive slots of one XCD: its L2 holds the patch's planes
  const int per_item = a.ph * a.pw * n_rg;
  const int item = L / per_item, rem = L - item * per_item, patch = rem / n_rg, rg = rem - patch * n_rg;
  if (a.only && !a.only[(int64_t)item * a.only_stride]) return; // a bf16x6 call (fgmm_conv16.hip), and the item is inside its domain
  const int py = patch / a.pw, r0 = py * kPR, q0 = (patch - py * a.pw) * kPC;
  const int hgt = a.h, wid = a.w, c_in = a.c_in;
  const int64_t hw = (int64_t)hgt * wid;
  const float *x = a.x + (int64_t)item * a.x_item_stride;
  // GRAD: gy's plane [c_in / 4, 2 h, 2 w] holds channel c at (c >> 2, 2 r + ((c >> 1) & 1), 2 q + (c & 1)) - the epilogue's store, inverted
  const bool g_sh = GRAD && a.g_shuffle == 2;
  const float *g_out = GRAD == 2 ? a.g_out + (int64_t)item * a.x_item_stride : nullptr;
  auto g_plane = [&](int c) { return g_sh ? (int64_t)(c >> 2) * 4 * hw + ((c >> 1) & 1) * 2 * wid + (c & 1) : (int64_t)c * hw; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  // the thread's halo elements e = tid + 256 j = (channel of the chunk, halo row, halo column): where they lie in a plane of the
  // image - the same for every chunk
  int goff[G::HALO_J];
  unsigned g_in = 0; // bit j: element j is one of the halo's and lies inside the image
#pragma unroll
  for (int j = 0; j < G::HALO_J; ++j) {
    const int e = tid + 256 * j;
    const int r = r0 + (e / G::HW) % G::HR - K / 2, q = q0 + e % G::HW - K / 2;
    const bool in = e < G::HALO_N && ckbd_inside(r, q, hgt, wid);
    goff[j] = in ? (g_sh ? 4 * r * wid + 2 * q : r * wid + q) : 0;
    g_in |= (in ? 1u : 0u) << j;
  }
  // ---- accumulators start at the bias
  f16_t acc[T];
  {
    const float *bp = a.bp + (int64_t)rg * kRows;
#pragma unroll
    for (int tl = 0; tl < T; ++tl) head_bias_tile(bp, tl, h, acc[tl]);
  }
  // ---- staging, branch-free in its loads: a load that would fall outside (a tile's words past its last, halo elements outside the
  // image or past the halo, channels past c_in) reads a valid address instead; what is written is decided when the chunk is stored
  const int n_ch = a.n_ch;
  const int64_t rt_words = (int64_t)n_ch * G::A_W;                 // 16-byte words between the packed row tiles
  const float *wp = a.wp + (int64_t)rg * T * rt_words * 4;          // row tile rg * T + tl, chunk ch: at wp + (tl * rt_words + ch * A_W) * 4
  float4_t ra[T][G::A_J];
  float rb[G::HALO_J];
  [[maybe_unused]] float ro[GRAD == 2 ? G::HALO_J : 1]; // GRAD 2: the saved output beside gy
  unsigned rb_ok = 0, rb_ch = 0; // bit j: rb[j] is an element inside the image of a channel below c_in; its channel is below c_in
  auto load_chunk = [&](int ch) {
    rb_ok = 0, rb_ch = 0;
    const float *tile = wp + (int64_t)ch * G::A_W * 4;
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int jj = 0; jj < G::A_J; ++jj) {
        const int f = tid + 256 * jj;
        ra[tl][jj] = mfma32_load_a(tile, (int64_t)tl * rt_words + ((f < G::A_W ? f : G::A_W - 1) - tid));
      }
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j) {
      const int c = ch * kCB + (tid + 256 * j) / (G::HR * G::HW);
      const bool k_ok = c < c_in;
      if constexpr (GRAD) {
        const int64_t at = g_plane(k_ok ? c : c_in - 1) + goff[j];
        rb[j] = ((const FGMM_GLOBAL float *)x)[at];
        if constexpr (GRAD == 2) ro[j] = ((const FGMM_GLOBAL float *)g_out)[at];
      } else {
        rb[j] = ((const FGMM_GLOBAL float *)(x + (int64_t)(k_ok ? c : c_in - 1) * hw))[goff[j]];
      }
      rb_ok |= (k_ok ? (g_in >> j) & 1u : 0u) << j;
      rb_ch |= (k_ok ? 1u : 0u) << j;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int jj = 0; jj < G::A_J; ++jj) {
        const int f = tid + 256 * jj;
        if (f < G::A_W) *reinterpret_cast<float4_t *>(&sA[(tl * 32 + f / (G::KC / 4)) * G::ALD + (f % (G::KC / 4)) * 4]) = ra[tl][jj];
      }
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j) {
      const int e = tid + 256 * j;
      float v = rb[j];
      if constexpr (GRAD == 2) v = grad_act(v, ro[j], a.g_act == FGMM_ACT_RELU, a.g_slope); // the select: here, where the loads have landed
      v = (rb_ok >> j) & 1u ? v : ((rb_ch >> j) & 1u ? 0.0f : -0.0f);
      if (e < G::HALO_N) sH[(e / (G::HR * G::HW)) * G::PLANE + ((e / G::HW) % G::HR) * G::PITCH + e % G::HW] = v;
    }
  };
  // ---- fragments of group g of the chunk: one 16-byte A read per row tile, one 4-byte B read per k-pair
  const float *a_base = sA + col * G::ALD + h * 4;
  const float *b_base = sH + (2 * wave + (col >> 4)) * G::PITCH + (col & 15);
  auto read_frag = [&](Mfma32Frag<T> &f, int g) {
#pragma unroll
    for (int tl = 0; tl < T; ++tl) f.a[tl] = *reinterpret_cast<const float4_t *>(a_base + tl * 32 * G::ALD + g * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) f.b[e] = b_base[h ? G::off(8 * g + 2 * e + 1) : G::off(8 * g + 2 * e)];
  };
#define FGMM_FENCE() __builtin_amdgcn_sched_barrier(0)
  load_chunk(0);
  store_chunk();
  __syncthreads();
  Mfma32Frag<T> f0, f1;
  read_frag(f0, 0);
  for (int ch = 0; ch < n_ch; ++ch) {
    // 4 T products per wave and group; before a group's, what a LATER step needs is issued: the global loads of the next chunk (the
    // last chunk loads itself again: harmless) and the fragments of the next group
    FGMM_FENCE();
    load_chunk(ch + 1 < n_ch ? ch + 1 : ch);
#pragma unroll
    for (int g = 0; g + 1 < G::NG; g += 2) {
      read_frag(f1, g + 1);
      FGMM_FENCE();
      mfma32_multiply(acc, f0);
      FGMM_FENCE();
      read_frag(f0, g + 2);
      FGMM_FENCE();
      mfma32_multiply(acc, f1);
      FGMM_FENCE();
    }
    mfma32_multiply(acc, f0);
    FGMM_FENCE();
    __syncthreads(); // every wave has read the chunk
    store_chunk();
    __syncthreads();
    read_frag(f0, 0); // (after the last chunk: a read that nobody uses)
  }
#undef FGMM_FENCE
  // ---- epilogue: register reg of row tile tl is output channel (rg * T + tl) * 32 + mfma32_row(reg, h) at the lane's position
  const int r = r0 + 2 * wave + (col >> 4), q = q0 + (col & 15);
  if (r >= hgt || q >= wid) return;
  const bool sh = a.shuffle == 2;
  // shuffle 2: channel o of the convolution is plane o >> 2, row 2 r + ((o >> 1) & 1), column 2 q + (o & 1) of [c_out / 4, 2 h, 2 w]
  const int64_t plane = sh ? 4 * hw : hw, w_out = sh ? 2 * wid : wid;
  float *out = a.out + (int64_t)item * a.c_out * hw + (sh ? 2 * r * w_out + 2 * q : r * w_out + q);
  auto store = [&](auto act) {
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
        const int64_t at = sh ? (int64_t)(o >> 2) * plane + ((o >> 1) & 1) * w_out + (o & 1) : (int64_t)o * plane;
        if (o < a.c_out) stg<float>(out + at, act(acc[tl][reg]));
      }
  };
  with_activation(a.act, a.slope, store);
}

template <int K, int T, int GRAD = 0> static int conv_go(const ConvArgs &a, int64_t n, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T;
  const int64_t total = n * a.ph * a.pw * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8); // every XCD gets as many slots (head_slot)
  hipLaunchKernelGGL((conv_kernel<K, T, GRAD>), dim3(blocks), dim3(256), 0, st, a, n_rg, (int)total);
  return (int)hipGetLastError();
}

template <int K, bool TR> static int conv_pack_go(const float *w, const float *bias, int c_out, int c_in, float *wp, float *bp, hipStream_t st) {
  const int64_t total = (int64_t)conv_packed_floats(c_out, c_in, K);
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL((conv_pack_kernel<K, TR>), dim3(grid), dim3(256), 0, st, w, bias, c_out, c_in, conv_row_tiles(c_out), conv_chunks(c_in), wp, bp);
  return (int)hipGetLastError();
}

} // namespace

int launch_conv_pack(const float *w, const float *bias, int c_out, int c_in, int k, bool transposed, float *wp, float *bp, void *stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (transposed) return k == 3 ? conv_pack_go<3, true>(w, bias, c_out, c_in, wp, bp, st) : conv_pack_go<5, true>(w, bias, c_out, c_in, wp, bp, st);
  return k == 3 ? conv_pack_go<3, false>(w, bias, c_out, c_in, wp, bp, st) : conv_pack_go<5, false>(w, bias, c_out, c_in, wp, bp, st);
}

// T: the most row tiles per block (4, 2, 1) at which the launch - n * patches blocks per group of T row tiles - still has a block for
// every CU; 1 when none has
int launch_conv(const ConvArgs &args, int k, int64_t n, void *stream) {
  return ckbd_row_tiles_go<4, 2, 1>(n * args.ph * args.pw, args.c_out, [&](auto T) {
    return k == 3 ? conv_go<3, T>(args, n, (hipStream_t)stream) : conv_go<5, T>(args, n, (hipStream_t)stream);
  });
}

// the data gradient (section 5f): the same kernel, block heights by the same rule over its output's rows (the layer's c_in)
int launch_conv_dgrad(const ConvArgs &args, int k, int64_t n, void *stream) {
  const hipStream_t st = (hipStream_t)stream;
  return ckbd_row_tiles_go<4, 2, 1>(n * args.ph * args.pw, args.c_out, [&](auto T) {
    if (args.g_act == FGMM_ACT_NONE) return k == 3 ? conv_go<3, T, 1>(args, n, st) : conv_go<5, T, 1>(args, n, st);
    return k == 3 ? conv_go<3, T, 2>(args, n, st) : conv_go<5, T, 2>(args, n, st);
  });
}

} // namespace fgmm
