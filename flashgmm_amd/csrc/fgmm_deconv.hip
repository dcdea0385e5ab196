// fgmm_deconv.hip — stride-2 transposed 3x3 / 5x5 convolutions (padding k / 2, output padding 1) on the matrix cores, in one fixed order
// (header section 5e).
//
// What it replaces: the two ConvTranspose2d(.., 5, stride=2, padding=2, output_padding=1) layers of ELIC's hyper-synthesis h_s
// (compressai/models/elic_gmm.py:142-148, deconv in models/utils.py:160-168), which MIOpen computed from the decoded z_hat.  (The third
// layer, stride 1, is section 5d's chain over the flipped, transposed weights: conv_pack_kernel<K, true> and conv_kernel, fgmm_conv.hip.)
//
// Arithmetic: per item i, output channel o and OUTPUT position (R, Q) of 2 h x 2 w, on v_mfma_f32_32x32x2_f32, bit for bit the chain
//     acc = bias[o] (+0 without);  for c ascending, for a' = 0 .. k - 1, b' = 0 .. k - 1 ascending with u = R + a' - k/2 and v = Q + b' - k/2 BOTH even:
//         acc = fmaf(W[c][o][k - 1 - a'][k - 1 - b'], x[i][c][u / 2][v / 2] (inside the image, else +0), acc);      out = act(acc)
// A tap with u or v odd is NO term (the zeros a zero-stuffed input would hold are not multiplied: 0 * inf never arises from them, a -0
// accumulator stays -0); a tap outside the image is a +0 TERM, as in 5b and 5d.
//   phases  : output (2 r + pr, 2 q + pc) of input position (r, q) is one of four PHASES p = 2 pr + pc, each a small dense convolution on
//             the INPUT grid with its own taps: along one axis parity 0 keeps a' = 0, 2, 4 (k = 5: input r - 1, r, r + 1) | a' = 1 (k = 3:
//             r), parity 1 keeps a' = 1, 3 (r, r + 1) | a' = 0, 2 (r, r + 1).  Taps per phase 9 | 6 | 6 | 4 (k = 5), 1 | 2 | 2 | 4 (k = 3): 25 | 9
//             products per channel and input position, the number the operator has.
//   block   = T row tiles of 32 output channels x an 8 x 16 PATCH of INPUT positions (5d's: wave wv owns patch rows 2 wv, 2 wv + 1, lane
//             column col = lane & 31 is position (2 wv + (col >> 4), col & 15), lane half h = lane >> 5 the odd k of a pair) x its phases:
//             all four (16 x 32 outputs a channel, four accumulator sets) or one.
//   K loop  = chunks of 8 input channels; a phase with nt taps has 8 nt K entries a chunk = nt whole groups of four k-pairs, K entry
//             kappa = c nt + ta ntc + tb (channel, kept tap row, kept tap column).  Per chunk the block stages, ONCE for all its phases,
//             (a) its packed weights: per row tile and phase [32 rows][8 nt], 16-byte loads, into sA with a row pitch of 8 nt + 4 floats
//             (76, 52, 36 | 12, 20, 36: 4 x an odd number - the 16 rows of a quarter wave's 16-byte reads start at 16 distinct multiples of
//             4 mod 64) and (b) the patch and its halo of the 8 channels into sH: 10 x 18 elements a channel for k = 5 (one row and column
//             on either side), 9 x 17 for k = 3 (the high side only); outside the image +0, a channel past c_in -0 over +0 weights (5d).
//   B reads = ONE 4-byte LDS read at sH[lane base + off(p, kappa)], off a literal of the unrolled loop (5d).  PITCH = 24, PLANE = 264
//             (k = 5) | 216 (k = 3).  The bank argument is 5d's with the phase's window: a k-pair's two entries lie d = 1 apart inside a
//             kept tap row, d = PITCH - (ntc - 1) = 24, 23, 22 at the end of one - runs [0, 15], [24, 39], [d, d + 15], [24 + d, 39 + d]
//             end below 64, and where they overlap the lanes read the SAME address - and d = PLANE - (ntr - 1) PITCH - (ntc - 1) at the
//             end of a channel.  A pair straddles a channel only where nt is odd: phase 0 alone (9 taps, ntr = 3 | 1 tap, ntr = 1); the
//             phases with 6, 4 and 2 taps never do, so ONE PLANE serves: PLANE = ntr(0) PITCH mod 64 makes phase 0's step the end-of-row
//             case (264 = 72, 216 = 24 mod 64).  No read of the loop collides.
//   loop    : 5d's - one LDS buffer, two barriers per chunk, the next chunk's global loads issued before this chunk's first product,
//             the fragments read one group ahead, the products of a chunk ONE fenced basic block.  The groups of the block's phases are
//             ONE sequence (25 | 9 for four phases; 9, 6, 6, 4 | 1, 2, 2, 4 for one), unrolled by index, so odd and even counts read alike.
//   forms   : 1. four phases, T = 2;  2. four phases, T = 1;  3. ONE phase per block, T = 1: four times the blocks, the halo staged once
//             per phase, phase 0 (the most taps) first within a patch.  The first of 1, 2 with at least 256 workgroups, else 3 (h_s sees
//             8 x 12 planes: one patch).  An output's chain depends on none of the form, n, the item's place, its patch: the same bits.
//   epilogue: the activation, then out[i][o][2 r + pr][2 q + pc]: 4-byte stores (an 8-byte store of the two column phases would ask `out`
//             for 8-byte alignment, which the ABI does not).  Lanes outside the image and rows past c_out store nothing.
// No atomics, no workspace.
#include <utility>
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"
#include "fgmm_hidden_act.h"

namespace fgmm {
namespace {

constexpr int kCB = kConvCB, kPR = kConvPR, kPC = kConvPC;

template <int K> struct DeconvGeom {
  static constexpr int KK = K * K, KC = kCB * KK;  // taps; K entries per chunk over the four phases
  static constexpr int LO = K == 5 ? 1 : 0;        // halo rows / columns before the patch
  static constexpr int HR = kPR + LO + 1, HW = kPC + LO + 1;
  static constexpr int PITCH = 24, PLANE = K == 5 ? 264 : 216; // sH: floats between two rows, two channels (the head comment)
  static constexpr int HALO_N = kCB * HR * HW, HALO_J = (HALO_N + 255) / 256;
  // one axis, output parity par: the kept taps a' = first + 2 j, j < count, and the halo row / column past the lane's own it reads
  __host__ __device__ static constexpr int first(int par) { return (par + K / 2) & 1; }
  __host__ __device__ static constexpr int count(int par) { return (K - first(par) + 1) / 2; }
  __host__ __device__ static constexpr int tap(int par, int j) { return first(par) + 2 * j; }
  __host__ __device__ static constexpr int halo(int par, int j) { return (par + tap(par, j) - K / 2 + 2 * LO) / 2; }
  // phase p = 2 pr + pc
  __host__ __device__ static constexpr int ntr(int p) { return count(p >> 1); }
  __host__ __device__ static constexpr int ntc(int p) { return count(p & 1); }
  __host__ __device__ static constexpr int nt(int p) { return ntr(p) * ntc(p); }   // taps = groups of four k-pairs per chunk
  __host__ __device__ static constexpr int gbeg(int p) { return p <= 0 ? 0 : gbeg(p - 1) + nt(p - 1); } // groups before phase p; gbeg(4) = KK
  __host__ __device__ static constexpr int ald(int p) { return 8 * nt(p) + 4; }     // sA: floats between two rows of phase p
  __host__ __device__ static constexpr int abeg(int p) { return p <= 0 ? 0 : abeg(p - 1) + 32 * ald(p - 1); } // sA floats of a row tile before phase p
  __host__ __device__ static constexpr int phase_of(int g) { return g < gbeg(1) ? 0 : g < gbeg(2) ? 1 : g < gbeg(3) ? 2 : 3; } // of group g of the chunk
  __host__ __device__ static constexpr int off(int p, int kappa) {
    return (kappa / nt(p)) * PLANE + halo(p >> 1, (kappa % nt(p)) / ntc(p)) * PITCH + halo(p & 1, (kappa % nt(p)) % ntc(p));
  }
};

template <int I, int N, typename F> __device__ __forceinline__ void static_for(const F &f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// packed weights: [n_rt row tiles][n_ch chunks][4 phases][32 rows][8 nt(p) columns], then the bias [n_rt][32] - conv_packed_floats'
// size.  Column 8 g + 4 h + e of a row holds K entry kappa = 8 g + 2 e + h of the phase's chunk (mfma32_pack_col's order within a group),
// kappa = c nt + ta ntc + tb: channel 8 ch + c, tap (a', b') = (tap(pr, ta), tap(pc, tb)), weight[c][o][k - 1 - a'][k - 1 - b'] of torch's
// [c_in, c_out, k, k].  Padding (rows past c_out, channels past c_in): +0
template <int K>
__global__ __launch_bounds__(256) void deconv_pack_kernel(const float *__restrict__ w, const float *__restrict__ bias, int c_out, int c_in, int n_rt, int n_ch,
                                                          float *__restrict__ wp, float *__restrict__ bp) {
  using G = DeconvGeom<K>;
  const int64_t total = (int64_t)n_rt * n_ch * 32 * G::KC, n_bias = (int64_t)n_rt * 32;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total + n_bias; i += (int64_t)gridDim.x * 256) {
    if (i >= total) {
      const int64_t o = i - total;
      bp[o] = (o < c_out && bias) ? bias[o] : 0.0f;
      continue;
    }
    const int j = (int)(i % (32 * G::KC)); // within the (row tile, chunk)
    const int ch = (int)((i / (32 * G::KC)) % n_ch), rt = (int)(i / ((int64_t)32 * G::KC * n_ch));
    const int p = G::phase_of(j / 256), nt = G::nt(p), ntc = G::ntc(p), jp = j - 256 * G::gbeg(p); // (phase p begins at float 32 * 8 gbeg(p))
    const int q = jp % (8 * nt), r = jp / (8 * nt);
    const int kappa = (q & ~7) + 2 * (q & 3) + ((q >> 2) & 1);
    const int c = ch * kCB + kappa / nt, t = kappa % nt;
    const int at = G::tap(p >> 1, t / ntc), bt = G::tap(p & 1, t % ntc);
    const int64_t o = (int64_t)rt * 32 + r;
    wp[i] = (o < c_out && c < c_in) ? w[((int64_t)c * c_out + o) * G::KK + (K - 1 - at) * K + (K - 1 - bt)] : 0.0f;
  }
}

// one block: phases [P0, P1) of patch `patch` of item `item`, row tiles rg * T .. + T - 1.  P < 0: all four
template <int K, int T, int P>
__device__ __forceinline__ void deconv_block(const ConvArgs &a, float *sA, float *sH, int item, int patch, int rg) {
  using G = DeconvGeom<K>;
  constexpr int P0 = P < 0 ? 0 : P, P1 = P < 0 ? 4 : P + 1, NP = P1 - P0;
  constexpr int G0 = G::gbeg(P0), NG = G::gbeg(P1) - G0;       // the block's groups of a chunk
  constexpr int A_W = 64 * NG, A_J = (A_W + 255) / 256;       // 16-byte words of its part of one packed tile (8 per row and group), per thread
  constexpr int A_WT = 8 * G::KC;                             // ... of a whole packed tile
  constexpr int TILE = G::abeg(P1) - G::abeg(P0);             // sA floats of one row tile
  constexpr int kRows = 32 * T;
  const int py = patch / a.pw, r0 = py * kPR, q0 = (patch - py * a.pw) * kPC;
  const int hgt = a.h, wid = a.w, c_in = a.c_in;
  const int64_t hw = (int64_t)hgt * wid;
  const float *x = a.x + (int64_t)item * a.x_item_stride;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  // the thread's halo elements e = tid + 256 j = (channel of the chunk, halo row, halo column): where they lie in a plane of the image
  int goff[G::HALO_J];
  unsigned g_in = 0; // bit j: element j is one of the halo's and lies inside the image
#pragma unroll
  for (int j = 0; j < G::HALO_J; ++j) {
    const int e = tid + 256 * j;
    const int r = r0 + (e / G::HW) % G::HR - G::LO, q = q0 + e % G::HW - G::LO;
    const bool in = e < G::HALO_N && ckbd_inside(r, q, hgt, wid);
    goff[j] = in ? r * wid + q : 0;
    g_in |= (in ? 1u : 0u) << j;
  }
  // ... and where its 16-byte words f = tid + 256 jj of the block's part of a packed tile go in sA: phase, row, four columns
  int sa_at[A_J];
#pragma unroll
  for (int jj = 0; jj < A_J; ++jj) {
    const int f = tid + 256 * jj;
    int at = 0;
    static_for<P0, P1>([&](auto PP) {
      constexpr int p = PP, w0 = 64 * (G::gbeg(p) - G0), w1 = 64 * (G::gbeg(p + 1) - G0), rw = 2 * G::nt(p); // the phase's words; per row
      if (f >= w0 && f < w1) at = G::abeg(p) - G::abeg(P0) + ((f - w0) / rw) * G::ald(p) + ((f - w0) % rw) * 4;
    });
    sa_at[jj] = at;
  }
  // ---- accumulators start at the bias, one set per phase
  f16_t acc[NP][T];
  {
    const float *bp = a.bp + (int64_t)rg * kRows;
#pragma unroll
    for (int tl = 0; tl < T; ++tl) {
      head_bias_tile(bp, tl, h, acc[0][tl]);
#pragma unroll
      for (int p = 1; p < NP; ++p) acc[p][tl] = acc[0][tl];
    }
  }
  // ---- staging, branch-free in its loads (5d): a load that would fall outside reads a valid address instead; what is written is
  // decided when the chunk is stored
  const int n_ch = a.n_ch;
  const int64_t rt_words = (int64_t)n_ch * A_WT;
  const float *wp = a.wp + ((int64_t)rg * T * rt_words + 64 * G0) * 4; // row tile rg * T + tl, chunk ch: at wp + (tl * rt_words + ch * A_WT) * 4
  float4_t ra[T][A_J];
  float rb[G::HALO_J];
  unsigned rb_ok = 0, rb_ch = 0; // bit j: rb[j] is an element inside the image of a channel below c_in; its channel is below c_in
  auto load_chunk = [&](int ch) {
    rb_ok = 0, rb_ch = 0;
    const float *tile = wp + (int64_t)ch * A_WT * 4;
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int jj = 0; jj < A_J; ++jj) {
        const int f = tid + 256 * jj;
        ra[tl][jj] = mfma32_load_a(tile, (int64_t)tl * rt_words + ((f < A_W ? f : A_W - 1) - tid));
      }
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j) {
      const int c = ch * kCB + (tid + 256 * j) / (G::HR * G::HW);
      const bool k_ok = c < c_in;
      rb[j] = ((const FGMM_GLOBAL float *)(x + (int64_t)(k_ok ? c : c_in - 1) * hw))[goff[j]];
      rb_ok |= (k_ok ? (g_in >> j) & 1u : 0u) << j;
      rb_ch |= (k_ok ? 1u : 0u) << j;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int jj = 0; jj < A_J; ++jj)
        if (tid + 256 * jj < A_W) *reinterpret_cast<float4_t *>(&sA[tl * TILE + sa_at[jj]]) = ra[tl][jj];
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j) {
      const int e = tid + 256 * j;
      const float v = (rb_ok >> j) & 1u ? rb[j] : ((rb_ch >> j) & 1u ? 0.0f : -0.0f);
      if (e < G::HALO_N) sH[(e / (G::HR * G::HW)) * G::PLANE + ((e / G::HW) % G::HR) * G::PITCH + e % G::HW] = v;
    }
  };
  // ---- fragments of group i of the block's sequence = group g of phase p: one 16-byte A read per row tile, one 4-byte B read per k-pair
  const float *a_base[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) a_base[p] = sA + (G::abeg(P0 + p) - G::abeg(P0)) + col * G::ald(P0 + p) + h * 4;
  const float *b_base = sH + (2 * wave + (col >> 4)) * G::PITCH + (col & 15);
  auto read_frag = [&](Mfma32Frag<T> &f, auto I) {
    constexpr int p = G::phase_of(G0 + I), g = G0 + I - G::gbeg(p);
#pragma unroll
    for (int tl = 0; tl < T; ++tl) f.a[tl] = *reinterpret_cast<const float4_t *>(a_base[p - P0] + tl * TILE + g * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) f.b[e] = b_base[h ? G::off(p, 8 * g + 2 * e + 1) : G::off(p, 8 * g + 2 * e)];
  };
#define FGMM_FENCE() __builtin_amdgcn_sched_barrier(0)
  load_chunk(0);
  store_chunk();
  __syncthreads();
  Mfma32Frag<T> f0, f1;
  read_frag(f0, std::integral_constant<int, 0>{});
  for (int ch = 0; ch < n_ch; ++ch) {
    // 4 T products per wave and group; before a group's, what a LATER step needs is issued: the global loads of the next chunk (the
    // last chunk loads itself again: harmless) and the fragments of the next group (even groups in f0, odd ones in f1)
    FGMM_FENCE();
    load_chunk(ch + 1 < n_ch ? ch + 1 : ch);
    static_for<0, NG>([&](auto I) {
      constexpr int i = I, p = G::phase_of(G0 + i) - P0;
      if constexpr (i + 1 < NG) read_frag(i & 1 ? f0 : f1, std::integral_constant<int, i + 1>{});
      FGMM_FENCE();
      mfma32_multiply(acc[p], i & 1 ? f1 : f0);
      FGMM_FENCE();
    });
    __syncthreads(); // every wave has read the chunk
    store_chunk();
    __syncthreads();
    read_frag(f0, std::integral_constant<int, 0>{}); // (after the last chunk: a read that nobody uses)
  }
#undef FGMM_FENCE
  // ---- epilogue: register reg of row tile tl of phase p is output channel (rg * T + tl) * 32 + mfma32_row(reg, h) at output position
  // (2 r + pr, 2 q + pc) of the lane's input position (r, q)
  const int r = r0 + 2 * wave + (col >> 4), q = q0 + (col & 15);
  if (r >= hgt || q >= wid) return;
  const int64_t plane = 4 * hw;
  const int w_out = 2 * wid;
  float *out = a.out + (int64_t)item * a.c_out * plane + (int64_t)2 * r * w_out + 2 * q;
  auto store = [&](auto act) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int tl = 0; tl < T; ++tl)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
          if (o < a.c_out) stg<float>(out + (int64_t)o * plane + ((P0 + p) >> 1) * w_out + ((P0 + p) & 1), act(acc[p][tl][reg]));
        }
  };
  with_activation(a.act, a.slope, store);
}

template <int K, int T, bool ALL> // kernel size; row tiles per block; four phases per block, or one (T = 1)
__global__ __launch_bounds__(256) void deconv_kernel(ConvArgs a, int n_rg, int total) {
  using G = DeconvGeom<K>;
  static_assert(ALL || T == 1, "one phase per block: one row tile");
  static_assert(G::gbeg(4) == G::KK && G::nt(0) % 2 == 1 && G::nt(1) % 2 == 0 && G::nt(2) % 2 == 0 && G::nt(3) % 2 == 0, "only phase 0 has pairs across channels");
  static_assert(G::HW <= G::PITCH && G::PLANE >= G::HR * G::PITCH && (G::PLANE - G::ntr(0) * G::PITCH) % 64 == 0 && 2 * G::PITCH + 16 <= 64, "the bank argument");
  static_assert(kPR - 1 + G::halo(1, G::count(1) - 1) < G::HR && kPC - 1 + G::halo(1, G::count(1) - 1) < G::HW && G::halo(0, 0) == 0, "the window lies in the halo");
  constexpr int kAFloats = ALL ? T * G::abeg(4) : 32 * (G::ald(0) > G::ald(3) ? G::ald(0) : G::ald(3));
  __shared__ __attribute__((aligned(16))) float sA[kAFloats];
  __shared__ __attribute__((aligned(16))) float sH[kCB * G::PLANE];
  const int L = head_slot();
  if (L >= total) return;
  // the blocks of one patch (its phases, their row groups) are consecutive slots of one XCD: its L2 holds the patch's planes
  constexpr int NPB = ALL ? 1 : 4;
  const int per_patch = NPB * n_rg, per_item = a.ph * a.pw * per_patch;
  const int item = L / per_item, rem = L - item * per_item, patch = rem / per_patch, sub = rem - patch * per_patch;
  if constexpr (ALL) {
    deconv_block<K, T, -1>(a, sA, sH, item, patch, sub);
  } else {
    const int phase = sub / n_rg, rg = sub - phase * n_rg; // phase 0, the one with the most taps (k = 5), first
    switch (phase) {
    case 0: deconv_block<K, 1, 0>(a, sA, sH, item, patch, rg); break;
    case 1: deconv_block<K, 1, 1>(a, sA, sH, item, patch, rg); break;
    case 2: deconv_block<K, 1, 2>(a, sA, sH, item, patch, rg); break;
    default: deconv_block<K, 1, 3>(a, sA, sH, item, patch, rg); break;
    }
  }
}

template <int K, int T, bool ALL> static int deconv_go(const ConvArgs &a, int64_t n, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T;
  const int64_t total = n * a.ph * a.pw * n_rg * (ALL ? 1 : 4);
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8); // every XCD gets as many slots (head_slot)
  hipLaunchKernelGGL((deconv_kernel<K, T, ALL>), dim3(blocks), dim3(256), 0, st, a, n_rg, (int)total);
  return (int)hipGetLastError();
}

template <int K> static int deconv_pack_go(const float *w, const float *bias, int c_out, int c_in, float *wp, float *bp, hipStream_t st) {
  const int64_t total = (int64_t)conv_packed_floats(c_out, c_in, K);
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(deconv_pack_kernel<K>, dim3(grid), dim3(256), 0, st, w, bias, c_out, c_in, conv_row_tiles(c_out), conv_chunks(c_in), wp, bp);
  return (int)hipGetLastError();
}

template <int K> static int deconv_form_go(const ConvArgs &a, int64_t n, hipStream_t st) {
  switch (deconv_form(n * a.ph * a.pw, a.c_out)) {
  case 1: return deconv_go<K, 2, true>(a, n, st);
  case 2: return deconv_go<K, 1, true>(a, n, st);
  }
  return deconv_go<K, 1, false>(a, n, st);
}

} // namespace

int launch_deconv_pack(const float *w, const float *bias, int c_out, int c_in, int k, float *wp, float *bp, void *stream) {
  if (k == 3) return deconv_pack_go<3>(w, bias, c_out, c_in, wp, bp, (hipStream_t)stream);
  return deconv_pack_go<5>(w, bias, c_out, c_in, wp, bp, (hipStream_t)stream);
}

int launch_deconv(const ConvArgs &args, int k, int64_t n, void *stream) {
  return k == 3 ? deconv_form_go<3>(args, n, (hipStream_t)stream) : deconv_form_go<5>(args, n, (hipStream_t)stream);
}

} // namespace fgmm
