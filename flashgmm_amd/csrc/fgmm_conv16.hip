// fgmm_conv16.hip — the dense 3x3 / 5x5 convolution layer on the BF16 matrix cores with binary32 accuracy ("bf16x6"), an OPTION beside
// the exact form of fgmm_conv.hip (FGMM_CONV_BF16X6 at fgmm_conv_create_ex; header section 5d).
//
// Arithmetic: the sum section 5d defines - the bias, the c_in channels, the k^2 taps row-major of each, a tap outside the image +0 -
// evaluated as fgmm_ckbd_ctx16.hip evaluates its sum: every weight and every input is split3's three bfloat16 parts (fgmm_split3.h), a
// product is the six part products (w1,x3) (w3,x1) (w2,x2) (w1,x2) (w2,x1) (w1,x1), smallest first, each ONE v_mfma_f32_32x32x16_bf16
// over 16 input channels OF ONE TAP, accumulated in binary32 from the bias; K tiles ascend with the channel tile of 16 outer and the tap
// (a k + b) inner: n16 = k^2 ceil(c_in / 16) matrix steps of six products; channels past c_in and taps outside the image are zero in all
// three parts.  Then fgmm_hidden_act.h's activation on the accumulator and conv_kernel's plain or PixelShuffle(2) store.
// Bound (tests/conv16_ref.py): tests/head_ref.py's bf16x6 derivation over W.reshape(c_out, c_in k^2), im2col(x) with this n16.
// What it is NOT: a sequence a CPU can restate bit for bit.  What it is: the SAME BITS FROM EVERY LAUNCH - an output's bits are a
// function of its row of the weights, its bias and the inputs its taps read: not of the block height, of n, of the item's place in a
// batch or in its patch (a matrix step's rows and columns do not mix; every padding is a zero operand in every launch shape alike).
// Domain: finite operands with |v| < 0x1.FFp127.  Weights outside are refused at creation; an ITEM with an input outside is flagged by
// the split kernel and computed by conv_kernel (fgmm_conv.hip, launched after this one with the flags): bit for bit the chain.
//
// Design.  Three launches per call: head16_split_kernel (fgmm_head16.hip: the input -> [channel tile of 16][part][position][16 channels]
// bf16, once per call - the k^2 taps and the row groups would otherwise each split the same inputs), conv16_kernel, and conv_kernel for
// the flagged items (its blocks return at once otherwise).
//   block  = 256 threads = 4 waves; T row tiles of 32 output channels x conv_kernel's 8 x 16 patch: wave wv owns patch rows 2 wv,
//            2 wv + 1, lane column col = lane & 31 is position (2 wv + (col >> 4), col & 15), lane half h = lane >> 5 the k half.  T = 4,
//            2 or 1 by conv_kernel's rule (the tallest that still gives every CU a block).
//   halo   = the patch with its halo - (8 + k - 1) x (16 + k - 1) positions x 3 parts x 2 k halves of sixteen-byte chunks, 1080 | 1440 -
//            is staged ONCE per channel tile, not once per tap, as [part][k half][halo position][8 bf16], double-buffered across channel
//            tiles: an input crosses from global memory once per block and channel tile, and all k^2 taps read the same staged halo.  A
//            position outside the image is staged as zeros (the load reads a valid address, the select is applied at the store);
//            channels past c_in are zeros in the split copy already.  A thread's chunks - (part, position, k half), the k half fastest:
//            32 contiguous bytes of the split copy per position - are the same for every channel tile: offsets and mask are computed once.
//   B read = tap (a, b)'s operand of a part is ONE sixteen-byte LDS read at the lane's base + (a HW + b), a literal (the tap loop is
//            unrolled).  Banks (64 of 4 bytes; a 16-byte read is served a quarter wave at a time): the 16 lanes of a quarter wave are
//            one patch row of one k half - 16 consecutive halo positions, 256 contiguous bytes, every bank once.  No read collides, at
//            any tap.  The (part, k half) planes are PLANE = 184 | 248 chunks apart, 8 mod 16: the two threads that stage the two k
//            halves of a position write 128 bytes apart mod 256 - sixteen lanes' writes cover every bank once.
//   W ring = the packed weights have the order of the LDS tile, [part][k half][32 rows][8 bf16], 3072 contiguous bytes per row tile and
//            matrix step: copied chunk for chunk into a ring of two buffers, ONE barrier per matrix step; a lane's operand is one
//            16-byte read, 32 lanes of a k half read 512 contiguous bytes.
//   LDS    = 2 halo buffers + 2 W buffers: 2 * 23 808 + 2 * 12 288 = 72 192 bytes at T = 4, k = 5 (35 328 + 24 576 at k = 3): two
//            blocks on a CU (160 KB), which __launch_bounds__(256, 2) keeps in registers too (8 waves a CU: 256 VGPRs each).
//   loads  = the weights of step s + D are issued before the products of step s, in D register sets (2 at T = 4 | 2, 4 at T = 1, where
//            a step is six products); the next channel tile's halo is issued at a tile's first tap and written at its last.  The loop
//            is unrolled over D channel tiles x k^2 taps, so register set, ring buffer and halo buffer of a step are literals.
//   products: row tiles in pairs - three W operands each, the three x operands shared - in the fixed order of the six parts.
// Placement (head_slot), the bias a tile starts from and the epilogue's register-to-row map: fgmm_headframe.h / fgmm_mfma32.h.
// No atomics, no scratch (build with -Rpass-analysis=kernel-resource-usage to see).
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"
#include "fgmm_hidden_act.h"
#include "fgmm_split3.h"

namespace fgmm {
namespace {

constexpr int kBK = kHead16BK;          // input channels per matrix step
constexpr int kPR = kConvPR, kPC = kConvPC;
constexpr int kAChunks = 3 * 2 * 32;    // sixteen-byte chunks of one row tile's W tile: [part][k half][32 rows]

template <int K> struct Conv16Geom {
  static constexpr int KK = K * K;
  static constexpr int HR = kPR + K - 1, HW = kPC + K - 1, HP = HR * HW; // the halo's rows, columns, positions
  static constexpr int PLANE = (HP + 7) / 16 * 16 + 8;                    // chunks between two (part, k half) planes
  static constexpr int HALO_N = 6 * HP, HALO_J = (HALO_N + 255) / 256;    // chunks of one staged halo, per thread
  static constexpr int BUF = 6 * PLANE;                                   // chunks of one halo buffer
  static_assert(PLANE >= HP && PLANE % 16 == 8, "the bank argument");
  static_assert((kPR - 1 + K - 1) * HW + (kPC - 1) + (K - 1) == HP - 1, "the last tap of the last lane reads the halo's last position");
};

// one thread per (row tile, channel tile, tap, row, channel): its three parts.  n_rt = conv_row_tiles(c_out), n_ct = conv16_tiles(c_in)
template <int K>
__global__ __launch_bounds__(256) void conv16_pack_kernel(const float *__restrict__ w, int c_out, int c_in, int n_rt, int n_ct, uint16_t *__restrict__ wp,
                                                          uint32_t *__restrict__ bad) {
  constexpr int KK = K * K;
  const int64_t total = (int64_t)n_rt * n_ct * KK * 32 * kBK;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int kc = (int)(i % kBK), r = (int)((i / kBK) % 32);
    const int64_t step = i / (32 * kBK); // (rt * n_ct + ct) * KK + t
    const int t = (int)(step % KK), ct = (int)((step / KK) % n_ct), rt = (int)(step / ((int64_t)KK * n_ct));
    const int c = ct * kBK + kc;
    const int64_t o = (int64_t)rt * 32 + r;
    const float v = (o < c_out && c < c_in) ? w[(o * c_in + c) * KK + t] : 0.0f;
    if (!in_domain(v)) *bad = 1u;
    const Split3 s = split3(v);
    uint16_t *tile = wp + step * (kAChunks * 8);
#pragma unroll
    for (int part = 0; part < 3; ++part) tile[((part * 2 + (kc >> 3)) * 32 + r) * 8 + (kc & 7)] = s.p[part];
  }
}

template <int T> constexpr int conv16_depth() { return T >= 2 ? 2 : 4; }
template <int K, int T> constexpr size_t conv16_lds() { return sizeof(u4_t) * (2 * (size_t)T * kAChunks + 2 * (size_t)Conv16Geom<K>::BUF); }

template <int K, int T> // kernel size; row tiles per block
__global__ __launch_bounds__(256, 2) void conv16_kernel(Conv16Args a, int n_rg, int total) {
  using G = Conv16Geom<K>;
  constexpr int kRows = 32 * T, kA = T * kAChunks, kD = conv16_depth<T>();
  constexpr int kAPer = (kA + 255) / 256; // W chunks per thread and step
  extern __shared__ __attribute__((aligned(16))) u4_t s16[];
  u4_t *const sW = s16, *const sX = s16 + 2 * kA; // the W ring | the two halo buffers
  const int L = head_slot();
  if (L >= total) return;
  const int per_item = a.ph * a.pw * n_rg;
  const int item = L / per_item, rem = L - item * per_item, patch = rem / n_rg, rg = rem - patch * n_rg;
  const int py = patch / a.pw, r0 = py * kPR, q0 = (patch - py * a.pw) * kPC;
  const int hgt = a.h, wid = a.w;
  const int64_t hw = (int64_t)hgt * wid;
  const uint16_t *xs = a.xs + (int64_t)item * a.xs_stride;
  if (*head16_oob_word(xs, a.c_in, hw)) return; // an input outside the domain: the exact kernel, launched next, takes the item
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  // the thread's halo chunks e = tid + 256 j = (part, halo position, k half): where they lie in a channel tile of the split copy and
  // in a halo buffer - the same for every channel tile
  int64_t goff[G::HALO_J];
  int soff[G::HALO_J];
  unsigned g_in = 0, g_has = 0; // bit j: chunk j lies inside the image; is one of the halo's
#pragma unroll
  for (int j = 0; j < G::HALO_J; ++j) {
    const int e = tid + 256 * j;
    const bool has = e < G::HALO_N;
    const int kh = e & 1, hp = has ? (e >> 1) % G::HP : 0, part = has ? (e >> 1) / G::HP : 0;
    const int r = r0 + hp / G::HW - K / 2, q = q0 + hp % G::HW - K / 2;
    const bool in = has && ckbd_inside(r, q, hgt, wid);
    goff[j] = ((int64_t)part * hw + (in ? r * wid + q : 0)) * 2 + kh;
    soff[j] = (part * 2 + kh) * G::PLANE + hp;
    g_in |= (in ? 1u : 0u) << j;
    g_has |= (has ? 1u : 0u) << j;
  }
  f16_t acc[T];
  {
    const float *bp = a.bp + (int64_t)rg * kRows;
#pragma unroll
    for (int tl = 0; tl < T; ++tl) head_bias_tile(bp, tl, h, acc[tl]);
  }
  const int n_ct = a.n_ct, n_steps = n_ct * G::KK;
  // row tile rg * T + j, step s = ct * KK + t: chunks ((rg * T + j) * n_steps + s) * kAChunks ..
  const FGMM_GLOBAL u4_t *wp = (const FGMM_GLOBAL u4_t *)a.wp16 + (int64_t)rg * T * n_steps * kAChunks;
  const FGMM_GLOBAL u4_t *xg = (const FGMM_GLOBAL u4_t *)xs;
  struct Stage {
    u4_t ra[kAPer];
  };
  auto load_w = [&](Stage &g, int s) {
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int f = tid + 256 * j, jt = f / kAChunks;
      if (f < kA) g.ra[j] = wp[((int64_t)jt * n_steps + s) * kAChunks + (f - jt * kAChunks)];
    }
  };
  auto store_w = [&](const Stage &g, u4_t *buf) {
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int f = tid + 256 * j;
      if (f < kA) buf[f] = g.ra[j];
    }
  };
  u4_t rh[G::HALO_J];
  auto load_halo = [&](int ct) {
    const FGMM_GLOBAL u4_t *tile = xg + (int64_t)ct * 3 * hw * 2;
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j) rh[j] = tile[goff[j]]; // (a chunk that is not the halo's reads the tile's first)
  };
  auto store_halo = [&](u4_t *buf) {
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j)
      if ((g_has >> j) & 1u) buf[soff[j]] = (g_in >> j) & 1u ? rh[j] : (u4_t){0u, 0u, 0u, 0u};
  };
#define FGMM_FENCE() __builtin_amdgcn_sched_barrier(0)
  Stage g[kD];
#pragma unroll
  for (int d = 0; d < kD; ++d) load_w(g[d], d < n_steps ? d : n_steps - 1);
  load_halo(0);
  store_w(g[0], sW);
  store_halo(sX);
  __syncthreads();
  // the lane's first chunk of a halo buffer: its k half's plane of part 0, its position
  const int b_lane = h * G::PLANE + (2 * wave + (col >> 4)) * G::HW + (col & 15);
  // step s = ct KK + t: tile s is multiplied out of ring buffer s & 1 and halo buffer ct & 1 while the loads of the steps up to s + D
  // are in flight; the weights of step s + 1 are written into the other ring buffer - last read a step ago, a barrier behind - at the
  // end of the step, the next channel tile's halo into the other halo buffer at the end of the tile's last step.  Steps past the last
  // load the last one again: written, never multiplied.  i = u KK + t is s modulo 2 D: D is even
  for (int ct0 = 0; ct0 < n_ct; ct0 += kD) {
#pragma unroll
    for (int u = 0; u < kD; ++u) {
      const int ct = ct0 + u;
      if (ct < n_ct) {
        const u4_t *bX = sX + (u & 1) * G::BUF + b_lane;
#pragma unroll
        for (int t = 0; t < G::KK; ++t) {
          const int i = u * G::KK + t, s = ct * G::KK + t;
          const u4_t *bA = sW + (i & 1) * kA;
          FGMM_FENCE();
          load_w(g[i % kD], s + kD < n_steps ? s + kD : n_steps - 1);
          if (t == 0) load_halo(ct + 1 < n_ct ? ct + 1 : ct);
          bf8_t b[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) b[q] = __builtin_bit_cast(bf8_t, bX[q * 2 * G::PLANE + (t / K) * G::HW + t % K]);
          constexpr int qa[6] = {0, 2, 1, 0, 1, 0}, qb[6] = {2, 0, 1, 1, 0, 0}; // the six part products, smallest first
#pragma unroll
          for (int t0 = 0; t0 < T; t0 += 2) {
            constexpr int kPair = T > 1 ? 2 : 1;
            bf8_t w[kPair][3];
#pragma unroll
            for (int j = 0; j < kPair; ++j)
#pragma unroll
              for (int q = 0; q < 3; ++q) w[j][q] = __builtin_bit_cast(bf8_t, bA[(t0 + j) * kAChunks + (q * 2 + h) * 32 + col]);
            if (t0 == 0) FGMM_FENCE();
#pragma unroll
            for (int t6 = 0; t6 < 6; ++t6)
#pragma unroll
              for (int j = 0; j < kPair; ++j) acc[t0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[j][qa[t6]], b[qb[t6]], acc[t0 + j], 0, 0, 0);
          }
          FGMM_FENCE();
          store_w(g[(i + 1) % kD], sW + ((i + 1) & 1) * kA);
          if (t == G::KK - 1) store_halo(sX + ((u + 1) & 1) * G::BUF);
          FGMM_FENCE();
          __syncthreads();
        }
      }
    }
  }
#undef FGMM_FENCE
  // ---- epilogue (conv_kernel's): register reg of row tile tl is output channel (rg * T + tl) * 32 + mfma32_row(reg, h) at the lane's position
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

template <int K, int T> int conv16_go(const Conv16Args &a, int64_t n, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T;
  const int64_t total = n * a.ph * a.pw * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8); // every XCD gets as many slots (head_slot)
  constexpr size_t lds = conv16_lds<K, T>();
  if (int e = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(conv16_kernel<K, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  hipLaunchKernelGGL((conv16_kernel<K, T>), dim3(blocks), dim3(256), lds, st, a, n_rg, (int)total);
  return (int)hipGetLastError();
}

template <int K> int conv16_pack_go(const float *w, int c_out, int c_in, uint16_t *wp16, uint32_t *bad, hipStream_t st) {
  const int n_rt = conv_row_tiles(c_out), n_ct = conv16_tiles(c_in);
  const int64_t total = (int64_t)n_rt * n_ct * K * K * 32 * kBK;
  hipLaunchKernelGGL(conv16_pack_kernel<K>, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, st, w, c_out, c_in, n_rt, n_ct, wp16, bad);
  return (int)hipGetLastError();
}

} // namespace

int launch_conv16_pack(const float *w, int c_out, int c_in, int k, void *wp16, uint32_t *bad, void *stream) {
  return k == 3 ? conv16_pack_go<3>(w, c_out, c_in, static_cast<uint16_t *>(wp16), bad, (hipStream_t)stream)
                : conv16_pack_go<5>(w, c_out, c_in, static_cast<uint16_t *>(wp16), bad, (hipStream_t)stream);
}

int launch_conv16(const Conv16Args &args, int k, int64_t n, void *stream) {
  return ckbd_row_tiles_go<4, 2, 1>(n * args.ph * args.pw, args.c_out, [&](auto T) {
    return k == 3 ? conv16_go<3, T>(args, n, (hipStream_t)stream) : conv16_go<5, T>(args, n, (hipStream_t)stream);
  });
}

} // namespace fgmm
