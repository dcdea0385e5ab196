// fgmm_ckbd_ctx16.hip — the checkerboard context convolution on the BF16 matrix cores with binary32 accuracy ("bf16x6"), an OPTION beside
// the exact form of fgmm_ckbd_ctx.hip (FGMM_CKBD_CTX_BF16X6 at fgmm_ckbd_ctx_create_ex; header section 5b).
//
// Arithmetic: the sum section 5b defines - the bias, the 12 kept taps row-major, the M channels of each, a tap outside the image +0 -
// evaluated as fgmm_head16.hip evaluates its sum: every weight and every anchor is split3's three bfloat16 parts (fgmm_split3.h), a
// product is the six part products (w1,x3) (w3,x1) (w2,x2) (w1,x2) (w2,x1) (w1,x1), smallest first, each ONE v_mfma_f32_32x32x16_bf16
// over 16 input channels OF ONE TAP, accumulated in binary32 from the bias; K tiles ascend by tap, then by channel tile: n16 =
// 12 ceil(M / 16) matrix steps of six products; channels past M are zero in all three parts.
// Bound (tests/ckbd_ctx16_ref.py): tests/head_ref.py's bf16x6 derivation over the gathered problem pack(W), gather(A) of
// tests/ckbd_ctx_ref.py with n16 = 12 ceil(M / 16) - not ceil(12 M / 16): a tap's last tile is padded -
//     |got - exact| <= R (sum |w x| + |b|) + 2^-133 (sum |w| + sum |x|) + 6 n16 2^-150,   R = 2^-23 (1 + 2^-6) + 6 n16 2^-24 (1 + 2^-7).
// What it is NOT: a sequence a CPU can restate bit for bit.  What it is: the SAME BITS FROM EVERY LAUNCH - an output's bits are a
// function of its row of the weights, its bias and the anchors its taps read: not of the block height, of n, of the item's place in a
// batch, of what lies beside it in a tile (a matrix step's rows and columns do not mix; every padding is a +0 operand in every launch
// shape alike) - so the encoder's batch of 24 and the decoder's single image agree on MI355X.
// Domain: finite operands with |v| < 0x1.FFp127.  Weights outside are refused at creation; an ITEM with an anchor outside is flagged by
// the split kernel and computed by ckbd_ctx_kernel (fgmm_ckbd_ctx.hip, launched after this one with the flags): bit for bit the chain.
//
// Design.  Three launches per call: head16_split_kernel (fgmm_head16.hip: the compact anchors -> [channel tile of 16][part][compact
// anchor position][16 channels] bf16, once per call - the twelve taps and the row groups would otherwise each split the same anchors),
// ckbd_ctx16_kernel, and ckbd_ctx_kernel for the flagged items (its blocks return at once otherwise).
//   block  = 256 threads = 4 waves; T row tiles of 32 output channels x 128 compact positions, a wave all rows x 32 positions: T
//            accumulator tiles.  T = 6, 2 or 1 by fgmm_ckbd_ctx.hip's rule (the tallest that still gives every CU a block).
//   K tile = 16 channels of one tap = one matrix step: a position's gather offset is constant over a tile.
//   LDS    = two buffers of (W tile | x tile), one barrier per K tile.  Both tiles lie as [part][k half][row or position][8 bf16]: a
//            lane's operand - eight consecutive k of its row - is ONE 16-byte read, 32 lanes of a k half read 512 contiguous bytes.
//            The packed weights have the same order, so a tile is copied chunk for chunk (3072 contiguous bytes per row tile); an x
//            chunk is half of the 32 contiguous bytes that hold one anchor's 16 channels of one part: two threads per position, three
//            parts each - sixteen-byte copies only.  The x tile's k halves are 128 bytes further apart than their 2048: the two
//            threads of a position write to different banks.
//   mask   = once per thread and tile: the thread's position is past the end, or the tile's tap reads outside the image -> its three
//            chunks are staged as zeros (the load reads a valid address, the select is applied when the tile is written, as in
//            fgmm_mfma32.h).  Padded channels are zeros in the split copy already.
//   loads  = the global loads of tile kt + D are issued before the products of tile kt, in D register sets: D = 1 at T = 6 (36
//            products per wave and tile cover a round trip), 2 at T = 2, 4 at T = 1, where a tile is six products.
//   products: row tiles in pairs - three W operands each, the three x operands shared - in the fixed order of the six parts.
// Placement (head_slot), the bias a tile starts from and the epilogue's register-to-row map: fgmm_headframe.h / fgmm_mfma32.h.
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"
#include "fgmm_split3.h"

namespace fgmm {
namespace {

constexpr int kBK = kHead16BK;          // input channels per K tile: one matrix step
constexpr int kPB = kMfma32PB;          // compact positions per block
constexpr int kAChunks = 3 * 2 * 32;    // sixteen-byte chunks of one row tile's W tile: [part][k half][32 rows]
constexpr int kBHalf = kPB + 8;         // chunks between the x tile's (part, k half) planes: 128 positions + 128 bytes
constexpr int kBChunks = 3 * 2 * kBHalf;

// one thread per (row tile, K tile, row, channel): its three parts.  M, c_out, n_rt as ckbd_ctx_pack_kernel's
__global__ __launch_bounds__(256) void ckbd_ctx16_pack_kernel(const float *__restrict__ w, int M, int c_out, int n_rt, int mt, uint16_t *__restrict__ wp,
                                                              uint32_t *__restrict__ bad) {
  const int n_kt = kCkbdCtxTaps * mt;
  const int64_t total = (int64_t)n_rt * n_kt * 32 * kBK;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i % kBK), r = (int)((i / kBK) % 32);
    const int kt = (int)((i / (32 * kBK)) % n_kt), rt = (int)(i / ((int64_t)32 * kBK * n_kt));
    const int t = kt / mt, c = (kt - t * mt) * kBK + k;
    const int64_t o = (int64_t)rt * 32 + r;
    const float v = (o < c_out && c < M) ? w[(o * M + c) * 25 + ckbd_tap_flat(t)] : 0.0f;
    if (!in_domain(v)) *bad = 1u;
    const Split3 s = split3(v);
    uint16_t *tile = wp + ((int64_t)rt * n_kt + kt) * (kAChunks * 8);
#pragma unroll
    for (int part = 0; part < 3; ++part) tile[((part * 2 + (k >> 3)) * 32 + r) * 8 + (k & 7)] = s.p[part];
  }
}

template <int T> constexpr int ckbd_ctx16_depth() { return T >= 6 ? 1 : T >= 2 ? 2 : 4; }

template <int T> // row tiles per block
__global__ __launch_bounds__(256, 2) void ckbd_ctx16_kernel(CkbdCtx16Args a, int n_rg, int total) {
  constexpr int kRows = 32 * T, kA = T * kAChunks, kBuf = kA + kBChunks, kD = ckbd_ctx16_depth<T>();
  constexpr int kAPer = (kA + 255) / 256; // W chunks per thread and tile
  __shared__ u4_t s16[2 * kBuf];
  const int L = head_slot();
  if (L >= total) return;
  const int per_item = a.pt * n_rg;
  const int item = L / per_item, rem = L - item * per_item, pt = rem / n_rg, rg = rem - pt * n_rg;
  const int hgt = a.h, w2 = a.w2, wid = 2 * a.w2, hw = a.h * a.w2, P0 = pt * kPB;
  const uint16_t *xs = a.xs + (int64_t)item * a.xs_stride;
  if (*head16_oob_word(xs, a.M, hw)) return; // an anchor outside the domain: the exact kernel, launched next, takes the item
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  // the thread's position of the x tile (it stages k half tid & 1 of it, in all three parts): row and full-size column of the non-anchor
  const int sq = P0 + (tid >> 1);
  const CkbdAt at = ckbd_nonanchor(sq < hw ? sq : 0, w2, a.odd);
  f16_t acc[T];
  {
    const float *bp = a.bp + (int64_t)rg * kRows;
#pragma unroll
    for (int tl = 0; tl < T; ++tl) head_bias_tile(bp, tl, h, acc[tl]);
  }
  const int n_kt = a.n_kt, mt = a.mt;
  // row tile rg * T + j, K tile kt: chunks ((rg * T + j) * n_kt + kt) * kAChunks ..
  const FGMM_GLOBAL u4_t *wp = (const FGMM_GLOBAL u4_t *)a.wp16 + (int64_t)rg * T * n_kt * kAChunks;
  const FGMM_GLOBAL u4_t *xg = (const FGMM_GLOBAL u4_t *)xs + (tid & 1);
  struct Stage {
    u4_t ra[kAPer], rb[3];
    bool ok; // the thread's position exists and the tile's tap reads inside the image (applied when the tile is written)
  };
  auto load_tile = [&](Stage &g, int kt) {
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int f = tid + 256 * j, jt = f / kAChunks;
      if (f < kA) g.ra[j] = wp[((int64_t)jt * n_kt + kt) * kAChunks + (f - jt * kAChunks)];
    }
    const int t = kt / mt, ct = kt - t * mt;
    const CkbdTap tap = ckbd_tap(t);
    const int rr = at.r + tap.di, cc = at.c + tap.dj;
    g.ok = sq < hw && ckbd_inside(rr, cc, hgt, wid);
    const int off = g.ok ? ckbd_anchor_at(rr, cc, w2) : 0;
#pragma unroll
    for (int part = 0; part < 3; ++part) g.rb[part] = xg[(((int64_t)ct * 3 + part) * hw + off) * 2];
  };
  auto store_tile = [&](const Stage &g, u4_t *buf) {
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int f = tid + 256 * j;
      if (f < kA) buf[f] = g.ra[j];
    }
#pragma unroll
    for (int part = 0; part < 3; ++part) buf[kA + (part * 2 + (tid & 1)) * kBHalf + (tid >> 1)] = g.ok ? g.rb[part] : (u4_t){0u, 0u, 0u, 0u};
  };
#define FGMM_FENCE() __builtin_amdgcn_sched_barrier(0)
  Stage g[kD];
#pragma unroll
  for (int d = 0; d < kD; ++d) load_tile(g[d], d < n_kt ? d : n_kt - 1);
  store_tile(g[0], s16);
  __syncthreads();
  // step kt: tile kt is multiplied out of buffer kt & 1 while the loads of the tiles up to kt + D are in flight; tile kt + 1 is written
  // into the other buffer - last read a tile ago, a barrier behind - at the end of the step.  `issue` (free: its tile is in LDS) takes
  // tile kt + D, `land` holds tile kt + 1.  Tiles past the last load the last one again: written, never multiplied
  auto step = [&](int kt, Stage &issue, const Stage &land) {
    const u4_t *bA = s16 + (kt & 1) * kBuf, *bB = bA + kA + wave * 32 + col;
    FGMM_FENCE();
    load_tile(issue, kt + kD < n_kt ? kt + kD : n_kt - 1);
    bf8_t b[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = __builtin_bit_cast(bf8_t, bB[(q * 2 + h) * kBHalf]);
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
    store_tile(land, s16 + ((kt + 1) & 1) * kBuf);
    FGMM_FENCE();
    __syncthreads();
  };
  for (int kt = 0; kt < n_kt; kt += kD) {
#pragma unroll
    for (int d = 0; d < kD; ++d)
      if (kt + d < n_kt) step(kt + d, g[d], g[(d + 1) % kD]);
  }
#undef FGMM_FENCE
  // ---- epilogue: register reg of row tile tl is output channel (rg * T + tl) * 32 + mfma32_row(reg, h) at the lane's position
  const int p = P0 + wave * 32 + col;
  if (p < hw) {
    float *out = a.out + (int64_t)item * a.c_out * hw + p;
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
        if (o < a.c_out) stg<float>(out + (int64_t)o * hw, acc[tl][reg]);
      }
  }
}

template <int T> int ckbd_ctx16_go(const CkbdCtx16Args &a, int64_t n, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T;
  const int64_t total = n * a.pt * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8); // every XCD gets as many slots (head_slot)
  hipLaunchKernelGGL(ckbd_ctx16_kernel<T>, dim3(blocks), dim3(256), 0, st, a, n_rg, (int)total);
  return (int)hipGetLastError();
}

} // namespace

int launch_ckbd_ctx16_pack(const float *w, int M, int c_out, void *wp16, uint32_t *bad, void *stream) {
  const int n_rt = ckbd_ctx_row_tiles(c_out), mt = ckbd_ctx16_mt(M);
  const int64_t total = (int64_t)n_rt * kCkbdCtxTaps * mt * 32 * kBK;
  hipLaunchKernelGGL(ckbd_ctx16_pack_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, M, c_out, n_rt, mt,
                     static_cast<uint16_t *>(wp16), bad);
  return (int)hipGetLastError();
}

int launch_ckbd_ctx16(const CkbdCtx16Args &args, int64_t n, void *stream) {
  return ckbd_row_tiles_go<6, 2, 1>(n * args.pt, args.c_out, [&](auto T) { return ckbd_ctx16_go<T>(args, n, (hipStream_t)stream); });
}

} // namespace fgmm
