// fgmm_hidden16.hip — a hidden layer of the entropy-parameter network on the BF16 matrix cores with binary32 accuracy ("bf16x6"), an OPTION
// beside the exact form of fgmm_hidden.hip (FGMM_HIDDEN_BF16X6 at fgmm_hidden_create_ex; header section 2c).
//
// Arithmetic: the layer section 2c defines - the bias, source a's channels, then source b's, an ABSENT source a taking no part, the
// activation on the binary32 accumulator - with the sum evaluated as fgmm_head16.hip and fgmm_ckbd_ctx16.hip evaluate theirs: every weight
// and every feature is split3's three bfloat16 parts (fgmm_split3.h), a product is the six part products (w1,x3) (w3,x1) (w2,x2) (w1,x2)
// (w2,x1) (w1,x1), smallest first, each ONE v_mfma_f32_32x32x16_bf16 over 16 input channels OF ONE SOURCE, accumulated in binary32 from
// the bias; K tiles ascend through source a, then source b.  Each source is padded to a multiple of 16 channels ON ITS OWN, with zeros
// in all three parts (in the packed weights and in the split copy alike): a tile never straddles the two, and the source is ONE pointer
// select per tile, as in hidden_kernel.  n16 = ceil(c_a / 16) + ceil(c_b / 16) matrix steps of six products; ceil(c_b / 16) with xa
// absent: its K tiles are not multiplied, and the packed weights are read from source b's first tile on.
// Bound (tests/hidden16_ref.py): tests/head_ref.py's bf16x6 derivation with this n16, through the activation -
//     |got - act(exact)| <= max(1, |slope|) (R (sum |w x| + |b|) + 2^-133 (sum |w| + sum |x|) + 6 n16 2^-150) + 2^-24 |act(exact)| + 2^-150,
//     R = 2^-23 (1 + 2^-6) + 6 n16 2^-24 (1 + 2^-7)                                          (the last two terms: LeakyReLU's multiply).
// What it is NOT: the fmaf chain, or a sequence a CPU can restate bit for bit.  What it is: the SAME BITS FROM EVERY LAUNCH - an output's
// bits are a function of its row of the weights, its bias and the features at its position: not of the block height, of n, of the item's
// place in a batch, of what lies beside it in a tile (a matrix step's rows and columns do not mix; every padding is a zero operand in
// every launch shape alike) - so the encoder's batch of 24 and the decoder's single image agree on MI355X.
// Domain: finite operands with |v| < 0x1.FFp127.  Weights outside are refused at creation (hidden16_pack_kernel raises a flag); an ITEM
// with a feature outside in any PRESENT source is flagged by the split kernel, left alone here, and computed by hidden_kernel
// (fgmm_hidden.hip, launched after this one with the flags): bit for bit the fmaf chain.
//
// Design.  Per call: head16_split_kernel (fgmm_head16.hip) once per present source - features -> [K tile of 16][part][position][16
// channels] bf16, the row groups of a position tile would otherwise each split the same features - then hidden16_kernel, then hidden_kernel
// for the flagged items (its blocks return at once otherwise).
//   block  = 256 threads = 4 waves; T row tiles of 32 output channels x 128 positions, a wave all T tiles x 32 positions: T accumulator
//            tiles.  T = 5, 2 or 1 by fgmm_hidden.hip's rule (hidden_tiles: the header's paragraph on block heights covers both forms);
//            at c_out = 640, T = 5 gives four row groups and no empty tile.
//   K tile = 16 channels of one source = one matrix step.
//   LDS    = two buffers of (W tile | x tile), one barrier per K tile.  Both tiles lie as [part][k half][row or position][8 bf16]: a
//            lane's operand - eight consecutive k of its row - is ONE 16-byte read, 32 lanes of a k half read 512 contiguous bytes.
//            The packed weights have the same order, so a tile is copied chunk for chunk (3072 contiguous bytes per row tile); an x
//            chunk is half of the 32 contiguous bytes that hold one position's 16 channels of one part: two threads per position, three
//            parts each - sixteen-byte copies only.  The x tile's k-half planes are 128 bytes further apart than their 2048: the two
//            threads of a position write to different banks.  T = 5: 2 x 28 416 bytes - two blocks a CU.
//   mask   = "position past hw", once per thread: its three chunks are staged as zeros (the load reads a valid address, the select is
//            applied when the tile is written, as in fgmm_mfma32.h).  A 1x1 layer has no taps.  Padded channels are zeros in the split
//            copy already.
//   loads  = the global loads of tile kt + D are issued before the products of tile kt, in D register sets.  D = 1 at T = 5: a tile is
//            30 products a wave, about a thousand matrix-pipe cycles and two waves a SIMD - more than a round trip to L2, where the packed
//            weights (four row groups share them) and the split copy live; a second set (28 registers) was measured 2 % SLOWER, 0.309 against
//            0.303 ms for the two layers of 24 halves (profiles/param_body_bf16x6.md).  D = 2 at
//            T = 2 (12 products), D = 4 at T = 1 (6 products): the shorter the tile, the more of them a round trip spans - the depths
//            ckbd_ctx16_kernel takes at its own heights, for its reason.
//   products: row tiles in pairs - three W operands each, the three x operands shared, the two accumulators alternating - in the fixed
//            order of the six parts.  T = 5 is odd: tiles (0, 1) and (2, 3) go as pairs, tile 4 ALONE after them, its six products back
//            to back on one accumulator (the matrix pipe forwards an accumulator to the next product of the same shape without a stall).
//            An accumulator sees the same six products in the same order whether its tile has a partner or not: the same bits.
// Placement (head_slot), the bias a tile starts from and the epilogue's register-to-row map: fgmm_headframe.h / fgmm_mfma32.h; the
// activations: fgmm_hidden_act.h, the text hidden_kernel runs.
#include "fgmm_headframe.h"
#include "fgmm_hidden_act.h"
#include "fgmm_split3.h"

namespace fgmm {
namespace {

constexpr int kBK = kHead16BK;          // input channels per K tile: one matrix step
constexpr int kPB = kMfma32PB;          // positions per block
constexpr int kAChunks = 3 * 2 * 32;    // sixteen-byte chunks of one row tile's W tile: [part][k half][32 rows]
constexpr int kBHalf = kPB + 8;         // chunks between the x tile's (part, k half) planes: 128 positions + 128 bytes
constexpr int kBChunks = 3 * 2 * kBHalf;

// one thread per (row tile, K tile, row, channel): its three parts.  K tile kt < kta: channels 16 kt ..+15 of source a; else channels
// 16 (kt - kta) ..+15 of source b - column c_a + that of w.  Padding (rows past c_out, a source's channels past its count): zero
__global__ __launch_bounds__(256) void hidden16_pack_kernel(const float *__restrict__ w, int c_out, int c_a, int c_b, int n_rt, int kta, int ktb,
                                                            uint16_t *__restrict__ wp, uint32_t *__restrict__ bad) {
  const int n_kt = kta + ktb;
  const int64_t total = (int64_t)n_rt * n_kt * 32 * kBK;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i % kBK), r = (int)((i / kBK) % 32);
    const int kt = (int)((i / (32 * kBK)) % n_kt), rt = (int)(i / ((int64_t)32 * kBK * n_kt));
    const bool src_a = kt < kta;
    const int c = (src_a ? kt : kt - kta) * kBK + k;
    const int64_t o = (int64_t)rt * 32 + r;
    const float v = (o < c_out && c < (src_a ? c_a : c_b)) ? w[o * ((int64_t)c_a + c_b) + (src_a ? c : c_a + c)] : 0.0f;
    if (!in_domain(v)) *bad = 1u;
    const Split3 s = split3(v);
    uint16_t *tile = wp + ((int64_t)rt * n_kt + kt) * (kAChunks * 8);
#pragma unroll
    for (int part = 0; part < 3; ++part) tile[((part * 2 + (k >> 3)) * 32 + r) * 8 + (k & 7)] = s.p[part];
  }
}

template <int T> constexpr int hidden16_depth() { return T >= 5 ? 1 : T >= 2 ? 2 : 4; }

template <int T> // row tiles per block
__global__ __launch_bounds__(256, 2) void hidden16_kernel(Hidden16Args a, int n_rg, int total) {
  constexpr int kRows = 32 * T, kA = T * kAChunks, kBuf = kA + kBChunks, kD = hidden16_depth<T>();
  constexpr int kAPer = (kA + 255) / 256; // W chunks per thread and tile
  __shared__ u4_t s16[2 * kBuf];
  const int L = head_slot();
  if (L >= total) return;
  // the row groups of one position tile are consecutive slots of one XCD: its L2 holds the x tile
  const int per_item = a.pt * n_rg;
  const int item = L / per_item, rem = L - item * per_item, pt = rem / n_rg, rg = rem - pt * n_rg;
  const int64_t hw = a.hw, P0 = (int64_t)pt * kPB;
  const int kta = a.kta, n_kt = a.n_kt;
  const uint16_t *xsb = a.xsb + (int64_t)item * a.xs_stride;
  const uint16_t *xsa = kta ? a.xsa + (int64_t)item * a.xs_stride : xsb; // (absent: no tile reads it)
  // a feature outside the domain in a present source: the exact kernel, launched next, takes the item
  if (*head16_oob_word(xsb, a.c_b, hw) | (kta ? *head16_oob_word(xsa, a.c_a, hw) : 0u)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  // the thread's position of the x tile: it stages k half tid & 1 of it, in all three parts
  const int64_t sp = P0 + (tid >> 1);
  const bool sp_ok = sp < hw;
  const int64_t sp_at = (sp_ok ? sp : 0) * 2 + (tid & 1); // (in chunks: a position's 16 channels of one part are two)
  f16_t acc[T];
  {
    const float *bp = a.bp + (int64_t)rg * kRows;
#pragma unroll
    for (int tl = 0; tl < T; ++tl) head_bias_tile(bp, tl, h, acc[tl]);
  }
  // row tile rg * T + j, K tile kt of the sum: chunks ((rg * T + j) * kt_all + kt0 + kt) * kAChunks ..
  const int64_t rt_chunks = (int64_t)a.kt_all * kAChunks;
  const FGMM_GLOBAL u4_t *wp = (const FGMM_GLOBAL u4_t *)a.wp16 + ((int64_t)rg * T * a.kt_all + a.kt0) * kAChunks;
  const FGMM_GLOBAL u4_t *xga = (const FGMM_GLOBAL u4_t *)xsa + sp_at, *xgb = (const FGMM_GLOBAL u4_t *)xsb + sp_at;
  struct Stage {
    u4_t ra[kAPer], rb[3];
  };
  auto load_tile = [&](Stage &g, int kt) {
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int f = tid + 256 * j, jt = f / kAChunks;
      if (f < kA) g.ra[j] = wp[jt * rt_chunks + (int64_t)kt * kAChunks + (f - jt * kAChunks)];
    }
    const bool src_a = kt < kta;
    const FGMM_GLOBAL u4_t *xg = src_a ? xga : xgb; // the source switch: a select, not a branch
    const int ct = src_a ? kt : kt - kta;
#pragma unroll
    for (int part = 0; part < 3; ++part) g.rb[part] = xg[((int64_t)ct * 3 + part) * hw * 2];
  };
  auto store_tile = [&](const Stage &g, u4_t *buf) {
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int f = tid + 256 * j;
      if (f < kA) buf[f] = g.ra[j];
    }
#pragma unroll
    for (int part = 0; part < 3; ++part) buf[kA + (part * 2 + (tid & 1)) * kBHalf + (tid >> 1)] = sp_ok ? g.rb[part] : (u4_t){0u, 0u, 0u, 0u};
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
    for (int t0 = 0; t0 < T; t0 += 2) { // a pair of row tiles; the last tile of an odd T alone
      bf8_t w[2][3];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (t0 + j < T) w[j][q] = __builtin_bit_cast(bf8_t, bA[(t0 + j) * kAChunks + (q * 2 + h) * 32 + col]);
      if (t0 == 0) FGMM_FENCE();
#pragma unroll
      for (int t6 = 0; t6 < 6; ++t6)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (t0 + j < T) acc[t0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[j][qa[t6]], b[qb[t6]], acc[t0 + j], 0, 0, 0);
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
  // ---- epilogue: register reg of row tile tl is output channel (rg * T + tl) * 32 + mfma32_row(reg, h) at the lane's position; the
  // activation on the binary32 accumulator, as hidden_kernel's
  const int64_t p = P0 + wave * 32 + col;
  if (p >= hw) return;
  float *out = a.out + (int64_t)item * a.c_out * hw + p;
  with_activation(a.act, a.slope, [&](auto act) {
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
        if (o < a.c_out) stg<float>(out + (int64_t)o * hw, act(acc[tl][reg]));
      }
  });
}

template <int T> int hidden16_go(const Hidden16Args &a, int64_t n, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T;
  const int64_t total = n * a.pt * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8); // every XCD gets as many slots (head_slot)
  hipLaunchKernelGGL(hidden16_kernel<T>, dim3(blocks), dim3(256), 0, st, a, n_rg, (int)total);
  return (int)hipGetLastError();
}

} // namespace

int launch_hidden16_pack(const float *w, int c_out, int c_a, int c_b, void *wp16, uint32_t *bad, void *stream) {
  const int n_rt = hidden_row_tiles(c_out), kta = hidden16_kt(c_a), ktb = hidden16_kt(c_b);
  const int64_t total = (int64_t)n_rt * (kta + ktb) * 32 * kBK;
  hipLaunchKernelGGL(hidden16_pack_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, c_out, c_a, c_b, n_rt,
                     kta, ktb, static_cast<uint16_t *>(wp16), bad);
  return (int)hipGetLastError();
}

int launch_hidden16(const Hidden16Args &args, int64_t n, int cus, void *stream) {
  switch (hidden_tiles(n, args.pt, args.c_out, cus)) { // fgmm_hidden.hip's rule
  case 5: return hidden16_go<5>(args, n, (hipStream_t)stream);
  case 2: return hidden16_go<2>(args, n, (hipStream_t)stream);
  default: return hidden16_go<1>(args, n, (hipStream_t)stream);
  }
}

} // namespace fgmm
