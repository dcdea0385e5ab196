// fgmm_ckbd_ctx_grad.hip — the weight and bias gradients of the checkerboard context convolution on the matrix cores, in one fixed order
// (header section 5c).  The data gradient needs no kernel of its own: it is ckbd_ctx_kernel (fgmm_ckbd_ctx.hip) over the filters
// ckbd_ctx_pack_kernel<true> packs, with the other parity.
//
// Arithmetic: the reduction runs over the compact non-anchor positions of ALL items, concatenated - s = item * hw + q, P = n * hw of
// them - cut into S slices of L positions by ckbd_wgrad_slices (a function of P alone).  For slice k, output channel o and column
// t M + c (tap t, input channel c), on v_mfma_f32_32x32x2_f32, bit for bit the chain
//     acc = +0;  for s ascending in the slice:  acc = fmaf(g(s)[o], x(s)(t, c), acc)
// with x the forward's gathered feature (the anchor tap t of the non-anchor at s reads; +0 outside the image, which takes part in the
// chain); column 12 M is the bias': x = 1.  ckbd_ctx_wgrad_finish_kernel adds the slices' partials ascending in binary32 and scatters
// them into [C_out, M, 5, 5] with +0 at the 13 dropped taps.  No atomics: every partial has one writer.
//   block  = 256 threads = 4 waves: T row tiles of 32 output channels (T x 16 accumulator registers per lane) x 4 column tiles (one per
//            wave: 32 input channels of ONE tap, so a position's gather offset is constant over the tile; or the bias' column) x ONE slice
//   K loop = chunks of 32 positions through LDS (a slice is a multiple of 32 long but for the last): the instruction's k is a PAIR of
//            positions - the tile of fgmm_mfma32.h with positions where it has input channels, its fragments and products, in a plain
//            loop.  g rows are contiguous along positions: 32 lanes load 32 consecutive positions of a row; the features likewise
//   T      = 4, 2 or 1 by the number of blocks of the launch, as ckbd_ctx_kernel picks among 6, 2 and 1 (six row tiles beside the staging
//            registers of a chunk spill here); an output's chain does not depend on it
// Padding: positions past the slice's end are g = +0, x = -0 (+0 * -0 = -0 leaves every accumulator's bits alone); rows past C_out and
// channels past M read valid addresses and their accumulators are never stored.
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"

namespace fgmm {
namespace {

constexpr int kCh = 32;        // positions per chunk
constexpr int kGLd = kMfma32ALd; // LDS row pitch of the g tile: the A tile's, its fragments are read by mfma32_read_frag
static_assert(kCh == kMfma32BK, "a chunk is one K tile");
constexpr int kXLd = kCh + 1;  // ... of a wave's feature tile [position][channel]

template <int T> // row tiles per block
__global__ __launch_bounds__(256, 2) void ckbd_ctx_wgrad_kernel(CkbdWgradArgs a, int n_rg, int n_cgrp) {
  constexpr int kRows = 32 * T;
  __shared__ __attribute__((aligned(16))) float sG[kRows * kGLd]; // [row][column (p & 1) * 16 + (p >> 1) = position p of the chunk]
  __shared__ float sX[4 * kCh * kXLd];                            // [wave][position][channel of the wave's column tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  const int B = (int)blockIdx.x, rg = B % n_rg, cg = (B / n_rg) % n_cgrp, k = B / (n_rg * n_cgrp);
  const int M = a.M, c_out = a.c_out, hgt = a.h, w2 = a.w2, wid = 2 * a.w2, hw = a.h * a.w2;
  const int s_begin = k * a.L, s_end = min(s_begin + a.L, a.P); // (k < S: s_begin < P)
  const int n_ch = (s_end - s_begin + kCh - 1) / kCh;
  // the wave's column tile: tap t, channels c0 .. c0 + 31; or the bias'
  const int jl = cg * 4 + wave, jt = a.col0 + jl;
  const bool active = jl < a.n_col, is_bias = jt == kCkbdCtxTaps * a.mt;
  const int t = is_bias ? 0 : jt / a.mt, c0 = is_bias ? 0 : (jt - t * a.mt) * 32;
  const CkbdTap tap = ckbd_tap(t);
  f16_t acc[T];
#pragma unroll
  for (int tl = 0; tl < T; ++tl)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tl][r] = 0.0f;
  float rg_[4 * T], rx[16];
  // Staging, branch-free as ckbd_ctx_kernel's: a load that would fall outside (a position past the slice, a row past C_out, a channel
  // past M, a tap outside the image) reads a valid address instead and is replaced
  auto load_chunk = [&](int ch) {
    const int s = s_begin + ch * kCh + col;
    const bool in = s < s_end;
    const int item = in ? s / hw : 0, q = in ? s - item * hw : 0;
    {
      const FGMM_GLOBAL float *gp = (const FGMM_GLOBAL float *)(a.g + (int64_t)item * c_out * hw + q);
#pragma unroll
      for (int j = 0; j < 4 * T; ++j) {
        const int o = rg * kRows + (tid >> 5) + 8 * j;
        const float v = gp[(int64_t)(o < c_out ? o : c_out - 1) * hw];
        rg_[j] = in ? v : 0.0f;
      }
    }
    if (!active) return;
    if (is_bias) {
#pragma unroll
      for (int i = 0; i < 16; ++i) rx[i] = in ? 1.0f : -0.0f;
      return;
    }
    const CkbdAt at = ckbd_nonanchor(q, w2, a.odd);
    const int rr = at.r + tap.di, cc = at.c + tap.dj;
    const bool ok = in && ckbd_inside(rr, cc, hgt, wid);
    const int off = ok ? ckbd_anchor_at(rr, cc, w2) : 0;
    const float fill = in ? 0.0f : -0.0f;
    const FGMM_GLOBAL float *xp = (const FGMM_GLOBAL float *)(a.anchors + (int64_t)item * M * hw + off);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = c0 + 2 * i + h;
      const float v = xp[(int64_t)(c < M ? c : M - 1) * hw];
      rx[i] = ok ? v : fill;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int j = 0; j < 4 * T; ++j) sG[((tid >> 5) + 8 * j) * kGLd + (col & 1) * 16 + (col >> 1)] = rg_[j];
    if (!active) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) sX[(wave * kCh + col) * kXLd + 2 * i + h] = rx[i];
  };
  auto multiply = [&]() {
    if (!active) return;
    const float *a_base = sG + col * kGLd + h * 16;
    const float *b_base = sX + (wave * kCh + h) * kXLd + col;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      Mfma32Frag<T> f;
      mfma32_read_frag(f, a_base + s4 * 4, b_base + 8 * s4 * kXLd, kXLd);
      mfma32_multiply(acc, f);
    }
  };
  load_chunk(0);
  store_chunk();
  __syncthreads();
  for (int ch = 0; ch < n_ch; ++ch) {
    const bool more = ch + 1 < n_ch;
    if (more) load_chunk(ch + 1); // in flight under the products of chunk ch
    multiply();
    __syncthreads(); // every wave has read the chunk
    if (more) store_chunk();
    __syncthreads();
  }
  // ---- epilogue: register reg of row tile tl is output channel rg * 32 T + tl * 32 + mfma32_row(reg, h), the lane's column
  if (!active) return;
  const int64_t n_col = (int64_t)kCkbdCtxTaps * M + 1; // ckbd_wgrad_cols
  int64_t column = -1;
  if (is_bias) column = col == 0 ? n_col - 1 : -1;
  else if (c0 + col < M) column = (int64_t)t * M + c0 + col;
  if (column < 0) return;
  float *out = a.partial + (int64_t)k * c_out * n_col + column;
#pragma unroll
  for (int tl = 0; tl < T; ++tl)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
      if (o < c_out) stg<float>(out + (int64_t)o * n_col, acc[tl][reg]);
    }
}

// dW[o][c][tap t] = ((partial_0 + partial_1) + partial_2) + ... at column t M + c, +0 at the dropped taps; dbias[o] at column 12 M
__global__ __launch_bounds__(256) void ckbd_ctx_wgrad_finish_kernel(const float *__restrict__ partial, int M, int c_out, int S, float *__restrict__ dw,
                                                                    float *__restrict__ db) {
  const int64_t n_col = (int64_t)kCkbdCtxTaps * M + 1, slice = (int64_t)c_out * n_col;
  const int64_t n_w = dw ? (int64_t)c_out * M * 25 : 0, n_b = db ? c_out : 0;
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_w + n_b; i += step) {
    int64_t at; // of partial_0
    if (i < n_w) {
      const int f = (int)(i % 25);
      if (f != ckbd_tap_flat(f >> 1)) { // a dropped tap
        dw[i] = 0.0f;
        continue;
      }
      const int64_t oc = i / 25, o = oc / M, c = oc - o * M;
      at = o * n_col + (int64_t)(f >> 1) * M + c;
    } else {
      at = (i - n_w) * n_col + n_col - 1;
    }
    float acc = partial[at];
    for (int k = 1; k < S; ++k) acc = acc + partial[at + k * slice];
    if (i < n_w) dw[i] = acc;
    else db[i - n_w] = acc;
  }
}

template <int T> int ckbd_wgrad_go(const CkbdWgradArgs &a, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T, n_cgrp = (a.n_col + 3) / 4;
  const int64_t total = (int64_t)a.S * n_cgrp * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ckbd_ctx_wgrad_kernel<T>, dim3((unsigned)total), dim3(256), 0, st, a, n_rg, n_cgrp);
  return (int)hipGetLastError();
}

} // namespace

// T: the most row tiles per block (4, 2, 1) at which the launch still has a block for every CU; 1 when none has
int ckbd_wgrad_tiles(int64_t S, int n_col, int c_out) {
  return ckbd_row_tiles_go<4, 2, 1>(S * ((n_col + 3) / 4), c_out, [](auto T) { return (int)T; });
}
int launch_ckbd_wgrad(const CkbdWgradArgs &args, void *stream) {
  return ckbd_row_tiles_go<4, 2, 1>((int64_t)args.S * ((args.n_col + 3) / 4), args.c_out, [&](auto T) { return ckbd_wgrad_go<T>(args, (hipStream_t)stream); });
}

int launch_ckbd_wgrad_finish(const float *partial, int M, int c_out, int S, float *dw, float *db, void *stream) {
  const int64_t total = (dw ? (int64_t)c_out * M * 25 : 0) + (db ? c_out : 0);
  if (total <= 0) return 0;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(ckbd_ctx_wgrad_finish_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, partial, M, c_out, S, dw, db);
  return (int)hipGetLastError();
}

} // namespace fgmm
