// fgmm_hidden_grad.hip — the gradients of the parameter network's hidden layers on the matrix cores, in one fixed order (header section
// 2d): the data gradients of the two sources, and the weight and bias gradients.  With fgmm_hidden.hip's forward over caller-owned packed
// weights (fgmm_hidden_apply_packed) a layer is a differentiable operator: flashgmm_amd.ops.pointwise_layer.
//
// The gradient of the PRE-activation is never stored.  Both kernels form it where they stage their tiles, from the gradient gy of the
// layer's output and the saved OUTPUT out (what the next layer keeps as its input anyway), one binary32 operation:
//     FGMM_ACT_NONE   gz = gy
//     FGMM_ACT_LEAKY  gz = out > 0 ? gy : gy * slope        (slope >= 0: out > 0 exactly where the accumulator was)
//     FGMM_ACT_RELU   gz = out > 0 ? gy : +0
// A NaN output takes the second branch.
//
// hidden_dgrad_kernel<T, VEC, ACT>: dx[i][k][p] = the chain  acc = +0; for o = 0 .. c_out-1 ascending: acc = fmaf(W[o][k], gz[i][o][p], acc)
// - hidden_kernel's tile and K loop (fgmm_mfma32.h's text) with the TRANSPOSED weights as the A tile (hidden_pack_t_kernel: rows = the
// c_a + c_b input channels, K = c_out, one source) and gz as the B tile: gy and out are loaded into registers while the previous tile
// multiplies, the select runs when the tile is written to LDS.  Padding as the forward's: packed +0, features -0.
//   rows   = the asked part [r0, r1) of [0, c_a + c_b): a block is T row tiles of 32 aligned at multiples of T from row 0 (the packing's
//            padding covers them), a tile may straddle the two outputs - the epilogue stores row r < c_a to dxa[r], else to dxb[r - c_a],
//            and nothing outside [r0, r1)
//   T      = 5, 2 or 1 by section 2c's rule over the blocks of the asked rows; a chain does not depend on it
//   ACT    : false (FGMM_ACT_NONE) never loads `out`
// hidden_wgrad_kernel<T>, hidden_wgrad_finish_kernel: ckbd_ctx_wgrad_kernel's block, chunks and padding (fgmm_ckbd_ctx_grad.hip; header
// section 5c's slice rule, ckbd_wgrad_slices, over P = n hw positions) with a column tile = 32 input channels of ONE source (each source
// padded to 32 on its own: the tile's source is a pointer select) or the bias' column, and the g tile = gz, formed when the chunk is
// written to LDS.  partial_k[o][c] = chain over the slice's positions ascending of fmaf(gz(s)[o], x(s)[c], acc); the finish kernel adds the
// slices ascending in binary32 and writes dW row-major [c_out, c_a + c_b] (+0 in the columns of an absent first source) and dbias.
// No atomics: every partial has one writer.
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"
#include "fgmm_hidden_act.h" // grad_act: gz from (gy, out)

namespace fgmm {
namespace {

constexpr int kBK = kMfma32BK;
constexpr int kTileW = kMfma32TileW;
constexpr int kPB = kMfma32PB;
constexpr int kALd = kMfma32ALd, kBLd = kMfma32BLd;

// the transposed packing: hidden_pack_kernel's layout (fgmm_hidden.hip) of the layer  W'[r][o] = w[o][r]  - c_a + c_b rows, ONE source of
// c_out channels, no bias: [n_rt row tiles][n_kt K tiles][32 rows][32 columns], then [n_rt][32] of +0.  Padding: +0
__global__ __launch_bounds__(256) void hidden_pack_t_kernel(const float *__restrict__ w, int c_out, int c_in, int n_rt, int n_kt, float *__restrict__ wp) {
  const int64_t total = (int64_t)n_rt * n_kt * kTileW, n_bias = (int64_t)n_rt * 32;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total + n_bias; i += (int64_t)gridDim.x * 256) {
    if (i >= total) {
      wp[i] = 0.0f;
      continue;
    }
    const int q = (int)(i % kBK), r = (int)((i / kBK) % 32);
    const int kt = (int)((i / kTileW) % n_kt), rt = (int)(i / ((int64_t)kTileW * n_kt));
    const int o = kt * kBK + mfma32_pack_col(q);
    const int64_t row = (int64_t)rt * 32 + r;
    wp[i] = (row < c_in && o < c_out) ? w[(int64_t)o * c_in + row] : 0.0f;
  }
}

template <int T, bool VEC, bool ACT> // row tiles per block; 16-byte loads of gy and out; an activation other than FGMM_ACT_NONE
__global__ __launch_bounds__(256, 2) void hidden_dgrad_kernel(HiddenDgradArgs a, int rg0, int n_rg, int total) {
  constexpr int kTiles = T, kRows = 32 * T;
  __shared__ __attribute__((aligned(16))) float sA[kRows * kALd];
  __shared__ __attribute__((aligned(16))) float sB[kBK * kBLd];
  const int L = head_slot();
  if (L >= total) return;
  const int per_item = a.pt * n_rg;
  const int item = L / per_item, rem = L - item * per_item, pt = rem / n_rg, rg = rg0 + (rem - pt * n_rg);
  const int64_t hw = a.hw, P0 = (int64_t)pt * kPB;
  const int c_out = a.c_out;
  const float *gy = a.gy + (int64_t)item * c_out * hw;
  const float *yo = a.out + (int64_t)item * c_out * hw;
  const bool relu = a.act == FGMM_ACT_RELU;
  const float slope = a.slope;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  f16_t acc[kTiles];
#pragma unroll
  for (int tl = 0; tl < kTiles; ++tl)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tl][r] = 0.0f;
  // ---- K loop (mfma32_k_loop) over the output channels: tile kt is channels 32 kt ..+31 of gz
  const int n_kt = a.n_kt;
  const int64_t rt_words = (int64_t)n_kt * (kTileW / 4);
  const float *wp = a.wp + (int64_t)rg * kTiles * rt_words * 4;
  // Staging, branch-free as hidden_kernel's: a load that would fall outside reads a valid address instead; the element becomes -0
  // when the tile is written
  float4_t ra[kTiles], rgy[4], ryo[4];
  unsigned rb_ok = 0;
  auto load_tile = [&](int kt) {
    rb_ok = 0;
#pragma unroll
    for (int j = 0; j < kTiles; ++j) ra[j] = mfma32_load_a(wp + (int64_t)kt * kTileW, (int64_t)j * rt_words);
    const int k0 = kt * kBK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = tid + 256 * j, kk = f >> 5, p4 = f & 31;
      const int kin = k0 + kk;
      const int64_t p = P0 + 4 * p4;
      const bool k_ok = kin < c_out;
      const int64_t row = (int64_t)(k_ok ? kin : c_out - 1) * hw;
      if constexpr (VEC) {
        const int64_t at = row + (p < hw ? p : 0);
        rgy[j] = ldg<float4_t>(gy + at);
        if constexpr (ACT) ryo[j] = ldg<float4_t>(yo + at);
        rb_ok |= (k_ok && p < hw ? 0xFu : 0u) << (4 * j);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t at = row + (p + e < hw ? p + e : 0);
          rgy[j][e] = ((const FGMM_GLOBAL float *)gy)[at];
          if constexpr (ACT) ryo[j][e] = ((const FGMM_GLOBAL float *)yo)[at];
          rb_ok |= (k_ok && p + e < hw ? 1u : 0u) << (4 * j + e);
        }
      }
    }
  };
  auto store_tile = [&]() { // the select: here, where the loads have to have landed anyway
    float4_t rz[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (ACT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) rz[j][e] = grad_act(rgy[j][e], ryo[j][e], relu, slope);
      } else {
        rz[j] = rgy[j];
      }
    }
    mfma32_store_tile(sA, sB, ra, rz, rb_ok, [](int) { return -0.0f; });
  };
  mfma32_k_loop(acc, sA, sB, n_kt, wave, h, col, load_tile, store_tile);
  // ---- epilogue: register reg of row tile tl is input channel r = (rg * T + tl) * 32 + mfma32_row(reg, h) at the lane's position
  const int64_t p = P0 + wave * 32 + col;
  if (p >= hw) return;
  const int c_a = a.c_a;
  float *dxa = a.dxa + (int64_t)item * c_a * hw + p; // (null: r0 >= c_a and no row reaches it)
  float *dxb = a.dxb + (int64_t)item * a.c_b * hw + p;
#pragma unroll
  for (int tl = 0; tl < kTiles; ++tl)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = rg * kRows + tl * 32 + mfma32_row(reg, h);
      if (r < a.r0 || r >= a.r1) continue;
      if (r < c_a) stg<float>(dxa + (int64_t)r * hw, acc[tl][reg]);
      else stg<float>(dxb + (int64_t)(r - c_a) * hw, acc[tl][reg]);
    }
}

// the blocks of T row tiles, aligned at multiples of T from tile 0, that hold a row of [r0, r1): [first, first + count)
struct RowGroups { int first, count; };
static RowGroups dgrad_row_groups(int r0, int r1, int T) {
  const int first = r0 / (32 * T);
  return {first, (r1 + 32 * T - 1) / (32 * T) - first};
}

template <int T> static int hidden_dgrad_go(const HiddenDgradArgs &a, int64_t n, bool vec, hipStream_t st) {
  const RowGroups g = dgrad_row_groups(a.r0, a.r1, T);
  const int64_t total = n * a.pt * g.count;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 7) / 8 * 8);
  const bool act = a.act != FGMM_ACT_NONE;
#define FGMM_GO(V, A) hipLaunchKernelGGL((hidden_dgrad_kernel<T, V, A>), dim3(blocks), dim3(256), 0, st, a, g.first, g.count, (int)total)
  if (vec) {
    if (act) FGMM_GO(true, true);
    else FGMM_GO(true, false);
  } else {
    if (act) FGMM_GO(false, true);
    else FGMM_GO(false, false);
  }
#undef FGMM_GO
  return (int)hipGetLastError();
}

// section 2c's height rule over the blocks of the asked rows: the first T of 5, 2, 1 at which the launch has a block for every one of
// the device's compute units; 1 when none has
template <int T, int... Ts, typename Go> static int hidden_dgrad_tiles_go(int64_t outer, int r0, int r1, int cus, const Go &go) {
  if constexpr (sizeof...(Ts) > 0)
    if (outer * dgrad_row_groups(r0, r1, T).count < cus) return hidden_dgrad_tiles_go<Ts...>(outer, r0, r1, cus, go);
  return go(std::integral_constant<int, T>{});
}

// ---- the weight and bias gradients ---------------------------------------------------------------------------------------------------
constexpr int kCh = 32;          // positions per chunk
constexpr int kGLd = kMfma32ALd; // LDS row pitch of the g tile: the A tile's, its fragments are read by mfma32_read_frag
static_assert(kCh == kMfma32BK, "a chunk is one K tile");
constexpr int kXLd = kCh + 1;    // ... of a wave's feature tile [position][channel]

template <int T> // row tiles per block
__global__ __launch_bounds__(256, 2) void hidden_wgrad_kernel(HiddenWgradArgs a, int n_rg, int n_cgrp) {
  constexpr int kRows = 32 * T;
  __shared__ __attribute__((aligned(16))) float sG[kRows * kGLd]; // [row][column (p & 1) * 16 + (p >> 1) = position p of the chunk]
  __shared__ float sX[4 * kCh * kXLd];                            // [wave][position][channel of the wave's column tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  const int B = (int)blockIdx.x, rg = B % n_rg, cg = (B / n_rg) % n_cgrp, k = B / (n_rg * n_cgrp);
  const int c_out = a.c_out, hw = a.hw;
  const int s_begin = k * a.L, s_end = min(s_begin + a.L, a.P); // (k < S: s_begin < P)
  const int n_ch = (s_end - s_begin + kCh - 1) / kCh;
  // the wave's column tile: 32 channels of source a (jt < mta), of source b, or the bias' (jt == mta + mtb)
  const int jl = cg * 4 + wave, jt = a.col0 + jl;
  const bool active = jl < a.n_col, is_bias = jt == a.mta + a.mtb, src_a = jt < a.mta;
  const float *xsrc = src_a ? a.xa : a.xb; // the source switch: a select
  const int c_src = src_a ? a.c_a : a.c_b, c0 = is_bias ? 0 : (src_a ? jt : jt - a.mta) * 32;
  const bool act = a.act != FGMM_ACT_NONE, relu = a.act == FGMM_ACT_RELU;
  const float slope = a.slope;
  f16_t acc[T];
#pragma unroll
  for (int tl = 0; tl < T; ++tl)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tl][r] = 0.0f;
  float rgy[4 * T], ryo[4 * T], rx[16];
  bool r_in = false; // the staged chunk's position of this lane lies inside the slice
  // Staging, branch-free as ckbd_ctx_wgrad_kernel's: a load that would fall outside (a position past the slice, a row past c_out, a
  // channel past its source) reads a valid address instead and is replaced
  auto load_chunk = [&](int ch) {
    const int s = s_begin + ch * kCh + col;
    const bool in = s < s_end;
    r_in = in;
    const int item = in ? s / hw : 0, q = in ? s - item * hw : 0;
    {
      const int64_t at = (int64_t)item * c_out * hw + q;
      const FGMM_GLOBAL float *gp = (const FGMM_GLOBAL float *)(a.gy + at);
      const FGMM_GLOBAL float *op = (const FGMM_GLOBAL float *)(a.out + at);
#pragma unroll
      for (int j = 0; j < 4 * T; ++j) {
        const int o = rg * kRows + (tid >> 5) + 8 * j;
        const int64_t row = (int64_t)(o < c_out ? o : c_out - 1) * hw;
        rgy[j] = gp[row];
        ryo[j] = act ? op[row] : 1.0f;
      }
    }
    if (!active) return;
    if (is_bias) {
#pragma unroll
      for (int i = 0; i < 16; ++i) rx[i] = in ? 1.0f : -0.0f;
      return;
    }
    const FGMM_GLOBAL float *xp = (const FGMM_GLOBAL float *)(xsrc + (int64_t)item * c_src * hw + q);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = c0 + 2 * i + h;
      const float v = xp[(int64_t)(c < c_src ? c : c_src - 1) * hw];
      rx[i] = in ? v : -0.0f;
    }
  };
  auto store_chunk = [&]() { // gz is formed here: g = +0 past the slice's end
#pragma unroll
    for (int j = 0; j < 4 * T; ++j) {
      const float gz = act ? grad_act(rgy[j], ryo[j], relu, slope) : rgy[j];
      sG[((tid >> 5) + 8 * j) * kGLd + (col & 1) * 16 + (col >> 1)] = r_in ? gz : 0.0f;
    }
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
  const int64_t n_col = (int64_t)a.c_a + a.c_b + 1; // a partial's row: source a's channels, source b's, the bias
  int64_t column = -1;
  if (is_bias) column = col == 0 ? n_col - 1 : -1;
  else if (c0 + col < c_src) column = (src_a ? 0 : a.c_a) + c0 + col;
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

// dW[o][c] = ((partial_0 + partial_1) + partial_2) + ... at column c, +0 at c < c_a when source a was absent; dbias[o] at the last column
__global__ __launch_bounds__(256) void hidden_wgrad_finish_kernel(const float *__restrict__ partial, int c_a, int c_b, int c_out, int has_xa, int S,
                                                                  float *__restrict__ dw, float *__restrict__ db) {
  const int64_t c_in = (int64_t)c_a + c_b, n_col = c_in + 1, slice = (int64_t)c_out * n_col;
  const int64_t n_w = dw ? (int64_t)c_out * c_in : 0, n_b = db ? c_out : 0;
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_w + n_b; i += step) {
    int64_t at; // of partial_0
    if (i < n_w) {
      const int64_t o = i / c_in, c = i - o * c_in;
      if (!has_xa && c < c_a) {
        dw[i] = 0.0f;
        continue;
      }
      at = o * n_col + c;
    } else {
      at = (i - n_w) * n_col + n_col - 1;
    }
    float acc = partial[at];
    for (int k = 1; k < S; ++k) acc = acc + partial[at + k * slice];
    if (i < n_w) dw[i] = acc;
    else db[i - n_w] = acc;
  }
}

template <int T> int hidden_wgrad_go(const HiddenWgradArgs &a, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T, n_cgrp = (a.n_col + 3) / 4;
  const int64_t total = (int64_t)a.S * n_cgrp * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(hidden_wgrad_kernel<T>, dim3((unsigned)total), dim3(256), 0, st, a, n_rg, n_cgrp);
  return (int)hipGetLastError();
}

} // namespace

int launch_hidden_pack_t(const float *w, int c_out, int c_a, int c_b, float *wp, void *stream) {
  const int c_in = c_a + c_b, n_rt = hidden_row_tiles(c_in), n_kt = (c_out + kBK - 1) / kBK;
  const int64_t total = (int64_t)hidden_packed_floats(c_in, 0, c_out);
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(hidden_pack_t_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, c_out, c_in, n_rt, n_kt, wp);
  return (int)hipGetLastError();
}

int hidden_dgrad_tiles(int64_t n, int64_t pt, int r0, int r1, int cus) {
  return hidden_dgrad_tiles_go<5, 2, 1>(n * pt, r0, r1, cus, [](auto T) { return (int)T; });
}
int launch_hidden_dgrad(const HiddenDgradArgs &args, int64_t n, int cus, bool vec, void *stream) {
  return hidden_dgrad_tiles_go<5, 2, 1>(n * args.pt, args.r0, args.r1, cus, [&](auto T) { return hidden_dgrad_go<T>(args, n, vec, (hipStream_t)stream); });
}

// T: the most row tiles per block (4, 2, 1) at which the launch still has a block for every CU; 1 when none has (section 5c's rule)
int hidden_wgrad_tiles(int64_t S, int n_col, int c_out) {
  return ckbd_row_tiles_go<4, 2, 1>(S * ((n_col + 3) / 4), c_out, [](auto T) { return (int)T; });
}
int launch_hidden_wgrad(const HiddenWgradArgs &args, void *stream) {
  return ckbd_row_tiles_go<4, 2, 1>((int64_t)args.S * ((args.n_col + 3) / 4), args.c_out, [&](auto T) { return hidden_wgrad_go<T>(args, (hipStream_t)stream); });
}

int launch_hidden_wgrad_finish(const float *partial, int c_a, int c_b, int c_out, bool has_xa, int S, float *dw, float *db, void *stream) {
  const int64_t total = (dw ? (int64_t)c_out * ((int64_t)c_a + c_b) : 0) + (db ? c_out : 0);
  if (total <= 0) return 0;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(hidden_wgrad_finish_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, partial, c_a, c_b, c_out, (int)has_xa, S, dw, db);
  return (int)hipGetLastError();
}

} // namespace fgmm
