// fgmm_conv_grad.hip — the weight and bias gradients of the dense 3x3 / 5x5 convolution layers on the matrix cores, in one fixed order
// (header section 5f).  The data gradient needs no kernel of its own: it is conv_kernel (fgmm_conv.hip) with a gradient staging, over the
// packing conv_pack_kernel<K, true> makes of the layer's own weight (launch_conv_dgrad, there).
//
// Arithmetic: the reduction runs over the positions of ALL items.  Their order: items ascending; in an item its BANDS of 8 image rows
// ascending; in a band its 8 x 16 patches left to right; in a patch its rows, then its columns (positions past the image do not exist).
// conv_wgrad_slices(n, h, w) cuts the n ceil(h / 8) bands into S <= 16 slices of B bands.  For slice k, output channel o and column
// c k^2 + t (input channel c, tap t), on v_mfma_f32_32x32x2_f32, bit for bit the chain
//     acc = +0;  for s ascending in the slice:  acc = fmaf(gz(s)[o], x(s)(c, t), acc)
// with gz formed from (gy, out) by section 2d's rule (grad_act) through the un-shuffle of the forward's store, and x(s)(c, t) the forward's
// tap: +0 outside the image, which takes part in the chain.  Column c_in k^2 is the bias': x = 1.  conv_wgrad_finish_kernel adds the
// slices' partials ascending in binary32 and writes dW [c_out, c_in, k, k] and dbias.  No atomics: every partial has one writer.
//   block  = 256 threads = 4 waves: (T row tiles of 32 output channels) x (a column group: CB = 14 | 10 input channels, CB k^2 = 126 | 250
//            columns and one more, the bias' - 127 | 251 of the 128 | 256 columns of four waves x NT = 1 | 2 tiles of 32) x ONE slice.
//            T x NT x 16 accumulator registers per lane: 128 at the most (k = 5, T = 4).
//   staging: per patch, ONCE, the halo of the group's CB channels into sH - conv_kernel's layout (PITCH 24, PLANE 264 | 312; an element
//            outside the image +0, a channel past c_in -0) - so that an input element crosses from global memory once per block and patch,
//            not k^2 times; and, per HALF patch of 4 rows = 64 positions, the gz tile [32 T rows][64 positions] into sG.  After the
//            channels' planes sH holds one plane of ONES: the bias' column is "channel CB, tap (0, 0)" of it, a column like any other.
//   B reads = the instruction's k is a PAIR of positions (lane half h: the odd one), its n the column: a lane's operand for its column
//            kappa at position p = (pr, pc) is sH[off(kappa) + pr PITCH + pc] - off per lane, computed once; the position a literal of
//            the unrolled loop.  The transpose of the forward, where the position is the lane's and the offset the literal.  A position
//            past the image inside the patch is gz = +0 (when the tile is written) and x = -0 (a select on the read: its taps may lie
//            INSIDE the image): +0 * -0 = -0 leaves every accumulator's bits alone, -0 included - section 5c's padding.
//   sG pitch: kGLd = 64 + 4 floats.  Written: a wave's 64 threads hold one row's 64 positions and write a permutation of 64 consecutive
//            floats - 64 banks.  Position p of the half lies at column (p >> 3) 8 + (p & 1) 4 + ((p & 7) >> 1): a lane's four k-pairs
//            of a group of 8 positions are ONE 16-byte read at row (lane & 31), column 8 g + 4 h.  Such a read is served a quarter
//            wave at a time: 16 lanes = 16 consecutive rows of one half, starting 68 = 4 (mod 64) banks apart - 0, 4, .. 60, sixteen
//            disjoint groups of four banks.  No conflict, either way.  (The B reads of 32 consecutive columns are NOT all disjoint: with
//            PLANE = k PITCH (mod 64) tap row a of channel c + 2 | c + 4 shares banks with row a + 2 | a + 4 - 1 of channel c: at most two
//            lanes a bank.  Lane half 1 reads the address of half 0's next column: a broadcast.)
//   T      = 4, 2 or 1 by the number of blocks of the launch (ckbd_row_tiles_go); a chain does not depend on it.
//   loop   : a slice is a flat sequence of stages (patch, half); one LDS buffer, two barriers per stage; the global loads of the NEXT stage -
//            its gy and out, and before a patch's first half its halo - are issued before this stage's products and land under them; what
//            is written (padding, gz = grad_act(gy, out)) is decided when the stage is stored, as conv_kernel does.
#include "fgmm_ckbd_geom.h"
#include "fgmm_headframe.h"
#include "fgmm_hidden_act.h"

namespace fgmm {
namespace {

constexpr int kPR = kConvPR, kPC = kConvPC;
constexpr int kHalf = kPR / 2 * kPC; // positions of a half patch
constexpr int kGLd = kHalf + 4;      // sG: floats between two rows (the head comment)
static_assert(kPC == 16 && kHalf == 64, "a half patch is 4 rows of 16: 8 groups of 8 positions, two to a row");

template <int K> struct WgradGeom {
  static constexpr int KK = K * K, CB = conv_wgrad_cb(K), KC = CB * KK; // taps; channels and columns of a column group (then the bias')
  static constexpr int NT = (KC + 1 + 127) / 128;                       // column tiles of 32 per wave
  static constexpr int HR = kPR + K - 1, HW = kPC + K - 1;              // the halo's rows and columns
  static constexpr int PITCH = 24, PLANE = K == 3 ? 264 : 312;          // conv_kernel's sH
  static constexpr int HALO_N = CB * HR * HW, HALO_J = (HALO_N + 255) / 256;
  static constexpr int ONES = CB * PLANE, SH = ONES + kPR * PITCH;      // the plane of ones; sH's floats
  static_assert(HW <= PITCH && PLANE >= HR * PITCH && KC + 1 <= 128 * NT, "the halo fits its plane, the columns their tiles");
  // column kappa of the group -> where its feature lies past a position's own (kappa >= KC: the bias' column, and the unused ones)
  __device__ static constexpr int off(int kappa) { return kappa < KC ? (kappa / KK) * PLANE + ((kappa % KK) / K) * PITCH + (kappa % KK) % K : ONES; }
};

template <int K, int T> // kernel size; row tiles per block
__global__ __launch_bounds__(256) void conv_wgrad_kernel(ConvWgradArgs a, int n_rg, int n_cg) {
  using G = WgradGeom<K>;
  constexpr int kRows = 32 * T, kGJ = kRows * kHalf / 256;
  __shared__ __attribute__((aligned(16))) float sG[kRows * kGLd];
  __shared__ float sH[G::SH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  const int B = (int)blockIdx.x, rg = B % n_rg, cg = (B / n_rg) % n_cg, sl = B / (n_rg * n_cg);
  const int hgt = a.h, wid = a.w, c_in = a.c_in, c_out = a.c_out;
  const int64_t hw = (int64_t)hgt * wid;
  const bool sh = a.shuffle == 2, has_act = a.act != FGMM_ACT_NONE, relu = a.act == FGMM_ACT_RELU;
  const float slope = a.slope;
  // the wave's columns: tile ti is columns (wave NT + ti) 32 ..+31 of the group; the lane's, col of them
  const float *bptr[G::NT];
#pragma unroll
  for (int ti = 0; ti < G::NT; ++ti) bptr[ti] = sH + G::off((wave * G::NT + ti) * 32 + col) + h;
  f16_t acc[G::NT][T];
#pragma unroll
  for (int ti = 0; ti < G::NT; ++ti)
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tl][r] = 0.0f;
  for (int i = tid; i < kPR * G::PITCH; i += 256) sH[G::ONES + i] = 1.0f; // (read after the first patch's barriers)
  const float *a_base = sG + col * kGLd + h * 4;
  // ---- the slice as a flat sequence of STAGES: stage st is half (st & 1) of patch (st >> 1) % pw of band b0 + (st >> 1) / pw
  const int b0 = sl * a.B, n_st = (min(b0 + a.B, a.nb) - b0) * a.pw * 2;
  struct At { const float *x; const FGMM_GLOBAL float *gy, *yo; int r0, q0; };
  auto place = [&](int st) {
    const int b = b0 + (st >> 1) / a.pw, item = b / a.bh;
    const int64_t g_at = (int64_t)item * c_out * hw;
    return At{a.x + (int64_t)item * a.x_item_stride, (const FGMM_GLOBAL float *)(a.gy + g_at), (const FGMM_GLOBAL float *)(has_act ? a.out + g_at : a.gy), // (out: null
              (b - item * a.bh) * kPR, ((st >> 1) % a.pw) * kPC};                                                                          // without an activation: not read)
  };
  // Staging, branch-free as conv_kernel's: a load that would fall outside reads a valid address instead; what is written - the element,
  // its padding, gz from (gy, out) - is decided when the stage is stored, where the loads have to have landed anyway
  float rh[G::HALO_J], rgy[kGJ], ryo[kGJ];
  unsigned rh_ok = 0, rh_ch = 0, rz_ok = 0; // bit j: the halo element is inside the image and below c_in; its channel is below c_in; gz's is real
  auto load_halo = [&](const At &p) {
    rh_ok = 0, rh_ch = 0;
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j) {
      const int e = tid + 256 * j, c = cg * G::CB + e / (G::HR * G::HW);
      const int r = p.r0 + (e / G::HW) % G::HR - K / 2, q = p.q0 + e % G::HW - K / 2;
      const bool k_ok = c < c_in, in = e < G::HALO_N && ckbd_inside(r, q, hgt, wid);
      rh[j] = ((const FGMM_GLOBAL float *)(p.x + (int64_t)(k_ok ? c : c_in - 1) * hw))[in ? r * wid + q : 0];
      rh_ok |= (in && k_ok ? 1u : 0u) << j, rh_ch |= (k_ok ? 1u : 0u) << j;
    }
  };
  auto load_gz = [&](const At &p, int half) { // thread's element j: row (tid >> 6) + 4 j, position tid & 63 of the half patch
    rz_ok = 0;
#pragma unroll
    for (int j = 0; j < kGJ; ++j) {
      const int o = rg * kRows + (tid >> 6) + 4 * j, pos = tid & 63;
      const int r = p.r0 + 4 * half + (pos >> 4), q = p.q0 + (pos & 15);
      const bool ok = o < c_out && r < hgt && q < wid;
      // shuffle 2: channel o of the convolution is plane o >> 2, row 2 r + ((o >> 1) & 1), column 2 q + (o & 1) of [c_out / 4, 2 h, 2 w]
      const int64_t at = !ok ? 0 : sh ? (int64_t)(o >> 2) * 4 * hw + (int64_t)(2 * r + ((o >> 1) & 1)) * 2 * wid + 2 * q + (o & 1) : (int64_t)o * hw + r * wid + q;
      rgy[j] = p.gy[at];
      if (has_act) ryo[j] = p.yo[at];
      rz_ok |= (ok ? 1u : 0u) << j;
    }
  };
  auto store_halo = [&]() {
#pragma unroll
    for (int j = 0; j < G::HALO_J; ++j) {
      const int e = tid + 256 * j;
      const float v = (rh_ok >> j) & 1u ? rh[j] : ((rh_ch >> j) & 1u ? 0.0f : -0.0f);
      if (e < G::HALO_N) sH[(e / (G::HR * G::HW)) * G::PLANE + ((e / G::HW) % G::HR) * G::PITCH + e % G::HW] = v;
    }
  };
  auto store_gz = [&]() {
#pragma unroll
    for (int j = 0; j < kGJ; ++j) {
      const int pos = tid & 63;
      const float g = has_act ? grad_act(rgy[j], ryo[j], relu, slope) : rgy[j];
      sG[((tid >> 6) + 4 * j) * kGLd + (pos >> 3) * 8 + (pos & 1) * 4 + ((pos & 7) >> 1)] = (rz_ok >> j) & 1u ? g : 0.0f;
    }
  };
  // 8 groups of four position pairs: group g is patch row 4 half + (g >> 1), columns 8 (g & 1) ..+7
  auto multiply = [&](const At &p, int half) {
    const int rv = hgt - p.r0, cvh = wid - p.q0 - h; // the patch's rows, and the lane half's columns, inside the image
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      float4_t av[T];
      float bv[G::NT][4];
#pragma unroll
      for (int tl = 0; tl < T; ++tl) av[tl] = *reinterpret_cast<const float4_t *>(a_base + tl * 32 * kGLd + g * 8);
      const bool row_in = 4 * half + (g >> 1) < rv;
#pragma unroll
      for (int ti = 0; ti < G::NT; ++ti)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = bptr[ti][half * 4 * G::PITCH + (g >> 1) * G::PITCH + (g & 1) * 8 + 2 * e];
          bv[ti][e] = row_in && (g & 1) * 8 + 2 * e < cvh ? v : -0.0f;
        }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int ti = 0; ti < G::NT; ++ti)
#pragma unroll
          for (int tl = 0; tl < T; ++tl) acc[ti][tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl][e], bv[ti][e], acc[ti][tl], 0, 0, 0);
    }
  };
  At cur = place(0);
  load_halo(cur);
  load_gz(cur, 0);
  for (int st = 0; st < n_st; ++st) {
    const int half = st & 1;
    __syncthreads(); // every wave has multiplied the stage before
    if (!half) store_halo();
    store_gz();
    __syncthreads();
    // the next stage's global loads are in flight under this stage's products (after the last stage: it loads itself again, harmless)
    const At nxt = place(st + 1 < n_st ? st + 1 : st);
    if (half) load_halo(nxt);
    load_gz(nxt, half ^ 1);
    multiply(cur, half);
    cur = nxt;
  }
  // ---- epilogue: register reg of row tile tl is output channel rg * 32 T + tl * 32 + mfma32_row(reg, h), at the lane's column
  const int64_t n_col = (int64_t)c_in * G::KK + 1; // conv_wgrad_cols
#pragma unroll
  for (int ti = 0; ti < G::NT; ++ti) {
    const int kappa = (wave * G::NT + ti) * 32 + col, c = cg * G::CB + kappa / G::KK;
    int64_t column = -1;
    if (kappa < G::KC) column = c < c_in ? (int64_t)c * G::KK + kappa % G::KK : -1;
    else if (kappa == G::KC && cg == 0) column = n_col - 1; // the bias': the first column group's
    if (column < 0) continue;
    float *out = a.partial + (int64_t)sl * c_out * n_col + column;
#pragma unroll
    for (int tl = 0; tl < T; ++tl)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int o = rg * kRows + tl * 32 + mfma32_row(reg, h);
        if (o < c_out) stg<float>(out + (int64_t)o * n_col, acc[ti][tl][reg]);
      }
  }
}

// dW[o][c][t] = ((partial_0 + partial_1) + partial_2) + ... at column c k^2 + t; dbias[o] at column c_in k^2
__global__ __launch_bounds__(256) void conv_wgrad_finish_kernel(const float *__restrict__ partial, int c_out, int64_t n_col, int S, float *__restrict__ dw,
                                                                float *__restrict__ db) {
  const int64_t n_w = (int64_t)c_out * (n_col - 1), n_b = db ? c_out : 0, slice = (int64_t)c_out * n_col;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_w + n_b; i += (int64_t)gridDim.x * 256) {
    const int64_t at = i < n_w ? i / (n_col - 1) * n_col + i % (n_col - 1) : (i - n_w) * n_col + n_col - 1; // of partial_0
    float acc = partial[at];
    for (int k = 1; k < S; ++k) acc = acc + partial[at + k * slice];
    if (i < n_w) dw[i] = acc;
    else db[i - n_w] = acc;
  }
}

template <int K, int T> int conv_wgrad_go(const ConvWgradArgs &a, hipStream_t st) {
  const int n_rg = ((a.c_out + 31) / 32 + T - 1) / T, n_cg = (a.c_in + WgradGeom<K>::CB - 1) / WgradGeom<K>::CB;
  const int64_t total = (int64_t)a.S * n_cg * n_rg;
  if (total <= 0) return 0;
  if (total > (1ll << 30)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((conv_wgrad_kernel<K, T>), dim3((unsigned)total), dim3(256), 0, st, a, n_rg, n_cg);
  return (int)hipGetLastError();
}

int64_t wgrad_outer(int64_t S, int c_in, int k) { return S * ((c_in + conv_wgrad_cb(k) - 1) / conv_wgrad_cb(k)); }

} // namespace

// T: the most row tiles per block (4, 2, 1) at which the launch still has a block for every CU; 1 when none has
int launch_conv_wgrad(const ConvWgradArgs &args, int k, void *stream) {
  return ckbd_row_tiles_go<4, 2, 1>(wgrad_outer(args.S, args.c_in, k), args.c_out, [&](auto T) {
    return k == 3 ? conv_wgrad_go<3, T>(args, (hipStream_t)stream) : conv_wgrad_go<5, T>(args, (hipStream_t)stream);
  });
}

int launch_conv_wgrad_finish(const float *partial, int c_out, int c_in, int k, int S, float *dw, float *db, void *stream) {
  const int64_t n_col = conv_wgrad_cols(c_in, k), total = (int64_t)c_out * (n_col - 1) + (db ? c_out : 0);
  if (total <= 0) return 0;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(conv_wgrad_finish_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, partial, c_out, n_col, S, dw, db);
  return (int)hipGetLastError();
}

} // namespace fgmm
