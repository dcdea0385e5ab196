// fgmm_ckbd_geom.h — the checkerboard's geometry, once, for the context convolution's kernels (fgmm_ckbd_ctx.hip, fgmm_ckbd_ctx_grad.hip):
// the 12 kept taps of the 5x5, where a compact non-anchor lies at full size and where the anchor a tap reads lies in the compact
// half; and the one rule by which their launchers pick the row tiles of a block.
#pragma once
#include <type_traits>
#include "fgmm_dev.h"

namespace fgmm {

// tap t = 0 .. 11: the kernel positions (i, j) with i + j odd, row-major - flat index 2 t + 1 of the 25, offset (i - 2, j - 2)
FGMM_HD constexpr int ckbd_tap_flat(int t) { return 2 * t + 1; }
struct CkbdTap { int di, dj; };
__device__ __forceinline__ CkbdTap ckbd_tap(int t) { return {ckbd_tap_flat(t) / 5 - 2, ckbd_tap_flat(t) % 5 - 2}; }
// compact non-anchor q of an [h, w2] half -> its row and FULL-SIZE column (odd: the parity of the non-anchors of row 0)
struct CkbdAt { int r, c; };
__device__ __forceinline__ CkbdAt ckbd_nonanchor(int q, int w2, int odd) {
  const int r = q / w2, j = q - r * w2;
  return {r, 2 * j + 1 - ((r + odd) & 1)};
}
// is full-size (rr, cc) inside the hgt x wid image?  A tap of a non-anchor that is, is an anchor: compact (rr, cc >> 1)
__device__ __forceinline__ bool ckbd_inside(int rr, int cc, int hgt, int wid) { return (unsigned)rr < (unsigned)hgt && (unsigned)cc < (unsigned)wid; }
__device__ __forceinline__ int ckbd_anchor_at(int rr, int cc, int w2) { return rr * w2 + (cc >> 1); }

// row tiles per block: the first of the candidates T, Ts... (descending) at which the launch - `outer` blocks per group of T row
// tiles - still has a block for every CU (kCkbdCtxFill); the last when none has.  -> go(std::integral_constant<int, T>)
template <int T, int... Ts, typename Go> static int ckbd_row_tiles_go(int64_t outer, int c_out, const Go &go) {
  const int64_t n_rt = (c_out + 31) / 32;
  if constexpr (sizeof...(Ts) > 0)
    if (outer * ((n_rt + T - 1) / T) < kCkbdCtxFill) return ckbd_row_tiles_go<Ts...>(outer, c_out, go);
  return go(std::integral_constant<int, T>{});
}

} // namespace fgmm
