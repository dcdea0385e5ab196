// fgmm_mfma32.h — the binary32 matrix-core tile that head_kernel (fgmm_head.hip) and ckbd_ctx_kernel (fgmm_ckbd_ctx.hip) share, and whose
// fragments ckbd_ctx_wgrad_kernel (fgmm_ckbd_ctx_grad.hip) reads: v_mfma_f32_32x32x2_f32, 256 threads = 4 waves, a block of T row tiles
// of 32 rows x 128 positions (a wave: all rows x 32 positions), K tiles of kMfma32BK staged through ONE LDS buffer.  A kernel adds
// what it loads and what it does with the accumulators; the chain  acc = fmaf(A[row][k], B[k][position], acc), k ascending  (lane half 0
// of the instruction holds the even k of a pair, half 1 the odd one) is the same bits in all of them because they run this text, not
// a copy of it.
#pragma once
#include "fgmm_dev.h"

namespace fgmm {

typedef float f16_t __attribute__((ext_vector_type(16))); // one 32x32 accumulator tile: row mfma32_row(reg, lane >> 5), column lane & 31

constexpr int kMfma32PB = 128;           // positions per block (4 waves x 32)
constexpr int kMfma32ALd = kMfma32BK + 4; // LDS row pitch of the A tile (floats): 16-byte reads of 64 lanes hit 64 different banks
constexpr int kMfma32BLd = kMfma32PB + 32; // ... of the B tile: the two lane halves read rows k, k + 1 -> banks 32 apart

// the row of a 32x32 accumulator tile that register reg of lane half h holds
__device__ __forceinline__ constexpr int mfma32_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
// packed A tiles: column q = h * 16 + s of a tile holds k = 2 s + h of the tile - a lane's 16-byte read is its half's four k-pairs
__device__ __forceinline__ constexpr int mfma32_pack_col(int q) { return 2 * (q & 15) + (q >> 4); }

// the fragments of four k-pairs: one 16-byte A read per row tile, one 4-byte B read per k-pair (b_ld: the B tile's pitch)
template <int T> struct Mfma32Frag {
  float4_t a[T];
  float b[4];
};
template <int T> __device__ __forceinline__ void mfma32_read_frag(Mfma32Frag<T> &f, const float *a_base, const float *b_base, int b_ld) {
#pragma unroll
  for (int tl = 0; tl < T; ++tl) f.a[tl] = *reinterpret_cast<const float4_t *>(a_base + tl * 32 * kMfma32ALd);
#pragma unroll
  for (int e = 0; e < 4; ++e) f.b[e] = b_base[2 * e * b_ld];
}
template <int T> __device__ __forceinline__ void mfma32_multiply(f16_t (&acc)[T], const Mfma32Frag<T> &f) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int tl = 0; tl < T; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[tl][e], f.b[e], acc[tl], 0, 0, 0);
}

// staging.  A: the thread's 16 bytes of one packed tile [32 rows][kMfma32BK columns] (256 threads x 16 bytes), `ahead` 16-byte words
// past `tile` - the kernel's row tile j: 256 j in the head, j * n_kt * 256 in the context kernel.  (One load, not the loop over the
// row tiles: a loop in here is unrolled before the kernel's own and the prologue's addresses take another register)
constexpr int kMfma32TileW = 32 * kMfma32BK; // floats of one packed tile
template <typename I> __device__ __forceinline__ float4_t mfma32_load_a(const float *tile, I ahead) {
  return ((const FGMM_GLOBAL float4_t *)tile)[(int)threadIdx.x + ahead];
}
// B: [kMfma32BK][128 positions], thread's register j = row (tid >> 5) + 8 j, positions 4 (tid & 31) ..+3.  A load that would have fallen
// outside read a valid address instead (the K loop stays ONE basic block) and is replaced here, when the tile is WRITTEN - a select
// right after the load would wait for it, and the loads are there to be in flight under a tile's products.  ok bit 4 j + e: element e
// of rb[j] is kept; else it becomes fill(j).  -0 where the packed A is +0 (padding): +0 * -0 = -0 adds nothing to any accumulator, -0
// included (+0 + -0 = +0 would turn a chain that ends at -0 into +0)
template <int T, typename Fill>
__device__ __forceinline__ void mfma32_store_tile(float *sA, float *sB, const float4_t (&ra)[T], const float4_t (&rb)[4], unsigned ok, Fill fill) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int f = tid + 256 * j;
    *reinterpret_cast<float4_t *>(&sA[(f >> 3) * kMfma32ALd + (f & 7) * 4]) = ra[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f = tid + 256 * j;
    const float fl = fill(j);
    float4_t v = rb[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (ok >> (4 * j + e)) & 1u ? v[e] : fl;
    *reinterpret_cast<float4_t *>(&sB[(f >> 5) * kMfma32BLd + (f & 31) * 4]) = v;
  }
}

// The K loop over sA [32 T][kMfma32ALd], sB [kMfma32BK][kMfma32BLd].  load_tile(kt) brings tile kt into the kernel's registers,
// store_tile() writes them to LDS.  The global loads of tile i + 1 are in flight while tile i is multiplied, the fragments are read
// one group of four k-pairs AHEAD of the products that use them; one LDS buffer, two barriers per tile - the CU's OTHER block
// multiplies meanwhile (two blocks drift out of phase by themselves: a block's prologue, barriers and epilogue fall under the other's
// products; one block per CU with twice the tile: 0.67 of the roof).  The loop is ONE basic block, so that the order below is the
// order issued, and __builtin_amdgcn_sched_barrier(0) lets nothing be scheduled across it: left to itself the scheduler sinks every
// LDS read to just before its first use and the global loads to just before the LDS writes - each then waited for with the matrix
// pipe idle.  wave, h = lane >> 5, col = lane & 31: the KERNEL's values - recomputed here they are one more live value through the
// loop, and the fragments' addresses change registers (profiles/mfma32_tile_refactor.md)
#define FGMM_FENCE() __builtin_amdgcn_sched_barrier(0)
template <int T, typename Load, typename Store>
__device__ __forceinline__ void mfma32_k_loop(f16_t (&acc)[T], const float *sA, const float *sB, int n_kt, int wave, int h, int col, Load &&load_tile,
                                              Store &&store_tile) {
  const float *a_base = sA + col * kMfma32ALd + h * 16;
  const float *b_base = sB + h * kMfma32BLd + wave * 32 + col;
  auto read_frag = [&](Mfma32Frag<T> &f, int s4) { mfma32_read_frag(f, a_base + s4 * 4, b_base + 8 * s4 * kMfma32BLd, kMfma32BLd); };
  load_tile(0);
  store_tile();
  __syncthreads();
  Mfma32Frag<T> f0, f1;
  read_frag(f0, 0);
  for (int kt = 0; kt < n_kt; ++kt) {
    // 16 T products per wave and tile in four groups; before a group, what a LATER step needs is issued: the global loads of the
    // next tile (the last tile loads itself again: harmless) and the fragments of the next group
    FGMM_FENCE();
    load_tile(kt + 1 < n_kt ? kt + 1 : kt);
    read_frag(f1, 1);
    FGMM_FENCE();
    mfma32_multiply(acc, f0);
    FGMM_FENCE();
    read_frag(f0, 2);
    FGMM_FENCE();
    mfma32_multiply(acc, f1);
    FGMM_FENCE();
    read_frag(f1, 3);
    FGMM_FENCE();
    mfma32_multiply(acc, f0);
    mfma32_multiply(acc, f1);
    FGMM_FENCE();
    __syncthreads(); // every wave has read the tile
    store_tile();
    __syncthreads();
    read_frag(f0, 0); // (after the last tile: a read that nobody uses)
  }
}
#undef FGMM_FENCE

} // namespace fgmm
