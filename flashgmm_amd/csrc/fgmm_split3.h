// fgmm_split3.h — the split of a binary32 into three bfloat16 parts and its domain, once, for the bf16x6 kernels: the parameter head's
// (fgmm_head16.hip) and the checkerboard context convolution's (fgmm_ckbd_ctx16.hip).  The parts one kernel multiplies are the parts the
// other does because they run this text, not a copy of it.
#pragma once
#include "fgmm_dev.h"

namespace fgmm {

typedef __bf16 bf8_t __attribute__((ext_vector_type(8)));    // one lane's operand of v_mfma_f32_32x32x16_bf16: eight consecutive k
typedef uint32_t u4_t __attribute__((ext_vector_type(4)));   // the same sixteen bytes as they are copied

struct Split3 {
  uint16_t p[3];
};
__device__ __forceinline__ uint16_t bf_bits(__bf16 b) { return __builtin_bit_cast(uint16_t, b); }
__device__ __forceinline__ Split3 split3(float v) {
  const __bf16 a = (__bf16)v; // round to nearest even (v_cvt_pk_bf16_f32)
  const float r1 = v - (float)a;
  const __bf16 b = (__bf16)r1;
  const float r2 = r1 - (float)b;
  const __bf16 c = (__bf16)r2;
  return Split3{{bf_bits(a), bf_bits(b), bf_bits(c)}};
}

// the operands whose three bfloat16 parts carry them: finite, and not rounding to an infinite first part (|v| < 0x1.FFp127; NaN fails
// the test).  Beyond, split3 gives (+-inf, NaN, NaN), and the six part products turn an infinite or a finite exact result into NaN.
__device__ __forceinline__ bool in_domain(float v) { return __builtin_fabsf(v) < 0x1.FFp127f; }

} // namespace fgmm
