// fgmm_hidden_act.h — the library's activations (header section 2c), one binary32 operation each, once, for the two forms of a hidden
// layer: hidden_kernel (fgmm_hidden.hip) and hidden16_kernel (fgmm_hidden16.hip) apply them to their binary32 accumulators.  Both files
// are compiled with the packed fp32 instructions off (build.sh): the sequences stay scalar.
#pragma once
#include "fgmm_dev.h"

namespace fgmm {

__device__ __forceinline__ float act_leaky(float v, float s) { return v > 0.0f ? v : v * s; }
__device__ __forceinline__ float act_relu(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }

// act (FGMM_ACT_*) chosen once per kernel, outside the loop over a lane's outputs: f(one of the three as a callable)
template <typename F> __device__ __forceinline__ void with_activation(int act, float slope, const F &f) {
  if (act == FGMM_ACT_LEAKY) f([slope](float v) { return act_leaky(v, slope); });
  else if (act == FGMM_ACT_RELU) f([](float v) { return act_relu(v); });
  else f([](float v) { return v; });
}

// the activation's derivative (header sections 2d and 5f): gz from (gy, out), the saved OUTPUT.  leaky, relu are the call's activation
// (both false: gz = gy, and `out` is whatever the caller passes); a NaN output takes the second branch
__device__ __forceinline__ float grad_act(float gy, float out, bool relu, float slope) {
  const float scaled = gy * slope;
  const float off = relu ? 0.0f : scaled;
  return out > 0.0f ? gy : off;
}

} // namespace fgmm
