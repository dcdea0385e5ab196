// fgmm_centroid.hip — centroid reconstruction of a decoded latent (include/flashgmm_amd.h section 3i), for CDNA4 / gfx950 (MI355X), wave64.
//
//   centroid_kernel   (y, sigma, mu, pi | logits) -> rec = rintf(y) + the bin's conditional mean offset under the mixture, where the
//                     model has something to say about the bin; the item's count of such latents
//
// The decoder-side twin of RDOQ: the twelve parameters of a latent say where inside [q - 1/2, q + 1/2) it most probably lay.  The
// kernel is like_kernel's forward with one more sum: the same frame (fgmm_encframe.h: placement in either grid, VEC-wide loads of
// float32 / float16 / bfloat16 planes widened exactly as they arrive, no chan_list - every channel), the same like_term per component,
// then the component's first moment about v - in the literal form for a narrow component, as a three-term series in h = 1/(2 s) for a
// wide one, where the literal form cancels to 1/(12 s^2) of its terms (both are evaluated, the result is the select: a wave's lanes
// differ).  52 B in and 4 B out per latent.  The arithmetic is section 3i's, literally: binary32, no contraction (-ffp-contract=off),
// correctly rounded '/'.  keep is counted per wave by ballot and popcount, one integer atomic per wave: the same bits on every run.
#include <hip/hip_runtime.h>

#include "fgmm_encframe.h"

namespace fgmm {

constexpr float kCentroidC23 = (float)(2.0 / 3.0), kCentroidC15 = (float)(1.0 / 15.0), kCentroidC420 = (float)(1.0 / 420.0);

// |first moment about v| of the bin under one component, from like_term's s, xu, xl and p (a = |v - mu|)
__device__ __forceinline__ float centroid_moment(float a, float s, float xu, float xl, float p) {
  const float narrow = a * p - s * (like_phi(xu) - like_phi(xl));
  const float h = 0.5f / s;
  const float xb = a * (h + h);
  const float h2 = h * h, x2 = xb * xb;
  const float q = (kCentroidC23 + (h2 * (x2 - 3.0f)) * kCentroidC15) + ((h2 * h2) * ((x2 - 10.0f) * x2 + 15.0f)) * kCentroidC420;
  const float wide = ((a * like_phi(xb)) * (h * h2)) * q;
  return s >= 2.0f ? wide : narrow; // (a NaN s: the narrow form's NaN)
}

template <int VEC, typename PT, bool LINEAR, bool LOGITS>
__global__ __launch_bounds__(kBlock) void centroid_kernel(const EncDesc *__restrict__ descs, const CentroidDesc *__restrict__ cdescs, float sb, float p_min) {
  const EncDesc &d = descs[blockIdx.z];
  const CentroidDesc &r = cdescs[blockIdx.z];
  const int64_t hw = d.hw;
  int c;
  int64_t p0;
  bool active;
  if (!enc_place<VEC, LINEAR>(hw, d.M, c, p0, active)) return;
  unsigned long long kept = 0; // wave-uniform: the wave's latents with keep
  if (active) {
    float v[VEC], rec[VEC];
    enc_load_y<VEC>(d, c, p0, v); // (before the store below: rec may be y)
    EncPlanes<PT, VEC> P;
    P.load(d, c, p0);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float mu[4], sg[4], pi[4];
      P.get(e, LOGITS, mu, sg, pi);
      bool ok = true; // every s_k finite: a component of infinite sigma carries no mass, the latent keeps v
      const float ve = __builtin_rintf(v[e]); // round-half-even == torch.round
      float L = 0.0f, N = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float s, xu, xl;
        const float p = like_term(ve, mu[k], sg[k], sb, s, xu, xl);
        L = L + p * pi[k];
        const float t = ve - mu[k];
        const float sgn = (float)((t > 0.0f) - (t < 0.0f));
        N = N + (pi[k] * sgn) * centroid_moment(__builtin_fabsf(t), s, xu, xl, p);
        ok = ok && s < INFINITY;
      }
      const float off = (-N) / L;
      const bool keep = ok && L >= p_min && __builtin_fabsf(off) <= 0.5f; // (false for any NaN)
      rec[e] = keep ? ve + off : ve;
      kept += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(keep));
      if constexpr (VEC == 1) break; // (one position: no loop, see EncPlanes<PT, 1>)
    }
    enc_st<float, VEC>(r.rec + (int64_t)c * hw + p0, rec);
  }
  // lanes past the end of a channel (tiled grid) took no part in the ballots; lane 0 is active whenever any lane is, and holds the count
  if ((threadIdx.x & 63) == 0 && kept) add64(r.kept, kept);
}

template <bool LOGITS> struct CentroidLaunch {
  const EncDesc *d;
  const CentroidDesc *r;
  float sb, p_min;
  static constexpr bool kVec8 = true;
  template <int VEC, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    hipLaunchKernelGGL((centroid_kernel<VEC, PT, LINEAR, LOGITS>), grid, dim3(kBlock), 0, s, d, r, sb, p_min);
  }
};

int launch_centroid(const EncDesc *d_descs, const CentroidDesc *d_cdescs, float scale_bound, float p_min, int count, int M_max, int64_t hw_max,
                    int64_t n_max, bool linear, int vec, int planes, bool logits, void *stream) {
  if (logits) return like_launch(CentroidLaunch<true>{d_descs, d_cdescs, scale_bound, p_min}, count, M_max, hw_max, n_max, linear, vec, planes, stream);
  return like_launch(CentroidLaunch<false>{d_descs, d_cdescs, scale_bound, p_min}, count, M_max, hw_max, n_max, linear, vec, planes, stream);
}

} // namespace fgmm
