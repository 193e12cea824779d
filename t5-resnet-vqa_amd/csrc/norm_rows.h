// Per-row forward arithmetic of the row normalisations, one wave per row: lane l holds
// float4 i*64 + l of the row (i < NV, D = NV * 256).  Shared by the stand-alone kernels
// (norms.hip) and the GEMM's fused norm tail (gemm_body.h), which must produce the same bits.
//
// FMA contraction is pinned: the functions compile with contraction off and spell out every
// fused multiply-add, exactly where the stand-alone kernels had them when their arithmetic
// still lived in norms.hip under the compiler's default contraction (read off their ISA):
//   RMSNorm    sum of squares: fma for every float4 of the lane but its last, mul + add there
//              (and the chain starts fma(x0, x0, x1*x1), not fma(x1, x1, x0*x0));
//   both       sum / D + eps:  fma(sum, 1/D, eps) when D is a power of two (256, 512, 1024),
//                              a true division then an add at D = 768;
//   LayerNorm  sum of squared deviations: mul + add;  (x - mu) * r * g + b: fma(.., g, b).
#pragma once
#include "common.h"

namespace {

template <int NV>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&x)[NV][4]) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float4 v = reinterpret_cast<const float4*>(p)[i * 64 + l];
    x[i][0] = v.x; x[i][1] = v.y; x[i][2] = v.z; x[i][3] = v.w;
  }
}
template <int NV>
__device__ __forceinline__ void store_row32(float* __restrict__ p, const float (&x)[NV][4]) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    reinterpret_cast<float4*>(p)[i * 64 + l] = make_float4(x[i][0], x[i][1], x[i][2], x[i][3]);
}
template <int NV>
__device__ __forceinline__ void store_row16(bf16_t* __restrict__ p, const float (&x)[NV][4]) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    uint2 u;
    u.x = (uint32_t)f2bf(x[i][0]) | ((uint32_t)f2bf(x[i][1]) << 16);
    u.y = (uint32_t)f2bf(x[i][2]) | ((uint32_t)f2bf(x[i][3]) << 16);
    reinterpret_cast<uint2*>(p)[i * 64 + l] = u;
  }
}
template <int NV>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float (&x)[NV][4]) { load_row<NV>(p, x); }

// multiply a row held as [NV][4] per lane by the dropout factors of row `row`
template <int NV>
__device__ __forceinline__ void drop_row(const DropK& k, int row, float (&x)[NV][4]) {
  if (!k.on) return;
  const int l = threadIdx.x & 63;
  const uint32_t base = (uint32_t)row * (uint32_t)(NV * 256);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) x[i][j] *= drop_mul(k, base + (uint32_t)((i * 64 + l) * 4 + j));
}

// sum / D + eps
template <int NV>
__device__ __forceinline__ float norm_mean_eps(float sum, float eps) {
#pragma clang fp contract(off)
  constexpr int D = NV * 256;
  if constexpr ((D & (D - 1)) == 0) return __builtin_fmaf(sum, 1.f / D, eps);
  else return sum / D + eps;
}

// T5LayerNorm: v <- g * (v * r), r = rsqrt(mean(v^2) + eps); returns r
template <int NV>
__device__ __forceinline__ float rmsnorm_row(float (&v)[NV][4], const float (&g)[NV][4], float eps) {
#pragma clang fp contract(off)
  // the first two squares of a lane with more than one float4: x0^2 fused onto the ROUNDED x1^2
  float ss = NV > 1 ? __builtin_fmaf(v[0][0], v[0][0], v[0][1] * v[0][1]) : 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (NV > 1 && i == 0 && j < 2) continue;
      ss = i < NV - 1 ? __builtin_fmaf(v[i][j], v[i][j], ss) : ss + v[i][j] * v[i][j];
    }
  ss = wave_sum(ss);
  const float r = rsqrtf(norm_mean_eps<NV>(ss, eps));
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = g[i][j] * (v[i][j] * r);
  return r;
}

// nn.LayerNorm statistics of a row: mu, and r = rsqrt(var + eps) (returned)
template <int NV>
__device__ __forceinline__ float layernorm_stats(const float (&v)[NV][4], float eps, float& mu_out) {
#pragma clang fp contract(off)
  constexpr int D = NV * 256;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += v[i][j];
  const float mu = wave_sum(s) / D;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) { float t = v[i][j] - mu; ss += t * t; }
  mu_out = mu;
  return rsqrtf(norm_mean_eps<NV>(wave_sum(ss), eps));
}

// v <- (v - mu) * r * g + b
template <int NV>
__device__ __forceinline__ void layernorm_apply(float (&v)[NV][4], float mu, float r, const float (&g)[NV][4],
                                                const float (&b)[NV][4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = __builtin_fmaf((v[i][j] - mu) * r, g[i][j], b[i][j]);
}

}  // namespace
