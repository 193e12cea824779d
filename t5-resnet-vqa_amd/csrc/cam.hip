// The CNN models' heat map (the reference's CNN_vqa_heatmap.py:131-137) and the FPN's top-down
// upsample, over NHWC bf16 feature maps.
//
//   vqa_channel_cam      per image: cam[p] = mean over the channels of x[b, p, :] (fp32), then
//                        heat = (cam - min_p cam) / (max_p cam - min_p cam)
//   vqa_upsample2x_nhwc  dst[b, y, x, :] = src[b, y / 2, x / 2, :] (nearest, exact 2x)
//
// vqa_channel_cam is a streaming read of B * P * C bf16 (12.8 MB for ResNet-50 at B = 64, 224^2),
// so one workgroup per image would leave most of 256 CUs idle at B <= 64.  The positions of an
// image are split over workgroups instead: a workgroup of 4 waves takes CAM_WAVES * (64 / G)
// consecutive positions, G = the lanes that share one position (the largest power of two
// <= min(64, C / 8): every lane loads 16 bytes along C).  A position's channel sum is formed by
// its G lanes in a fixed order (each lane its 16-byte chunks j, j + G, ... in ascending order, the
// 8 values of a chunk pairwise; then a G-lane butterfly), so it does not depend on how the
// positions were split.  The channel means go to `heat` (and `mean`) write-through; the
// workgroup that arrives last on the image's counter (the hand-off of vqa_grad_sqnorm_final:
// sc1 stores, the storing waves drain, barrier, one relaxed agent-scope add on a counter word
// that has a 256-byte line to itself; the last arriver puts it back to zero) reads the image's
// P means back with sc1 loads, past its L1, takes min and max and overwrites `heat` with the
// normalised map.  (With an agent-scope release fence in every workgroup instead of the drained
// sc1 stores, and the images' counters side by side in two lines, a call took 37 us at
// 64 x 49 x 2048; this form 9.0 us issued eagerly, 5.6 us replayed from a graph.)  No float
// atomics: the same bits every run.  A constant map (P = 1 included) gives 0 / 0 = NaN, as the
// reference's expression does.
#include "common.h"

namespace {

typedef __attribute__((address_space(1))) unsigned gu32;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

constexpr int CAM_THREADS = 256, CAM_WAVES = CAM_THREADS / 64, CAM_MAX_P = 1024;

__device__ __forceinline__ float sum8(uint4 u) {
  const float a0 = __uint_as_float(u.x << 16), a1 = __uint_as_float(u.x & 0xffff0000u);
  const float a2 = __uint_as_float(u.y << 16), a3 = __uint_as_float(u.y & 0xffff0000u);
  const float a4 = __uint_as_float(u.z << 16), a5 = __uint_as_float(u.z & 0xffff0000u);
  const float a6 = __uint_as_float(u.w << 16), a7 = __uint_as_float(u.w & 0xffff0000u);
  return ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
}

// grid = batch * chunks; G lanes per position, pw = CAM_WAVES * (64 / G) positions per workgroup
__global__ __launch_bounds__(CAM_THREADS) void channel_cam(const bf16_t* __restrict__ x, int positions, int c8,
                                                           int G, int chunks, float* mean, float* heat,
                                                           unsigned* cnt) {
  __shared__ float red[2 * CAM_WAVES];
  __shared__ int flag;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int per_wave = 64 / G;
  const int p = (chunk * CAM_WAVES + w) * per_wave + l / G, j = l & (G - 1);
  const bool ok = p < positions;
  float s = 0.f;
  if (ok) {
    const uint4* row = reinterpret_cast<const uint4*>(x + ((long)b * positions + p) * (8l * c8));
    int i = j;
    for (; i + 3 * G < c8; i += 4 * G) {                  // four 16-byte loads in flight per lane
      const uint4 u0 = row[i], u1 = row[i + G], u2 = row[i + 2 * G], u3 = row[i + 3 * G];
      s += sum8(u0); s += sum8(u1); s += sum8(u2); s += sum8(u3);
    }
    for (; i < c8; i += G) s += sum8(row[i]);
  }
  for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);   // (uniform: every lane takes part)
  const float m = s / (float)(8 * c8);
  float* hrow = heat + (long)b * positions;
  if (ok && j == 0) {
    __hip_atomic_store((gu32*)(hrow + p), __float_as_uint(m), RLX_AGENT);
    if (mean) mean[(long)b * positions + p] = m;
  }
  if (chunks > 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its sc1 stores
    __syncthreads();
    if (tid == 0) {
      gu32* c = (gu32*)(cnt + (long)b * VQA_CAM_COUNTER_STRIDE);
      const int last = __hip_atomic_fetch_add(c, 1u, RLX_AGENT) == (unsigned)(chunks - 1);
      if (last) __hip_atomic_store(c, 0u, RLX_AGENT);
      flag = last;
    }
    __syncthreads();
    if (!flag) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the sc1 loads below
  } else {
    __syncthreads();                                      // the one workgroup of the image wrote every mean
  }
  // the image's last workgroup: min / max over its P means, then the normalised map
  float v[CAM_MAX_P / CAM_THREADS];
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < CAM_MAX_P / CAM_THREADS; ++u) {
    const int q = tid + u * CAM_THREADS;
    v[u] = 0.f;
    if (q < positions) {
      v[u] = __uint_as_float(__hip_atomic_load((gu32*)(hrow + q), RLX_AGENT));
      mn = fminf(mn, v[u]);
      mx = fmaxf(mx, v[u]);
    }
  }
  mx = wave_max(mx);
  mn = -wave_max(-mn);
  if (l == 0) { red[w] = mn; red[CAM_WAVES + w] = mx; }
  __syncthreads();
  mn = red[0]; mx = red[CAM_WAVES];
#pragma unroll
  for (int i = 1; i < CAM_WAVES; ++i) { mn = fminf(mn, red[i]); mx = fmaxf(mx, red[CAM_WAVES + i]); }
  const float range = mx - mn;
#pragma unroll
  for (int u = 0; u < CAM_MAX_P / CAM_THREADS; ++u) {
    const int q = tid + u * CAM_THREADS;
    if (q < positions) hrow[q] = (v[u] - mn) / range;
  }
}

// one thread per 16 bytes of dst
__global__ __launch_bounds__(256) void upsample2x(const uint4* __restrict__ src, uint4* __restrict__ dst, int h, int w,
                                                  int c8, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % c8);
  long r = i / c8;
  const int ox = (int)(r % (2 * w));
  r /= 2 * w;
  const int oy = (int)(r % (2 * h));
  const long b = r / (2 * h);
  dst[i] = src[((b * h + (oy >> 1)) * w + (ox >> 1)) * c8 + c];
}

}  // namespace

extern "C" int vqa_channel_cam(const void* x, int batch, int positions, int channels, float* mean, float* heat,
                               unsigned* counter, hipStream_t s) {
  VQA_REQUIRE(x && heat && counter, "vqa_channel_cam: null x / heat / counter");
  VQA_REQUIRE(batch >= 1 && channels >= 8 && channels % 8 == 0,
              "vqa_channel_cam: batch >= 1, channels a positive multiple of 8 (16-byte loads along C), got %d, %d",
              batch, channels);
  VQA_REQUIRE(positions >= 1 && positions <= CAM_MAX_P, "vqa_channel_cam: positions must be 1..%d, got %d", CAM_MAX_P,
              positions);
  VQA_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)heat & 3) == 0, "vqa_channel_cam: x must be 16-byte aligned");
  const int c8 = channels / 8;
  int G = 1;
  while (2 * G <= c8 && 2 * G <= 64) G *= 2;
  const int pw = CAM_WAVES * (64 / G);
  const int chunks = (positions + pw - 1) / pw;
  const long grid = (long)batch * chunks;
  VQA_REQUIRE(grid < (1l << 31), "vqa_channel_cam: grid too large");
  hipLaunchKernelGGL(channel_cam, dim3((unsigned)grid), dim3(CAM_THREADS), 0, s, (const bf16_t*)x, positions, c8, G,
                     chunks, mean, heat, counter);
  return vqa::check_launch("vqa_channel_cam");
}

extern "C" int vqa_upsample2x_nhwc(const void* src, void* dst, int batch, int h, int w, int channels, hipStream_t s) {
  VQA_REQUIRE(src && dst && src != dst, "vqa_upsample2x_nhwc: null or aliased src / dst");
  VQA_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && channels >= 8 && channels % 8 == 0,
              "vqa_upsample2x_nhwc: batch, h, w >= 1, channels a positive multiple of 8");
  VQA_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "vqa_upsample2x_nhwc: src / dst must be 16-byte aligned");
  const long total = (long)batch * (2 * h) * (2 * w) * (channels / 8);
  const long grid = (total + 255) / 256;
  VQA_REQUIRE(grid < (1l << 31), "vqa_upsample2x_nhwc: grid too large");
  hipLaunchKernelGGL(upsample2x, dim3((unsigned)grid), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, h, w,
                     channels / 8, total);
  return vqa::check_launch("vqa_upsample2x_nhwc");
}
