// GPU side of the ViT collate (dataset_utils/vit_vqa_daquar_dataset.py:133-138): the
// reference feeds cv2.imread + cvtColor(BGR2RGB) arrays to ViTImageProcessor, which does,
// per image,
//   PIL resize(224 x 224, BILINEAR) -> rescale 1/255 -> normalise (mean 0.5, std 0.5)
// on the host.  Here the host decodes and packs the uint8 RGB images (as for
// vqa_resize_linear_u8, image.hip) and one call resamples the whole batch.
//
// Numerics are Pillow's ImagingResample for 8-bit images with the triangle filter
// (src/libImaging/Resample.c): an antialiased resample whose support grows with the
// down-scale (640 -> 224 takes up to 7 taps), run as two 8-bit passes with 22-bit
// fixed-point coefficients, horizontal first:
//   mid[y][ox][c] = clip8((2^21 + sum_t src[y][xmin(ox) + t][c] * kx[ox][t]) >> 22)
//   dst[oy][ox][c] = clip8((2^21 + sum_t mid[ymin(oy) + t][ox][c] * ky[oy][t]) >> 22)
//   out[c][oy][ox] = lut[c][dst[oy][ox][c]]              (rescale + normalise, 3 x 256 fp32)
// The per-axis tables {xmin, taps}[out] and k[out][ksize] are made on the host in fp64
// (data.pil_bilinear_coeffs): hipcc contracts fp64 multiply-adds in device code, and one
// different last bit of `center` moves an (int) truncation.  A pass with in == out has
// the coefficients {2^22, 0} and copies its input, so both passes always run.
//
// Two kernels, one thread per pixel of their output (3 channels): the horizontal pass
// gathers from the packed source (a block's taps span a few KB of one or two rows, L1 / L2
// resident) and writes the uint8 intermediate, which for a 64-frame batch stays in the
// last-level cache; the vertical pass reads it with lanes on consecutive pixels and writes
// the fp32 planes coalesced.  Sums fit 32 bits: 255 * (2^22 + ksize) + 2^21 < 2^31.
#include "common.h"

namespace {

constexpr int PIL_BITS = 22;                      // Resample.c PRECISION_BITS = 32 - 8 - 2
constexpr int PIL_MAX_SIDE = 8192;

__device__ __forceinline__ int clip8(int v) { return min(max(v >> PIL_BITS, 0), 255); }

// table of one (in, out) pair at `tab`: bounds[out][2] = {first source index, taps}, then
// k[out][ksize].  The bounds are clamped to the source and to ksize, so that a wrong table
// gives wrong pixels and never a read outside the image.
struct Taps {
  int first, n;
  const int* k;
};
__device__ __forceinline__ Taps taps_of(const int* __restrict__ tab, int o, int out, int ksize, int in) {
  Taps t;
  t.first = max(min(tab[2 * o], in - 1), 0);
  t.n = min(min(tab[2 * o + 1], ksize), in - t.first);
  t.k = tab + 2 * out + (long)o * ksize;
  return t;
}

// src (packed, desc[b]) -> mid[b][y][ox][3] for the image's h rows
__global__ __launch_bounds__(256) void pil_horizontal_kernel(const unsigned char* __restrict__ src,
                                                             const vqa_pil_image_desc* __restrict__ desc,
                                                             const int* __restrict__ tables,
                                                             unsigned char* __restrict__ mid, long mid_stride,
                                                             int max_h, int ow) {
  const int b = blockIdx.y;
  const vqa_pil_image_desc d = desc[b];
  const int h = min(d.h, max_h);                   // the workspace holds max_h rows per image
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int y = p / ow, ox = p - y * ow;
  if (y >= h) return;
  const Taps t = taps_of(tables + d.xtab, ox, ow, d.xk, d.w);
  const unsigned char* s = src + d.offset + ((long)y * d.w + t.first) * 3;
  int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
  for (int i = 0; i < t.n; ++i) {
    const int k = t.k[i];
    a0 += (int)s[3 * i] * k;
    a1 += (int)s[3 * i + 1] * k;
    a2 += (int)s[3 * i + 2] * k;
  }
  unsigned char* m = mid + (long)b * mid_stride + (long)p * 3;
  m[0] = (unsigned char)clip8(a0);
  m[1] = (unsigned char)clip8(a1);
  m[2] = (unsigned char)clip8(a2);
}

// mid[b][y][ox][3] -> out[b][c][oy][ox] = lut[c][.]
__global__ __launch_bounds__(256) void pil_vertical_lut_kernel(const unsigned char* __restrict__ mid, long mid_stride,
                                                               const vqa_pil_image_desc* __restrict__ desc,
                                                               const int* __restrict__ tables,
                                                               const float* __restrict__ lut, float* __restrict__ out,
                                                               int max_h, int oh, int ow) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= oh * ow) return;
  const vqa_pil_image_desc d = desc[b];
  const int h = min(d.h, max_h);
  const int oy = p / ow, ox = p - oy * ow;
  const Taps t = taps_of(tables + d.ytab, oy, oh, d.yk, h);
  const long row = (long)ow * 3;
  const unsigned char* m = mid + (long)b * mid_stride + (long)t.first * row + ox * 3;
  int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
  for (int i = 0; i < t.n; ++i) {
    const int k = t.k[i];
    a0 += (int)m[i * row] * k;
    a1 += (int)m[i * row + 1] * k;
    a2 += (int)m[i * row + 2] * k;
  }
  const long plane = (long)oh * ow;
  float* o = out + (long)b * 3 * plane + p;
  o[0] = lut[clip8(a0)];
  o[plane] = lut[256 + clip8(a1)];
  o[2 * plane] = lut[512 + clip8(a2)];
}

}  // namespace

extern "C" int vqa_resize_pil_bilinear_u8(const void* src, const vqa_pil_image_desc* desc, int batch, int max_h,
                                          int max_w, int oh, int ow, const int* tables, const float* lut, void* work,
                                          long long work_stride, float* out, hipStream_t s) {
  VQA_REQUIRE(src && desc && out && batch > 0 && batch <= 65535 && oh > 0 && ow > 0 && (long)oh * ow < (1l << 30),
              "vqa_resize_pil_bilinear_u8: bad arguments");
  VQA_REQUIRE(max_h >= 1 && max_w >= 1 && max_h <= PIL_MAX_SIDE && max_w <= PIL_MAX_SIDE,
              "vqa_resize_pil_bilinear_u8: source sides %d x %d, supported 1..%d", max_h, max_w, PIL_MAX_SIDE);
  VQA_REQUIRE(tables && lut, "vqa_resize_pil_bilinear_u8: null coefficient tables or look-up table");
  VQA_REQUIRE(work, "vqa_resize_pil_bilinear_u8: null workspace");
  VQA_REQUIRE(work_stride >= (long long)max_h * ow * 3 && (long long)max_h * ow < (1ll << 31),
              "vqa_resize_pil_bilinear_u8: workspace stride %lld < max_h * ow * 3 = %lld", work_stride,
              (long long)max_h * ow * 3);
  hipLaunchKernelGGL(pil_horizontal_kernel, dim3(vqa::cdiv((long)max_h * ow, 256), batch), dim3(256), 0, s,
                     (const unsigned char*)src, desc, tables, (unsigned char*)work, (long)work_stride, max_h, ow);
  hipLaunchKernelGGL(pil_vertical_lut_kernel, dim3(vqa::cdiv((long)oh * ow, 256), batch), dim3(256), 0, s,
                     (const unsigned char*)work, (long)work_stride, desc, tables, lut, out, max_h, oh, ow);
  return vqa::check_launch("vqa_resize_pil_bilinear_u8");
}
