// Gradient accumulation: k micro-batches of one global batch per optimizer step.
//   vqa_grad_accumulate  acc = g (micro-batch 0) or acc += g, one fp32 add per element: the
//                        step's gradient arena streamed into the accumulator the optimizer reads
//   vqa_accum_advance    the micro-batch's log-probs into their rows of the global batch's, its
//                        loss share into the fp64 sum, then the micro-batch counter + 1
//   vqa_accum_finish     loss = sum / k, counter = 0 (the end of the optimizer step)
// The counter lives on the device, so ONE captured micro-batch graph serves every position of
// the step.  Each launch reads the counter a previous launch left: the accumulate never writes
// it, and the two launches that do are a single workgroup / a single thread.
#include "common.h"

namespace {

// Grid-stride over float4s, four loads of each stream issued before their adds and stores.
// Both streams are touched once per micro-batch and are far larger than the Infinity Cache:
// non-temporal, as the AdamW pass that reads `acc` next.
template <bool FIRST>
__device__ __forceinline__ void accumulate_range(f32x4_t* __restrict__ a4, const f32x4_t* __restrict__ g4, long n4) {
  const long st = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * st < n4; i += 4 * st) {
    f32x4_t g[4], a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) g[u] = __builtin_nontemporal_load(g4 + i + u * st);
    if (!FIRST) {
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = __builtin_nontemporal_load(a4 + i + u * st);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(FIRST ? g[u] : a[u] + g[u], a4 + i + u * st);
  }
  for (; i < n4; i += st) {
    const f32x4_t g = __builtin_nontemporal_load(g4 + i);
    if (FIRST) {
      __builtin_nontemporal_store(g, a4 + i);
    } else {
      const f32x4_t a = __builtin_nontemporal_load(a4 + i);
      __builtin_nontemporal_store(a + g, a4 + i);
    }
  }
}

__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                              long n4, const int* __restrict__ micro) {
  f32x4_t* a4 = reinterpret_cast<f32x4_t*>(acc);
  const f32x4_t* g4 = reinterpret_cast<const f32x4_t*>(g);
  if (micro[0] == 0) accumulate_range<true>(a4, g4, n4);       // a dense copy, zeros included
  else accumulate_range<false>(a4, g4, n4);
}

// One workgroup: every thread reads the counter before the barrier, thread 0 writes it after.
// A counter outside [0, k) (a step driven past its k micro-batches) writes nothing.
__global__ __launch_bounds__(256) void accum_advance_kernel(const float* __restrict__ logp, float* __restrict__ logp_all,
                                                            long n, int k, const float* __restrict__ loss,
                                                            double* __restrict__ acc_loss, int* __restrict__ micro) {
  const int m = micro[0];
  __syncthreads();
  if (m < 0 || m >= k) return;
  float* dst = logp_all + (long)m * n;
  for (long i = threadIdx.x; i < n; i += 256) dst[i] = logp[i];
  if (threadIdx.x == 0) {
    acc_loss[0] = (m == 0 ? 0.0 : acc_loss[0]) + (double)loss[0];
    micro[0] = m + 1;
  }
}

__global__ void accum_finish_kernel(float* __restrict__ loss, const double* __restrict__ acc_loss,
                                    int* __restrict__ micro, int k) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    loss[0] = (float)(acc_loss[0] / (double)k);
    micro[0] = 0;
  }
}

}  // namespace

extern "C" int vqa_grad_accumulate(float* acc, const float* g, long long n, const int* micro, hipStream_t s) {
  VQA_REQUIRE(acc && g && micro && n > 0 && n % 4 == 0 && (((uintptr_t)acc | (uintptr_t)g) & 15) == 0 &&
                  ((uintptr_t)micro & 3) == 0,
              "vqa_grad_accumulate: bad arguments (n > 0, n %% 4 == 0, acc and g 16-byte aligned)");
  const long n4 = (long)(n / 4);
  const long blocks = (n4 + 255) / 256;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, acc, g,
                     n4, micro);
  return vqa::check_launch("vqa_grad_accumulate");
}

extern "C" int vqa_accum_advance(const float* logp, float* logp_all, int batch, int answers, int k, const float* loss,
                                 double* acc_loss, int* micro, hipStream_t s) {
  VQA_REQUIRE(logp && logp_all && loss && acc_loss && micro && batch >= 1 && answers >= 1 && k >= 1 &&
                  ((uintptr_t)acc_loss & 7) == 0 && ((uintptr_t)micro & 3) == 0,
              "vqa_accum_advance: bad arguments (batch, answers, k >= 1; acc_loss 8-byte aligned)");
  hipLaunchKernelGGL(accum_advance_kernel, dim3(1), dim3(256), 0, s, logp, logp_all, (long)batch * answers, k, loss,
                     acc_loss, micro);
  return vqa::check_launch("vqa_accum_advance");
}

extern "C" int vqa_accum_finish(float* loss, const double* acc_loss, int* micro, int k, hipStream_t s) {
  VQA_REQUIRE(loss && acc_loss && micro && k >= 1 && ((uintptr_t)acc_loss & 7) == 0 && ((uintptr_t)micro & 3) == 0,
              "vqa_accum_finish: bad arguments (k >= 1; acc_loss 8-byte aligned)");
  hipLaunchKernelGGL(accum_finish_kernel, dim3(1), dim3(64), 0, s, loss, acc_loss, micro, k);
  return vqa::check_launch("vqa_accum_finish");
}
