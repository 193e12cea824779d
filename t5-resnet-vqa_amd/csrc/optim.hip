// Optimiser tail of train_one_step (faster_rcnn_vqa_trainer.py:399-404):
//   clip_grad_norm_(params, 1.0)  ->  AdamW(wd=0.1, amsgrad=True) over the
//   trainer's param groups (:231-267)  ->  get_linear_schedule_with_warmup
//   (:279-287, TF/optimization.py:101-107).
// Everything stays on the device so the whole step can be one hipGraph:
//   1. vqa_grad_sqnorm    grid-stride partial sums of g^2 (fp64 accumulators)
//   2. vqa_optim_finalize one thread: norm, clip coefficient, LR multiplier
//                         lambda(step), bias corrections; advances `step`
//   3. vqa_adamw_amsgrad  one fused HBM pass over p, g, m, v, vmax -> p, m, v,
//                         vmax and the bf16 shadow copy used by the GEMMs.
// The DP average (1/world) enters as grad_scale in steps 2 and 3.
#include "adamw.h"

namespace {

// One squared-norm range of `nblk` blocks, block `bid`: grid-stride partial sum of g^2 (fp64).
// Four grid-stride loads issued before their (in-order) accumulation: the sum is the
// same as the one-load loop's, bit for bit, with 4x the loads in flight per wave.
__device__ __forceinline__ double sq_term(const float4 v) {
  return (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
}

__device__ __forceinline__ double sq_range(const float* __restrict__ g, long n4, int bid, int nblk) {
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const long st = (long)nblk * 256;
  double s = 0.0;
  long i = (long)bid * 256 + threadIdx.x;
  for (; i + 3 * st < n4; i += 4 * st) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = g4[i + u * st];
#pragma unroll
    for (int u = 0; u < 4; ++u) s += sq_term(v[u]);
  }
  for (; i < n4; i += st) s += sq_term(g4[i]);
  return s;
}

// The same range where the float4s from lead4 on are rows of d4 float4s and a row whose mark is
// not `step` is known to hold exact zeros (vqa_grad_sqnorm_final's table range): such a float4 is
// not loaded.  Every element keeps its thread and its place in the thread's in-order sum, and
// s + (+0.0) == s for the s >= +0 (or inf / NaN) of a sum of squares, so the partial is
// bit-identical to sq_range's -- also where a slot past the range adds its zero.  Eight marks,
// then the eight loads they allow, per round trip.
__device__ __forceinline__ double sq_range_rows(const float* __restrict__ g, long n4, int bid, int nblk,
                                                const int* __restrict__ mark, int step, long lead4, unsigned d4) {
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const long st = (long)nblk * 256;
  double s = 0.0;
  for (long i = (long)bid * 256 + threadIdx.x; i < n4; i += 8 * st) {
    int mk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long j = i + u * st;
      mk[u] = j >= n4 ? step - 1 : (j < lead4 ? step : mark[(unsigned)(j - lead4) / d4]);
    }
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = mk[u] == step ? g4[i + u * st] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += sq_term(v[u]);
  }
  return s;
}

// the block's sum of its threads' partials (fixed order); valid in thread 0.  red: >= 4 doubles
__device__ __forceinline__ double sq_block_sum(double s, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, long n4, double* __restrict__ ws) {
  __shared__ double red[4];
  const double s = sq_block_sum(sq_range(g, n4, blockIdx.x, gridDim.x), red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// the LR multiplier lambda(step) and the bias corrections of the update at step counter `step`
// (get_linear_schedule_with_warmup, TF/optimization.py:101-107; torch AdamW's 1 - beta^t): one
// function for vqa_optim_finalize and the embedding rows' early update, so both round alike
__device__ __forceinline__ void schedule_at(double step, int warmup, int total, float beta1, float beta2,
                                            float& lam_f, float& bc1, float& bc2s) {
  double lam;
  if (step < warmup) lam = step / (double)(warmup > 1 ? warmup : 1);
  else lam = fmax(0.0, (double)(total - step) / (double)((total - warmup) > 1 ? (total - warmup) : 1));
  const double t = step + 1.0;
  lam_f = (float)lam;
  bc1 = (float)(1.0 - pow((double)beta1, t));
  bc2s = (float)sqrt(1.0 - pow((double)beta2, t));
}

typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;

// The finalize routine, by one workgroup of 256 threads: fixed-order two-level sum of the
// partials, then the norm, clip coefficient, schedule and bias corrections.  SC1 (the last
// arriver of vqa_grad_sqnorm_final): the partials are read by sc1 loads, past this CU's L1.
template <bool SC1>
__device__ __forceinline__ void finalize_body(const double* __restrict__ ws, int parts, float grad_scale,
                                              float max_norm, int warmup, int total, float beta1, float beta2,
                                              float* __restrict__ st, double* red) {
  // the thread's partials i = tid, tid + 256, ... summed in that order; sixteen loads are issued
  // before their adds, so the 3 x 1024 partials' twelve loads per thread are one round trip
  double part = 0.0;
  for (int i0 = threadIdx.x; i0 < parts; i0 += 16 * 256) {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = i0 + u * 256;
      v[u] = 0.0;
      if (i < parts) {
        if (SC1)
          v[u] = __longlong_as_double((long long)__hip_atomic_load((gu64*)(ws + i), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT));
        else
          v[u] = ws[i];
      }
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (i0 + u * 256 < parts) part += v[u];
  }
  red[threadIdx.x] = part;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double ss = 0.0;
  for (int i = 0; i < 256; ++i) ss += red[i];
  const float norm = (float)(sqrt(ss) * (double)grad_scale);
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(1.f, max_norm / (norm + 1e-6f));
  const double step = (double)st[VQA_ST_STEP];
  float lam, bc1, bc2s;
  schedule_at(step, warmup, total, beta1, beta2, lam, bc1, bc2s);
  st[VQA_ST_GRAD_NORM] = norm;
  st[VQA_ST_CLIP_COEF] = coef;
  st[VQA_ST_LR_SCALE] = lam;
  st[VQA_ST_BC1] = bc1;
  st[VQA_ST_BC2_SQRT] = bc2s;
  st[VQA_ST_STEP] = (float)(step + 1.0);
  st[VQA_ST_PENDING] = 1.f;
}

__global__ __launch_bounds__(256) void finalize_kernel(const double* __restrict__ ws, int parts, float grad_scale,
                                                       float max_norm, int warmup, int total, float beta1,
                                                       float beta2, float* __restrict__ st) {
  __shared__ double red[256];
  finalize_body<false>(ws, parts, grad_scale, max_norm, warmup, total, beta1, beta2, st, red);
}

// The step's last squared-norm work and the finalize in ONE launch (vqa_grad_sqnorm_final).
// Blocks [0, K) sum range 0 into ws[fin - 2K, fin - K), blocks [K, 2K) range 1 into ws[fin - K, fin),
// each with the partition a K-block vqa_grad_sqnorm has.  Hand-off in the split-K form of
// gemm_body.h: the partial is stored write-through (sc1), the storing wave drains, the block
// barriers and counts its arrival with relaxed agent-scope adds; the block that arrives last
// resets the counter and runs the finalize routine over all `fin` partials with sc1 loads (those
// of earlier launches are ordered by the stream).  Nobody waits on anybody.
constexpr int SQ_NSUB = 32, SQ_CNT_STRIDE = 64;          // sub-counters, words between counters
static_assert((1 + SQ_NSUB) * SQ_CNT_STRIDE == VQA_SQNORM_FINAL_COUNTER_WORDS, "counter block");
struct SqFinalArgs {
  const float* g0; long n4_0;
  const float* g1; long n4_1;
  double* ws; int parts, fin;
  const int* mark; long lead4; unsigned d4;
  unsigned* cnt;
  float grad_scale, max_norm; int warmup, total; float beta1, beta2;
  float* st;
};

__global__ __launch_bounds__(256) void sqnorm_final_kernel(SqFinalArgs A) {
  __shared__ double red[256];                            // block sum, then the flag, then finalize
  const int K = A.parts;
  const int b = blockIdx.x;
  double s;
  if (b < K) s = sq_range(A.g0, A.n4_0, b, K);
  else if (A.mark) s = sq_range_rows(A.g1, A.n4_1, b - K, K, A.mark, (int)A.st[VQA_ST_STEP], A.lead4, A.d4);
  else s = sq_range(A.g1, A.n4_1, b - K, K);
  s = sq_block_sum(s, red);
  int* flag = reinterpret_cast<int*>(red + 8);
  if (threadIdx.x == 0) {
    __hip_atomic_store((gu64*)(A.ws + (A.fin - 2 * K) + b), (unsigned long long)__double_as_longlong(s),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the storing wave drains its sc1 store
    // Two-level arrival count: one word takes ~88 returning adds per us, and 2 x 1024 arrivals on a
    // single counter made the launch as long as the three it replaces (48 us; 33 us this way).
    // Block b counts on sub-counter b % SQ_NSUB (a 256-byte line each); the last of a sub-counter's
    // members counts on the top word, the last there finalizes.  Each last arriver resets its word.
    const int nb = 2 * K, grp = b % SQ_NSUB;
    const unsigned members = (unsigned)((nb - grp + SQ_NSUB - 1) / SQ_NSUB);
    const unsigned groups = (unsigned)(nb < SQ_NSUB ? nb : SQ_NSUB);
    gu32* sub = (gu32*)(A.cnt + (1 + grp) * SQ_CNT_STRIDE);
    int last = 0;
    if (__hip_atomic_fetch_add(sub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1) {
      __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = __hip_atomic_fetch_add((gu32*)A.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
      if (last) __hip_atomic_store((gu32*)A.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    *flag = last;
  }
  __syncthreads();
  if (!*flag) return;
  __syncthreads();                                        // every thread has read the flag: red is free
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below
  finalize_body<true>(A.ws, A.fin, A.grad_scale, A.max_norm, A.warmup, A.total, A.beta1, A.beta2, A.st, red);
}

// The embedding table's update split by rows.  mark[id] = the step counter for every id of the
// step's tokens (embed_mark_kernel, before the step's finalize).  A row no token touched has an
// exactly zero gradient, so its AdamW update needs neither the gradient nor the clip coefficient
// (g * gscale * coef = +0 for any finite coef) -- only the schedule of the coming finalize: MODE 0
// applies it to those rows, beside the backward, before finalize.  MODE 1 (after finalize, which
// advanced the counter) applies the full update to the marked rows.  Every row gets the same
// arithmetic as the dense pass (adamw_update4_with), so the table ends bit-identical to it; a row
// marked but not touched (a warm-up's ids) gets g = 0 in MODE 1, the same result as in MODE 0.
__global__ __launch_bounds__(256) void embed_mark_kernel(const long long* __restrict__ ids, int n, int rows,
                                                         int* __restrict__ mark, const float* __restrict__ st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long id = ids[i];
  if (id >= 0 && id < rows) mark[id] = (int)st[VQA_ST_STEP];
}

// one block per row, or (rows_per_block > 1) a grid of rows / rows_per_block blocks striding over
// the rows: the untouched rows' pass runs beside the latency-bound backward chain, where a
// 32k-block grid would hold CU slots the chain's launches wait for
template <int MODE>
__global__ __launch_bounds__(192) void adamw_rows_kernel(AdamArgs A, const int* __restrict__ mark, int rows, int d4,
                                                         int warmup, int total) {
  const int step = (int)A.st[VQA_ST_STEP];
  float coef, lam, bc1, bc2s;
  if (MODE == 0) {
    coef = 1.f;
    schedule_at((double)A.st[VQA_ST_STEP], warmup, total, A.b1, A.b2, lam, bc1, bc2s);
  } else {
    if (A.st[VQA_ST_PENDING] == 0.f) return;
    coef = A.st[VQA_ST_CLIP_COEF];
    lam = A.st[VQA_ST_LR_SCALE];
    bc1 = A.st[VQA_ST_BC1];
    bc2s = A.st[VQA_ST_BC2_SQRT];
  }
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
  const bool touched = mark[row] == (MODE == 0 ? step : step - 1);
  if (MODE == 0 ? touched : !touched) continue;
  for (int c = threadIdx.x; c < d4; c += 192) {
    const long i = (long)row * d4 + c;
    f32x4_t p = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.p) + i);
    f32x4_t g4 = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 1) g4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.g) + i);
    f32x4_t m = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.m) + i);
    f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.v) + i);
    f32x4_t vm = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.vm) + i);
    adamw_update4_with(A, i, p, g4, m, v, vm, coef, lam, bc1, bc2s);
    __builtin_nontemporal_store(p, reinterpret_cast<f32x4_t*>(A.p) + i);
    __builtin_nontemporal_store(m, reinterpret_cast<f32x4_t*>(A.m) + i);
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4_t*>(A.v) + i);
    __builtin_nontemporal_store(vm, reinterpret_cast<f32x4_t*>(A.vm) + i);
    if (A.p16) {
      uint2 u;
      u.x = (uint32_t)f2bf(p[0]) | ((uint32_t)f2bf(p[1]) << 16);
      u.y = (uint32_t)f2bf(p[2]) | ((uint32_t)f2bf(p[3]) << 16);
      reinterpret_cast<uint2*>(A.p16)[i] = u;
    }
  }
  }
}

// One float4 of every stream per thread, no grid-stride loop: 138k blocks of
// 256 keep ~2k threads x 5 x 16 B of loads in flight per CU.  Every stream is
// touched once per step (5.4 GB >> the 256 MiB Infinity Cache), so loads and
// stores are non-temporal.
__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n4 || A.st[VQA_ST_PENDING] == 0.f) return;   // nothing to apply (see VQA_ST_PENDING)
  f32x4_t p = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.p) + i);
  const f32x4_t g4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.g) + i);
  f32x4_t m = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.m) + i);
  f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.v) + i);
  f32x4_t vm = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(A.vm) + i);
  adamw_update4(A, i, p, g4, m, v, vm);
  __builtin_nontemporal_store(p, reinterpret_cast<f32x4_t*>(A.p) + i);
  __builtin_nontemporal_store(m, reinterpret_cast<f32x4_t*>(A.m) + i);
  __builtin_nontemporal_store(v, reinterpret_cast<f32x4_t*>(A.v) + i);
  __builtin_nontemporal_store(vm, reinterpret_cast<f32x4_t*>(A.vm) + i);
  if (A.p16) {
    uint2 u;
    u.x = (uint32_t)f2bf(p[0]) | ((uint32_t)f2bf(p[1]) << 16);
    u.y = (uint32_t)f2bf(p[2]) | ((uint32_t)f2bf(p[3]) << 16);
    reinterpret_cast<uint2*>(A.p16)[i] = u;            // the next forward reads it: keep it cacheable
  }
}

int grid_for(long n4) {
  long b = (n4 + 255) / 256;
  return (int)(b < 4096 ? b : 4096);
}

}  // namespace

extern "C" int vqa_grad_sqnorm(const float* g, long long n, double* ws, int parts, hipStream_t s) {
  VQA_REQUIRE(g && ws && n % 4 == 0 && parts > 0 && ((uintptr_t)g & 15) == 0,
              "vqa_grad_sqnorm: bad arguments (n %% 4 == 0, g 16-byte aligned)");
  hipLaunchKernelGGL(sqnorm_kernel, dim3(parts), dim3(256), 0, s, g, (long)(n / 4), ws);
  return vqa::check_launch("vqa_grad_sqnorm");
}

extern "C" int vqa_optim_finalize(const double* ws, int parts, float grad_scale, float max_norm, int warmup, int total,
                                  float beta1, float beta2, float* state, hipStream_t s) {
  VQA_REQUIRE(ws && state && parts > 0, "vqa_optim_finalize: bad arguments");
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, ws, parts, grad_scale, max_norm, warmup, total, beta1,
                     beta2, state);
  return vqa::check_launch("vqa_optim_finalize");
}

extern "C" int vqa_grad_sqnorm_final(const float* g0, long long n0, const float* g1, long long n1, double* ws,
                                     int parts, int fin_parts, const int* mark, long long lead, int cols,
                                     unsigned* counter, float grad_scale, float max_norm, int warmup, int total,
                                     float beta1, float beta2, float* state, hipStream_t s) {
  VQA_REQUIRE(g0 && g1 && ws && counter && state && parts > 0 && fin_parts >= 2 * parts && n0 >= 0 && n1 >= 0 &&
                  n0 % 4 == 0 && n1 % 4 == 0 && ((uintptr_t)g0 & 15) == 0 && ((uintptr_t)g1 & 15) == 0,
              "vqa_grad_sqnorm_final: bad arguments (n %% 4 == 0, 16-byte aligned ranges, fin_parts >= 2 parts)");
  VQA_REQUIRE(!mark || (cols > 0 && cols % 4 == 0 && lead >= 0 && lead % 4 == 0 && lead <= n1 &&
                        (n1 - lead) % cols == 0 && n1 / 4 < (1ll << 31)),
              "vqa_grad_sqnorm_final: range 1 must be `lead` floats then whole rows of `cols` (both %% 4 == 0)");
  SqFinalArgs A;
  A.g0 = g0; A.n4_0 = (long)(n0 / 4); A.g1 = g1; A.n4_1 = (long)(n1 / 4);
  A.ws = ws; A.parts = parts; A.fin = fin_parts;
  A.mark = mark; A.lead4 = (long)(lead / 4); A.d4 = mark ? (unsigned)(cols / 4) : 1u;
  A.cnt = counter;
  A.grad_scale = grad_scale; A.max_norm = max_norm; A.warmup = warmup; A.total = total;
  A.beta1 = beta1; A.beta2 = beta2; A.st = state;
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(2 * parts), dim3(256), 0, s, A);
  return vqa::check_launch("vqa_grad_sqnorm_final");
}

extern "C" int vqa_adamw_amsgrad(const vqa_adamw_desc* d, hipStream_t s) {
  AdamArgs A;
  if (int rc = adam_args(d, A)) return rc;
  hipLaunchKernelGGL(adamw_kernel, dim3(vqa::cdiv(A.n4, 256)), dim3(256), 0, s, A);
  return vqa::check_launch("vqa_adamw_amsgrad");
}

extern "C" int vqa_embed_mark(const long long* ids, int n, int rows, int* mark, const float* state, hipStream_t s) {
  VQA_REQUIRE(ids && mark && state && n > 0 && rows > 0, "vqa_embed_mark: bad arguments");
  hipLaunchKernelGGL(embed_mark_kernel, dim3(vqa::cdiv(n, 256)), dim3(256), 0, s, ids, n, rows, mark, state);
  return vqa::check_launch("vqa_embed_mark");
}

extern "C" int vqa_adamw_rows(const vqa_adamw_desc* d, const int* mark, int rows, int cols, int touched, int warmup,
                              int total, hipStream_t s) {
  AdamArgs A;
  if (int rc = adam_args(d, A)) return rc;
  VQA_REQUIRE(mark && rows > 0 && cols > 0 && cols % 4 == 0 && (long long)rows * cols == d->n,
              "vqa_adamw_rows: rows x cols must be the descriptor's n (cols %% 4 == 0)");
  // touched > 1 (the untouched-rows pass only): a grid of `touched` blocks striding over the rows
  const int grid = touched > 1 && touched < rows ? touched : rows;
  if (touched == 1)
    hipLaunchKernelGGL(adamw_rows_kernel<1>, dim3(rows), dim3(192), 0, s, A, mark, rows, cols / 4, warmup, total);
  else
    hipLaunchKernelGGL(adamw_rows_kernel<0>, dim3(grid), dim3(192), 0, s, A, mark, rows, cols / 4, warmup, total);
  return vqa::check_launch("vqa_adamw_rows");
}
