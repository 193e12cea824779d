// Attention rollout of the frozen ViT (BASELINE config 4), the heat map of the reference's
// ViT_vqa_heatmap.py:104-137: per image, each layer's attention map is averaged over its heads,
// the identity is added and every row divided by its sum (A_l); the maps are chained,
// J_0 = A_0, J_l = A_l J_{l-1}, and the heat map is row 0 (the CLS query) of the last J without
// its column 0.  Only that row is used, and J_last[0, :] = e_0^T A_last ... A_0, so the chain is
// `layers - 1` vector-matrix products, not matrix products.
//
//   vqa_attn_headmean   one layer's A_l [batch, n, n] from its q | k, never writing the
//                       per-head maps: one wave per (image, 32-query block) loops the heads
//   vqa_rollout_cls     the chain over the layers' A_l, one workgroup per image
//
// Both are free of atomics and sum in a fixed order: the output is the same bits every run.
#include "common.h"

namespace {

// ---- MFMA helpers (the layouts of attention_mfma.hip: v_mfma_f32_32x32x16_bf16, S^T tile in
// "X" layout -- lane = query l & 31, register r = key (r & 3) + 8 (r >> 2) + 4 (l >> 5) of a
// 32-key tile, so a register quad is 4 consecutive keys)
__device__ __forceinline__ uint32_t okmask(bool ok) { return ok ? 0xffffffffu : 0u; }

// `row` must point at a valid row (callers clamp the index); ok = 0 zeroes the fragment
__device__ __forceinline__ bf16x8_t ld_frag(const bf16_t* row, bool ok) {
  uint4 u = *reinterpret_cast<const uint4*>(row);
  const uint32_t m = okmask(ok);
  u.x &= m; u.y &= m; u.z &= m; u.w &= m;
  return __builtin_bit_cast(bf16x8_t, u);
}

__device__ __forceinline__ f32x16_t mfma(bf16x8_t a, bf16x8_t b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

struct HeadMeanP {
  const bf16_t *q, *k; long ldq, ldk;
  float* aug; long ld;
  int heads, n;
  float scale, inv_heads;
};

// NT = ceil(n / 32) key tiles, all of one head's scores in registers (NT x 16 per lane) next to
// the running sum over the heads (as many): the softmax is the exact two-step one (row max, then
// exp(s - max) / sum); nothing is multiplied by V, so there is nothing an online form would save.
template <int DH, int NT>
__global__ __launch_bounds__(64) void attn_headmean(HeadMeanP P) {
  constexpr int KS = DH / 16;
  const int l = threadIdx.x, h5 = l >> 5, l31 = l & 31;
  const int n = P.n;
  const int qblocks = (n + 31) >> 5;
  const int b = blockIdx.x / qblocks, qb = blockIdx.x - b * qblocks;
  const int nq = min(32, n - 32 * qb);
  const bool qok = l31 < nq;
  const bf16_t* Q = P.q + ((long)b * n + 32 * qb + min(l31, nq - 1)) * P.ldq + 8 * h5;
  const bf16_t* K = P.k + (long)b * n * P.ldk + 8 * h5;
  f32x16_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  for (int hh = 0; hh < P.heads; ++hh) {                  // fixed order 0 .. heads-1
    bf16x8_t qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = ld_frag(Q + hh * DH + 16 * s, qok);
    f32x16_t sa[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int nk = min(32, n - 32 * t);                 // >= 1: NT is exactly ceil(n / 32)
      const bf16_t* Kr = K + (long)(32 * t + min(l31, nk - 1)) * P.ldk + hh * DH;
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[t][r] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) sa[t] = mfma(ld_frag(Kr + 16 * s, l31 < nk), qf[s], sa[t]);
    }
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h5;
        const float v = key < n ? sa[t][r] * P.scale : -INFINITY;
        sa[t][r] = v;
        m = fmaxf(m, v);
      }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float z = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = sa[t][r] == -INFINITY ? 0.f : __expf(sa[t][r] - m);
        sa[t][r] = e;
        z += e;
      }
    z += __shfl_xor(z, 32, 64);
    const float iz = 1.f / z;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] += sa[t][r] * iz;
  }
  // mean over the heads, + I, row sum -- in registers, before the one store
  const int qi = 32 * qb + l31;
  float rs = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h5;
      float v = acc[t][r] * P.inv_heads + (key == qi ? 1.f : 0.f);
      v = key < n ? v : 0.f;
      acc[t][r] = v;
      rs += v;
    }
  rs += __shfl_xor(rs, 32, 64);
  if (!qok) return;                                       // query rows >= n are not stored
  float* row = P.aug + ((long)b * n + qi) * P.ld;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * t + 8 * g + 4 * h5;                // 4 consecutive keys: one 16-byte store
      if (c + 3 < n) {
        f32x4_t o = {acc[t][4 * g] / rs, acc[t][4 * g + 1] / rs, acc[t][4 * g + 2] / rs, acc[t][4 * g + 3] / rs};
        *reinterpret_cast<f32x4_t*>(row + c) = o;
      } else {                                            // the ragged quad: the pad columns stay untouched
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < n) row[c + e] = acc[t][4 * g + e] / rs;
      }
    }
}

template <int DH>
void launch_headmean(const HeadMeanP& P, int nt, unsigned grid, hipStream_t s) {
  switch (nt) {
    case 1: hipLaunchKernelGGL((attn_headmean<DH, 1>), dim3(grid), dim3(64), 0, s, P); break;
    case 2: hipLaunchKernelGGL((attn_headmean<DH, 2>), dim3(grid), dim3(64), 0, s, P); break;
    case 3: hipLaunchKernelGGL((attn_headmean<DH, 3>), dim3(grid), dim3(64), 0, s, P); break;
    case 4: hipLaunchKernelGGL((attn_headmean<DH, 4>), dim3(grid), dim3(64), 0, s, P); break;
    case 5: hipLaunchKernelGGL((attn_headmean<DH, 5>), dim3(grid), dim3(64), 0, s, P); break;
    case 6: hipLaunchKernelGGL((attn_headmean<DH, 6>), dim3(grid), dim3(64), 0, s, P); break;
    case 7: hipLaunchKernelGGL((attn_headmean<DH, 7>), dim3(grid), dim3(64), 0, s, P); break;
    default: hipLaunchKernelGGL((attn_headmean<DH, 8>), dim3(grid), dim3(64), 0, s, P); break;
  }
}

// ------------------------------------------------------------------ the chain
constexpr int RC_COLS = 256, RC_GROUPS = 4, RC_MAX_N = 1024;

// One workgroup per image: r (n floats in LDS) starts as row 0 of the last layer's map and is
// multiplied by each earlier layer's, r <- r A_l.  Thread (g, c) sums column j = j0 + c over
// the g-th quarter of the rows i in ascending order (two interleaved partial sums), so a wave
// reads 64 consecutive floats of one row; the four quarters are combined in a fixed order.
__global__ __launch_bounds__(RC_COLS * RC_GROUPS) void rollout_cls(const float* aug, int layers, int n, long ld,
                                                                   long layer_stride, float* mask, float* unit) {
  __shared__ float r[2][RC_MAX_N];
  __shared__ float part[RC_GROUPS][RC_COLS];
  __shared__ float red[RC_COLS * RC_GROUPS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, g = tid / RC_COLS, c = tid - g * RC_COLS;
  const float* A = aug + (long)b * n * ld;
  for (int j = tid; j < n; j += RC_COLS * RC_GROUPS) r[0][j] = A[(long)(layers - 1) * layer_stride + j];
  __syncthreads();
  const int chunk = (n + RC_GROUPS - 1) / RC_GROUPS;
  const int i0 = min(n, g * chunk), i1 = min(n, i0 + chunk);
  int cur = 0;
  for (int l = layers - 2; l >= 0; --l) {
    const float* Al = A + (long)l * layer_stride;
    const float* rc = r[cur];
    for (int j0 = 0; j0 < n; j0 += RC_COLS) {
      const int j = j0 + c;
      float s0 = 0.f, s1 = 0.f;
      if (j < n) {
        int i = i0;
        for (; i + 1 < i1; i += 2) {
          s0 += rc[i] * Al[(long)i * ld + j];
          s1 += rc[i + 1] * Al[(long)(i + 1) * ld + j];
        }
        if (i < i1) s0 += rc[i] * Al[(long)i * ld + j];
      }
      part[g][c] = s0 + s1;
      __syncthreads();
      if (g == 0 && j < n) r[cur ^ 1][j] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
      __syncthreads();
    }
    cur ^= 1;
  }
  const float* rf = r[cur];
  float* mrow = mask + (long)b * (n - 1);
  float mx = -INFINITY;
  for (int j = 1 + tid; j < n; j += RC_COLS * RC_GROUPS) {
    mrow[j - 1] = rf[j];
    mx = fmaxf(mx, rf[j]);
  }
  if (!unit) return;                                      // (uniform: no barrier is skipped by a part of the block)
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < RC_COLS * RC_GROUPS / 64; ++w) mx = fmaxf(mx, red[w]);
  float* urow = unit + (long)b * (n - 1);
  for (int j = 1 + tid; j < n; j += RC_COLS * RC_GROUPS) urow[j - 1] = rf[j] / mx;
}

}  // namespace

extern "C" int vqa_attn_headmean(const vqa_attn_desc* d, float* aug, long long ld_aug, hipStream_t s) {
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  VQA_REQUIRE(d && d->q && d->k && aug, "vqa_attn_headmean: null q / k / aug");
  VQA_REQUIRE(d->batch > 0 && d->heads > 0 && d->lq >= 1 && d->lq == d->lk && d->lq <= 256,
              "vqa_attn_headmean: self-attention maps only (lq == lk, 1..256 tokens)");
  VQA_REQUIRE(d->dh == 64 || d->dh == 96, "vqa_attn_headmean: dh must be 64 or 96");
  VQA_REQUIRE(!d->bias && !d->key_mask && d->groups <= 1, "vqa_attn_headmean: no bias, key mask or groups");
  // the long forward's operand rules (vqa_attn_long_ok): 16-byte rows of q and k
  VQA_REQUIRE(d->ldq % 8 == 0 && d->ldk % 8 == 0 && al16(d->q) && al16(d->k),
              "vqa_attn_headmean: q / k must be 16-byte aligned with row strides that are multiples of 8");
  VQA_REQUIRE(ld_aug % 4 == 0 && ld_aug >= d->lq && al16(aug),
              "vqa_attn_headmean: aug must be 16-byte aligned, ld_aug a multiple of 4 and >= n");
  HeadMeanP P;
  P.q = (const bf16_t*)d->q; P.k = (const bf16_t*)d->k; P.ldq = d->ldq; P.ldk = d->ldk;
  P.aug = aug; P.ld = ld_aug; P.heads = d->heads; P.n = d->lq;
  P.scale = d->scale; P.inv_heads = 1.f / (float)d->heads;
  const int nt = (d->lq + 31) / 32;
  const long grid = (long)d->batch * nt;
  VQA_REQUIRE(grid < (1l << 31), "vqa_attn_headmean: grid too large");
  if (d->dh == 64) launch_headmean<64>(P, nt, (unsigned)grid, s);
  else launch_headmean<96>(P, nt, (unsigned)grid, s);
  return vqa::check_launch("vqa_attn_headmean");
}

extern "C" int vqa_rollout_cls(const float* aug, int layers, int batch, int n, long long ld_aug,
                               long long layer_stride, float* mask, float* mask_unit, hipStream_t s) {
  VQA_REQUIRE(aug && mask, "vqa_rollout_cls: null aug / mask");
  VQA_REQUIRE(layers >= 1 && batch >= 1 && n >= 2 && n <= RC_MAX_N, "vqa_rollout_cls: layers, batch >= 1, n in 2..%d",
              RC_MAX_N);
  VQA_REQUIRE(ld_aug >= n, "vqa_rollout_cls: ld_aug < n");
  VQA_REQUIRE(layers == 1 || layer_stride >= (long long)batch * n * ld_aug,
              "vqa_rollout_cls: the layers' maps overlap (layer_stride < batch * n * ld_aug)");
  hipLaunchKernelGGL(rollout_cls, dim3(batch), dim3(RC_COLS * RC_GROUPS), 0, s, aug, layers, n, (long)ld_aug,
                     (long)layer_stride, mask, mask_unit);
  return vqa::check_launch("vqa_rollout_cls");
}
