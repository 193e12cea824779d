// Evaluation tail (include/vqa_hip.h "evaluation"): per-row top-k of the answer head's
// log-probs and the epoch's metrics, on the device -- the reference's valid_one_epoch takes
// argmax / topk of exp(log-probs) and averages the loss and WUPS on the host
// (trainer/faster_rcnn_vqa_trainer.py:408-480, CNN_vqa_heatmap.py:75-87).
//   eval_topk_kernel   one wave per row (4 rows per workgroup), lanes striding the answers as in
//                      head_lse_kernel: the row sits in registers, k rounds of a 64-lane
//                      (value, index) arg-max over the entries not taken yet
//   eval_accum_kernel  one workgroup: thread b stages row b's contribution in LDS, then one
//                      thread adds them in ascending row order (fp64, fixed order: a host loop
//                      doing the same adds reproduces the sums bit for bit) and appends the
//                      prediction / target log
// No atomics anywhere: the accumulator block is read and written by one thread of one launch.
#include "common.h"

namespace {

constexpr int MAXA = 1024, MAXB = 1024, MAXK = 16;
constexpr int NONE = 0x7fffffff;                       // index of "no candidate left" (k > answers)

// (value, index) order of the selection: larger value first, equal values by ascending index.
// -inf == -inf, so rows holding -inf entries still yield each index once; the NONE candidate
// (-inf, NONE) loses against every real entry.
__device__ __forceinline__ bool eval_before(float va, int ia, float vb, int ib) {
  return va > vb || (va == vb && ia < ib);
}

template <int NI>                                      // answers per lane: A <= 64 * NI
__global__ __launch_bounds__(256) void eval_topk_kernel(const float* __restrict__ lp, int* __restrict__ oidx,
                                                        float* __restrict__ oval, int B, int A, int K) {
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + wv;
  if (b >= B) return;                                  // wave-uniform: the shuffles below stay whole
  float v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = lp[(long)b * A + min(l + 64 * i, A - 1)];
  unsigned taken = 0;                                  // bit i: entry l + 64 i already selected
  int ri = -1;                                         // lane j keeps the j-th selection
  float rv = -INFINITY;
  for (int j = 0; j < K; ++j) {
    float bv = -INFINITY;
    int bi = NONE;
#pragma unroll
    for (int i = 0; i < NI; ++i) {                     // ascending index: strict > keeps the first
      const bool ok = l + 64 * i < A && !((taken >> i) & 1u);
      if (ok && (bi == NONE || v[i] > bv)) { bv = v[i]; bi = l + 64 * i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                 // butterfly: every lane ends with the winner
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (eval_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (bi != NONE && (bi & 63) == l) taken |= 1u << (bi >> 6);
    if (l == j) { ri = bi == NONE ? -1 : bi; rv = bv; }
  }
  if (l < K) {
    oidx[(long)b * K + l] = ri;
    oval[(long)b * K + l] = rv;
  }
}

struct EvalAcc {                                       // the 64-byte accumulator block
  long long steps, rows, top1, topk, cursor;
  double loss_sum, nll_sum, sim_sum;
};
static_assert(sizeof(EvalAcc) == 64, "accumulator block is eight 8-byte words");

__global__ __launch_bounds__(1024) void eval_accum_kernel(const int* __restrict__ tidx, const long long* __restrict__ tgt,
                                                          const float* __restrict__ nll, const float* __restrict__ loss,
                                                          const float* __restrict__ sim, int B, int A, int K,
                                                          EvalAcc* __restrict__ acc, int* __restrict__ pred_log,
                                                          int* __restrict__ tgt_log, long long capacity) {
  __shared__ int s_tgt[MAXB], s_pred[MAXB];            // s_tgt < 0: the row is ignored
  __shared__ float s_nll[MAXB], s_sim[MAXB];
  const int b = threadIdx.x;
  int hit1 = 0, hitk = 0;
  if (b < B) {
    const long long t64 = tgt[b];
    const bool valid = t64 >= 0 && t64 < (long long)A;
    const int t = valid ? (int)t64 : -1;
    const int pred = min(max(tidx[(long)b * K], 0), A - 1);      // column 0 is always a real answer
    for (int j = 0; j < K; ++j) hitk |= valid && tidx[(long)b * K + j] == t;
    hit1 = valid && pred == t;
    s_tgt[b] = t;
    s_pred[b] = pred;
    s_nll[b] = (valid && nll) ? nll[b] : 0.f;
    s_sim[b] = (valid && sim) ? sim[(long)pred * A + t] : 0.f;   // pred, t in [0, A): inside the table
  }
  const int n1 = __syncthreads_count(hit1), nk = __syncthreads_count(hitk);   // (also the LDS barrier)
  if (threadIdx.x != 0) return;
  EvalAcc a = *acc;
  long long rows = 0;
  for (int r = 0; r < B; ++r) {                        // ascending rows: the contract's fixed order
    if (s_tgt[r] < 0) continue;
    ++rows;
    a.nll_sum += (double)s_nll[r];
    a.sim_sum += (double)s_sim[r];
    if (a.cursor >= 0 && a.cursor < capacity) {        // (>= 0: a block nobody zeroed writes nowhere)
      pred_log[a.cursor] = s_pred[r];
      tgt_log[a.cursor] = s_tgt[r];
    }
    ++a.cursor;
  }
  if (rows == 0) return;                               // every row ignored: the block stays as it is
  a.steps += 1;
  if (loss) a.loss_sum += (double)loss[0];
  a.rows += rows;
  a.top1 += n1;
  a.topk += nk;
  *acc = a;
}

}  // namespace

extern "C" int vqa_eval_rows(const vqa_eval_desc* d, hipStream_t s) {
  VQA_REQUIRE(d, "vqa_eval_rows: null descriptor");
  VQA_REQUIRE(d->logp && d->topk_idx && d->topk_logp, "vqa_eval_rows: null logp / topk_idx / topk_logp");
  VQA_REQUIRE(d->batch >= 1 && d->batch <= MAXB && d->answers >= 1 && d->answers <= MAXA,
              "vqa_eval_rows: shape out of range (1<=batch<=1024, 1<=answers<=1024)");
  VQA_REQUIRE(d->k >= 1 && d->k <= MAXK, "vqa_eval_rows: k out of range (1<=k<=16)");
  VQA_REQUIRE(d->capacity >= 0 && (d->capacity == 0 || (d->acc && d->pred_log && d->tgt_log)),
              "vqa_eval_rows: a log capacity needs acc, pred_log and tgt_log");
  VQA_REQUIRE(((uintptr_t)d->acc & 7) == 0, "vqa_eval_rows: acc must be 8-byte aligned");
  const dim3 grid(vqa::cdiv(d->batch, 4));
  if (d->answers <= 256)
    hipLaunchKernelGGL(eval_topk_kernel<4>, grid, dim3(256), 0, s, d->logp, d->topk_idx, d->topk_logp, d->batch,
                       d->answers, d->k);
  else
    hipLaunchKernelGGL(eval_topk_kernel<16>, grid, dim3(256), 0, s, d->logp, d->topk_idx, d->topk_logp, d->batch,
                       d->answers, d->k);
  int rc = vqa::check_launch("vqa_eval_rows/topk");
  if (rc) return rc;
  if (!d->acc || !d->targets) return VQA_OK;           // no accumulators, or every row ignored
  hipLaunchKernelGGL(eval_accum_kernel, dim3(1), dim3(1024), 0, s, d->topk_idx, d->targets, d->nll, d->loss,
                     d->similarity, d->batch, d->answers, d->k, (EvalAcc*)d->acc, d->pred_log, d->tgt_log,
                     d->capacity);
  return vqa::check_launch("vqa_eval_rows/accumulate");
}
