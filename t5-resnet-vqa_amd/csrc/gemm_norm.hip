// GEMM + row norm in one launch (vqa_gemm_desc.norm): the NORM instantiations of the tile body
// (gemm_body.h), in a translation unit of their own so that the code objects of gemm.hip and
// gemm_fp8.hip -- every other kernel of the family -- stay exactly as they are.
//
// Forward Linear layout only (k-contiguous A and B, no implicit im2col, no split-K).  After
// the usual epilogue has stored the tile's fp32 c32 values, the workgroup counts itself on
// the counter of its (batch, row block); the last of the row block's column tiles reads the
// block's rows back and normalises them (norm_tail, gemm_common.h: the hand-off and why
// nothing can hang) with the row arithmetic the stand-alone kernels use (norm_rows.h), so
// the outputs are bit for bit those of vqa_gemm + vqa_layernorm_fwd / vqa_rmsnorm_fwd.
//
// Instantiated, in bf16 and in e4m3, for the NORM rows of VQA_GEMM_TILE_TABLE (include/vqa_hip.h):
// what vqa_gemm_select returns on auto for a norm descriptor (3, 4; e4m3: 4), and the configs
// the committed tuning table holds for the SAME GEMMs without a norm -- 21 for the T5 o and SGA
// m2 / fc2 projections at D = 768 and for every e4m3 one at D = 1024, 6 for the batched SGA
// merge, 5 for T5 wo -- plus 7.  The table has no entries for norm descriptors (their key
// carries the norm kind): an engine that autotunes with fuse_norm on times these six configs
// for each norm-carrying shape at start-up.
#include "gemm_body.h"

namespace {

template <int BM, int BN, int STAGES, int NWM, int NWN, int BKT = BK, bool F8 = false>
__global__ __launch_bounds__(64 * NWM * NWN) void gemm_norm_kernel(GemmParams P, NormParams Q) {
  __shared__ __attribute__((aligned(1024))) char smem[TileCfg<BM, BN, STAGES, BKT>::LDS];
  gemm_body<BM, BN, STAGES, NWM, NWN, true, true, false, false, false, BKT, F8, true>(P, blockIdx.x, smem, &Q);
}

template <int BM, int BN, int STAGES, int NWM, int NWN, int BKT = BK, bool F8 = false>
int launch_norm(GemmParams& P, NormParams& Q, int batch, hipStream_t s) {
  P.tiles_m = vqa::cdiv(P.m, BM);
  P.tiles_n = vqa::cdiv(P.n, BN);
  if ((long long)P.tiles_m * batch > NORM_MAX_BLOCKS)
    return vqa::fail(VQA_ERR_INVALID, "vqa_gemm(norm): needs <= %lld (batch, row block) pairs", NORM_MAX_BLOCKS);
  hipLaunchKernelGGL((gemm_norm_kernel<BM, BN, STAGES, NWM, NWN, BKT, F8>), dim3(P.tiles_m * P.tiles_n, 1, batch),
                     dim3(64 * NWM * NWN), 0, s, P, Q);
  return vqa::check_launch("vqa_gemm(norm)");
}

// the NORM rows of the tile table
template <bool F8>
int dispatch_norm(GemmParams& P, NormParams& Q, int batch, int config, hipStream_t s) {
  return with_tile(config, [&](auto c) {
    constexpr Tile T = TILES[decltype(c)::value];
    constexpr const char* why = tile_lacks(T, true, false, F8, true, false);
    if constexpr (why != nullptr)
      return vqa::fail(VQA_ERR_INVALID, "vqa_gemm(norm): tile config %d %s", T.id, why);
    else
      return launch_norm<T.bm, T.bn, T.stages, T.wm, T.wn, T.bkt, F8>(P, Q, batch, s);
  });
}

}  // namespace

// called by vqa_gemm for norm descriptors (gemm.hip has validated the descriptor, resolved the
// config and filled P and Q; the translation units share the layouts of gemm_common.h)
int vqa_gemm_norm_dispatch(void* pp, void* qq, int batch, int config, int fp8, hipStream_t s) {
  GemmParams& P = *static_cast<GemmParams*>(pp);
  NormParams& Q = *static_cast<NormParams*>(qq);
  return fp8 ? dispatch_norm<true>(P, Q, batch, config, s) : dispatch_norm<false>(P, Q, batch, config, s);
}
