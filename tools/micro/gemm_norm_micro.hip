// GEMM + row norm in one launch (vqa_gemm_desc.norm) against GEMM + the stand-alone norm
// launch, on the two shapes the step's forward norms hang on:
//   SGA merge  2048 x 768 x 768  + bias + fp32 residual + LayerNorm
//   T5 wo      2048 x 768 x 3072 + fp32 residual + RMSNorm
// Prints, per shape x tile config: microseconds per launch of the fused form and of the pair
// (20 back-to-back launches per event pair, median of 9 rounds, both forms interleaved in
// one process), whether the outputs agree bit for bit, and the fused launch's phase stamps
// (100 MHz wall clock, VQA_GEMM_STAMP hooks): span, k-loop, epilogue, the hand-off (epilogue
// end to the last arriver's first row load) and the last arriver's row-block time (read the
// BM x 768 fp32 block, normalise, write).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../include gemm_norm_micro.hip \
//     ../../t5-resnet-vqa_amd/csrc/api.hip -o gemm_norm_micro
#include <hip/hip_runtime.h>
__device__ unsigned long long g_st[16384 * 8];
#define VQA_GEMM_STAMP(i)                                                                       \
  do {                                                                                          \
    if (threadIdx.x == 0 && blockIdx.z == 0) g_st[blockIdx.x * 8 + (i)] = wall_clock64();      \
  } while (0)
#define VQA_GEMM_MICRO 1
#include "../../t5-resnet-vqa_amd/csrc/gemm.hip"
#include "../../t5-resnet-vqa_amd/csrc/gemm_norm.hip"
#include "../../t5-resnet-vqa_amd/csrc/norms.hip"
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

static unsigned lcg = 12345u;
static float frand() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) & 0xffff) / 32768.f - 1.f; }
static unsigned short f2b(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }

template <int BM, int BN, int S, int BKT = 64>
void run(const char* tag, int kind, int M, int N, int K, int cfg) {
  std::vector<unsigned short> ha((size_t)M * K), hb((size_t)N * K);
  std::vector<float> hr((size_t)M * N), hg(N), hbeta(N), hbias(N);
  for (auto& v : ha) v = f2b(frand());
  for (auto& v : hb) v = f2b(0.05f * frand());
  for (auto& v : hr) v = frand();
  for (int i = 0; i < N; ++i) { hg[i] = 1.f + 0.1f * frand(); hbeta[i] = 0.1f * frand(); hbias[i] = frand(); }
  bf16_t *a, *b, *y16[2];
  float *c32[2], *y32[2], *mu[2], *rs[2], *r32, *g, *beta, *bias;
  void* ws;
  CK(hipMalloc(&a, ha.size() * 2)); CK(hipMalloc(&b, hb.size() * 2)); CK(hipMalloc(&r32, hr.size() * 4));
  CK(hipMalloc(&g, N * 4)); CK(hipMalloc(&beta, N * 4)); CK(hipMalloc(&bias, N * 4)); CK(hipMalloc(&ws, 65536));
  CK(hipMemset(ws, 0, 65536));
  for (int i = 0; i < 2; ++i) {
    CK(hipMalloc(&c32[i], (size_t)M * N * 4)); CK(hipMalloc(&y32[i], (size_t)M * N * 4));
    CK(hipMalloc(&y16[i], (size_t)M * N * 2)); CK(hipMalloc(&mu[i], M * 4)); CK(hipMalloc(&rs[i], M * 4));
    CK(hipMemset(mu[i], 0, M * 4));
  }
  CK(hipMemcpy(a, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(b, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(r32, hr.data(), hr.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(g, hg.data(), N * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(beta, hbeta.data(), N * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(bias, hbias.data(), N * 4, hipMemcpyHostToDevice));
  const float eps = kind == 1 ? 1e-5f : 1e-6f;
  auto desc = [&](int i, bool norm) {
    vqa_gemm_desc d{};
    d.a = a; d.lda = K; d.b = b; d.ldb = K; d.m = M; d.n = N; d.k = K; d.alpha = 1.f; d.batch = 1;
    d.c32 = c32[i]; d.ldc32 = N; d.res32 = r32; d.ldres = N; d.config = cfg;
    if (kind == 1) d.bias = bias;
    if (norm) {
      d.norm = kind; d.norm_w = g; d.norm_b = kind == 1 ? beta : nullptr; d.norm_eps = eps;
      d.norm_y32 = y32[i]; d.norm_y16 = y16[i]; d.norm_mean = kind == 1 ? mu[i] : nullptr; d.norm_rstd = rs[i];
      d.workspace = ws; d.workspace_bytes = 65536;
    }
    return d;
  };
  const vqa_gemm_desc df = desc(0, true), du = desc(1, false);
  GemmParams Pf, Pu;
  NormParams Q;
  if (prepare(&df, Pf) || prepare_norm(&df, Pf, Q) || prepare(&du, Pu)) { printf("prepare failed: %s\n", vqa_last_error()); exit(1); }
  auto fused = [&]() { GemmParams P = Pf; launch_norm<BM, BN, S, 2, 2, BKT>(P, Q, 1, 0); };
  auto pair = [&]() {
    GemmParams P = Pu;
    launch<BM, BN, S, 2, 2, true, true, false, false, BKT>(P, 1, 0);
    if (kind == 1) vqa_layernorm_fwd(c32[1], g, beta, y32[1], y16[1], mu[1], rs[1], M, N, eps, 0);
    else vqa_rmsnorm_fwd(c32[1], g, y32[1], y16[1], rs[1], M, N, eps, nullptr, 0);
  };
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<float> tf, tp;
  for (int q = 0; q < 10; ++q)
    for (int which = 0; which < 2; ++which) {
      CK(hipEventRecord(e0, 0));
      for (int i = 0; i < 20; ++i) { if (which) pair(); else fused(); }
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (q) (which ? tp : tf).push_back(ms * 1e3f / 20);
    }
  std::sort(tf.begin(), tf.end()); std::sort(tp.begin(), tp.end());
  // bitwise agreement
  auto eq = [&](const void* p0, const void* p1, size_t n) {
    std::vector<char> h0(n), h1(n);
    CK(hipMemcpy(h0.data(), p0, n, hipMemcpyDeviceToHost)); CK(hipMemcpy(h1.data(), p1, n, hipMemcpyDeviceToHost));
    return memcmp(h0.data(), h1.data(), n) == 0;
  };
  CK(hipDeviceSynchronize());
  const bool same = eq(c32[0], c32[1], (size_t)M * N * 4) && eq(y32[0], y32[1], (size_t)M * N * 4) &&
                    eq(y16[0], y16[1], (size_t)M * N * 2) && eq(rs[0], rs[1], M * 4) && eq(mu[0], mu[1], M * 4);
  // one stamped fused launch
  const int nwg = vqa::cdiv(M, BM) * vqa::cdiv(N, BN);
  std::vector<unsigned long long> st((size_t)nwg * 8, 0);
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_st), st.data(), st.size() * 8));
  fused();
  CK(hipDeviceSynchronize());
  CK(hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_st), st.size() * 8));
  int rate_khz = 0;
  CK(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, 0));
  const double us = 1e3 / rate_khz;
  unsigned long long t0 = ~0ull, tend = 0, t4max = 0;
  std::vector<double> kl, ep, ho, rb, cnt;
  for (int w = 0; w < nwg; ++w) {
    const unsigned long long* s = &st[(size_t)w * 8];
    t0 = std::min(t0, s[0]); tend = std::max(tend, s[5]); t4max = std::max(t4max, s[4]);
    kl.push_back((s[3] - s[2]) * us); ep.push_back((s[4] - s[3]) * us);
    if (s[6]) { ho.push_back((s[6] - s[4]) * us); rb.push_back((s[5] - s[6]) * us); }
    else cnt.push_back((s[5] - s[4]) * us);
  }
  auto med = [](std::vector<double>& v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
  auto mx = [](std::vector<double>& v) { return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()); };
  printf("%-5s %s %4dx%4dx%4d cfg %2d (%3dx%3d s%d bk%3d) wg %4d | fused %6.2f us (min %6.2f)  gemm+norm %6.2f us (min %6.2f)  %s | "
         "span %6.2f  k-loop %5.2f  epilogue %5.2f  count (not last) %4.2f | last arrivers %zu: hand-off %4.2f (max %4.2f)  "
         "row block %5.2f (max %5.2f)  after the last epilogue %5.2f\n",
         tag, kind == 1 ? "LN " : "RMS", M, N, K, cfg, BM, BN, S, BKT, nwg, tf[tf.size() / 2], tf[0], tp[tp.size() / 2], tp[0],
         same ? "bitwise==" : "MISMATCH", (tend - t0) * us, med(kl), med(ep), med(cnt), rb.size(), med(ho), mx(ho), med(rb), mx(rb),
         (tend - t4max) * us);
  fflush(stdout);
  CK(hipFree(a)); CK(hipFree(b)); CK(hipFree(r32)); CK(hipFree(g)); CK(hipFree(beta)); CK(hipFree(bias)); CK(hipFree(ws));
  for (int i = 0; i < 2; ++i) { CK(hipFree(c32[i])); CK(hipFree(y32[i])); CK(hipFree(y16[i])); CK(hipFree(mu[i])); CK(hipFree(rs[i])); }
}

int main() {
  run<64, 64, 2>("merge", 1, 2048, 768, 768, 4);
  run<64, 64, 2, 128>("merge", 1, 2048, 768, 768, 21);
  run<128, 64, 2>("merge", 1, 2048, 768, 768, 6);
  run<64, 128, 2>("merge", 1, 2048, 768, 768, 7);
  run<64, 64, 4>("wo", 2, 2048, 768, 3072, 3);
  run<64, 64, 3>("wo", 2, 2048, 768, 3072, 5);
  run<64, 64, 2, 128>("wo", 2, 2048, 768, 3072, 21);
  run<128, 64, 2>("wo", 2, 2048, 768, 3072, 6);
  return 0;
}
