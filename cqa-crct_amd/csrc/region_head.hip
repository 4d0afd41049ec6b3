// Masked-region head (params['img_loss_coeff'] > 0; BertImagePredictionHead, vilbert.py:1065-1077, with ViLBERT's masked-region
// classification over the regions whose image_label is 1): the two loss kernels.  Everything else of the head -- row gather, the padded
// decoder operands, the three products, LayerNorm, GELU derivative, column sums, row scatter -- is the masked-LM head's machinery
// (lm_head.hip, rowops.hip, gemm.hip) on this head's tensors.
// C = v_target_size classes (1601) is 25 floats per lane of ONE wave, so a row lives in registers: one wave per row, four rows per
// 256-thread workgroup, the row's logits read exactly once (the vocabulary kernels sweep 30522 columns twice with a workgroup).  Lane l
// owns the float4 chunks l, l + 64, ... of the row (columns 4 (64 q + l) .. + 3, q < NQ): NQ is a template parameter, so the chunks are
// named registers -- nothing is indexed dynamically, nothing spills.  C <= 2048 = 8 chunks per lane.
// The step uses them for SOFT targets; on hard targets the vocabulary kernels measured no slower at C = 1601 (EXPERIMENTS.md) and the step
// calls those.  Both forms are instantiated and tested.
// Nothing here reads a pad COLUMN of the logits into a result, and every pad row and pad column of dL is written as +0.
// Every kernel: vector loads and stores, no atomics, no LDS, fixed summation order (bit-reproducible).
#include "common.hip.h"
#include "crct_internal.h"

namespace {

constexpr int REGION_MAX_NQ = 8;      // float4 chunks per lane: C <= 64 * 4 * 8 = 2048

// The row's real columns into registers: a chunk that starts at or past C is not loaded, a column at or past C holds -inf (no part in
// the maximum, exp(-inf - m) = +0 in the sum).  x: the row, 16-byte aligned, with at least (C + 3) / 4 * 4 floats.
template <int NQ>
__device__ __forceinline__ void region_load_row(const float* __restrict__ x, int C, int lane, float4 (&v)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = 4 * (64 * q + lane);
    float4 a = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (c < C) {
      a = *reinterpret_cast<const float4*>(x + c);
      if (c + 1 >= C) a.y = -INFINITY;
      if (c + 2 >= C) a.z = -INFINITY;
      if (c + 3 >= C) a.w = -INFINITY;
    }
    v[q] = a;
  }
}

// Target row t (fp32 [C], 4-byte aligned: C = 1601 rows of a [N][C] tensor) into registers by dword loads; +0 at and past C.
template <int NQ>
__device__ __forceinline__ void region_load_target(const float* __restrict__ t, int C, int lane, float4 (&v)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = 4 * (64 * q + lane);
    float4 a;
    a.x = c < C ? t[c] : 0.f;
    a.y = c + 1 < C ? t[c + 1] : 0.f;
    a.z = c + 2 < C ? t[c + 2] : 0.f;
    a.w = c + 3 < C ? t[c + 3] : 0.f;
    v[q] = a;
  }
}

// lse = m + log(sum exp(x - m)) of the row in registers, wave-uniform: per lane chunk by chunk, component by component, then the fixed tree
template <int NQ>
__device__ __forceinline__ float region_row_lse(const float4 (&v)[NQ]) {
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) m = fmaxf(m, fmaxf(fmaxf(v[q].x, v[q].y), fmaxf(v[q].z, v[q].w)));
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    s += expf(v[q].x - m);
    s += expf(v[q].y - m);
    s += expf(v[q].z - m);
    s += expf(v[q].w - m);
  }
  s = wave_sum(s);
  return m + logf(s);
}

__device__ __forceinline__ float region_kl_term(float t, float x, float lse) { return t > 0.f ? t * (logf(t) - (x - lse)) : 0.f; }

// Forward of one row per wave.  Hard (labels int32 [R]): loss = lse - x[label], written by the lane that owns the label's column.
// Soft (targets fp32 [N][C] read in place at row rows[r]): loss = sum_j t_j (log t_j - (x_j - lse)), a term with t_j == 0 is 0.
template <bool SOFT, int NQ>
__global__ __launch_bounds__(256) void region_ce_fwd_kernel(const float* __restrict__ logits, long ld, const int32_t* __restrict__ labels,
                                                            const float* __restrict__ targets, const int32_t* __restrict__ rows,
                                                            float* __restrict__ loss, float* __restrict__ lse, int R, int C) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  float4 v[NQ];
  region_load_row<NQ>(logits + (long)r * ld, C, lane, v);
  const float l = region_row_lse<NQ>(v);
  if (lane == 0) lse[r] = l;
  if constexpr (SOFT) {
    const float* t = targets + (long)rows[r] * C;
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = 4 * (64 * q + lane);
      if (c < C) acc += region_kl_term(t[c], v[q].x, l);
      if (c + 1 < C) acc += region_kl_term(t[c + 1], v[q].y, l);
      if (c + 2 < C) acc += region_kl_term(t[c + 2], v[q].z, l);
      if (c + 3 < C) acc += region_kl_term(t[c + 3], v[q].w, l);
    }
    acc = wave_sum(acc);
    if (lane == 0) loss[r] = acc;
  } else {
    const int lab = labels[r], chunk = lab >> 2, k = lab & 3;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (64 * q + lane == chunk) loss[r] = l - (k == 0 ? v[q].x : (k == 1 ? v[q].y : (k == 2 ? v[q].z : v[q].w)));
  }
}

// dL[r][j] = (exp(x[r][j] - lse[r]) * s_r - t[r][j]) * (g * inv_n) as bf16 [Rp][ldd], s_r = sum_j t[r][j] (1 for a hard target, whose t is the
// one-hot of the label: the product with s_r is then left out); columns C .. Cp-1 and rows R .. Rp-1 are +0.  One wave per row, one sweep:
// the logits and, soft, the target row are read once.  g: device scalar.  ld % 4 == 0, ldd % 4 == 0 (8-byte bf16 stores), Cp <= 256 NQ.
template <bool SOFT, int NQ>
__global__ __launch_bounds__(256) void region_ce_bwd_kernel(const float* __restrict__ logits, long ld, const int32_t* __restrict__ labels,
                                                            const float* __restrict__ targets, const int32_t* __restrict__ rows,
                                                            const float* __restrict__ lse, const float* __restrict__ g, float inv_n,
                                                            bf16_t* __restrict__ dL, long ldd, int R, int Rp, int C, int Cp) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= Rp) return;
  bf16_t* d = dL + (long)r * ldd;
  if (r >= R) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = 4 * (64 * q + lane);
      if (c < Cp) *reinterpret_cast<uint2*>(d + c) = make_uint2(0u, 0u);
    }
    return;
  }
  float4 v[NQ];
  region_load_row<NQ>(logits + (long)r * ld, C, lane, v);
  const float l = lse[r], sc = g[0] * inv_n;
  float4 t[SOFT ? NQ : 1];
  float sr = 1.f;
  int lab = -1;
  if constexpr (SOFT) {
    region_load_target<NQ>(targets + (long)rows[r] * C, C, lane, t);
    sr = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) { sr += t[q].x; sr += t[q].y; sr += t[q].z; sr += t[q].w; }
    sr = wave_sum(sr);
  } else {
    lab = labels[r];
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = 4 * (64 * q + lane);
    if (c >= Cp) continue;
    const float in[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
    float tq[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SOFT) { tq[0] = t[q].x; tq[1] = t[q].y; tq[2] = t[q].z; tq[3] = t[q].w; }
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float p;
      if constexpr (SOFT) p = expf(in[k] - l) * sr - tq[k];
      else p = expf(in[k] - l) - (c + k == lab ? 1.f : 0.f);
      o[k] = c + k < C ? p * sc : 0.f;
    }
    *reinterpret_cast<uint2*>(d + c) = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
  }
}

bool aligned16(const void* a, const void* b = nullptr) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

// kernel<SOFT, NQ> for the run-time (soft, nq): the eight chunk counts are eight instantiations
#define REGION_NQ_CASE(KERNEL, N, ...)                                                                            \
  case N:                                                                                                         \
    if (soft) crct_launch(KERNEL<true, N>, grid, dim3(256), 0, st, __VA_ARGS__);                                  \
    else crct_launch(KERNEL<false, N>, grid, dim3(256), 0, st, __VA_ARGS__);                                      \
    break;
#define REGION_DISPATCH(KERNEL, ...)                                                                              \
  switch (nq) {                                                                                                   \
    REGION_NQ_CASE(KERNEL, 1, __VA_ARGS__) REGION_NQ_CASE(KERNEL, 2, __VA_ARGS__) REGION_NQ_CASE(KERNEL, 3, __VA_ARGS__) \
    REGION_NQ_CASE(KERNEL, 4, __VA_ARGS__) REGION_NQ_CASE(KERNEL, 5, __VA_ARGS__) REGION_NQ_CASE(KERNEL, 6, __VA_ARGS__) \
    REGION_NQ_CASE(KERNEL, 7, __VA_ARGS__) REGION_NQ_CASE(KERNEL, 8, __VA_ARGS__)                                 \
    default: break;                                                                                               \
  }

}  // namespace

extern "C" int crct_region_ce_fwd(const float* logits, int64_t ld, const int32_t* labels, const float* targets, const int32_t* rows,
                                  float* loss, float* lse, float* img_loss, int R, int C, float inv_n, crct_stream_t stream) {
  CRCT_REQUIRE(logits && loss && lse, "region_ce_fwd: null argument");
  CRCT_REQUIRE((labels != nullptr) != (targets != nullptr) && (targets == nullptr || rows != nullptr),
               "region_ce_fwd: either labels (hard) or targets with rows (soft)");
  CRCT_REQUIRE(R >= 1 && C >= 1 && C <= 256 * REGION_MAX_NQ && ld >= (C + 3) / 4 * 4 && ld % 4 == 0 && aligned16(logits),
               "region_ce_fwd: R=%d C=%d ld=%ld (1 <= C <= %d, ld a multiple of 4 covering C, 16-byte aligned rows)", R, C, (long)ld, 256 * REGION_MAX_NQ);
  const bool soft = targets != nullptr;
  const int nq = (C + 255) / 256;
  const dim3 grid((R + 3) / 4);
  const hipStream_t st = (hipStream_t)stream;
  REGION_DISPATCH(region_ce_fwd_kernel, logits, (long)ld, labels, targets, rows, loss, lse, R, C)
  if (img_loss) crct_loss_mean(loss, img_loss, R, inv_n, st);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_region_ce_bwd(const float* logits, int64_t ld, const int32_t* labels, const float* targets, const int32_t* rows,
                                  const float* lse, const float* g, float inv_n, void* dL_bf16, int64_t ldd, int R, int Rp, int C, int Cp,
                                  crct_stream_t stream) {
  CRCT_REQUIRE(logits && lse && g && dL_bf16, "region_ce_bwd: null argument");
  CRCT_REQUIRE((labels != nullptr) != (targets != nullptr) && (targets == nullptr || rows != nullptr),
               "region_ce_bwd: either labels (hard) or targets with rows (soft)");
  CRCT_REQUIRE(R >= 1 && Rp >= R && C >= 1 && Cp >= C && Cp % 4 == 0 && Cp <= 256 * REGION_MAX_NQ && ld >= (C + 3) / 4 * 4 && ld % 4 == 0 &&
                   ldd >= Cp && ldd % 4 == 0 && aligned16(logits, dL_bf16),
               "region_ce_bwd: R=%d Rp=%d C=%d Cp=%d ld=%ld ldd=%ld (Cp a multiple of 4 covering C, at most %d; ld covering C, ldd covering Cp)",
               R, Rp, C, Cp, (long)ld, (long)ldd, 256 * REGION_MAX_NQ);
  const bool soft = targets != nullptr;
  const int nq = (Cp + 255) / 256;
  const dim3 grid((Rp + 3) / 4);
  const hipStream_t st = (hipStream_t)stream;
  REGION_DISPATCH(region_ce_bwd_kernel, logits, (long)ld, labels, targets, rows, lse, g, inv_n, (bf16_t*)dL_bf16, (long)ldd, R, Rp, C, Cp)
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}
