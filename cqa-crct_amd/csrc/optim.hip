// Fused multi-tensor AdamW over the flat fp32 parameter / gradient / moment buffers.
// Semantics: torch.optim.AdamW as the reference constructs it (CRCT/utils.py:228-249: one group per
// tensor, lr by language_weights.json, weight_decay 0 for bias / LayerNorm, betas (0.9, 0.999),
// eps 1e-8) -- decoupled decay p *= 1 - lr*wd, then the bias-corrected Adam update -- plus the
// refresh of the bf16 weight shadow the GEMMs read.  HBM-bound: 16 B read + 12 B (+2 B) written per
// parameter; each workgroup owns up to 4096 contiguous elements of ONE tensor (no divergence on
// lr / wd), float4 accesses.  With an exponential moving average of the weights (crct_adamw_step_ema, adamw_kernel<true>) 4 B more
// are read and 4 B more written per parameter, in the same loop.
#include <stdlib.h>

#include "common.hip.h"
#include "crct_internal.h"

// non-temporal streaming of the optimizer state: measured 8.73 -> 8.60 ms per step (the next forward keeps its operands in
// L2 / Infinity Cache while 7 GB of state stream past)
#ifndef CRCT_ADAMW_NT
#define CRCT_ADAMW_NT 1
#endif
namespace {
constexpr int ADAMW_CHUNK = 4096;
#ifdef CRCT_GEMM_LAB
__global__ __launch_bounds__(1024) void lab_spin_kernel(long long ticks) {      // ticks of 10 ns; no clock reads, no memory instruction at all
  const long long n = ticks * 24 / (127 * 64);                                  // s_sleep 127 = 127 x 64 cycles at ~2.4 GHz
  for (long long i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(127);
}
#endif

// Exponential moving average of the weights, folded into the update's own launch (EMA = true): behind the store of the new weight p'
// the average e of that element moves towards it by the fraction w = 1 - decay,
//     d = p' - e            one fp32 subtraction, rounded
//     e' = fmaf(w, d, e)    one fused multiply-add, rounded once
// spelled with the explicit fmaf so that no contraction is left to the compiler: the vector path and the scalar tail round alike, and
// tests/ema_ref.py derives its budget from exactly these two roundings.  w = 0 returns e bit for bit for every finite d; a NaN / inf in
// p' or e arrives in e' of that element alone.
__device__ __forceinline__ float ema_update(float e, float p_new, float w) {
  const float d = p_new - e;
  return fmaf(w, d, e);
}

// EMA = false is the update as it always was (`ema`, `ema_w` are not read); EMA = true adds one stream to the same loop: `ema`, a flat
// fp32 buffer with the element offsets of p, is loaded with p / g / m / v and stored with them (4 B read + 4 B written per parameter on top
// of 30, no LDS, no atomics).  The element index is the loop's own, so the plain chunk and the 64 x 64 tile walk are covered alike.
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16_t* __restrict__ pb,
                                                    const int64_t* __restrict__ seg_off, const int64_t* __restrict__ seg_len,
                                                    const float* __restrict__ seg_lr, const float* __restrict__ seg_wd,
                                                    const int32_t* __restrict__ blk_seg, const int64_t* __restrict__ blk_off,
                                                    float beta1, float beta2, float eps, float inv_bc1, float inv_sqrt_bc2,
                                                    const float* __restrict__ inv_scale_dev, const CrctAmpState amp, const CrctFp8Shadow f8,
                                                    int n_blk, int zero_g, const bf16_t* __restrict__ g16,
                                                    float* __restrict__ ema, float ema_w) {
 // loss scaling (torch.amp.GradScaler): a step whose gradients held an inf / nan is skipped as a whole, the scale divides
 // the gradients, and the step count behind the bias corrections is the device counter that only advances on real steps
 if (amp.found_inf && amp.found_inf[0] != 0.f) return;
 if (amp.step) {
   const float st = (float)amp.step[0];
   inv_bc1 = 1.0f / (1.0f - powf(beta1, st));
   inv_sqrt_bc2 = 1.0f / sqrtf(1.0f - powf(beta2, st));
 }
 __shared__ uint32_t tile[64][17];          // e4m3 bytes of one 64 x 64 weight tile (transposed shadow), 68-byte rows
 for (int blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
  const int sgi = blk_seg[blk];
  const int64_t off = blk_off[blk];
  int64_t base = seg_off[sgi] + off;
  int64_t n = seg_len[sgi] - off;
  if (n > ADAMW_CHUNK) n = ADAMW_CHUNK;
  // A weight [out][in] that also keeps a TRANSPOSED e4m3 shadow (fp8 data gradients) is walked tile by tile instead of chunk by
  // chunk: chunk number c of the tensor is the 64 x 64 tile (c / (in / 64), c % (in / 64)), so that the workgroup holds whole
  // columns of the tile and can write them as 16-byte runs of the transposed copy.  Everything else in the update is elementwise.
  const int tin = (f8.qt && f8.seg_in && f8.seg_t_base && f8.seg_t_ld) ? f8.seg_in[sgi] : 0;
  int64_t row_stride = 64, t_base = 0;
  int t_out = 0;
  if (tin > 0) {
    const int tiles_in = tin >> 6;
    const int64_t c = off / ADAMW_CHUNK;
    const int tr = (int)(c / tiles_in), tc = (int)(c % tiles_in);
    t_out = f8.seg_t_ld[sgi];                      // rows of the whole (possibly fused) weight = row length of its transposed copy
    base = seg_off[sgi] + (int64_t)tr * 64 * tin + (int64_t)tc * 64;
    row_stride = tin;
    t_base = f8.seg_t_base[sgi] + (int64_t)tc * 64 * t_out + (int64_t)tr * 64;
  }
  const float lr = seg_lr[sgi], wd = seg_wd[sgi];
  const float decay = 1.0f - lr * wd, step_size = lr * inv_bc1;
  float gsc = inv_scale_dev ? inv_scale_dev[0] : 1.0f;
  if (amp.grad_scale) gsc /= amp.grad_scale[0];
  // e4m3 shadow of the weights the fp8 forward GEMMs read (BASELINE configs[4]): written with the tensor's CURRENT scale
  // (from the amax one step back: delayed scaling, saturating), while max |w| of the new values feeds the next scale
  const int qslot = f8.q ? f8.seg_slot[sgi] : -1;
  const float qs = qslot >= 0 ? f8.scale[qslot] : 0.f;
  float qmax = 0.f;
  for (int64_t i = (int64_t)threadIdx.x * 4; i < n; i += 1024) {
    const int64_t e = base + (i >> 6) * row_stride + (i & 63);      // row_stride == 64: the plain chunk, e = base + i
    if (i + 4 <= n) {
#if CRCT_ADAMW_NT      // streamed once per step: non-temporal, so the 7 GB do not evict the forward's operands from L2 / MALL
      const f4_t pv = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(p + e));
      f4_t gv;
      if (g16) {      // the exchanged bf16 gradient as it lies in the communication buffer (8 bytes per 4 elements)
        typedef unsigned u2_t __attribute__((ext_vector_type(2)));
        const u2_t raw = __builtin_nontemporal_load(reinterpret_cast<const u2_t*>(g16 + e));
        gv = f4_t{bf2f((bf16_t)(raw[0] & 0xffff)), bf2f((bf16_t)(raw[0] >> 16)), bf2f((bf16_t)(raw[1] & 0xffff)), bf2f((bf16_t)(raw[1] >> 16))};
      } else {
        gv = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(g + e));
      }
      const f4_t mv = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(m + e));
      const f4_t vv = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(v + e));
      f4_t ev;
      if constexpr (EMA) ev = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(ema + e));
#else
      const f4_t pv = *reinterpret_cast<const f4_t*>(p + e);
      f4_t gv = g16 ? f4_t{bf2f(g16[e]), bf2f(g16[e + 1]), bf2f(g16[e + 2]), bf2f(g16[e + 3])} : *reinterpret_cast<const f4_t*>(g + e);
      const f4_t mv = *reinterpret_cast<const f4_t*>(m + e), vv = *reinterpret_cast<const f4_t*>(v + e);
      f4_t ev;
      if constexpr (EMA) ev = *reinterpret_cast<const f4_t*>(ema + e);
#endif
      float pa[4] = {pv[0], pv[1], pv[2], pv[3]}, ga[4] = {gv[0] * gsc, gv[1] * gsc, gv[2] * gsc, gv[3] * gsc};
      float ma[4] = {mv[0], mv[1], mv[2], mv[3]}, va[4] = {vv[0], vv[1], vv[2], vv[3]};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pa[k] *= decay;
        ma[k] = beta1 * ma[k] + (1.0f - beta1) * ga[k];
        va[k] = beta2 * va[k] + (1.0f - beta2) * ga[k] * ga[k];
        pa[k] -= step_size * ma[k] / (sqrtf(va[k]) * inv_sqrt_bc2 + eps);
      }
#if CRCT_ADAMW_NT
      __builtin_nontemporal_store(f4_t{pa[0], pa[1], pa[2], pa[3]}, reinterpret_cast<f4_t*>(p + e));
      __builtin_nontemporal_store(f4_t{ma[0], ma[1], ma[2], ma[3]}, reinterpret_cast<f4_t*>(m + e));
      __builtin_nontemporal_store(f4_t{va[0], va[1], va[2], va[3]}, reinterpret_cast<f4_t*>(v + e));
      if constexpr (EMA)
        __builtin_nontemporal_store(f4_t{ema_update(ev[0], pa[0], ema_w), ema_update(ev[1], pa[1], ema_w), ema_update(ev[2], pa[2], ema_w),
                                         ema_update(ev[3], pa[3], ema_w)}, reinterpret_cast<f4_t*>(ema + e));
#else
      *reinterpret_cast<float4*>(p + e) = make_float4(pa[0], pa[1], pa[2], pa[3]);
      *reinterpret_cast<float4*>(m + e) = make_float4(ma[0], ma[1], ma[2], ma[3]);
      *reinterpret_cast<float4*>(v + e) = make_float4(va[0], va[1], va[2], va[3]);
      if constexpr (EMA)
        *reinterpret_cast<float4*>(ema + e) = make_float4(ema_update(ev[0], pa[0], ema_w), ema_update(ev[1], pa[1], ema_w),
                                                          ema_update(ev[2], pa[2], ema_w), ema_update(ev[3], pa[3], ema_w));
#endif
      if (pb) *reinterpret_cast<uint2*>(pb + e) = make_uint2(pack2bf(pa[0], pa[1]), pack2bf(pa[2], pa[3]));
      if (qslot >= 0) {
        qmax = amax_join(amax_join(qmax, amax_pair(pa[0], pa[1])), amax_pair(pa[2], pa[3]));
        uint32_t w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(pa[0] * qs), f8_clamp(pa[1] * qs), w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(pa[2] * qs), f8_clamp(pa[3] * qs), w, true);
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(f8.q) + e) = w;
        if (tin > 0) tile[i >> 6][(i & 63) >> 2] = w;
      }
      if (zero_g) __builtin_nontemporal_store(f4_t{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4_t*>(g + e));
    } else {
      for (int64_t k = i; k < n; ++k) {
        const int64_t q = base + k;
        float pa = p[q] * decay;
        const float ga = (g16 ? bf2f(g16[q]) : g[q]) * gsc;
        const float ma = beta1 * m[q] + (1.0f - beta1) * ga;
        const float va = beta2 * v[q] + (1.0f - beta2) * ga * ga;
        pa -= step_size * ma / (sqrtf(va) * inv_sqrt_bc2 + eps);
        p[q] = pa; m[q] = ma; v[q] = va;
        if constexpr (EMA) ema[q] = ema_update(ema[q], pa, ema_w);
        if (pb) pb[q] = f2bf(pa);
        if (zero_g) g[q] = 0.f;
      }
    }
  }
  if (qslot >= 0) {          // fp8-shadowed tensors are multiples of 4 elements (Linear weights): the scalar tail never holds them
    qmax = amax_wave(qmax);
    if ((threadIdx.x & 63) == 0) amax_update(f8.amax + (long)qslot * CRCT_FP8_AMAX_LANES, qmax);
  }
  if (tin > 0) {             // uniform over the workgroup (one tensor per chunk)
    __syncthreads();
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(&tile[0][0]);
    const int c = threadIdx.x >> 2, ch = (threadIdx.x & 3) * 16;      // transposed row = in index c, 16 consecutive out indices
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = (uint32_t)tb[(ch + 4 * k) * 68 + c] | ((uint32_t)tb[(ch + 4 * k + 1) * 68 + c] << 8) |
             ((uint32_t)tb[(ch + 4 * k + 2) * 68 + c] << 16) | ((uint32_t)tb[(ch + 4 * k + 3) * 68 + c] << 24);
    *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(f8.qt) + t_base + (int64_t)c * t_out + ch) = make_uint4(w[0], w[1], w[2], w[3]);
    __syncthreads();
  }
 }
}
__global__ void adamw_advance_kernel(int32_t* step, const float* found_inf) {
  if (threadIdx.x == 0 && (!found_inf || found_inf[0] == 0.f)) step[0] += 1;
}
// g[off[r] + blk_off .. ) = 0 over the chunk table of crct_adamw_plan (same chunking as the update itself)
__global__ __launch_bounds__(256) void zero_runs_kernel(float* __restrict__ g, const int64_t* __restrict__ run_off,
                                                        const int64_t* __restrict__ run_len, const int32_t* __restrict__ blk_seg,
                                                        const int64_t* __restrict__ blk_off, int n_blk) {
  for (int blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
    const int r = blk_seg[blk];
    const int64_t off = blk_off[blk], base = run_off[r] + off;
    int64_t n = run_len[r] - off;
    if (n > ADAMW_CHUNK) n = ADAMW_CHUNK;
    const int64_t head = (4 - (base & 3)) & 3;            // elements in front of the first 16-byte boundary
    for (int64_t i = threadIdx.x; i < (head < n ? head : n); i += 256) g[base + i] = 0.f;
    const int64_t nv = n > head ? (n - head) / 4 : 0;
    for (int64_t i = threadIdx.x; i < nv; i += 256)
      __builtin_nontemporal_store(f4_t{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4_t*>(g + base + head) + i);
    for (int64_t i = head + nv * 4 + threadIdx.x; i < n; i += 256) g[base + i] = 0.f;
  }
}
// ---- global-norm gradient clipping (crct_grad_sumsq / crct_grad_norm_finalize / crct_scale_runs) ----------------------
// One streaming, read-only pass over the gradient buffer the next update will consume, walked by the update's own chunk
// table: one fp32 partial per chunk, no atomics and no hand-off between workgroups, so every result is bit-reproducible.
// KIND 0 = sum of squares, KIND 1 = max |g|.  Both work on non-negative values, and the maximum is taken on the BIT
// PATTERNS (for non-negative floats the unsigned order is the float order, with every NaN above +inf): a NaN anywhere
// comes out as NaN, which fmaxf alone would drop.
template <int KIND>
__device__ __forceinline__ float nrm_join(float a, float b) {
  if (KIND) {
    const uint32_t ua = __float_as_uint(a), ub = __float_as_uint(b);
    return __uint_as_float(ua > ub ? ua : ub);
  }
  return a + b;
}
// four consecutive elements -> one value.  The fused multiply-adds are spelled out: the fp32 and the bf16 source must round
// alike (two steps from either buffer are compared bit for bit), which a contraction left to the compiler does not promise.
template <int KIND>
__device__ __forceinline__ float nrm_quad(float x0, float x1, float x2, float x3) {
  if (KIND) return nrm_join<1>(nrm_join<1>(nrm_join<1>(fabsf(x0), fabsf(x1)), fabsf(x2)), fabsf(x3));
  return fmaf(x3, x3, fmaf(x2, x2, fmaf(x1, x1, x0 * x0)));
}
template <int KIND>
__device__ __forceinline__ float nrm_wave(float v) {       // the DPP tree of wave_sum / wave_max (common.hip.h) with nrm_join
  v = nrm_join<KIND>(v, dpp_f32<0xB1>(v));
  v = nrm_join<KIND>(v, dpp_f32<0x4E>(v));
  v = nrm_join<KIND>(v, dpp_f32<0x141>(v));
  v = nrm_join<KIND>(v, dpp_f32<0x140>(v));
  return nrm_join<KIND>(nrm_join<KIND>(lane_f32(v, 0), lane_f32(v, 16)), nrm_join<KIND>(lane_f32(v, 32), lane_f32(v, 48)));
}
// A chunk (<= 4096 elements of one tensor, 16-byte aligned base) is 1024 quads.  Every lane loads 16 bytes at a time -- one quad
// of fp32, two of bf16 -- and leaves its quad values in LDS; from there on the tree depends on neither the source format nor
// the workgroup that runs it: lane t joins quads t, t + 256, t + 512, t + 768, then the wave tree, then the four waves.
// Longest chain of dependent fp32 roundings: 4 (quad) + 3 + 6 (wave) + 2 = 15.  Quads past the end of the chunk count as 0.
template <int KIND, bool BF16>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const bf16_t* __restrict__ g16,
                                                         const int64_t* __restrict__ seg_off, const int64_t* __restrict__ seg_len,
                                                         const int32_t* __restrict__ blk_seg, const int64_t* __restrict__ blk_off,
                                                         float* __restrict__ partials, int n_blk) {
  __shared__ float quad[1024];
  __shared__ float wave_part[4];
  const int tid = threadIdx.x;
  for (int blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
    const int sgi = blk_seg[blk];
    const int64_t off = blk_off[blk], base = seg_off[sgi] + off;
    int64_t n = seg_len[sgi] - off;
    if (n > ADAMW_CHUNK) n = ADAMW_CHUNK;
    if (BF16) {
      typedef unsigned u4_t __attribute__((ext_vector_type(4)));
      float x[2][8];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int64_t i = (int64_t)k * 2048 + tid * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[k][j] = 0.f;
        if (i + 8 <= n) {      // streamed once: non-temporal, as in adamw_kernel
          const u4_t raw = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(g16 + base + i));
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            x[k][2 * j] = bf2f((bf16_t)(raw[j] & 0xffff));
            x[k][2 * j + 1] = bf2f((bf16_t)(raw[j] >> 16));
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (i + j < n) x[k][j] = bf2f(g16[base + i + j]);
        }
      }
#pragma unroll
      for (int k = 0; k < 2; ++k)
        *reinterpret_cast<float2*>(&quad[k * 512 + tid * 2]) = make_float2(nrm_quad<KIND>(x[k][0], x[k][1], x[k][2], x[k][3]),
                                                                           nrm_quad<KIND>(x[k][4], x[k][5], x[k][6], x[k][7]));
    } else {
      float x[4][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t i = (int64_t)k * 1024 + tid * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) x[k][j] = 0.f;
        if (i + 4 <= n) {
          const f4_t v = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(g + base + i));
          x[k][0] = v[0]; x[k][1] = v[1]; x[k][2] = v[2]; x[k][3] = v[3];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j < n) x[k][j] = g[base + i + j];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) quad[k * 256 + tid] = nrm_quad<KIND>(x[k][0], x[k][1], x[k][2], x[k][3]);
    }
    __syncthreads();
    float a = nrm_join<KIND>(nrm_join<KIND>(nrm_join<KIND>(quad[tid], quad[tid + 256]), quad[tid + 512]), quad[tid + 768]);
    a = nrm_wave<KIND>(a);
    if ((tid & 63) == 0) wave_part[tid >> 6] = a;
    __syncthreads();           // also: every read of quad[] is done before the next chunk overwrites it
    if (tid == 0) partials[blk] = nrm_join<KIND>(nrm_join<KIND>(wave_part[0], wave_part[1]), nrm_join<KIND>(wave_part[2], wave_part[3]));
  }
}

// fp64 from here on.  kind 1: the larger value, a NaN on either side wins.
__device__ __forceinline__ double nrm_join64(double a, double b, int kind) {
  if (kind) return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
  return a + b;
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xf, 0xf, true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double lane_f64(double v, int lane) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double nrm_wave64(double v, int kind) {
  v = nrm_join64(v, dpp_f64<0xB1>(v), kind);
  v = nrm_join64(v, dpp_f64<0x4E>(v), kind);
  v = nrm_join64(v, dpp_f64<0x141>(v), kind);
  v = nrm_join64(v, dpp_f64<0x140>(v), kind);
  return nrm_join64(nrm_join64(lane_f64(v, 0), lane_f64(v, 16), kind), nrm_join64(lane_f64(v, 32), lane_f64(v, 48), kind), kind);
}
// First index i of the ascending a[0 .. n) with a[i] >= key, found by the whole wave: 64 probes per round instead of one (four
// rounds of one load each for 60 k chunks; a one-lane bisection is 16 dependent loads).  Every lane returns the same value.
__device__ __forceinline__ int wave_lower_bound(const int32_t* __restrict__ a, int n, int key, int lane) {
  int lo = 0, hi = n;                                   // the answer lies in [lo, hi]
  while (hi > lo) {
    const int step = (hi - lo + 63) / 64;
    const int idx = lo + step * (lane + 1) - 1;         // ascending over the lanes, so the lanes that see "less" are the first cnt
    const bool less = idx < hi && a[idx] < key;
    const int cnt = __popcll(__ballot(less));
    const int top = lo + step * (cnt + 1) - 1;          // the first probe that is not less (or lies behind the range)
    lo += step * cnt;
    hi = top < hi ? top : hi;
  }
  return lo;
}
// sum / max of p[b0 + lane], p[b0 + lane + stride], ... below b1 in that order, eight loads in flight at a time (0 is neutral for both
// kinds: every partial is non-negative)
__device__ __forceinline__ double nrm_strided64(const float* __restrict__ p, int b0, int b1, int stride, int kind) {
  double a = 0.0;
  for (int i = b0; i < b1; i += 8 * stride) {
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (i + k * stride < b1) ? p[i + k * stride] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) a = nrm_join64(a, (double)x[k], kind);
  }
  return a;
}
// One small launch, fixed order, no hand-off between its workgroups.  Workgroup 0, the total: lane t of the workgroup takes partials
// t, t + 1024, ..., then the wave tree, then the 16 waves in order; from it the coefficient, torch's clip_grad_norm_ arithmetic in
// fp32 and not special-cased: an inf norm gives 0, a NaN norm gives NaN, a norm that needs no clipping gives exactly 1.  Workgroups
// 1 ..: a wave per tensor, whose chunks are one run of the table (crct_adamw_plan lists them tensor by tensor).
__global__ __launch_bounds__(1024) void grad_norm_finalize_kernel(const float* __restrict__ partials, const int32_t* __restrict__ blk_seg,
                                                                  int n_blk, int n_seg, int kind, float max_norm,
                                                                  const float* __restrict__ grad_scale, const float* __restrict__ mul,
                                                                  float* __restrict__ out, float* __restrict__ seg_norm) {
  __shared__ double wave_part[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double gs = grad_scale ? (double)grad_scale[0] : 1.0;
  if (blockIdx.x > 0) {
    const int s = ((int)blockIdx.x - 1) * 16 + wave;
    if (s >= n_seg) return;
    const int b0 = wave_lower_bound(blk_seg, n_blk, s, lane), b1 = wave_lower_bound(blk_seg, n_blk, s + 1, lane);
    const double v = nrm_wave64(nrm_strided64(partials, b0 + lane, b1, 64, kind), kind);
    if (lane == 0) seg_norm[s] = (float)((kind ? v : sqrt(v)) / gs);
    return;
  }
  const double a = nrm_wave64(nrm_strided64(partials, tid, n_blk, 1024, kind), kind);
  if (lane == 0) wave_part[wave] = a;
  __syncthreads();
  if (tid == 0) {
    double t = wave_part[0];
    for (int w = 1; w < 16; ++w) t = nrm_join64(t, wave_part[w], kind);
    const float norm = (float)((kind ? t : sqrt(t)) / gs);
    float c = max_norm / (norm + 1e-6f);
    c = c > 1.0f ? 1.0f : c;
    out[0] = norm;
    out[1] = c * (mul ? mul[0] : 1.0f);
  }
}

// g *= *coef over the chunk table, one fp32 product per element.  A coefficient of exactly 1 (nothing to clip: the common step)
// ends every workgroup before its first gradient load.
__global__ __launch_bounds__(256) void scale_runs_kernel(float* __restrict__ g, const float* __restrict__ coef,
                                                         const int64_t* __restrict__ seg_off, const int64_t* __restrict__ seg_len,
                                                         const int32_t* __restrict__ blk_seg, const int64_t* __restrict__ blk_off, int n_blk) {
  const float c = coef[0];
  if (c == 1.0f) return;
  for (int blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
    const int sgi = blk_seg[blk];
    const int64_t off = blk_off[blk], base = seg_off[sgi] + off;
    int64_t n = seg_len[sgi] - off;
    if (n > ADAMW_CHUNK) n = ADAMW_CHUNK;
    for (int64_t i = (int64_t)threadIdx.x * 4; i < n; i += 1024) {
      if (i + 4 <= n) {
        const f4_t v = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(g + base + i));
        __builtin_nontemporal_store(f4_t{v[0] * c, v[1] * c, v[2] * c, v[3] * c}, reinterpret_cast<f4_t*>(g + base + i));
      } else {
        for (int64_t k = i; k < n; ++k) g[base + k] *= c;
      }
    }
  }
}
}  // namespace

extern "C" int crct_zero_runs(float* base, const int64_t* off, const int64_t* len, const int32_t* blk_seg,
                              const int64_t* blk_off, int64_t n_blk, crct_stream_t stream) {
  CRCT_REQUIRE(base && off && len && blk_seg && blk_off, "zero_runs: null argument");
  if (n_blk <= 0) return 0;
  const long grid = n_blk > 1024 ? 1024 : n_blk;
  crct_launch(zero_runs_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, base, off, len, blk_seg, blk_off,
                     (int)n_blk);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t crct_adamw_plan(const int64_t* seg_len, int n_seg, int32_t* blk_seg, int64_t* blk_off, int64_t cap) {
  int64_t nb = 0;
  for (int s = 0; s < n_seg; ++s)
    for (int64_t o = 0; o < seg_len[s]; o += ADAMW_CHUNK) {
      if (blk_seg && blk_off && nb < cap) { blk_seg[nb] = s; blk_off[nb] = o; }
      ++nb;
    }
  return nb;
}

// the one host path of crct_adamw_step (ema == NULL: adamw_kernel<false>) and crct_adamw_step_ema
static int adamw_step_host(float* p, float* g, float* m, float* v, void* p_bf16, const int64_t* seg_off,
                           const int64_t* seg_len, const float* seg_lr, const float* seg_wd, const int32_t* blk_seg,
                           const int64_t* blk_off, int64_t n_blk, float beta1, float beta2, float eps, int step,
                           const float* inv_scale_dev, const CrctAmpState* amp_state, const CrctFp8Shadow* fp8_shadow,
                           int max_workgroups, int zero_grads, const void* g_bf16, float* ema, float ema_weight, crct_stream_t stream) {
  CRCT_REQUIRE(step >= 1, "adamw: step must be >= 1 (got %d)", step);
  CRCT_REQUIRE(ema_weight >= 0.f && ema_weight <= 1.f, "adamw: ema_weight must lie in [0, 1] (got %g)", (double)ema_weight);
  CRCT_REQUIRE(((uintptr_t)ema & 15) == 0, "adamw: ema must be 16-byte aligned (got %p)", (void*)ema);
  CrctAmpState amp = {nullptr, nullptr, nullptr};
  if (amp_state) amp = *amp_state;
  CrctFp8Shadow f8 = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (fp8_shadow) f8 = *fp8_shadow;
  CRCT_REQUIRE(!f8.q || (f8.seg_slot && f8.scale && f8.amax), "adamw: incomplete fp8 shadow description");
  if (n_blk <= 0) return 0;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  // max_workgroups > 0: a grid-stride launch of at most that many workgroups.  An update that runs BESIDE the next
  // forward on its own stream is throttled this way (256 = one workgroup per CU): at full width it saturates HBM for
  // 1.4 ms and the first layers of the forward crawl (measured: 10.25-10.36 -> 10.03 ms per step).
  const long grid = (max_workgroups > 0 && n_blk > max_workgroups) ? max_workgroups : n_blk;
#ifdef CRCT_GEMM_LAB   // timing only: the update as a kernel of the same grid and duration that touches no memory (what its TRAFFIC costs the forward beside it)
  static const double lab_spin_tbps = getenv("CRCT_LAB_ADAMW_SPIN") ? atof(getenv("CRCT_LAB_ADAMW_SPIN")) : 0.0;
  if (lab_spin_tbps > 0.0) {
    const long long ticks = (long long)((double)n_blk * ADAMW_CHUNK * 30.0 / (lab_spin_tbps * 1e12) * 1e8);
    static const int spin_threads = getenv("CRCT_LAB_ADAMW_SPIN_THREADS") ? atoi(getenv("CRCT_LAB_ADAMW_SPIN_THREADS")) : 256;
    static const int spin_grid = getenv("CRCT_LAB_ADAMW_SPIN_GRID") ? atoi(getenv("CRCT_LAB_ADAMW_SPIN_GRID")) : 0;
    crct_launch(lab_spin_kernel, dim3((unsigned)(spin_grid > 0 ? spin_grid : grid)), dim3(spin_threads), 0, (hipStream_t)stream, ticks);
    return 0;
  }
#endif
#define CRCT_ADAMW_LAUNCH(EMA)                                                                                                  \
  crct_launch(adamw_kernel<EMA>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16,          \
              seg_off, seg_len, seg_lr, seg_wd, blk_seg, blk_off, beta1, beta2, eps, (float)(1.0 / bc1),                        \
              (float)(1.0 / sqrt(bc2)), inv_scale_dev, amp, f8, (int)n_blk, zero_grads, (const bf16_t*)g_bf16, ema, ema_weight)
  if (ema) CRCT_ADAMW_LAUNCH(true); else CRCT_ADAMW_LAUNCH(false);
#undef CRCT_ADAMW_LAUNCH
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_adamw_step(float* p, float* g, float* m, float* v, void* p_bf16, const int64_t* seg_off,
                               const int64_t* seg_len, const float* seg_lr, const float* seg_wd, const int32_t* blk_seg,
                               const int64_t* blk_off, int64_t n_blk, float beta1, float beta2, float eps, int step,
                               const float* inv_scale_dev, const CrctAmpState* amp_state, const CrctFp8Shadow* fp8_shadow,
                               int max_workgroups, int zero_grads, const void* g_bf16, crct_stream_t stream) {
  return adamw_step_host(p, g, m, v, p_bf16, seg_off, seg_len, seg_lr, seg_wd, blk_seg, blk_off, n_blk, beta1, beta2, eps, step,
                         inv_scale_dev, amp_state, fp8_shadow, max_workgroups, zero_grads, g_bf16, nullptr, 0.f, stream);
}

extern "C" int crct_adamw_step_ema(float* p, float* g, float* m, float* v, void* p_bf16, const int64_t* seg_off,
                                   const int64_t* seg_len, const float* seg_lr, const float* seg_wd, const int32_t* blk_seg,
                                   const int64_t* blk_off, int64_t n_blk, float beta1, float beta2, float eps, int step,
                                   const float* inv_scale_dev, const CrctAmpState* amp_state, const CrctFp8Shadow* fp8_shadow,
                                   int max_workgroups, int zero_grads, const void* g_bf16, float* ema, float ema_weight,
                                   crct_stream_t stream) {
  return adamw_step_host(p, g, m, v, p_bf16, seg_off, seg_len, seg_lr, seg_wd, blk_seg, blk_off, n_blk, beta1, beta2, eps, step,
                         inv_scale_dev, amp_state, fp8_shadow, max_workgroups, zero_grads, g_bf16, ema, ema_weight, stream);
}

extern "C" int crct_adamw_advance(int32_t* step_dev, const float* found_inf_dev, crct_stream_t stream) {
  CRCT_REQUIRE(step_dev, "adamw_advance: null step counter");
  crct_launch(adamw_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_dev, found_inf_dev);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_grad_sumsq(const float* g_f32, const void* g_bf16, const int64_t* seg_off, const int64_t* seg_len,
                               const int32_t* blk_seg, const int64_t* blk_off, int64_t n_blk, float* partials, int norm_kind,
                               int max_workgroups, crct_stream_t stream) {
  CRCT_REQUIRE(g_f32 || g_bf16, "grad_sumsq: no gradient buffer (g_f32 and g_bf16 are both null)");
  CRCT_REQUIRE(seg_off && seg_len && blk_seg && blk_off, "grad_sumsq: null chunk table");
  CRCT_REQUIRE(partials, "grad_sumsq: null partials");
  CRCT_REQUIRE(n_blk >= 0 && n_blk <= INT32_MAX, "grad_sumsq: n_blk out of range (got %lld)", (long long)n_blk);
  CRCT_REQUIRE(norm_kind == 0 || norm_kind == 1, "grad_sumsq: norm_kind must be 0 (sum of squares) or 1 (max), got %d", norm_kind);
  CRCT_REQUIRE(max_workgroups >= 0, "grad_sumsq: negative max_workgroups (%d)", max_workgroups);
  if (n_blk == 0) return 0;
  const long grid = (max_workgroups > 0 && n_blk > max_workgroups) ? max_workgroups : n_blk;
  const bf16_t* g16 = (const bf16_t*)g_bf16;
#define CRCT_SUMSQ_LAUNCH(KIND, BF)                                                                                          \
  crct_launch(grad_sumsq_kernel<KIND, BF>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g_f32, g16, seg_off, seg_len, \
              blk_seg, blk_off, partials, (int)n_blk)
  if (g16) { if (norm_kind) CRCT_SUMSQ_LAUNCH(1, true); else CRCT_SUMSQ_LAUNCH(0, true); }
  else     { if (norm_kind) CRCT_SUMSQ_LAUNCH(1, false); else CRCT_SUMSQ_LAUNCH(0, false); }
#undef CRCT_SUMSQ_LAUNCH
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_grad_norm_finalize(const float* partials, const int32_t* blk_seg, int64_t n_blk, int n_seg, int norm_kind,
                                       float max_norm, const float* grad_scale_dev, const float* mul_dev, float* out,
                                       float* seg_norm, crct_stream_t stream) {
  CRCT_REQUIRE(out, "grad_norm_finalize: null out");
  CRCT_REQUIRE(n_blk >= 0 && n_blk <= INT32_MAX && n_seg >= 0, "grad_norm_finalize: negative count (n_blk %lld, n_seg %d)", (long long)n_blk, n_seg);
  CRCT_REQUIRE(n_blk == 0 || partials, "grad_norm_finalize: null partials");
  CRCT_REQUIRE(!seg_norm || n_blk == 0 || blk_seg, "grad_norm_finalize: per-tensor norms need the chunk table (null blk_seg)");
  CRCT_REQUIRE(norm_kind == 0 || norm_kind == 1, "grad_norm_finalize: norm_kind must be 0 (sum of squares) or 1 (max), got %d", norm_kind);
  CRCT_REQUIRE(!(max_norm < 0.f), "grad_norm_finalize: negative max_norm (%g)", (double)max_norm);
  crct_launch(grad_norm_finalize_kernel, dim3(1u + (seg_norm ? (unsigned)((n_seg + 15) / 16) : 0u)), dim3(1024), 0, (hipStream_t)stream, partials, blk_seg, (int)n_blk, n_seg, norm_kind,
              max_norm, grad_scale_dev, mul_dev, out, seg_norm);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_scale_runs(float* g_f32, const float* coef_dev, const int64_t* seg_off, const int64_t* seg_len,
                               const int32_t* blk_seg, const int64_t* blk_off, int64_t n_blk, int max_workgroups, crct_stream_t stream) {
  CRCT_REQUIRE(g_f32 && coef_dev, "scale_runs: null gradient buffer or coefficient");
  CRCT_REQUIRE(seg_off && seg_len && blk_seg && blk_off, "scale_runs: null chunk table");
  CRCT_REQUIRE(n_blk >= 0 && n_blk <= INT32_MAX, "scale_runs: n_blk out of range (got %lld)", (long long)n_blk);
  CRCT_REQUIRE(max_workgroups >= 0, "scale_runs: negative max_workgroups (%d)", max_workgroups);
  if (n_blk == 0) return 0;
  const long grid = (max_workgroups > 0 && n_blk > max_workgroups) ? max_workgroups : n_blk;
  crct_launch(scale_runs_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g_f32, coef_dev, seg_off, seg_len, blk_seg,
              blk_off, (int)n_blk);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}
