// Masked-LM head (params['lm_loss_coeff'] > 0; vilbert.py:1016-1037, CrossEntropyLoss(ignore_index=-1) over the masked token rows): the
// bandwidth kernels around the three vocabulary-sized GEMMs, which run on the ordinary launcher from PADDED operands -- the vocabulary
// (30522 = 2 * 3 * 5087) is a multiple of neither 8 nor 64, so the feature owns a [Vp][H] bf16 copy of the word table (Vp = V rounded up to
// 64, pad rows zero), a padded bias, a compact [Rp][H] bf16 block of the R masked rows (Rp = R rounded up to 64, pad rows zero) and fp32
// logits [Rp][Vp].  Nothing here reads a pad COLUMN of the logits (the GEMM leaves 0 . z + 0 there, a caller anything), and every pad row
// and pad column of the gradient dL is written as +0, so the padded products equal the unpadded ones.
// Every kernel: vector loads and stores, no atomics, fixed summation order (bit-reproducible).
#include "common.hip.h"
#include "crct_internal.h"

namespace {

__device__ __forceinline__ uint4 pack8bf(const float4 a, const float4 b) {
  uint4 o;
  o.x = pack2bf(a.x, a.y); o.y = pack2bf(a.z, a.w); o.z = pack2bf(b.x, b.y); o.w = pack2bf(b.z, b.w);
  return o;
}

// dst[r][:] = bf16(src[rows[r]][:]) for r < R, +0 for R <= r < Rp.  One thread per 8 elements; H % 8 == 0.
__global__ __launch_bounds__(256) void lm_gather_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ rows,
                                                             bf16_t* __restrict__ dst, int R, int Rp, int H) {
  const int h8 = H >> 3;
  const long n = (long)Rp * h8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / h8), c = (int)(i - (long)r * h8) * 8;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (r < R) {
      const float* s = src + (long)rows[r] * H + c;
      o = pack8bf(*reinterpret_cast<const float4*>(s), *reinterpret_cast<const float4*>(s + 4));
    }
    *reinterpret_cast<uint4*>(dst + (long)r * H + c) = o;
  }
}

// dst[rows[r]][:] = src[r][:] for r < R (fp32, distinct rows: plain stores).  One thread per 4 elements; H % 4 == 0.
__global__ __launch_bounds__(256) void lm_scatter_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ rows,
                                                              float* __restrict__ dst, int R, int H) {
  const int h4 = H >> 2;
  const long n = (long)R * h4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / h4), c = (int)(i - (long)r * h4) * 4;
    *reinterpret_cast<float4*>(dst + (long)rows[r] * H + c) = *reinterpret_cast<const float4*>(src + (long)r * H + c);
  }
}

// The padded table copy: dst [Vp][H] = src [V][H] (bf16), rows V .. Vp-1 zero.  One thread per 8 elements.
__global__ __launch_bounds__(256) void lm_pad_table_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int V, int Vp, int H) {
  const long n = (long)Vp * H / 8, live = (long)V * H / 8;      // H % 8 == 0: a group never straddles rows
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    *reinterpret_cast<uint4*>(dst + i * 8) = i < live ? *reinterpret_cast<const uint4*>(src + i * 8) : make_uint4(0u, 0u, 0u, 0u);
}
__global__ __launch_bounds__(256) void lm_pad_bias_kernel(const float* __restrict__ src, float* __restrict__ dst, int V, int Vp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Vp) dst[i] = i < V ? src[i] : 0.f;
}

// workgroup reductions over 4 waves in a fixed order; every thread gets the result
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// THE max / sum-of-exp sweep of one row per workgroup over the V real columns of its fp32 logits (ld % 4 == 0, rows 16-byte aligned): returns
// (m, s) = (max, sum exp(x - m)) in every thread; lse = m + logf(s).  Both row kernels below call it, so their lse agree to the bit.  Two
// sweeps of the row (122 KB at V = 30522: the second comes from L2).  each(value, column) sees every real column exactly once, in the first
// sweep, and has no part in m or s.
template <class F>
__device__ __forceinline__ float2 lm_row_max_sumexp(const float* __restrict__ x, int V, float* sh, F&& each) {
  const int v4 = (V + 3) >> 2;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < v4; i += 256) {
    const float4 a = *reinterpret_cast<const float4*>(x + 4 * i);      // 4 i + 3 < ld: the row's own pad columns at most
    const int c = 4 * i;
    m = fmaxf(m, a.x); each(a.x, c);
    if (c + 1 < V) { m = fmaxf(m, a.y); each(a.y, c + 1); }
    if (c + 2 < V) { m = fmaxf(m, a.z); each(a.z, c + 2); }
    if (c + 3 < V) { m = fmaxf(m, a.w); each(a.w, c + 3); }
  }
  m = block_max(m, sh);
  float s = 0.f;
  for (int i = threadIdx.x; i < v4; i += 256) {
    const float4 a = *reinterpret_cast<const float4*>(x + 4 * i);
    const int c = 4 * i;
    s += expf(a.x - m);
    if (c + 1 < V) s += expf(a.y - m);
    if (c + 2 < V) s += expf(a.z - m);
    if (c + 3 < V) s += expf(a.w - m);
  }
  s = block_sum(s, sh);
  return make_float2(m, s);
}

// Cross-entropy forward of one row per workgroup: lse = max + log(sum exp(x - max)), loss = lse - x[label].
__global__ __launch_bounds__(256) void lm_ce_fwd_kernel(const float* __restrict__ logits, long ld, const int32_t* __restrict__ labels,
                                                        float* __restrict__ loss, float* __restrict__ lse, int V) {
  __shared__ float sh[4];
  const int r = blockIdx.x;
  const float* x = logits + (long)r * ld;
  const float2 ms = lm_row_max_sumexp(x, V, sh, [](float, int) {});
  if (threadIdx.x == 0) {
    const float l = ms.x + logf(ms.y);
    lse[r] = l;
    loss[r] = l - x[labels[r]];
  }
}

// ---- top-k of a row.  The ORDER of the columns of one row: larger value first, then smaller column index, compared on ONE 64-bit integer
// key per column, (monotone key of the float bits) << 32 | ~column, larger key = earlier.  The 32-bit key flips the sign bit of a
// non-negative float and all bits of a negative one, so it is total on the non-NaN floats with -0 BELOW +0 (two distinct keys: torch.topk
// calls them equal); every NaN, whatever its sign and payload, gets the one key above +inf's, as in torch.topk.  No real column has key 0
// (the smallest, -inf's, is 0x007fffff << 32): 0 is the empty list entry.
typedef unsigned long long u64;
__device__ __forceinline__ u64 lm_order_key(float v, int col) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t k = (u & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
  return ((u64)k << 32) | (uint32_t)~(uint32_t)col;
}
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
  return ((u64)(uint32_t)dpp_i32<CTRL>((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)dpp_i32<CTRL>((int)(uint32_t)v);
}
__device__ __forceinline__ u64 lane_u64(u64 v, int lane) {
  return ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}
// the wave_max / wave_sum trees of common.hip.h on keys and counts: DPP inside the 16-lane rows, v_readlane across them; wave-uniform result
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
  v = umax64(v, dpp_u64<0xB1>(v));
  v = umax64(v, dpp_u64<0x4E>(v));
  v = umax64(v, dpp_u64<0x141>(v));
  v = umax64(v, dpp_u64<0x140>(v));
  return umax64(umax64(lane_u64(v, 0), lane_u64(v, 16)), umax64(lane_u64(v, 32), lane_u64(v, 48)));
}
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += dpp_i32<0xB1>(v);
  v += dpp_i32<0x4E>(v);
  v += dpp_i32<0x141>(v);
  v += dpp_i32<0x140>(v);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) + (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// compare-exchange of two list entries: the larger key ends in a
#define LM_CE(a, b) { const u64 hi_ = umax64(a, b), lo_ = (a) > (b) ? (b) : (a); (a) = hi_; (b) = lo_; }

// One workgroup per row r: the K first columns of the order above (ids, logprob = x - lse), lse -- the bits of lm_ce_fwd_kernel's, the sweep
// is shared -- and, with labels, the label's log-probability and its RANK = the number of real columns in front of it in the order.  A
// label outside [0, V) (the caller checks) gives NaN and rank V instead of a read outside the row.  Each thread keeps the K best keys of
// its columns in NAMED registers c0 >= c1 >= ... (an indexed array would live in scratch), filled by an unrolled compare-exchange insert
// behind one comparison with the list's last entry; then K rounds of wave arg-max, each popping the winner's list; the four waves' K
// winners through LDS; K rounds in wave 0.  Keys are distinct (the column is part of them), so every arg-max has one owner.
template <int K>
__global__ __launch_bounds__(256) void lm_topk_rows_kernel(const float* __restrict__ logits, long ld, const int32_t* __restrict__ labels,
                                                           int32_t* __restrict__ ids, float* __restrict__ logprob, float* __restrict__ lse,
                                                           float* __restrict__ label_logprob, int32_t* __restrict__ label_rank, int V) {
  static_assert(K == 1 || K == 5 || K == 8, "lm_topk_rows_kernel: K in {1, 5, 8}");
  __shared__ float sh[4];
  __shared__ u64 best[4 * 8];
  __shared__ int ahead[4];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = logits + (long)r * ld;
  int lab = -1;
  u64 lab_key = ~0ull;                                   // nothing is in front of it: no label, no count
  if (labels) {
    lab = labels[r];
    if ((unsigned)lab < (unsigned)V) lab_key = lm_order_key(x[lab], lab); else lab = -1;
  }
  u64 c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0;
  int n_ahead = 0;
  const float2 ms = lm_row_max_sumexp(x, V, sh, [&](float v, int col) {
    const u64 k = lm_order_key(v, col);
    n_ahead += k > lab_key ? 1 : 0;
    if constexpr (K == 1) {
      c0 = umax64(c0, k);
    } else if constexpr (K == 5) {
      if (k > c4) { c4 = k; LM_CE(c3, c4) LM_CE(c2, c3) LM_CE(c1, c2) LM_CE(c0, c1) }
    } else {
      if (k > c7) { c7 = k; LM_CE(c6, c7) LM_CE(c5, c6) LM_CE(c4, c5) LM_CE(c3, c4) LM_CE(c2, c3) LM_CE(c1, c2) LM_CE(c0, c1) }
    }
  });
  const float l = ms.x + logf(ms.y);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const u64 w = wave_max_u64(c0);
    if (c0 == w) { c0 = c1; c1 = c2; c2 = c3; c3 = c4; c4 = c5; c5 = c6; c6 = c7; c7 = 0; }
    if (lane == 0) best[wave * 8 + j] = w;
  }
  n_ahead = wave_sum_i32(n_ahead);
  if (lane == 0) ahead[wave] = n_ahead;
  __syncthreads();
  if (wave != 0) return;
  u64 cand = lane < 32 && (lane & 7) < K ? best[lane] : 0, mine = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const u64 w = wave_max_u64(cand);
    if (cand == w) cand = 0;
    if (lane == j) mine = w;
  }
  if (lane < K) {
    const int id = (int)~(uint32_t)mine;
    if ((unsigned)id < (unsigned)V) {                    // always, with V >= K: the K winners are real columns
      ids[(long)r * K + lane] = id;
      logprob[(long)r * K + lane] = x[id] - l;
    }
  }
  if (lane == 0) {
    lse[r] = l;
    if (labels) {
      label_logprob[r] = lab >= 0 ? x[lab] - l : __uint_as_float(0x7fc00000u);
      label_rank[r] = lab >= 0 ? (ahead[0] + ahead[1]) + (ahead[2] + ahead[3]) : V;
    }
  }
}
#undef LM_CE

// lm_loss = inv_n * sum_r loss[r]: one workgroup, thread t sums rows t, t + 256, ... in order, then the fixed tree
__global__ __launch_bounds__(256) void lm_loss_mean_kernel(const float* __restrict__ loss, float* __restrict__ out, int R, float inv_n) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < R; i += 256) s += loss[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = s * inv_n;
}

// dL[r][j] = (exp(x[r][j] - lse[r]) - [j == label[r]]) * (g * inv_n) as bf16 [Rp][ldd]; columns V .. Vp-1 and rows R .. Rp-1 are +0.
// One workgroup per row, one thread per 8 columns (Vp % 8 == 0, ld % 4 == 0, ldd % 8 == 0).  g: device scalar.
__global__ __launch_bounds__(256) void lm_ce_bwd_kernel(const float* __restrict__ logits, long ld, const int32_t* __restrict__ labels,
                                                        const float* __restrict__ lse, const float* __restrict__ g, float inv_n,
                                                        bf16_t* __restrict__ dL, long ldd, int R, int V, int Vp) {
  const int r = blockIdx.x;
  bf16_t* d = dL + (long)r * ldd;
  const int n8 = Vp >> 3;
  if (r >= R) {
    for (int i = threadIdx.x; i < n8; i += 256) *reinterpret_cast<uint4*>(d + 8 * i) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const float* x = logits + (long)r * ld;
  const float l = lse[r], sc = g[0] * inv_n;
  const int lab = labels[r];
  for (int i = threadIdx.x; i < n8; i += 256) {
    const int c = 8 * i;
    const float4 a = *reinterpret_cast<const float4*>(x + c), b = *reinterpret_cast<const float4*>(x + c + 4);
    const float in[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float p = expf(in[k] - l) - (c + k == lab ? 1.f : 0.f);
      o[k] = c + k < V ? p * sc : 0.f;
    }
    *reinterpret_cast<uint4*>(d + c) = pack8bf(make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7]));
  }
}

// dL[r][j] = bf16(c * g[r][j]) for r < R, j < V from fp32 g with row stride ldg, as bf16 [Rp][ldd]; columns V .. Vp-1 and rows R .. Rp-1 are
// +0: an upstream gradient on the scores in the form lm_ce_bwd_kernel leaves the loss's, so the same backward chain takes it.  Layout and
// threading as there (Vp % 8 == 0, ldg % 4 == 0, ldd % 8 == 0).  Nothing of g at or past column V of a row is read.  c: by value.
__global__ __launch_bounds__(256) void lm_scores_grad_pack_kernel(const float* __restrict__ g, long ldg, float c, bf16_t* __restrict__ dL, long ldd,
                                                                  int R, int V, int Vp) {
  const int r = blockIdx.x;
  bf16_t* d = dL + (long)r * ldd;
  const int n8 = Vp >> 3;
  if (r >= R) {
    for (int i = threadIdx.x; i < n8; i += 256) *reinterpret_cast<uint4*>(d + 8 * i) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const float* x = g + (long)r * ldg;
  for (int i = threadIdx.x; i < n8; i += 256) {
    const int col = 8 * i;
    float4 h[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int cc = col + 4 * k;
      if (cc + 3 < V) {
        h[k] = *reinterpret_cast<const float4*>(x + cc);
      } else {                                           // the group that holds column V (or lies past it): real columns one by one
        h[k].x = cc < V ? x[cc] : 0.f;
        h[k].y = cc + 1 < V ? x[cc + 1] : 0.f;
        h[k].z = cc + 2 < V ? x[cc + 2] : 0.f;
        h[k].w = 0.f;
      }
    }
    const float in[8] = {h[0].x, h[0].y, h[0].z, h[0].w, h[1].x, h[1].y, h[1].z, h[1].w};
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = col + k < V ? c * in[k] : 0.f;
    *reinterpret_cast<uint4*>(d + col) = pack8bf(make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7]));
  }
}

// dst[i] = (accumulate ? dst[i] : 0) + src[i], i < n (fp32; both 16-byte aligned): the first V rows of the decoder weight gradient's
// [Vp][H] scratch onto the word-table gradient, the first V column sums onto the bias gradient.  Nothing at or past n is touched.
__global__ __launch_bounds__(256) void lm_add_f32_kernel(float* __restrict__ dst, const float* __restrict__ src, long n, int accumulate) {
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 s = *reinterpret_cast<const float4*>(src + 4 * i);
    if (accumulate) {
      const float4 d = *reinterpret_cast<const float4*>(dst + 4 * i);
      s.x += d.x; s.y += d.y; s.z += d.z; s.w += d.w;
    }
    *reinterpret_cast<float4*>(dst + 4 * i) = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long j = 4 * n4 + threadIdx.x;
    dst[j] = (accumulate ? dst[j] : 0.f) + src[j];
  }
}

// dx = bf16(dy * gelu'(pre)) (bf16, n % 8 == 0): the GELU between the transform's Linear and its LayerNorm, whose backward is a row kernel
__global__ __launch_bounds__(256) void lm_gelu_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ pre, bf16_t* __restrict__ dx, long n) {
  const long n8 = n >> 3;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const uint4 a = *reinterpret_cast<const uint4*>(dy + 8 * i), p = *reinterpret_cast<const uint4*>(pre + 8 * i);
    const uint32_t av[4] = {a.x, a.y, a.z, a.w}, pv[4] = {p.x, p.y, p.z, p.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      o[k] = pack2bf(bf2f((bf16_t)(av[k] & 0xffff)) * gelu_erf_grad(bf2f((bf16_t)(pv[k] & 0xffff))),
                     bf2f((bf16_t)(av[k] >> 16)) * gelu_erf_grad(bf2f((bf16_t)(pv[k] >> 16))));
    *reinterpret_cast<uint4*>(dx + 8 * i) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

int stream_grid(long items) {      // one thread per item, at most 2048 workgroups (the rest by grid stride)
  long b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace

void crct_loss_mean(const float* loss, float* out, int R, float inv_n, hipStream_t s) {
  crct_launch(lm_loss_mean_kernel, dim3(1), dim3(256), 0, s, loss, out, R, inv_n);
}

extern "C" int crct_lm_gather_rows(const float* src, const int32_t* rows, void* dst_bf16, int R, int Rp, int H, crct_stream_t stream) {
  CRCT_REQUIRE(src && dst_bf16 && (rows || R == 0), "lm_gather_rows: null argument");
  CRCT_REQUIRE(R >= 0 && Rp >= R && Rp >= 1 && H >= 8 && H % 8 == 0, "lm_gather_rows: R=%d Rp=%d H=%d (0 <= R <= Rp, H a multiple of 8)", R, Rp, H);
  CRCT_REQUIRE(aligned16(src, dst_bf16), "lm_gather_rows: 16-byte aligned buffers");
  crct_launch(lm_gather_rows_kernel, dim3(stream_grid((long)Rp * (H / 8))), dim3(256), 0, (hipStream_t)stream, src, rows, (bf16_t*)dst_bf16, R, Rp, H);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_scatter_rows(const float* src, const int32_t* rows, float* dst, int R, int H, crct_stream_t stream) {
  CRCT_REQUIRE(R >= 0 && H >= 4 && H % 4 == 0, "lm_scatter_rows: R=%d H=%d (H a multiple of 4)", R, H);
  if (R == 0) return 0;
  CRCT_REQUIRE(src && rows && dst && aligned16(src, dst), "lm_scatter_rows: null or unaligned argument");
  crct_launch(lm_scatter_rows_kernel, dim3(stream_grid((long)R * (H / 4))), dim3(256), 0, (hipStream_t)stream, src, rows, dst, R, H);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_pad_operands(const void* table_bf16, const float* bias, void* table_pad, float* bias_pad, int V, int Vp, int H,
                                    crct_stream_t stream) {
  CRCT_REQUIRE(V >= 1 && Vp >= V && Vp % 64 == 0 && H >= 8 && H % 8 == 0, "lm_pad_operands: V=%d Vp=%d H=%d (Vp a multiple of 64 >= V, H a multiple of 8)", V, Vp, H);
  CRCT_REQUIRE((table_bf16 != nullptr) == (table_pad != nullptr) && (bias != nullptr) == (bias_pad != nullptr), "lm_pad_operands: a source without its copy");
  CRCT_REQUIRE(aligned16(table_bf16, table_pad), "lm_pad_operands: 16-byte aligned tables");
  if (table_bf16) crct_launch(lm_pad_table_kernel, dim3(stream_grid((long)Vp * H / 8)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)table_bf16, (bf16_t*)table_pad, V, Vp, H);
  if (bias) crct_launch(lm_pad_bias_kernel, dim3((Vp + 255) / 256), dim3(256), 0, (hipStream_t)stream, bias, bias_pad, V, Vp);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_ce_fwd(const float* logits, int64_t ld, const int32_t* labels, float* loss, float* lse, float* lm_loss, int R, int V,
                              float inv_n, crct_stream_t stream) {
  CRCT_REQUIRE(logits && labels && loss && lse, "lm_ce_fwd: null argument");
  CRCT_REQUIRE(R >= 1 && V >= 1 && ld >= (V + 3) / 4 * 4 && ld % 4 == 0 && aligned16(logits), "lm_ce_fwd: R=%d V=%d ld=%ld (ld a multiple of 4 covering V, 16-byte aligned rows)", R, V, (long)ld);
  crct_launch(lm_ce_fwd_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, labels, loss, lse, V);
  if (lm_loss) crct_loss_mean(loss, lm_loss, R, inv_n, (hipStream_t)stream);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_ce_bwd(const float* logits, int64_t ld, const int32_t* labels, const float* lse, const float* g, float inv_n,
                              void* dL_bf16, int64_t ldd, int R, int Rp, int V, int Vp, crct_stream_t stream) {
  CRCT_REQUIRE(logits && labels && lse && g && dL_bf16, "lm_ce_bwd: null argument");
  CRCT_REQUIRE(R >= 1 && Rp >= R && V >= 1 && Vp >= V && Vp % 8 == 0 && ld >= Vp && ld % 4 == 0 && ldd >= Vp && ldd % 8 == 0 && aligned16(logits, dL_bf16),
               "lm_ce_bwd: R=%d Rp=%d V=%d Vp=%d ld=%ld ldd=%ld (Vp a multiple of 8 covering V, both leading dimensions covering Vp)", R, Rp, V, Vp, (long)ld, (long)ldd);
  crct_launch(lm_ce_bwd_kernel, dim3(Rp), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, labels, lse, g, inv_n, (bf16_t*)dL_bf16, (long)ldd, R, V, Vp);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_add_f32(float* dst, const float* src, int64_t n, int accumulate, crct_stream_t stream) {
  if (n <= 0) return 0;
  CRCT_REQUIRE(dst && src && aligned16(dst, src), "lm_add_f32: null or unaligned argument");
  crct_launch(lm_add_f32_kernel, dim3(stream_grid((long)(n / 4))), dim3(256), 0, (hipStream_t)stream, dst, src, (long)n, accumulate);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_gelu_bwd(const void* dy, const void* pre, void* dx, int64_t n, crct_stream_t stream) {
  if (n <= 0) return 0;
  CRCT_REQUIRE(dy && pre && dx && n % 8 == 0 && aligned16(dy, pre, dx), "lm_gelu_bwd: n=%ld must be a multiple of 8 and the buffers 16-byte aligned", (long)n);
  crct_launch(lm_gelu_bwd_kernel, dim3(stream_grid((long)(n / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)pre, (bf16_t*)dx, (long)n);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_topk_rows(const float* logits, int64_t ld, const int32_t* labels, int32_t* ids, float* logprob, float* lse,
                                 float* label_logprob, int32_t* label_rank, int R, int V, int K, crct_stream_t stream) {
  CRCT_REQUIRE(K == 1 || K == 5 || K == 8, "lm_topk_rows: K=%d (1, 5 or 8)", K);
  CRCT_REQUIRE(R >= 0 && V >= K && ld >= (V + 3) / 4 * 4 && ld % 4 == 0, "lm_topk_rows: R=%d V=%d K=%d ld=%ld (V >= K, ld a multiple of 4 covering V)", R, V, K, (long)ld);
  if (R == 0) return 0;
  CRCT_REQUIRE(logits && ids && logprob && lse && aligned16(logits), "lm_topk_rows: null or unaligned argument");
  CRCT_REQUIRE(!labels || (label_logprob && label_rank), "lm_topk_rows: labels without label_logprob / label_rank");
  const hipStream_t st = (hipStream_t)stream;
  if (K == 1) crct_launch(lm_topk_rows_kernel<1>, dim3(R), dim3(256), 0, st, logits, (long)ld, labels, ids, logprob, lse, label_logprob, label_rank, V);
  else if (K == 5) crct_launch(lm_topk_rows_kernel<5>, dim3(R), dim3(256), 0, st, logits, (long)ld, labels, ids, logprob, lse, label_logprob, label_rank, V);
  else crct_launch(lm_topk_rows_kernel<8>, dim3(R), dim3(256), 0, st, logits, (long)ld, labels, ids, logprob, lse, label_logprob, label_rank, V);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_lm_scores_grad_pack(const float* g, int64_t ldg, float c, void* dL_bf16, int64_t ldd, int R, int Rp, int V, int Vp,
                                        crct_stream_t stream) {
  CRCT_REQUIRE(dL_bf16 && (g || R == 0), "lm_scores_grad_pack: null argument");
  CRCT_REQUIRE(R >= 0 && Rp >= R && Rp >= 1 && V >= 1 && Vp >= V && Vp % 8 == 0 && ldg >= V && ldg % 4 == 0 && ldd >= Vp && ldd % 8 == 0 && aligned16(g, dL_bf16),
               "lm_scores_grad_pack: R=%d Rp=%d V=%d Vp=%d ldg=%ld ldd=%ld (Vp a multiple of 8 covering V, ldg a multiple of 4 covering V, ldd covering Vp)",
               R, Rp, V, Vp, (long)ldg, (long)ldd);
  crct_launch(lm_scores_grad_pack_kernel, dim3(Rp), dim3(256), 0, (hipStream_t)stream, g, (long)ldg, c, (bf16_t*)dL_bf16, (long)ldd, R, V, Vp);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}
