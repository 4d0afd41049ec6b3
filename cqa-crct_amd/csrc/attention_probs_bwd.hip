// Backward of an attention map (attention_probs.hip): the map as a differentiable output of the training step.  With the upstream gradient
// G (fp32 [B][heads][Tq][Tk], contiguous) of the map M = keep / (1 - p) o P, P = softmax_2(q k^T scale log2e + key term), and a scalar c
// (the step's gradient scale):
//   dP = c G o keep / (1 - p) ;  delta_i = sum_j P_ij dP_ij ;  dS = P o (dP - delta)
//   dq[b, i, h d + x] = bf16(float(dq) + scale sum_j dS_ij k_jx)        dk[b, j, h d + x] = bf16(float(dk) + scale sum_i dS_ij q_ix)
// added onto the bf16 dq / dk that the layer's own attention backward wrote (accumulate = 0: the sum alone).  Same operands, shapes, exp2
// domain, fp32 constants, key term (0 attended, -10000 log2e masked, -inf ABSENT) and Philox numbering as crct_attention_probs, so P and
// keep are the very values the map carried.  No forward kernel stores probabilities, hence two kernels of their own:
//   * map_bwd_dq, a wave per QUERY tile (K of the (batch, head) pair as an LDS image, Q fragments from global memory, the layout of
//     attn_probs_kernel): sweep 1 over the key-tile pairs keeps m, l and dl = sum_j e_ij dP_ij online (attention_long.hip phase A),
//     sweep 2 recomputes S^T (same MFMAs, same order: same bits), forms dS^T = P^T (dP^T - delta) and accumulates dq^T += K^T dS^T (dS^T
//     rounded to bf16 is the B operand as it lies).  m, 1 / l, delta go to the caller's fp32 scratch [B][heads][Tq][3];
//   * map_bwd_dk, a wave per KEY tile (Q as an LDS image, K fragments from global memory): per query tile S^T again (the same operand
//     roles and order as in map_bwd_dq: the same bits), P and dS from the scratch statistics, dS through the wave's 16 x 16 LDS tile to
//     become the B operand of dk^T += Q^T dS (attention_long.hip phase B).
// Every output element is summed by ONE wave in a fixed order: no atomics, bit-reproducible.  Few (batch, head) pairs with many tiles
// are spread over up to `split` workgroups as in launch_probs (each loads its image itself).
// LDS at d = 128 (row stride 272 B) and 512 x 512: dq 512 x 272 + 2 048 = 141 312 B; dk 512 x 272 + 8 192 (statistics) + 4 x 768
// (transposition tiles) = 150 528 B of the 163 840.
#include "common.hip.h"
#include "crct_internal.h"
#include "attention_args.h"
#include "attention_tiles.hip.h"

namespace {

constexpr int NW = 4;
constexpr int SCR_STB = 48;          // row stride of a wave's 16 x 16 bf16 transposition tile (32 B of data + 16)

struct MapBwdArgs {
  const float* g;          // upstream gradient of the map
  float* stats;            // [B][heads][Tq][3]: m, 1 / l, delta
  bf16_t* dq; bf16_t* dk;
  int d, lddq, lddk;
  float scale, c;
  uint32_t thr; float dscale; uint32_t site; uint64_t seed;
  int vec;                 // the rows of G are 16-byte aligned: float4 loads
  int accumulate;
};

// rows [T][d] bf16 (row stride ld) -> row-major LDS image of `rows` rows: 16-byte chunks, 2 ND per row (a chunk beyond d or a row beyond T is
// zero; its load re-reads an in-bounds chunk)
template <int ND>
__device__ __forceinline__ void load_image_tail(char* img, const bf16_t* src, int ld, int T, int d, int rows, int tid) {
  constexpr int STB = 32 * ND + 16;
  const int total = rows * 2 * ND;
  for (int c = tid; c < total; c += 64 * NW) {
    const int r = c / (2 * ND), cc = (c - r * 2 * ND) << 3;
    const bool ok = r < T && cc < d;
    const uint4 t = *reinterpret_cast<const uint4*>(src + (long)min(r, T - 1) * ld + (cc < d ? cc : 0));
    const uint32_t m = ok ? 0xffffffffu : 0u;
    *reinterpret_cast<uint4*>(img + r * STB + cc * 2) = make_uint4(t.x & m, t.y & m, t.z & m, t.w & m);
  }
}
// G[i][j0 .. j0 + 3] of the lane's query row (`row` points at a row inside the matrix for every lane); 0 beyond Tq x Tk
__device__ __forceinline__ f4_t load_g4(const float* row, int j0, int Tk, bool rowok, int vec) {
  f4_t v = f4_t{0.f, 0.f, 0.f, 0.f};
  if (rowok && j0 < Tk) {
    if (vec) {          // Tk % 4 == 0: j0 < Tk means j0 + 3 < Tk
      v = *reinterpret_cast<const f4_t*>(row + j0);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j0 + r < Tk) v[r] = row[j0 + r];
    }
  }
  return v;
}
// dP of four keys: c G keep / (1 - p) (cds = c / (1 - p), c without dropout)
__device__ __forceinline__ f4_t dp_of(f4_t g4, uint32_t nib, float cds) {
  f4_t dp;
#pragma unroll
  for (int r = 0; r < 4; ++r) dp[r] = ((nib >> r) & 1u) ? g4[r] * cds : 0.f;
  return dp;
}
// result tile t (lane: row `row` of the row-major matrix, columns col0 .. col0 + 3) added onto / written over 8 bytes of bf16
__device__ __forceinline__ void store_tile_acc(bf16_t* dst, long ld, long row, int col0, f4_t t, int accumulate) {
  uint2* p = reinterpret_cast<uint2*>(dst + row * ld + col0);
  if (accumulate) {
    const uint2 o = *p;
    t[0] += bf2f((bf16_t)(o.x & 0xffff)); t[1] += bf2f((bf16_t)(o.x >> 16));
    t[2] += bf2f((bf16_t)(o.y & 0xffff)); t[3] += bf2f((bf16_t)(o.y >> 16));
  }
  *p = make_uint2(pack2bf(t[0], t[1]), pack2bf(t[2], t[3]));
}

template <int ND>
__global__ __launch_bounds__(64 * NW) void map_bwd_dq(const bf16_t* q, const bf16_t* k, const uint8_t* keymask, int B, int heads, int Tq, int Tk,
                                                      int ldq, int ldk, const MapBwdArgs a) {
  constexpr int STB = 32 * ND + 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4, wv = tid >> 6;
  const int NQ = (Tq + 15) >> 4, NKP = (((Tk + 15) >> 4) + 1) & ~1;
  const long bh = blockIdx.x;
  const int b = (int)(bh / heads), h = (int)(bh % heads), d = a.d;
  char* Ks = smem;
  float* kbias = reinterpret_cast<float*>(Ks + 16 * NKP * STB);
  load_image_tail<ND>(Ks, k + (long)b * Tk * ldk + h * d, ldk, Tk, d, 16 * NKP, tid);
  load_keybias(kbias, keymask + (long)b * Tk, Tk, 16 * NKP, tid, 64 * NW);
  __syncthreads();
  const float sc = a.scale * LOG2E, cds = a.thr ? a.c * a.dscale : a.c;
  const bf16_t* qg = q + (long)b * Tq * ldq + h * d;
  for (int it = blockIdx.y * NW + wv; it < NQ; it += NW * gridDim.y) {
    const int i = 16 * it + n;
    const bool rowok = i < Tq;
    s4_t qf[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks)
      qf[ks] = 16 * ks + 16 <= d ? frag_rows_global(qg, ldq, Tq, 16 * it, 16 * ks, lane) : frag_rows_global_tail(qg, ldq, Tq, d, 16 * it, 16 * ks, lane);
    const float* grow = a.g + ((long)bh * Tq + min(i, Tq - 1)) * Tk;
    // x (exp2 domain) and dP of the key-tile pair jt, jt + 1: ONE Philox call for the pair, none at all without dropout
    auto tiles = [&](int jt, f4_t (&s)[2], f4_t (&dp)[2]) {
      uint32_t kb8 = 0xffu;
      if (a.thr && 16 * jt + 4 * g < Tk && rowok) kb8 = attn_keep8(a.seed, a.site, bh, Tq, Tk, i, jt >> 1, g, a.thr);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        s[u] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < ND; ++ks) s[u] = mma16(frag_rows(Ks, STB, 16 * (jt + u), 16 * ks, lane), qf[ks], s[u]);      // S^T[j][i]
        const f4_t kb = *reinterpret_cast<const f4_t*>(kbias + 16 * (jt + u) + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[u][r] = fmaf(s[u][r], sc, kb[r]);
        dp[u] = dp_of(load_g4(grow, 16 * (jt + u) + 4 * g, Tk, rowok, a.vec), (kb8 >> (4 * u)) & 0xfu, cds);
      }
    };
    // ---- sweep 1: m, l and dl = sum_j e_ij dP_ij, online
    float m = -INFINITY, l = 0.f, dl = 0.f;
#pragma unroll 1
    for (int jt = 0; jt < NKP; jt += 2) {
      f4_t s[2], dp[2];
      tiles(jt, s, dp);
      float cm = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) cm = fmaxf(cm, s[u][r]);
      const float mn = fmaxf(m, xmax2(cm));          // finite: key 16 jt exists (a masked key carries -10000 log2e, not -inf)
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      float ps = 0.f, pd = 0.f;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(s[u][r] - mn);
          ps += e;
          pd = fmaf(e, dp[u][r], pd);
        }
      l = fmaf(l, alpha, ps);
      dl = fmaf(dl, alpha, pd);
      m = mn;
    }
    const float inv = 1.0f / xsum2(l);
    const float delta = xsum2(dl) * inv;
    if (g == 0 && rowok) {
      float* st = a.stats + (bh * Tq + i) * 3;
      st[0] = m; st[1] = inv; st[2] = delta;
    }
    // ---- sweep 2: dS^T = P^T (dP^T - delta), dq^T += K^T dS^T
    f4_t dq[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) dq[ct] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int jt = 0; jt < NKP; jt += 2) {
      f4_t s[2], dp[2];
      tiles(jt, s, dp);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        f4_t dsv;
#pragma unroll
        for (int r = 0; r < 4; ++r) dsv[r] = __builtin_amdgcn_exp2f(s[u][r] - m) * inv * (dp[u][r] - delta);
        const s4_t dsb = pack4(dsv);
#pragma unroll
        for (int ct = 0; ct < ND; ++ct) dq[ct] = mma16(frag_cols(Ks, STB, 16 * (jt + u), 16 * ct, lane), dsb, dq[ct]);      // dq^T[c][i]
      }
    }
    if (rowok) {
#pragma unroll
      for (int ct = 0; ct < ND; ++ct)
        if (16 * ct + 4 * g < d) store_tile_acc(a.dq, a.lddq, (long)b * Tq + i, h * d + 16 * ct + 4 * g, dq[ct] * a.scale, a.accumulate);
    }
  }
}

template <int ND>
__global__ __launch_bounds__(64 * NW) void map_bwd_dk(const bf16_t* q, const bf16_t* k, const uint8_t* keymask, int B, int heads, int Tq, int Tk,
                                                      int ldq, int ldk, const MapBwdArgs a) {
  constexpr int STB = 32 * ND + 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4, wv = tid >> 6;
  const int NQ = (Tq + 15) >> 4, NK = (Tk + 15) >> 4;
  const long bh = blockIdx.x;
  const int b = (int)(bh / heads), h = (int)(bh % heads), d = a.d;
  char* Qs = smem;
  float4* stats = reinterpret_cast<float4*>(Qs + 16 * NQ * STB);      // per query: m, 1 / l, delta
  char* scr = reinterpret_cast<char*>(stats + 16 * NQ) + wv * 16 * SCR_STB;
  load_image_tail<ND>(Qs, q + (long)b * Tq * ldq + h * d, ldq, Tq, d, 16 * NQ, tid);
  // a query past Tq (padding of the last tile: its q row is zero) gets m = +inf: its probabilities are exactly 0 whatever its scores
  for (int i = tid; i < 16 * NQ; i += 64 * NW) {
    const float* st = a.stats + (bh * Tq + min(i, Tq - 1)) * 3;
    stats[i] = i < Tq ? make_float4(st[0], st[1], st[2], 0.f) : make_float4(INFINITY, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const float sc = a.scale * LOG2E, cds = a.thr ? a.c * a.dscale : a.c;
  const bf16_t* kg = k + (long)b * Tk * ldk + h * d;
  const uint8_t* km = keymask + (long)b * Tk;
  for (int jt = blockIdx.y * NW + wv; jt < NK; jt += NW * gridDim.y) {
    const int j = 16 * jt + n, j0 = 16 * jt + 4 * g;
    s4_t kf[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks)
      kf[ks] = 16 * ks + 16 <= d ? frag_rows_global(kg, ldk, Tk, 16 * jt, 16 * ks, lane) : frag_rows_global_tail(kg, ldk, Tk, d, 16 * jt, 16 * ks, lane);
    f4_t kb;
#pragma unroll
    for (int r = 0; r < 4; ++r) kb[r] = j0 + r < Tk ? (km[j0 + r] ? 0.f : -10000.f * LOG2E) : -INFINITY;
    f4_t dk[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) dk[ct] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int it = 0; it < NQ; ++it) {
      const int i = 16 * it + n;
      const bool rowok = i < Tq;
      f4_t s = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < ND; ++ks) s = mma16(kf[ks], frag_rows(Qs, STB, 16 * it, 16 * ks, lane), s);      // S^T[j][i]
      const float4 st = stats[i];
      uint32_t nib = 0xfu;
      if (a.thr && 32 * (jt >> 1) + 4 * g < Tk && rowok) nib = (attn_keep8(a.seed, a.site, bh, Tq, Tk, i, jt >> 1, g, a.thr) >> (4 * (jt & 1))) & 0xfu;
      const f4_t dp = dp_of(load_g4(a.g + ((long)bh * Tq + min(i, Tq - 1)) * Tk, j0, Tk, rowok, a.vec), nib, cds);
      f4_t dsv;
#pragma unroll
      for (int r = 0; r < 4; ++r) dsv[r] = __builtin_amdgcn_exp2f(fmaf(s[r], sc, kb[r]) - st.x) * st.y * (dp[r] - st.z);
      // accumulator layout (query = column) -> [query][key] tile in LDS -> B operand of the product that contracts over the queries
      put_tile_t(scr, SCR_STB, 0, 0, dsv, lane);
      wave_sync();
      const s4_t sf = frag_cols(scr, SCR_STB, 0, 0, lane);
      wave_sync();
#pragma unroll
      for (int ct = 0; ct < ND; ++ct) dk[ct] = mma16(frag_cols(Qs, STB, 16 * it, 16 * ct, lane), sf, dk[ct]);      // dk^T[c][j] += q[i][c] dS[i][j]
    }
    if (j < Tk) {
#pragma unroll
      for (int ct = 0; ct < ND; ++ct)
        if (16 * ct + 4 * g < d) store_tile_acc(a.dk, a.lddk, (long)b * Tk + j, h * d + 16 * ct + 4 * g, dk[ct] * a.scale, a.accumulate);
    }
  }
}

inline size_t dq_lds(int Tk, int ND) {
  const int NKP = (((Tk + 15) >> 4) + 1) & ~1;
  return (size_t)16 * NKP * (32 * ND + 16) + (size_t)64 * NKP;
}
inline size_t dk_lds(int Tq, int ND) {
  const int NQ = (Tq + 15) >> 4;
  return (size_t)16 * NQ * (32 * ND + 16) + (size_t)256 * NQ + (size_t)NW * 16 * SCR_STB;
}
// few (batch, head) pairs with many tiles: the tiles of a pair are spread over up to `split` workgroups (each loads its image itself)
inline unsigned split_for(long pairs, int tiles) {
  const int groups = (tiles + NW - 1) / NW;
  int split = (int)((1024 + pairs - 1) / pairs);
  if (split > groups) split = groups;
  return (unsigned)(split < 1 ? 1 : split);
}

template <int ND>
hipError_t launch_map_bwd(const bf16_t* q, const bf16_t* k, const uint8_t* km, int B, int heads, int Tq, int Tk, int ldq, int ldk, const MapBwdArgs& a,
                          hipStream_t s) {
  const long pairs = (long)B * heads;
  const size_t lq = dq_lds(Tk, ND), lk = dk_lds(Tq, ND);
  auto kq = map_bwd_dq<ND>;
  auto kk = map_bwd_dk<ND>;
  hipError_t e = crct_lds_limit(kq, lq > 64 * 1024 ? dq_lds(CRCT_ATTN_MAX_LEN, ND) : lq);
  if (e != hipSuccess) return e;
  e = crct_lds_limit(kk, lk > 64 * 1024 ? dk_lds(CRCT_ATTN_MAX_LEN, ND) : lk);
  if (e != hipSuccess) return e;
  crct_launch(kq, dim3((unsigned)pairs, split_for(pairs, (Tq + 15) >> 4)), dim3(64 * NW), lq, s, q, k, km, B, heads, Tq, Tk, ldq, ldk, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // same stream: the statistics of every query are in the scratch before the first key tile reads them
  crct_launch(kk, dim3((unsigned)pairs, split_for(pairs, (Tk + 15) >> 4)), dim3(64 * NW), lk, s, q, k, km, B, heads, Tq, Tk, ldq, ldk, a);
  return hipGetLastError();
}

}  // namespace

extern "C" int crct_attention_probs_bwd(const void* q, const void* k, const uint8_t* keymask, const float* d_probs, float c, void* dq, void* dk,
                                        float* scratch, int accumulate, int B, int heads, int Tq, int Tk, int d, int64_t ldq, int64_t ldk,
                                        int64_t lddq, int64_t lddk, uint32_t drop_thr, float drop_scale, uint32_t drop_site, uint64_t seed,
                                        crct_stream_t stream) {
  CRCT_REQUIRE(Tq >= 1 && Tk >= 1 && Tq <= CRCT_ATTN_MAX_LEN && Tk <= CRCT_ATTN_MAX_LEN, "attention_probs_bwd: Tq=%d Tk=%d must be in [1,%d]", Tq, Tk,
               CRCT_ATTN_MAX_LEN);
  CRCT_REQUIRE((d % 8 == 0 && d >= 8 && d <= 64) || d == 128, "attention_probs_bwd: head size %d must be a multiple of 8 in [8,64], or 128", d);
  CRCT_REQUIRE(B >= 0 && heads >= 0 && (int64_t)B * heads <= 0x7fffffffLL, "attention_probs_bwd: bad B=%d heads=%d", B, heads);
  CRCT_REQUIRE(dq && dk, "attention_probs_bwd: null dq / dk");
  CRCT_REQUIRE(q && k && keymask && d_probs, "attention_probs_bwd: null q / k / keymask / d_probs");
  CRCT_REQUIRE(scratch, "attention_probs_bwd: null statistics scratch (B * heads * Tq * 3 floats)");
  CRCT_REQUIRE(ldq >= (int64_t)heads * d && ldk >= (int64_t)heads * d && ldq % 8 == 0 && ldk % 8 == 0 && ldq <= 0x7fffffffLL && ldk <= 0x7fffffffLL,
               "attention_probs_bwd: leading dimensions ldq=%lld ldk=%lld must be multiples of 8, at least heads * d = %lld and below 2^31",
               (long long)ldq, (long long)ldk, (long long)heads * d);
  CRCT_REQUIRE(lddq >= (int64_t)heads * d && lddk >= (int64_t)heads * d && lddq % 4 == 0 && lddk % 4 == 0 && lddq <= 0x7fffffffLL && lddk <= 0x7fffffffLL,
               "attention_probs_bwd: leading dimensions lddq=%lld lddk=%lld must be multiples of 4, at least heads * d = %lld and below 2^31",
               (long long)lddq, (long long)lddk, (long long)heads * d);
  CRCT_REQUIRE(((uintptr_t)q | (uintptr_t)k) % 16 == 0 && ((uintptr_t)dq | (uintptr_t)dk) % 8 == 0 && ((uintptr_t)d_probs | (uintptr_t)scratch) % 4 == 0,
               "attention_probs_bwd: q / k must be 16-byte aligned, dq / dk 8-byte aligned, d_probs and the scratch 4-byte aligned");
  CRCT_REQUIRE(c - c == 0.f,"attention_probs_bwd: the scalar c must be finite");
  if (B * heads == 0) return 0;
  MapBwdArgs a = {};
  a.g = d_probs; a.stats = scratch; a.dq = (bf16_t*)dq; a.dk = (bf16_t*)dk;
  a.d = d; a.lddq = (int)lddq; a.lddk = (int)lddk;
  a.scale = 1.0f / sqrtf((float)d); a.c = c;
  a.thr = drop_thr; a.dscale = drop_scale; a.site = drop_site; a.seed = seed;
  a.vec = (Tk % 4 == 0 && (uintptr_t)d_probs % 16 == 0) ? 1 : 0;
  a.accumulate = accumulate ? 1 : 0;
  const bf16_t* qb = (const bf16_t*)q;
  const bf16_t* kb = (const bf16_t*)k;
  hipStream_t s = (hipStream_t)stream;
  switch ((d + 15) / 16) {
    case 1: CRCT_CHECK_HIP(launch_map_bwd<1>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    case 2: CRCT_CHECK_HIP(launch_map_bwd<2>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    case 3: CRCT_CHECK_HIP(launch_map_bwd<3>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    case 8: CRCT_CHECK_HIP(launch_map_bwd<8>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    default: CRCT_CHECK_HIP(launch_map_bwd<4>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
  }
  return 0;
}
