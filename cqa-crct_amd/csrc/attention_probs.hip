// The attention probabilities themselves, on request after a forward (the three attention implementations store none: their backward
// recomputes P).  What the reference hands out as attention maps (BertSelfAttention.forward vilbert.py:392-412 returns attention_probs,
// BertImageSelfAttention :522-543, BertBiAttention :684-723 attention_probs1 / 2):
//   P[b][h][i][j] = keep_ij / (1 - p) softmax_j(q_i . k_j / sqrt(d) + (1 - keymask[b][j]) * -10000)          fp32 [B][heads][Tq][Tk]
// Same operands as the forward kernels (bf16 column slices of fused buffers, head h at column h d), the same exp2 domain and fp32
// constants (scale log2e folded into one fma, the mask offset -10000.f * log2e), the same Philox numbering (attention_args.h attn_keep8):
// a map carries the very dropout mask its forward applied.
//
// ONE rule for every length up to CRCT_ATTN_MAX_LEN and every head size d % 8 == 0 up to 64, and 128 (ND = ceil(d / 16) contraction slices; the
// tail of a head size that is no multiple of 16 is zero-filled).  LDS is the K image and the key term: at d = 128 (row stride 272 B) and 512
// keys 512 x 272 + 2 048 = 141 312 B of the 163 840, so K stays one resident image at every length:
//   * a workgroup of NW = 4 waves belongs to one (batch, head): K as a row-major LDS image (rows beyond Tk and columns beyond d zero),
//     the additive key term as fp32 (0 attended, -10000 log2e masked, -inf ABSENT: the padding keys of the last tile pair are no keys);
//   * a wave owns 16 queries at a time (Q fragments straight from global memory) and computes S^T = K Q^T per 16-key tile, the forward's
//     orientation: a lane holds query (lane & 15), keys 16 jt + 4 g .. + 3 -- four consecutive floats of one output row;
//   * sweep 1 over the key-tile pairs: running maximum m and running sum l (online, as attention_long.hip's forward); sweep 2 recomputes
//     the scores (the same MFMAs in the same order: the same bits) and stores exp2(x - m) * (1 / l) [* 1 / (1 - p), or 0].  Two sweeps
//     instead of a 16 x Tk score strip in registers (128 VGPRs at 512 keys, and a register array a run-time tile count cannot index):
//     the footprint is constant, the second QK^T costs d / 8 MFMAs per 2 KB of output.
// Rounding: bf16 products accumulate in fp32 (MFMA), one fma into the exp2 domain, v_exp_f32, fp32 row sum, one fp32 reciprocal.
// Stores: 16 bytes per lane where the rows are 16-byte aligned (Tk % 4 == 0 and an aligned base), else dwords.
#include "common.hip.h"
#include "crct_internal.h"
#include "attention_args.h"
#include "attention_tiles.hip.h"

namespace {

constexpr int NW = 4;

#ifdef CRCT_PROBS_NT
#define PROBS_STORE(ptr, v) __builtin_nontemporal_store((v), (ptr))
#else
#define PROBS_STORE(ptr, v) (*(ptr) = (v))
#endif

struct ProbArgs {
  float* probs;
  int d;
  float scale;
  uint32_t thr; float dscale; uint32_t site; uint64_t seed;
  int vec;          // rows are 16-byte aligned: float4 stores
};

template <int ND>
__global__ __launch_bounds__(64 * NW) void attn_probs_kernel(const bf16_t* q, const bf16_t* k, const uint8_t* keymask, int B, int heads, int Tq,
                                                             int Tk, int ldq, int ldk, const ProbArgs a) {
  constexpr int STB = 32 * ND + 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4, wv = tid >> 6;
  const int NQ = (Tq + 15) >> 4, NKP = (((Tk + 15) >> 4) + 1) & ~1;
  const long bh = blockIdx.x;
  const int b = (int)(bh / heads), h = (int)(bh % heads), d = a.d;
  char* Ks = smem;
  float* kbias = reinterpret_cast<float*>(Ks + 16 * NKP * STB);
  {
    // K image: 16-byte chunks, 2 ND per row (a chunk beyond d or a row beyond Tk is zero; its load re-reads an in-bounds chunk)
    const bf16_t* kg = k + (long)b * Tk * ldk + h * d;
    const int total = 16 * NKP * 2 * ND;
    for (int c = tid; c < total; c += 64 * NW) {
      const int r = c / (2 * ND), cc = (c - r * 2 * ND) << 3;
      const bool ok = r < Tk && cc < d;
      const uint4 t = *reinterpret_cast<const uint4*>(kg + (long)min(r, Tk - 1) * ldk + (cc < d ? cc : 0));
      const uint32_t m = ok ? 0xffffffffu : 0u;
      *reinterpret_cast<uint4*>(Ks + r * STB + cc * 2) = make_uint4(t.x & m, t.y & m, t.z & m, t.w & m);
    }
    const uint8_t* km = keymask + (long)b * Tk;
    for (int j = tid; j < 16 * NKP; j += 64 * NW) kbias[j] = j < Tk ? (km[j] ? 0.f : -10000.f * LOG2E) : -INFINITY;
  }
  __syncthreads();
  const float sc = a.scale * LOG2E, ds = a.thr ? a.dscale : 1.0f;
  const bf16_t* qg = q + (long)b * Tq * ldq + h * d;
  for (int it = blockIdx.y * NW + wv; it < NQ; it += NW * gridDim.y) {
    const int i = 16 * it + n;
    s4_t qf[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks)
      qf[ks] = 16 * ks + 16 <= d ? frag_rows_global(qg, ldq, Tq, 16 * it, 16 * ks, lane) : frag_rows_global_tail(qg, ldq, Tq, d, 16 * it, 16 * ks, lane);
    // x of the key-tile pair jt, jt + 1 in the exp2 domain
    auto scores = [&](int jt, f4_t (&s)[2]) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        s[u] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < ND; ++ks) s[u] = mma16(frag_rows(Ks, STB, 16 * (jt + u), 16 * ks, lane), qf[ks], s[u]);      // S^T[j][i]
        const f4_t kb = *reinterpret_cast<const f4_t*>(kbias + 16 * (jt + u) + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[u][r] = fmaf(s[u][r], sc, kb[r]);
      }
    };
    // ---- sweep 1: row maximum and sum
    float m = -INFINITY, l = 0.f;
#pragma unroll 1
    for (int jt = 0; jt < NKP; jt += 2) {
      f4_t s[2];
      scores(jt, s);
      float cm = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) cm = fmaxf(cm, s[u][r]);
      const float mn = fmaxf(m, xmax2(cm));          // finite: key 16 jt exists (a masked key carries -10000 log2e, not -inf)
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) ps += __builtin_amdgcn_exp2f(s[u][r] - mn);
      l = fmaf(l, alpha, ps);
      m = mn;
    }
    const float w = (1.0f / xsum2(l)) * ds;
    // ---- sweep 2: the probabilities
    float* row = a.probs + ((long)bh * Tq + min(i, Tq - 1)) * Tk;
#pragma unroll 1
    for (int jt = 0; jt < NKP; jt += 2) {
      f4_t s[2];
      scores(jt, s);
      uint32_t kb8 = 0xffu;          // the lane's 8 keep bits of the pair: ONE Philox call, none at all without dropout
      if (a.thr && 16 * jt + 4 * g < Tk && i < Tq) kb8 = attn_keep8(a.seed, a.site, bh, Tq, Tk, i, jt >> 1, g, a.thr);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t nib = (kb8 >> (4 * u)) & 0xfu;
        const int j0 = 16 * (jt + u) + 4 * g;
        f4_t p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = ((nib >> r) & 1u) ? __builtin_amdgcn_exp2f(s[u][r] - m) * w : 0.f;
        if (i < Tq && j0 < Tk) {
          if (a.vec) {          // Tk % 4 == 0: j0 < Tk means j0 + 3 < Tk
            PROBS_STORE(reinterpret_cast<f4_t*>(row + j0), p);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (j0 + r < Tk) PROBS_STORE(row + j0 + r, p[r]);
          }
        }
      }
    }
  }
}

inline size_t probs_lds(int Tk, int ND) {
  const int NKP = (((Tk + 15) >> 4) + 1) & ~1;
  return (size_t)16 * NKP * (32 * ND + 16) + (size_t)64 * NKP;
}

template <int ND>
hipError_t launch_probs(const bf16_t* q, const bf16_t* k, const uint8_t* km, int B, int heads, int Tq, int Tk, int ldq, int ldk, const ProbArgs& a,
                        hipStream_t s) {
  const size_t lds = probs_lds(Tk, ND);
  auto kern = attn_probs_kernel<ND>;
  const hipError_t e = crct_lds_limit(kern, lds > 64 * 1024 ? probs_lds(CRCT_ATTN_MAX_LEN, ND) : lds);
  if (e != hipSuccess) return e;
  // few (batch, head) pairs with many query tiles: the tiles of a pair are spread over up to `split` workgroups (each loads K itself)
  const int NQ = (Tq + 15) >> 4, groups = (NQ + NW - 1) / NW;
  const long pairs = (long)B * heads;
  int split = (int)((1024 + pairs - 1) / pairs);
  if (split > groups) split = groups;
  if (split < 1) split = 1;
  crct_launch(kern, dim3((unsigned)pairs, (unsigned)split), dim3(64 * NW), lds, s, q, k, km, B, heads, Tq, Tk, ldq, ldk, a);
  return hipGetLastError();
}

}  // namespace

extern "C" int crct_attention_probs(const void* q, const void* k, const uint8_t* keymask, float* probs, int B, int heads, int Tq, int Tk, int d,
                                    int64_t ldq, int64_t ldk, uint32_t drop_thr, float drop_scale, uint32_t drop_site, uint64_t seed,
                                    crct_stream_t stream) {
  CRCT_REQUIRE(Tq >= 1 && Tk >= 1 && Tq <= CRCT_ATTN_MAX_LEN && Tk <= CRCT_ATTN_MAX_LEN, "attention_probs: Tq=%d Tk=%d must be in [1,%d]", Tq, Tk,
               CRCT_ATTN_MAX_LEN);
  CRCT_REQUIRE((d % 8 == 0 && d >= 8 && d <= 64) || d == 128, "attention_probs: head size %d must be a multiple of 8 in [8,64], or 128", d);
  CRCT_REQUIRE(B >= 0 && heads >= 0 && (int64_t)B * heads <= 0x7fffffffLL, "attention_probs: bad B=%d heads=%d", B, heads);
  CRCT_REQUIRE(probs, "attention_probs: null output");
  CRCT_REQUIRE(q && k && keymask, "attention_probs: null q / k / keymask");
  CRCT_REQUIRE(ldq >= (int64_t)heads * d && ldk >= (int64_t)heads * d && ldq % 8 == 0 && ldk % 8 == 0 && ldq <= 0x7fffffffLL && ldk <= 0x7fffffffLL,
               "attention_probs: leading dimensions ldq=%lld ldk=%lld must be multiples of 8, at least heads * d = %lld and below 2^31",
               (long long)ldq, (long long)ldk, (long long)heads * d);
  CRCT_REQUIRE(((uintptr_t)q | (uintptr_t)k) % 16 == 0 && (uintptr_t)probs % 4 == 0, "attention_probs: q / k must be 16-byte aligned, the output 4-byte aligned");
  if (B * heads == 0) return 0;
  ProbArgs a = {};
  a.probs = probs; a.d = d; a.scale = 1.0f / sqrtf((float)d);
  a.thr = drop_thr; a.dscale = drop_scale; a.site = drop_site; a.seed = seed;
  a.vec = (Tk % 4 == 0 && (uintptr_t)probs % 16 == 0) ? 1 : 0;
  const bf16_t* qb = (const bf16_t*)q;
  const bf16_t* kb = (const bf16_t*)k;
  hipStream_t s = (hipStream_t)stream;
  switch ((d + 15) / 16) {
    case 1: CRCT_CHECK_HIP(launch_probs<1>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    case 2: CRCT_CHECK_HIP(launch_probs<2>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    case 3: CRCT_CHECK_HIP(launch_probs<3>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    case 8: CRCT_CHECK_HIP(launch_probs<8>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
    default: CRCT_CHECK_HIP(launch_probs<4>(qb, kb, keymask, B, heads, Tq, Tk, (int)ldq, (int)ldk, a, s)); break;
  }
  return 0;
}
