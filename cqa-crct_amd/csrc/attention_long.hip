// MFMA attention for sequences beyond the 112 x 112 register-resident kernels of attention_mfma.hip: the reference's own PlotQA
// shape (config/plotqa.json:5-6: 124 text tokens x 44 visual elements; options.py:27 defaults to 256 tokens), up to
// CRCT_ATTN_MAX_LEN = 512 queries x 512 keys (the text position table of config/vilbert.json) at head sizes 32 / 48 / 64, and at head size 128 (the original
// ViLBERT config's visual stream and co-attention: 8 heads on 1024) for EVERY length 1 .. 512 -- the blocked kernels attn_fwd_blk /
// attn_bwd_blk further down ("head size 128"), the same tile steps over image blocks of 256 rows.  Same math, same -10000 additive key mask, same
// Philox element numbering (and therefore the same dropout masks) as attention.hip / attention_mfma.hip:
//   P = softmax(q k^T / sqrt(d) + (1 - keymask) * -10000) ; ctx = dropout(P) v
// Reference: BertSelfAttention.forward vilbert.py:392-412, BertImageSelfAttention :522-543, BertBiAttention :684-723.
//
// One workgroup of NW waves per (batch, head); the tile counts are RUN-TIME values (one instantiation per head size), the
// loops over 16-key / 16-query tiles keep a constant register footprint.
//
// Forward: K and V of the pair as row-major LDS images; a wave owns 16 queries at a time (Q fragments straight from global
// memory), sweeps the key tiles two at a time with an ONLINE softmax (running maximum m, running sum l, the context
// accumulator rescaled by exp2(m_old - m_new)) and divides by l at the end.  As in attention_mfma.hip the score tile is
// computed transposed (S^T = K Q^T): a lane owns one query and four consecutive keys per tile, its probabilities are the B
// operand of ctx^T = V^T P^T as they lie.
//
// Backward (q, k, v; and, when the caller kept them, the forward's output and row statistics -- see LSE below): Q, dO, K, V as LDS images (beyond 256 x 256 x 64: K, V for phase A and Q, dO
// in the same space for phase B, a wave's OWN tile straight from global memory), then
//   phase A, a wave per QUERY tile: sweep 1 over the key tiles gives the row statistics -- m, 1 / l and
//            delta_i = sum_j P_ij dP_ij, accumulated online like l -- and keeps the dropout bits of the tile row (4 bits per
//            lane and key tile); sweep 2 recomputes S^T and dP^T per key tile, dS^T = P^T (dP^T - delta) and accumulates
//            dq^T += K^T dS^T (dS^T is the B operand as it lies).  The statistics go to LDS.
//   phase B, a wave per KEY tile: for every query tile S^T, dP^T again, P and dS from the statistics; both tiles pass through
//            a 16 x 16 LDS tile of the wave (written from the accumulator layout, read back transposed) to become the B
//            operands of dv^T += dO^T Pd and dk^T += Q^T dS.
//   LSE (the forward wrote lse_i = log2 sum_j exp2(s_ij), and its output is still there -- the step engine keeps both): sweep 1 is
//            dropped.  P_ij = exp2(s_ij - lse_i) needs no running maximum, and delta_i = sum_j P_ij dP_ij = dO_i . O_i (with dropout
//            too: O = (mask o P / (1 - p)) V) is a d-element dot product per query.  A quarter of the kernel's instructions.
// Every output element is accumulated by ONE wave in a fixed order: no atomics, bit-reproducible.  The price is 9 d / 16 MFMAs
// per tile pair instead of the minimal 5 d / 16 -- on < 3 % of the step's arithmetic.
//
// Every TILE STEP of the backward's loops is written once, as a __device__ function on ND that attn_bwd_long and attn_bwd_blk call with the
// two resident images, the row offset of the tile within them (16 jt in the whole-image kernel, 16 jl within a block) and the GLOBAL tile
// indices (Philox, key bias, keep cache): stats_tile (sweep 1), dq_tile (sweep 2), store_dq; kv_tile (phase B), store_dkv.  None of them
// holds a workgroup barrier.  The kernels keep what differs: the LDS carve-up, load_image / load_block with every __syncthreads, the SHARE
// fragment sources, the rounds, the sweep direction and where the keep words of sweep 1 live.  On the host: one launcher (launch_kern), one
// rule for the dropout-bit cache (add_keep_cache).  STILL WRITTEN TWICE, change both: the forward's tile-pair step and epilogue
// (attn_fwd_long, attn_fwd_blk) -- as functions they cost attn_fwd_long<4, 8> 5 % at 512 x 512 -- and phase A's kept statistics (the
// `if constexpr (LSE)` blocks of the two backward kernels) -- as a function it moved h * d of attn_bwd_blk<8, 8, true> into 64-bit scalar
// arithmetic with more SGPR spills, 0.7 % at 512 x 512 (profiles/attention_long_refactor.txt).
#include "common.hip.h"
#include "crct_internal.h"
#include "attention_args.h"
#include "attention_tiles.hip.h"

namespace {

constexpr int SCR_STB = 48;                  // row stride of a wave's 16 x 16 bf16 transposition tile (32 B of data + 16)
constexpr int LDS_CAP = 160 * 1024;

// rows [T][16 * ND] bf16 (row stride ld) -> row-major LDS image of `rows` rows (rows >= T zero), all threads of the workgroup;
// four 16-byte loads in flight per thread (unconditional: a row past T re-reads row T - 1 and is masked to zero)
template <int ND>
__device__ __forceinline__ void load_image(char* img, const bf16_t* __restrict__ src, long ld, int T, int rows, int tid, int nthr) {
  constexpr int CPR = 2 * ND, STB = 32 * ND + 16;
  const int total = rows * CPR;
  for (int c0 = tid; c0 < total; c0 += 4 * nthr) {
    uint4 u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k * nthr, r = c / CPR, cc = (c - r * CPR) << 3;
      const uint32_t m = r < T ? 0xffffffffu : 0u;
      const uint4 t = *reinterpret_cast<const uint4*>(src + (long)min(r, T - 1) * ld + cc);
      u[k] = make_uint4(t.x & m, t.y & m, t.z & m, t.w & m);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k * nthr, r = c / CPR, cc = (c - r * CPR) << 3;
      if (c < total) *reinterpret_cast<uint4*>(img + r * STB + cc * 2) = u[k];
    }
  }
}
// the lane's 8 keep bits of the key-tile PAIR jp for query i (bit 4 u + r: key 16 (2 jp + u) + 4 g + r is kept): one Philox call, the
// numbering all three implementations share (attention_args.h, attn_keep8)
__device__ __forceinline__ uint32_t keep_byte(const AttnArgs& a, long bh, int i, int jp, int g) {
  uint32_t kb = 0xffu;
  if (a.thr && 32 * jp + 4 * g < a.Tk && i < a.Tq) kb = attn_keep8(a.seed, a.site, bh, a.Tq, a.Tk, i, jp, g, a.thr);
  return kb;
}
// Result tile t (lane: column `row` of the transposed product, its rows 4 g + r = columns col0 .. col0 + 3 of the row-major matrix)
// -> 8 bytes of bf16 to global memory, optionally with the fp8 copy of the bf16-rounded values (E4M3: OCP e4m3, else e5m2;
// saturating) and their running maximum in `am` (include/crct_hip.h CrctAttnQuant; same convention as attention_mfma.hip)
template <bool E4M3>
__device__ __forceinline__ void store_tile_t(bf16_t* dst, uint8_t* qdst, long ld, long row, int col0, f4_t t, const float* qscale, float& am) {
  const uint2 pk = make_uint2(pack2bf(t[0], t[1]), pack2bf(t[2], t[3]));
  *reinterpret_cast<uint2*>(dst + row * ld + col0) = pk;
  if (qdst) {
    const float f[4] = {bf2f((bf16_t)(pk.x & 0xffff)), bf2f((bf16_t)(pk.x >> 16)), bf2f((bf16_t)(pk.y & 0xffff)), bf2f((bf16_t)(pk.y >> 16))};
    *reinterpret_cast<uint32_t*>(qdst + row * ld + col0) = sat_cvt4<E4M3>(f, qscale[0], am);
  }
}

// LDS bytes: forward = K, V images of NKP = NK rounded up to 2 key tiles + the key bias; backward = Q, dO, K, V images (or, SHARE, one
// pair of images: K, V in phase A, Q, dO in phase B, in the same place) + row statistics (16 B per query) + key bias + one
// transposition tile per wave
inline size_t fwd_lds(int NK, int ND) { const int NKP = (NK + 1) & ~1; return (size_t)32 * NKP * (32 * ND + 16) + 64 * NKP; }
inline size_t bwd_lds(int NQ, int NK, int ND, int NW, bool share) {
  const int rows = share ? 2 * (NQ > NK ? NQ : NK) : 2 * (NQ + NK);      // image tiles of 16 rows
  return (size_t)16 * rows * (32 * ND + 16) + 256 * NQ + 64 * NK + (size_t)NW * 16 * SCR_STB;
}
// + the dropout bits of the whole score matrix, one byte per lane and tile pair (phase A writes, phase B reads): where it fits
inline size_t keep_cache_bytes(int NQ, int NK) { return (size_t)64 * NQ * NK; }

// ---------------------------------------------------------------------------------------------------------------- the tile steps
// Tile indices passed to the steps (it: query tile, jt: key tile) are GLOBAL (Philox, key bias of every key of the pair in `kbias`, keep cache);
// r0 is the row of the tile within the two images it is read from.  sc = scale log2 e; ds = 1 / (1 - p), 1 without dropout; bh = the (batch,
// head) pair of the workgroup.  Backward, where `cached`: keepc holds the dropout bits phase A parks for phase B, [NQ][NK][64 lanes].
// S^T and dP^T tiles of (key tile jt at row r0 of the K, V images, the wave's query fragments): s <- scores in the exp2 domain (scaled, key
// bias added), gp <- (dO v^T)^T, unscaled and before the dropout mask
template <int ND>
__device__ __forceinline__ void score_tiles(f4_t& s, f4_t& gp, int lane, float sc, const float* kbias, const char* Ks, const char* Vs, int r0,
                                            int jt, const s4_t (&qf)[ND], const s4_t (&of)[ND]) {
  constexpr int STB = 32 * ND + 16;
  s = f4_t{0.f, 0.f, 0.f, 0.f};
  gp = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < ND; ++ks) {
    s = mma16(frag_rows(Ks, STB, r0, 16 * ks, lane), qf[ks], s);
    gp = mma16(frag_rows(Vs, STB, r0, 16 * ks, lane), of[ks], gp);
  }
  const f4_t kb = *reinterpret_cast<const f4_t*>(kbias + 16 * jt + 4 * (lane >> 4));
#pragma unroll
  for (int r = 0; r < 4; ++r) s[r] = fmaf(s[r], sc, kb[r]);
}
// The lane's 4 keep bits of (query tile it, key tile jt) where phase A makes them: one Philox call per tile PAIR (kb8 carries the pair's
// byte from the even tile to the odd one; the caller walks the key tiles upwards from an even one), parked for phase B where `cached`
__device__ __forceinline__ uint32_t make_keep_nibble(const AttnArgs& a, long bh, int lane, uint8_t* keepc, bool cached, int NK, int it, int jt,
                                                     uint32_t& kb8) {
  if (!(jt & 1)) kb8 = keep_byte(a, bh, 16 * it + (lane & 15), jt >> 1, lane >> 4);
  const uint32_t nib = (kb8 >> (4 * (jt & 1))) & 0xfu;
  if (cached) keepc[(it * NK + jt) * 64 + lane] = (uint8_t)nib;
  return nib;
}
// Phase A sweep 1: row-statistics step of key tile jt -- m, l and dl = sum_j e_ij dP_ij accumulated online; returns the keep bits it made
template <int ND>
__device__ __forceinline__ uint32_t stats_tile(const AttnArgs& a, long bh, int lane, float sc, float ds, const float* kbias, uint8_t* keepc, bool cached,
                                               int NK, const char* Ks, const char* Vs, int r0, int it, int jt, const s4_t (&qf)[ND],
                                               const s4_t (&of)[ND], uint32_t& kb8, float& m, float& l, float& dl) {
  f4_t s, gp;
  score_tiles<ND>(s, gp, lane, sc, kbias, Ks, Vs, r0, jt, qf, of);
  const float cm = xmax2(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])));
  const float mn = fmaxf(m, cm);
  const float alpha = __builtin_amdgcn_exp2f(m - mn);
  const uint32_t nib = make_keep_nibble(a, bh, lane, keepc, cached, NK, it, jt, kb8);
  float ps = 0.f, pd = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float e = __builtin_amdgcn_exp2f(s[r] - mn);
    ps += e;
    pd = fmaf(e, ((nib >> r) & 1u) ? gp[r] * ds : 0.f, pd);
  }
  l = fmaf(l, alpha, ps);
  dl = fmaf(dl, alpha, pd);
  m = mn;
  return nib;
}
// Phase A sweep 2: dS^T = P^T (dP^T - delta) of key tile jt and dq^T += K^T dS^T.  The keep bits are sweep 1's (nib1) or, LSE (no sweep 1),
// made and parked here
template <int ND, bool LSE>
__device__ __forceinline__ void dq_tile(const AttnArgs& a, long bh, int lane, float sc, float ds, const float* kbias, uint8_t* keepc, bool cached, int NK,
                                        const char* Ks, const char* Vs, int r0, int it, int jt, const s4_t (&qf)[ND], const s4_t (&of)[ND],
                                        uint32_t nib1, uint32_t& kb8, float m, float inv, float delta, f4_t (&dq)[ND]) {
  constexpr int STB = 32 * ND + 16;
  f4_t s, gp;
  score_tiles<ND>(s, gp, lane, sc, kbias, Ks, Vs, r0, jt, qf, of);
  uint32_t nib = nib1;
  if constexpr (LSE) nib = make_keep_nibble(a, bh, lane, keepc, cached, NK, it, jt, kb8);
  f4_t dsv;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float p = __builtin_amdgcn_exp2f(s[r] - m) * inv;
    dsv[r] = p * ((((nib >> r) & 1u) ? gp[r] * ds : 0.f) - delta);
  }
  const s4_t dsb = pack4(dsv);
#pragma unroll
  for (int ct = 0; ct < ND; ++ct) dq[ct] = mma16(frag_cols(Ks, STB, r0, 16 * ct, lane), dsb, dq[ct]);      // dq^T[c][i]
}
// Output stores of phase A (row i < Tq: dq, scaled) and, below, phase B (row j < Tk: dv, dk scaled), with their e5m2 copies
template <int ND>
__device__ __forceinline__ void store_dq(const AttnArgs& a, int b, int h, int lane, int i, const f4_t (&dq)[ND], float& am) {
  constexpr int d = 16 * ND;
  const int g = lane >> 4;
#pragma unroll
  for (int ct = 0; ct < ND; ++ct)
    store_tile_t<false>(a.dq, a.dq_q, a.lddq, (long)b * a.Tq + i, h * d + 16 * ct + 4 * g, dq[ct] * a.scale, a.dq_qscale, am);
}
// Phase B: query tile `it` (at row r0 of the Q, dO images) for the wave's key tile jt (fragments kf, vf, key bias kb): S^T, dP^T, P and dS
// from the row statistics, the two transpositions through the wave's LDS tile, dv^T += dO^T Pd and dk^T += Q^T dS
template <int ND>
__device__ __forceinline__ void kv_tile(const AttnArgs& a, long bh, int lane, float sc, float ds, uint8_t* keepc, bool cached, int NK,
                                        const char* Qs, const char* Os, int r0, int it, int jt, const s4_t (&kf)[ND], const s4_t (&vf)[ND], f4_t kb,
                                        const float4* stats, char* scr, f4_t (&dv)[ND], f4_t (&dk)[ND]) {
  constexpr int STB = 32 * ND + 16;
  const int g = lane >> 4, i = 16 * it + (lane & 15);
  f4_t s = f4_t{0.f, 0.f, 0.f, 0.f}, gp = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < ND; ++ks) {
    s = mma16(kf[ks], frag_rows(Qs, STB, r0, 16 * ks, lane), s);
    gp = mma16(vf[ks], frag_rows(Os, STB, r0, 16 * ks, lane), gp);
  }
  const float4 st = stats[i];
  const uint32_t nib = cached ? keepc[(it * NK + jt) * 64 + lane] : (keep_byte(a, bh, i, jt >> 1, g) >> (4 * (jt & 1))) & 0xfu;
  f4_t pdv, dsv;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sc, kb[r]) - st.x) * st.y;
    const bool kp = (nib >> r) & 1u;
    pdv[r] = kp ? p * ds : 0.f;
    dsv[r] = p * ((kp ? gp[r] * ds : 0.f) - st.z);
  }
  // accumulator layout (query = column) -> [query][key] tile in LDS -> B operand of the products that contract over the queries
  put_tile_t(scr, SCR_STB, 0, 0, pdv, lane);
  wave_sync();
  const s4_t pf = frag_cols(scr, SCR_STB, 0, 0, lane);
  wave_sync();
  put_tile_t(scr, SCR_STB, 0, 0, dsv, lane);
  wave_sync();
  const s4_t sf = frag_cols(scr, SCR_STB, 0, 0, lane);
  wave_sync();
#pragma unroll
  for (int ct = 0; ct < ND; ++ct) {
    dv[ct] = mma16(frag_cols(Os, STB, r0, 16 * ct, lane), pf, dv[ct]);       // dv^T[c][j] += dO[i][c] Pd[i][j]
    dk[ct] = mma16(frag_cols(Qs, STB, r0, 16 * ct, lane), sf, dk[ct]);       // dk^T[c][j] += q[i][c] dS[i][j]
  }
}
template <int ND>
__device__ __forceinline__ void store_dkv(const AttnArgs& a, int b, int h, int lane, int j, const f4_t (&dv)[ND], const f4_t (&dk)[ND],
                                          float& am) {
  constexpr int d = 16 * ND;
  const int g = lane >> 4;
#pragma unroll
  for (int ct = 0; ct < ND; ++ct) {
    store_tile_t<false>(a.dv, a.dv_q, a.lddv, (long)b * a.Tk + j, h * d + 16 * ct + 4 * g, dv[ct], a.dkv_qscale, am);
    store_tile_t<false>(a.dk, a.dk_q, a.lddk, (long)b * a.Tk + j, h * d + 16 * ct + 4 * g, dk[ct] * a.scale, a.dkv_qscale, am);
  }
}

// ---------------------------------------------------------------------------------------------------------------- whole images resident
template <int ND, int NW>
__global__ __launch_bounds__(64 * NW) void attn_fwd_long(ATTN_HOT_PARAMS) {
  ATTN_HOT_UNPACK
  constexpr int STB = 32 * ND + 16, d = 16 * ND;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4, wv = tid >> 6;
  const int NQ = (a.Tq + 15) >> 4, NK = (a.Tk + 15) >> 4, NKP = (NK + 1) & ~1;
  const long bh = blockIdx.x;
  const int b = (int)(bh / a.heads), h = (int)(bh % a.heads);
  char* Ks = smem;
  char* Vs = Ks + 16 * NKP * STB;
  float* kbias = reinterpret_cast<float*>(Vs + 16 * NKP * STB);
  load_image<ND>(Ks, a.k + (long)b * a.Tk * a.ldk + h * d, a.ldk, a.Tk, 16 * NKP, tid, 64 * NW);
  load_image<ND>(Vs, a.v + (long)b * a.Tk * a.ldv + h * d, a.ldv, a.Tk, 16 * NKP, tid, 64 * NW);
  load_keybias(kbias, a.keymask + (long)b * a.Tk, a.Tk, 16 * NKP, tid, 64 * NW);
  __syncthreads();
  const float sc = a.scale * LOG2E, ds = a.thr ? a.dscale : 1.0f;
  const bf16_t* qg = a.q + (long)b * a.Tq * a.ldq + h * d;
  float am = 0.f;
  for (int it = wv; it < NQ; it += NW) {
    const int i = 16 * it + n;
    s4_t qf[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks) qf[ks] = frag_rows_global(qg, a.ldq, a.Tq, 16 * it, 16 * ks, lane);
    float m = -INFINITY, l = 0.f;
    f4_t o[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) o[ct] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int jt = 0; jt < NKP; jt += 2) {
      f4_t s[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        s[u] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < ND; ++ks) s[u] = mma16(frag_rows(Ks, STB, 16 * (jt + u), 16 * ks, lane), qf[ks], s[u]);      // S^T[j][i]
      }
      float cm = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f4_t kb = *reinterpret_cast<const f4_t*>(kbias + 16 * (jt + u) + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[u][r] = fmaf(s[u][r], sc, kb[r]); cm = fmaxf(cm, s[u][r]); }
      }
      const float mn = fmaxf(m, xmax2(cm));          // finite: key 16 jt exists
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      float ps = 0.f;
      s4_t pb[2];
      const uint32_t kb8 = keep_byte(a, bh, i, jt >> 1, g);          // jt is even: one call for the pair
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t nib = (kb8 >> (4 * u)) & 0xfu;
        f4_t p;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(s[u][r] - mn);
          ps += e;
          p[r] = ((nib >> r) & 1u) ? e * ds : 0.f;
        }
        pb[u] = pack4(p);
      }
      l = fmaf(l, alpha, ps);
      m = mn;
#pragma unroll
      for (int ct = 0; ct < ND; ++ct) {
        o[ct] = o[ct] * alpha;
#pragma unroll
        for (int u = 0; u < 2; ++u) o[ct] = mma16(frag_cols(Vs, STB, 16 * (jt + u), 16 * ct, lane), pb[u], o[ct]);        // ctx^T[c][i]
      }
    }
    const float lsum = xsum2(l);
    const float inv = 1.0f / lsum;
    if (i < a.Tq) {
#pragma unroll
      for (int ct = 0; ct < ND; ++ct)
        store_tile_t<true>(a.ctx, a.ctx_q, a.ldo, (long)b * a.Tq + i, h * d + 16 * ct + 4 * g, o[ct] * inv, a.ctx_qscale, am);
      if (a.lse && g == 0) a.lse[bh * a.Tq + i] = m + __builtin_amdgcn_logf(lsum);      // v_log_f32: log2
    }
  }
  if (a.ctx_q) wave_amax(a.ctx_qamax, am, lane);
}

// SHARE = false: all four images resident (up to 256 x 256 x 64) -- every fragment out of LDS.  SHARE = true (beyond that, up to 512 x 512 x 64):
// the images of the two phases share one space and a wave's OWN tile (q / dO in phase A, k / v in phase B) comes straight from global
// memory; costs the PlotQA-shaped step 0.27 ms (18.95 against 18.68) where both fit, hence only where it must.
template <int ND, int NW, bool SHARE, bool LSE>
__global__ __launch_bounds__(64 * NW) void attn_bwd_long(ATTN_HOT_PARAMS) {
  ATTN_HOT_UNPACK
  constexpr int STB = 32 * ND + 16, d = 16 * ND;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4, wv = tid >> 6;
  const int NQ = (a.Tq + 15) >> 4, NK = (a.Tk + 15) >> 4;
  const long bh = blockIdx.x;
  const int b = (int)(bh / a.heads), h = (int)(bh % a.heads);
  // SHARE: phase A reads K, V from LDS (every wave sweeps all key tiles) and its own q / dO fragments from global memory; phase B reads
  // Q, dO from LDS (every wave sweeps all query tiles) and its own k / v fragments from global memory; the images of the two phases
  // share the space: 2 x max(Tq, Tk) rows instead of 2 x (Tq + Tk) -- 512 x 512 x 64 fits the 160 KB exactly
  const int NX = NQ > NK ? NQ : NK;
  char* Ks = smem;
  char* Vs = Ks + 16 * (SHARE ? NX : NK) * STB;
  char* Qs = SHARE ? Ks : Vs + 16 * NK * STB;
  char* Os = SHARE ? Vs : Qs + 16 * NQ * STB;          // dO
  float4* stats = reinterpret_cast<float4*>(SHARE ? Vs + 16 * NX * STB : Os + 16 * NQ * STB);      // per query: m, 1 / l, delta
  float* kbias = reinterpret_cast<float*>(stats + 16 * NQ);
  char* scr = reinterpret_cast<char*>(kbias + 16 * NK) + wv * 16 * SCR_STB;
  // dropout bits of tile pair (it, jt) as phase A's lanes hold them -- the layout phase B needs them in (lane = query 16 it + n, keys
  // 16 jt + 4 g ..): one Philox call per lane and tile pair instead of two (~140 SIMD cycles a wave-call at 7 rounds:
  // tools/lab/philox_rate.hip; a fifth of this issue-bound kernel's instructions with dropout on)
  uint8_t* keepc = reinterpret_cast<uint8_t*>(kbias + 16 * NK) + NW * 16 * SCR_STB;
  const bf16_t* qg = a.q + (long)b * a.Tq * a.ldq + h * d;
  const bf16_t* og = a.dctx + (long)b * a.Tq * a.ldo + h * d;
  const bf16_t* kg = a.k + (long)b * a.Tk * a.ldk + h * d;
  const bf16_t* vg = a.v + (long)b * a.Tk * a.ldv + h * d;
  if constexpr (!SHARE) {
    load_image<ND>(Qs, qg, a.ldq, a.Tq, 16 * NQ, tid, 64 * NW);
    load_image<ND>(Os, og, a.ldo, a.Tq, 16 * NQ, tid, 64 * NW);
  }
  load_image<ND>(Ks, kg, a.ldk, a.Tk, 16 * NK, tid, 64 * NW);
  load_image<ND>(Vs, vg, a.ldv, a.Tk, 16 * NK, tid, 64 * NW);
  load_keybias(kbias, a.keymask + (long)b * a.Tk, a.Tk, 16 * NK, tid, 64 * NW);
  __syncthreads();
  const bool cached = a.keep_cache != 0;
  const float sc = a.scale * LOG2E, ds = a.thr ? a.dscale : 1.0f;
  float am_q = 0.f, am_kv = 0.f;
  // ---------------------------------------------------------------- phase A: statistics and dq of the wave's query tiles
  for (int it = wv; it < NQ; it += NW) {
    const int i = 16 * it + n;
    s4_t qf[ND], of[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks) {
      if constexpr (SHARE) {
        qf[ks] = frag_rows_global(qg, a.ldq, a.Tq, 16 * it, 16 * ks, lane);
        of[ks] = frag_rows_global(og, a.ldo, a.Tq, 16 * it, 16 * ks, lane);
      } else {
        qf[ks] = frag_rows(Qs, STB, 16 * it, 16 * ks, lane);
        of[ks] = frag_rows(Os, STB, 16 * it, 16 * ks, lane);
      }
    }
    float m = -INFINITY, l = 0.f, dl = 0.f;
    uint32_t kw[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};      // keep bits, 4 per key tile (up to 32 key tiles)
    if constexpr (LSE) {
      // the forward's statistics: m <- lse (then exp2(s - m) IS the probability: l = 1), delta from the forward's output
      const bf16_t* cg = a.ctx + ((long)b * a.Tq + min(i, a.Tq - 1)) * a.ldc + h * d + 4 * g;
#pragma unroll
      for (int ks = 0; ks < ND; ++ks) {
        const uint2 ov = *reinterpret_cast<const uint2*>(cg + 16 * ks);
        dl = fmaf(bf2f((bf16_t)(ov.x & 0xffff)), bf2f((bf16_t)of[ks][0]), dl);
        dl = fmaf(bf2f((bf16_t)(ov.x >> 16)), bf2f((bf16_t)of[ks][1]), dl);
        dl = fmaf(bf2f((bf16_t)(ov.y & 0xffff)), bf2f((bf16_t)of[ks][2]), dl);
        dl = fmaf(bf2f((bf16_t)(ov.y >> 16)), bf2f((bf16_t)of[ks][3]), dl);
      }
      // a query past Tq (padding of the last tile: q and dO rows are zero) gets m = +inf: its probabilities are exactly 0 whatever its scores
      m = i < a.Tq ? a.lse[bh * a.Tq + i] : INFINITY;
      l = 0.25f;                                   // xsum2 over the four lane groups below: 1
    }
#pragma unroll
    for (int jo = 0; jo < 4; ++jo) {
      if (!LSE && 8 * jo < NK) {
        uint32_t kwo = 0u, kb8 = 0xffu;
        const int je = min(8, NK - 8 * jo);
#pragma unroll 1
        for (int ji = 0; ji < je; ++ji) {
          const int jt = 8 * jo + ji;
          kwo |= stats_tile<ND>(a, bh, lane, sc, ds, kbias, keepc, cached, NK, Ks, Vs, 16 * jt, it, jt, qf, of, kb8, m, l, dl) << (4 * ji);
        }
        kw[jo] = kwo;
      }
    }
    const float inv = 1.0f / xsum2(l);
    const float delta = xsum2(dl) * inv;
    if (g == 0) stats[i] = make_float4(m, inv, delta, 0.f);
    f4_t dq[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) dq[ct] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jo = 0; jo < 4; ++jo) {
      if (8 * jo < NK) {
        const uint32_t kwo = kw[jo];
        uint32_t kb8 = 0xffu;
        const int je = min(8, NK - 8 * jo);
#pragma unroll 1
        for (int ji = 0; ji < je; ++ji) {
          const int jt = 8 * jo + ji;
          dq_tile<ND, LSE>(a, bh, lane, sc, ds, kbias, keepc, cached, NK, Ks, Vs, 16 * jt, it, jt, qf, of, (kwo >> (4 * ji)) & 0xfu, kb8, m, inv,
                           delta, dq);
        }
      }
    }
    if (i < a.Tq) store_dq<ND>(a, b, h, lane, i, dq, am_q);
  }
  if (a.dq_q) wave_amax(a.dq_qamax, am_q, lane);
  __syncthreads();                          // the statistics of every query tile are in LDS; every wave is done with the K, V images
  if constexpr (SHARE) {
    load_image<ND>(Qs, qg, a.ldq, a.Tq, 16 * NQ, tid, 64 * NW);
    load_image<ND>(Os, og, a.ldo, a.Tq, 16 * NQ, tid, 64 * NW);
    __syncthreads();
  }
  // ---------------------------------------------------------------- phase B: dv and dk of the wave's key tiles
  for (int jt = wv; jt < NK; jt += NW) {
    const int j = 16 * jt + n;
    s4_t kf[ND], vf[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks) {
      if constexpr (SHARE) {
        kf[ks] = frag_rows_global(kg, a.ldk, a.Tk, 16 * jt, 16 * ks, lane);
        vf[ks] = frag_rows_global(vg, a.ldv, a.Tk, 16 * jt, 16 * ks, lane);
      } else {
        kf[ks] = frag_rows(Ks, STB, 16 * jt, 16 * ks, lane);
        vf[ks] = frag_rows(Vs, STB, 16 * jt, 16 * ks, lane);
      }
    }
    const f4_t kb = *reinterpret_cast<const f4_t*>(kbias + 16 * jt + 4 * g);
    f4_t dv[ND], dk[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) { dv[ct] = f4_t{0.f, 0.f, 0.f, 0.f}; dk[ct] = f4_t{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
    for (int it = 0; it < NQ; ++it) kv_tile<ND>(a, bh, lane, sc, ds, keepc, cached, NK, Qs, Os, 16 * it, it, jt, kf, vf, kb, stats, scr, dv, dk);
    if (j < a.Tk) store_dkv<ND>(a, b, h, lane, j, dv, dk, am_kv);
  }
  if (a.dv_q || a.dk_q) wave_amax(a.dkv_qamax, am_kv, lane);
}

// ---------------------------------------------------------------------------------------------------------------- head size 128
// At d = 128 a row of an image is 272 B: the K and V images of 512 keys are 278 528 B against 163 840 B of LDS, so the resident images
// become BLOCKS of BLK_T = 16 tiles (256 rows; two images of a block: 139 264 B).  One pair of image slots serves the whole kernel (K, V
// blocks in the forward and in phase A, Q, dO blocks in phase B); a wave's OWN tile always comes straight from global memory, as in the
// SHARE form above.  The work is handed out in ROUNDS of NW tiles (round rd: wave wv owns tile rd NW + wv) and every round sweeps the blocks,
// its state in registers: the online-softmax m, l and the ctx^T accumulator in the forward; m, l, delta, then dq^T in phase A; dv^T, dk^T in
// phase B.  A block that is already resident is not loaded again, and successive sweeps run over the blocks in alternating directions, so
// with one block per side (up to 256 x 256) every image is loaded once and with two a sweep loads one block.  The order in which a tile's
// blocks are accumulated is a function of the shape alone: still one wave per output element, a fixed order, no atomics.
constexpr int BLK_T = 16;          // even: a key-tile pair never straddles two blocks
static_assert(CRCT_ATTN_MAX_LEN <= 2 * 16 * BLK_T, "phase A keeps the dropout bits of at most two key blocks (kw0, kw1)");

// LDS bytes: two image slots of min(tiles, BLK_T) tiles + key bias (forward: NK rounded up to a tile pair) [+ backward: row statistics,
// one transposition tile per wave]
inline size_t fwd_blk_lds(int NK, int ND) {
  const int NKP = (NK + 1) & ~1, RT = NKP < BLK_T ? NKP : BLK_T;
  return (size_t)32 * RT * (32 * ND + 16) + 64 * NKP;
}
inline size_t bwd_blk_lds(int NQ, int NK, int ND, int NW) {
  const int NX = NQ > NK ? NQ : NK, RT = NX < BLK_T ? NX : BLK_T;
  return (size_t)32 * RT * (32 * ND + 16) + 256 * NQ + 64 * NK + (size_t)NW * 16 * SCR_STB;
}

// the block `blk` of BLK_T tiles of two matrices (rows 256 blk .. of T; `tiles` tiles in all) becomes resident in the two image slots;
// every wave of the workgroup calls this at the same point (the barriers), `resident` is uniform
template <int ND>
__device__ __forceinline__ void load_block(char* img0, char* img1, const bf16_t* __restrict__ s0, long ld0, const bf16_t* __restrict__ s1, long ld1,
                                           int T, int tiles, int blk, int& resident, int tid, int nthr) {
  if (blk == resident) return;
  __syncthreads();                          // every wave is done with the block that leaves
  const int r0 = 16 * BLK_T * blk, rows = 16 * min(tiles - BLK_T * blk, BLK_T);
  load_image<ND>(img0, s0 + (long)r0 * ld0, ld0, T - r0, rows, tid, nthr);
  load_image<ND>(img1, s1 + (long)r0 * ld1, ld1, T - r0, rows, tid, nthr);
  __syncthreads();
  resident = blk;
}

template <int ND, int NW>
__global__ __launch_bounds__(64 * NW) void attn_fwd_blk(ATTN_HOT_PARAMS) {
  ATTN_HOT_UNPACK
  constexpr int STB = 32 * ND + 16, d = 16 * ND;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4, wv = tid >> 6;
  const int NQ = (a.Tq + 15) >> 4, NK = (a.Tk + 15) >> 4, NKP = (NK + 1) & ~1;
  const int NB = (NKP + BLK_T - 1) / BLK_T, RT = min(NKP, BLK_T);
  const long bh = blockIdx.x;
  const int b = (int)(bh / a.heads), h = (int)(bh % a.heads);
  char* Ks = smem;
  char* Vs = Ks + 16 * RT * STB;
  float* kbias = reinterpret_cast<float*>(Vs + 16 * RT * STB);
  load_keybias(kbias, a.keymask + (long)b * a.Tk, a.Tk, 16 * NKP, tid, 64 * NW);      // visible after load_block's barriers
  const float sc = a.scale * LOG2E, ds = a.thr ? a.dscale : 1.0f;
  const bf16_t* qg = a.q + (long)b * a.Tq * a.ldq + h * d;
  const bf16_t* kg = a.k + (long)b * a.Tk * a.ldk + h * d;
  const bf16_t* vg = a.v + (long)b * a.Tk * a.ldv + h * d;
  float am = 0.f;
  int resident = -1;
  const int rounds = (NQ + NW - 1) / NW;
#pragma unroll 1
  for (int rd = 0; rd < rounds; ++rd) {
    const int it = rd * NW + wv, i = 16 * it + n;
    const bool active = it < NQ;               // wave-uniform; an idle wave of the last round still meets the barriers
    s4_t qf[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks) qf[ks] = frag_rows_global(qg, a.ldq, a.Tq, active ? 16 * it : 0, 16 * ks, lane);
    float m = -INFINITY, l = 0.f;
    f4_t o[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) o[ct] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kk = 0; kk < NB; ++kk) {
      const int blk = (rd & 1) ? NB - 1 - kk : kk;
      load_block<ND>(Ks, Vs, kg, a.ldk, vg, a.ldv, a.Tk, NKP, blk, resident, tid, 64 * NW);
      if (!active) continue;
      const int je = min(NKP - BLK_T * blk, BLK_T);      // even
#pragma unroll 1
      for (int jl = 0; jl < je; jl += 2) {
        const int jt = BLK_T * blk + jl;
        f4_t s[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          s[u] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < ND; ++ks) s[u] = mma16(frag_rows(Ks, STB, 16 * (jl + u), 16 * ks, lane), qf[ks], s[u]);      // S^T[j][i]
        }
        float cm = -INFINITY;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f4_t kb = *reinterpret_cast<const f4_t*>(kbias + 16 * (jt + u) + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) { s[u][r] = fmaf(s[u][r], sc, kb[r]); cm = fmaxf(cm, s[u][r]); }
        }
        const float mn = fmaxf(m, xmax2(cm));          // finite: key 16 jt exists
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        float ps = 0.f;
        s4_t pb[2];
        const uint32_t kb8 = keep_byte(a, bh, i, jt >> 1, g);          // jt is even: one call for the pair
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const uint32_t nib = (kb8 >> (4 * u)) & 0xfu;
          f4_t p;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(s[u][r] - mn);
            ps += e;
            p[r] = ((nib >> r) & 1u) ? e * ds : 0.f;
          }
          pb[u] = pack4(p);
        }
        l = fmaf(l, alpha, ps);
        m = mn;
#pragma unroll
        for (int ct = 0; ct < ND; ++ct) {
          o[ct] = o[ct] * alpha;
#pragma unroll
          for (int u = 0; u < 2; ++u) o[ct] = mma16(frag_cols(Vs, STB, 16 * (jl + u), 16 * ct, lane), pb[u], o[ct]);        // ctx^T[c][i]
        }
      }
    }
    if (active) {
      const float lsum = xsum2(l);
      const float inv = 1.0f / lsum;
      if (i < a.Tq) {
#pragma unroll
        for (int ct = 0; ct < ND; ++ct)
          store_tile_t<true>(a.ctx, a.ctx_q, a.ldo, (long)b * a.Tq + i, h * d + 16 * ct + 4 * g, o[ct] * inv, a.ctx_qscale, am);
        if (a.lse && g == 0) a.lse[bh * a.Tq + i] = m + __builtin_amdgcn_logf(lsum);      // v_log_f32: log2
      }
    }
  }
  if (a.ctx_q) wave_amax(a.ctx_qamax, am, lane);
}

// (the second launch bound is the least number of waves per SIMD the kernel is compiled for: 2 at 4 waves, where two workgroups share a CU
// wherever their LDS fits, so a wave gets at most 256 registers; 1, the default, at 8 waves)
template <int ND, int NW, bool LSE>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void attn_bwd_blk(ATTN_HOT_PARAMS) {
  ATTN_HOT_UNPACK
  constexpr int STB = 32 * ND + 16, d = 16 * ND;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4, wv = tid >> 6;
  const int NQ = (a.Tq + 15) >> 4, NK = (a.Tk + 15) >> 4;
  const int NX = NQ > NK ? NQ : NK, RT = min(NX, BLK_T);
  const int NKB = (NK + BLK_T - 1) / BLK_T, NQB = (NQ + BLK_T - 1) / BLK_T;
  const long bh = blockIdx.x;
  const int b = (int)(bh / a.heads), h = (int)(bh % a.heads);
  char* I0 = smem;                          // K block (phase A), Q block (phase B)
  char* I1 = I0 + 16 * RT * STB;            // V block (phase A), dO block (phase B)
  float4* stats = reinterpret_cast<float4*>(I1 + 16 * RT * STB);      // per query: m, 1 / l, delta
  float* kbias = reinterpret_cast<float*>(stats + 16 * NQ);
  char* scr = reinterpret_cast<char*>(kbias + 16 * NK) + wv * 16 * SCR_STB;
  uint8_t* keepc = reinterpret_cast<uint8_t*>(kbias + 16 * NK) + NW * 16 * SCR_STB;      // as in attn_bwd_long
  const bf16_t* qg = a.q + (long)b * a.Tq * a.ldq + h * d;
  const bf16_t* og = a.dctx + (long)b * a.Tq * a.ldo + h * d;
  const bf16_t* kg = a.k + (long)b * a.Tk * a.ldk + h * d;
  const bf16_t* vg = a.v + (long)b * a.Tk * a.ldv + h * d;
  load_keybias(kbias, a.keymask + (long)b * a.Tk, a.Tk, 16 * NK, tid, 64 * NW);      // visible after load_block's barriers
  const bool cached = a.keep_cache != 0;
  const float sc = a.scale * LOG2E, ds = a.thr ? a.dscale : 1.0f;
  float am_q = 0.f, am_kv = 0.f;
  int resident = -1, sweep = 0;
  // ---------------------------------------------------------------- phase A: statistics and dq of the wave's query tile of the round
  const int rounds_q = (NQ + NW - 1) / NW;
#pragma unroll 1
  for (int rd = 0; rd < rounds_q; ++rd) {
    const int it = rd * NW + wv, i = 16 * it + n;
    const bool active = it < NQ;
    s4_t qf[ND], of[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks) {
      qf[ks] = frag_rows_global(qg, a.ldq, a.Tq, active ? 16 * it : 0, 16 * ks, lane);
      of[ks] = frag_rows_global(og, a.ldo, a.Tq, active ? 16 * it : 0, 16 * ks, lane);
    }
    float m = -INFINITY, l = 0.f, dl = 0.f;
    uint64_t kw0 = ~0ull, kw1 = ~0ull;      // keep bits of sweep 1 for sweep 2: 4 per key tile, one word per key block
    if constexpr (LSE) {
      // the forward's statistics: m <- lse (then exp2(s - m) IS the probability: l = 1), delta from the forward's output
      const bf16_t* cg = a.ctx + ((long)b * a.Tq + min(i, a.Tq - 1)) * a.ldc + h * d + 4 * g;
#pragma unroll
      for (int ks = 0; ks < ND; ++ks) {
        const uint2 ov = *reinterpret_cast<const uint2*>(cg + 16 * ks);
        dl = fmaf(bf2f((bf16_t)(ov.x & 0xffff)), bf2f((bf16_t)of[ks][0]), dl);
        dl = fmaf(bf2f((bf16_t)(ov.x >> 16)), bf2f((bf16_t)of[ks][1]), dl);
        dl = fmaf(bf2f((bf16_t)(ov.y & 0xffff)), bf2f((bf16_t)of[ks][2]), dl);
        dl = fmaf(bf2f((bf16_t)(ov.y >> 16)), bf2f((bf16_t)of[ks][3]), dl);
      }
      // a query past Tq (padding of the last tile: q and dO rows are zero) gets m = +inf: its probabilities are exactly 0 whatever its scores
      m = i < a.Tq ? a.lse[bh * a.Tq + i] : INFINITY;
      l = 0.25f;                                   // xsum2 over the four lane groups below: 1
    } else {
#pragma unroll 1
      for (int kk = 0; kk < NKB; ++kk) {
        const int blk = (sweep & 1) ? NKB - 1 - kk : kk;
        load_block<ND>(I0, I1, kg, a.ldk, vg, a.ldv, a.Tk, NK, blk, resident, tid, 64 * NW);
        if (!active) continue;
        const int je = min(NK - BLK_T * blk, BLK_T);
        uint64_t kwb = 0ull;
        uint32_t kb8 = 0xffu;
#pragma unroll 1
        for (int jl = 0; jl < je; ++jl)
          kwb |= (uint64_t)stats_tile<ND>(a, bh, lane, sc, ds, kbias, keepc, cached, NK, I0, I1, 16 * jl, it, BLK_T * blk + jl, qf, of, kb8, m, l,
                                          dl) << (4 * jl);
        if (blk == 0) kw0 = kwb; else kw1 = kwb;
      }
      ++sweep;
    }
    const float inv = 1.0f / xsum2(l);
    const float delta = xsum2(dl) * inv;
    if (active && g == 0) stats[i] = make_float4(m, inv, delta, 0.f);
    f4_t dq[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) dq[ct] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kk = 0; kk < NKB; ++kk) {
      const int blk = (sweep & 1) ? NKB - 1 - kk : kk;
      load_block<ND>(I0, I1, kg, a.ldk, vg, a.ldv, a.Tk, NK, blk, resident, tid, 64 * NW);
      if (!active) continue;
      const int je = min(NK - BLK_T * blk, BLK_T);
      const uint64_t kwb = blk == 0 ? kw0 : kw1;
      uint32_t kb8 = 0xffu;
#pragma unroll 1
      for (int jl = 0; jl < je; ++jl)
        dq_tile<ND, LSE>(a, bh, lane, sc, ds, kbias, keepc, cached, NK, I0, I1, 16 * jl, it, BLK_T * blk + jl, qf, of,
                         (uint32_t)(kwb >> (4 * jl)) & 0xfu, kb8, m, inv, delta, dq);
    }
    ++sweep;
    if (active && i < a.Tq) store_dq<ND>(a, b, h, lane, i, dq, am_q);
  }
  if (a.dq_q) wave_amax(a.dq_qamax, am_q, lane);
  // ---------------------------------------------------------------- phase B: dv and dk of the wave's key tile of the round
  // (load_block's first barrier: the statistics of every query tile are in LDS and every wave is done with the K, V block)
  resident = -1;
  const int rounds_k = (NK + NW - 1) / NW;
#pragma unroll 1
  for (int rd = 0; rd < rounds_k; ++rd) {
    const int jt = rd * NW + wv, j = 16 * jt + n;
    const bool active = jt < NK;
    s4_t kf[ND], vf[ND];
#pragma unroll
    for (int ks = 0; ks < ND; ++ks) {
      kf[ks] = frag_rows_global(kg, a.ldk, a.Tk, active ? 16 * jt : 0, 16 * ks, lane);
      vf[ks] = frag_rows_global(vg, a.ldv, a.Tk, active ? 16 * jt : 0, 16 * ks, lane);
    }
    f4_t dv[ND], dk[ND];
#pragma unroll
    for (int ct = 0; ct < ND; ++ct) { dv[ct] = f4_t{0.f, 0.f, 0.f, 0.f}; dk[ct] = f4_t{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
    for (int kk = 0; kk < NQB; ++kk) {
      const int blk = (rd & 1) ? NQB - 1 - kk : kk;
      load_block<ND>(I0, I1, qg, a.ldq, og, a.ldo, a.Tq, NQ, blk, resident, tid, 64 * NW);
      if (!active) continue;
      const f4_t kb = *reinterpret_cast<const f4_t*>(kbias + 16 * jt + 4 * g);
      const int ie = min(NQ - BLK_T * blk, BLK_T);
#pragma unroll 1
      for (int il = 0; il < ie; ++il)
        kv_tile<ND>(a, bh, lane, sc, ds, keepc, cached, NK, I0, I1, 16 * il, BLK_T * blk + il, jt, kf, vf, kb, stats, scr, dv, dk);
    }
    if (active && j < a.Tk) store_dkv<ND>(a, b, h, lane, j, dv, dk, am_kv);
  }
  if (a.dv_q || a.dk_q) wave_amax(a.dkv_qamax, am_kv, lane);
}

// ---------------------------------------------------------------------------------------------------------------- host
// every kernel of this file has one signature; NW waves per (batch, head)
using attn_kernel_t = void (*)(ATTN_HOT_PARAMS);
hipError_t launch_kern(attn_kernel_t kern, int NW, const AttnArgs& a, size_t lds, hipStream_t s) {
  const hipError_t e = crct_lds_limit(kern, lds > 64 * 1024 ? LDS_CAP : lds);
  if (e != hipSuccess) return e;
  if (a.ldq > 0x7fffffffL || a.ldk > 0x7fffffffL || a.ldv > 0x7fffffffL) return hipErrorInvalidValue;      // preloaded as 32-bit scalars
  crct_launch(kern, dim3(a.B * a.heads), dim3(64 * NW), lds, s, ATTN_HOT_ARGS(a) a);
  return hipGetLastError();
}
// Backward with dropout: the dropout-bit cache (keep_cache_bytes) joins the kernel's LDS where it fits and does not lower the number of
// workgroups a CU's 160 KB hold
inline void add_keep_cache(AttnArgs& a, size_t& lds, bool bwd, int NQ, int NK) {
  a.keep_cache = 0;
  if (bwd && a.thr && lds + keep_cache_bytes(NQ, NK) <= (size_t)LDS_CAP && LDS_CAP / (lds + keep_cache_bytes(NQ, NK)) == LDS_CAP / lds) {
    a.keep_cache = 1;
    lds += keep_cache_bytes(NQ, NK);
  }
}
// Waves per (batch, head).  Forward: 8 when there are at least 8 query tiles to hand out, else 4.  Backward: phase A hands out the query
// tiles, phase B the key tiles, so 8 waves only when BOTH sides have 8 tiles -- the co-attention shapes (124 x 44: 8 x 3 tiles) keep
// 3 of 8 waves busy in one of the two phases, and with thousands of (batch, head) pairs queued a CU is better filled by twice as many
// 4-wave workgroups (wave-slot utilisation 0.82 - 0.90 against 0.47 - 0.64; in the step the two are within noise: 19.00 against 19.03 ms)
inline int waves_for(bool bwd, int NQ, int NK) { return (bwd ? (NQ < NK ? NQ : NK) : NQ) >= 8 ? 8 : 4; }
// backward: four resident images where they fit, the shared image pair beyond (bwd_share)
inline bool bwd_share(int NQ, int NK, int ND, int NW) { return bwd_lds(NQ, NK, ND, NW, false) > (size_t)LDS_CAP; }
template <int ND, int NW>
attn_kernel_t bwd_long_kernel(bool share, bool lse) {
  if (lse) return share ? attn_bwd_long<ND, NW, true, true> : attn_bwd_long<ND, NW, false, true>;
  return share ? attn_bwd_long<ND, NW, true, false> : attn_bwd_long<ND, NW, false, false>;
}
template <bool BWD, int ND>
hipError_t launch_d(const AttnArgs& a_in, hipStream_t s) {
  AttnArgs a = a_in;
  const int NQ = (a.Tq + 15) >> 4, NK = (a.Tk + 15) >> 4;
  const int NW = waves_for(BWD, NQ, NK);
  const bool share = BWD && bwd_share(NQ, NK, ND, NW);
  size_t lds = BWD ? bwd_lds(NQ, NK, ND, NW, share) : fwd_lds(NK, ND);
  add_keep_cache(a, lds, BWD, NQ, NK);
  attn_kernel_t kern;
  if constexpr (BWD) {
    const bool lse = a.lse && a.ctx;      // the forward's statistics and output are at hand: no statistics sweep
    kern = NW == 8 ? bwd_long_kernel<ND, 8>(share, lse) : bwd_long_kernel<ND, 4>(share, lse);
  } else {
    kern = NW == 8 ? attn_fwd_long<ND, 8> : attn_fwd_long<ND, 4>;
  }
  return launch_kern(kern, NW, a, lds, s);
}
// head size 128: the blocked kernels, same wave counts and the same rule for the dropout-bit cache
template <bool BWD, int ND>
hipError_t launch_blk(const AttnArgs& a_in, hipStream_t s) {
  AttnArgs a = a_in;
  const int NQ = (a.Tq + 15) >> 4, NK = (a.Tk + 15) >> 4;
  const int NW = waves_for(BWD, NQ, NK);
  size_t lds = BWD ? bwd_blk_lds(NQ, NK, ND, NW) : fwd_blk_lds(NK, ND);
  if (lds > (size_t)LDS_CAP) return hipErrorInvalidValue;
  add_keep_cache(a, lds, BWD, NQ, NK);
  attn_kernel_t kern;
  if constexpr (BWD) {
    if (a.lse && a.ctx) kern = NW == 8 ? attn_bwd_blk<ND, 8, true> : attn_bwd_blk<ND, 4, true>;
    else kern = NW == 8 ? attn_bwd_blk<ND, 8, false> : attn_bwd_blk<ND, 4, false>;
  } else {
    kern = NW == 8 ? attn_fwd_blk<ND, 8> : attn_fwd_blk<ND, 4>;
  }
  return launch_kern(kern, NW, a, lds, s);
}
template <bool BWD>
hipError_t launch(const AttnArgs& a, hipStream_t s) {
  switch (a.d) {
    case 32: return launch_d<BWD, 2>(a, s);
    case 48: return launch_d<BWD, 3>(a, s);
    case 64: return launch_d<BWD, 4>(a, s);
    case 128: return launch_blk<BWD, 8>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

// Both directions must fit (the forward of a shape the backward cannot take is of no use to the step): head size 32 / 48 / 64 / 128
// and at most CRCT_ATTN_MAX_LEN queries and keys -- 512 x 512 x 64: forward 146 KB for the K, V images, backward exactly the 160 KB
// (two images + statistics + key bias + eight transposition tiles).  512 x 512 x 128 (row stride 272 B, blocks of 256 rows): forward
// 2 x 256 x 272 = 139 264 B of image slots + 2 048 B of key bias = 141 312 B; backward 139 264 + 8 192 (statistics) + 2 048 (key bias) +
// 8 x 768 (transposition tiles) = 155 648 B of the 163 840 -- every length 1 .. 512 fits, in both directions.
bool crct_attention_long_ok(int Tq, int Tk, int d) {
  if (!(d == 32 || d == 48 || d == 64 || d == 128) || Tq < 1 || Tk < 1 || Tq > CRCT_ATTN_MAX_LEN || Tk > CRCT_ATTN_MAX_LEN) return false;
  const int NQ = (Tq + 15) >> 4, NK = (Tk + 15) >> 4, ND = d / 16;
  if (d == 128) return bwd_blk_lds(NQ, NK, ND, waves_for(true, NQ, NK)) <= (size_t)LDS_CAP && fwd_blk_lds(NK, ND) <= (size_t)LDS_CAP;
  return bwd_lds(NQ, NK, ND, waves_for(true, NQ, NK), true) <= (size_t)LDS_CAP && fwd_lds(NK, ND) <= (size_t)LDS_CAP;
}
hipError_t crct_attention_long_fwd(const AttnArgs& a, hipStream_t s) { return launch<false>(a, s); }
hipError_t crct_attention_long_bwd(const AttnArgs& a, hipStream_t s) { return launch<true>(a, s); }
