// Device helpers shared by the MFMA attention kernels (attention_mfma.hip: short sequences, everything in registers;
// attention_long.hip: key-tile loop with online softmax; attention_probs.hip): v_mfma_f32_16x16x16_bf16 fragments out of row-major LDS
// images, the wave amax reduction and the saturating fp8 convert of the fp8 copies, LOG2E and the additive key term.
#pragma once
#include "common.hip.h"
#include "attention_args.h"

namespace {

typedef s4_t __attribute__((address_space(3))) * lds_s4_ptr;

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}


__device__ __forceinline__ f4_t mma16(s4_t a, s4_t b, f4_t c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }

// fragment X[r0 + (lane & 15)][c0 + 4 (lane >> 4) + e]: contraction along the image's columns
__device__ __forceinline__ s4_t frag_rows(const char* img, int stb, int r0, int c0, int lane) {
  return *reinterpret_cast<const s4_t*>(img + (r0 + (lane & 15)) * stb + (c0 + 4 * (lane >> 4)) * 2);
}
// fragment X[k0 + 4 (lane >> 4) + e][c0 + (lane & 15)]: contraction along the image's rows (transposed read;
// EXEC must be all ones, every lane supplies an in-bounds address)
__device__ __forceinline__ s4_t frag_cols(const char* img, int stb, int k0, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const char* addr = img + (k0 + 4 * g + q) * stb + (c0 + 4 * p) * 2;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(uintptr_t)(uint32_t)(uintptr_t)addr);
}
// result tile (rows 4g + r, col lane & 15) -> transposed into a row-major image: img[col][row0 + 4g .. + 3]
__device__ __forceinline__ void put_tile_t(char* img, int stb, int row_of_col0, int col_of_row0, f4_t v, int lane) {
  uint2 u;
  u.x = pack2bf(v[0], v[1]); u.y = pack2bf(v[2], v[3]);
  *reinterpret_cast<uint2*>(img + (row_of_col0 + (lane & 15)) * stb + (col_of_row0 + 4 * (lane >> 4)) * 2) = u;
}
__device__ __forceinline__ s4_t pack4(f4_t v) {
  uint2 u;
  u.x = pack2bf(v[0], v[1]); u.y = pack2bf(v[2], v[3]);
  return __builtin_bit_cast(s4_t, u);
}
__device__ __forceinline__ float xmax2(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xsum2(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// wave maximum of `am` into the amax slot of the workgroup (fp8 copies: CrctAttnQuant).  amax_wave is the DPP / v_readlane tree of
// common.hip.h: ALL 64 LANES MUST BE ACTIVE at the call (an inactive lane's value is undefined in a DPP read), so call it only
// under wave-uniform conditions and behind reconverged loops, as every caller does
__device__ __forceinline__ void wave_amax(float* dst, float am, int lane) {
  am = amax_wave(am);           // on bit patterns: a NaN reaches the words (common.hip.h)
  if (lane == 0) amax_update(dst, am);
}
// four values -> four fp8 bytes of f * qs (E4M3: OCP e4m3, else e5m2), saturated to the format's largest finite value; am <- max(am, |f|)
template <bool E4M3>
__device__ __forceinline__ uint32_t sat_cvt4(const float (&v)[4], float qs, float& am) {
  constexpr float LIM = E4M3 ? 448.f : 57344.f;
  float f[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { am = amax_join(am, v[r]); f[r] = fp8_sat(v[r] * qs, LIM); }
  uint32_t o = 0u;
  if constexpr (E4M3) {
    o = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], o, false);
    o = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], o, true);
  } else {
    o = __builtin_amdgcn_cvt_pk_bf8_f32(f[0], f[1], o, false);
    o = __builtin_amdgcn_cvt_pk_bf8_f32(f[2], f[3], o, true);
  }
  return o;
}

constexpr float LOG2E = 1.4426950408889634f;
// additive key term in the exp2 domain: 0 (attended), -10000 log2 e (masked), -inf (no such key: padding of the last tile)
__device__ __forceinline__ void load_keybias(float* kb, const uint8_t* km, int Tk, int n, int tid, int nthr) {
  for (int j = tid; j < n; j += nthr) kb[j] = j < Tk ? (km[j] ? 0.f : -10000.f * LOG2E) : -INFINITY;
}

// fragment X[r0 + (lane & 15)][c0 + 4 (lane >> 4) + e] straight from global memory (rows >= T read as zero)
__device__ __forceinline__ s4_t frag_rows_global(const bf16_t* src, long ld, int T, int r0, int c0, int lane) {
  const int r = r0 + (lane & 15);
  // unconditional load (last row for the padding rows) and a mask: no branch, the loads stay batched
  const uint2 u = *reinterpret_cast<const uint2*>(src + (long)min(r, T - 1) * ld + c0 + 4 * (lane >> 4));
  const uint32_t m = r < T ? 0xffffffffu : 0u;
  return __builtin_bit_cast(s4_t, make_uint2(u.x & m, u.y & m));
}

// fragment X[r0 + (lane & 15)][c0 + 4 (lane >> 4) + e] from global memory, for head sizes that are no multiple of 16; rows >= T and columns >= d read as zero (never touched)
__device__ __forceinline__ s4_t frag_rows_global_tail(const bf16_t* src, long ld, int T, int d, int r0, int c0, int lane) {
  const int r = r0 + (lane & 15), c = c0 + 4 * (lane >> 4);
  const bool ok = r < T && c < d;
  const uint2 u = *reinterpret_cast<const uint2*>(src + (long)min(r, T - 1) * ld + (c < d ? c : 0));
  const uint32_t m = ok ? 0xffffffffu : 0u;
  return __builtin_bit_cast(s4_t, make_uint2(u.x & m, u.y & m));
}

// Kernel-argument preload (gemm.hip, GEMM_HOT_PARAMS): what the first instructions need (operand pointers, sizes, leading dimensions) as 15
// leading scalar arguments -- gfx950 hands the first argument dwords to the wave in SGPRs; a struct passed by value is fetched by scalar loads.
#define ATTN_HOT_PARAMS const bf16_t* hq, const bf16_t* hk, const bf16_t* hv, const uint8_t* hkm, int hB, int hheads, int hTq, int hTk, int hldq, int hldk, int hldv, const AttnArgs a_in
#define ATTN_HOT_UNPACK AttnArgs a = a_in; a.q = hq; a.k = hk; a.v = hv; a.keymask = hkm; a.B = hB; a.heads = hheads; a.Tq = hTq; a.Tk = hTk; a.ldq = hldq; a.ldk = hldk; a.ldv = hldv;
#define ATTN_HOT_ARGS(a) (a).q, (a).k, (a).v, (a).keymask, (a).B, (a).heads, (a).Tq, (a).Tk, (int)(a).ldq, (int)(a).ldk, (int)(a).ldv,

}  // namespace
