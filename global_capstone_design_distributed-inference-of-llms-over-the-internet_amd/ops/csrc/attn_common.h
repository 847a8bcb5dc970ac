// Device helpers of the decode attention kernels (attention.hip): DPP lane sums over a token's lane
// group, packed bf16 dot products, the fused RoPE of one 8-element chunk; and the split-K combine
// kernel every attention launcher ends in.
#pragma once
#include "common.h"

namespace mp {

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Sum over groups of LPT consecutive lanes (LPT in {8, 16}); result valid in every lane.
template <int LPT>
__device__ __forceinline__ float group_sum(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]  (xor 1)
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]  (xor 2)
  v += dpp_mov<0x141>(v);  // row_half_mirror      (8-lane total)
  if constexpr (LPT == 16) v += dpp_mov<0x140>(v);  // row_mirror (16-lane total)
  return v;
}

typedef __attribute__((ext_vector_type(4))) unsigned u32x4a;

// c + a.lo * b.lo + a.hi * b.hi over packed bf16 pairs (v_dot2c_f32_bf16: fp32 accumulate, no
// bf16 -> fp32 unpacking of either operand)
__device__ __forceinline__ float dot2bf(unsigned a, unsigned b, float c) {
  typedef __attribute__((ext_vector_type(2))) __bf16 v2bf;
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, a), __builtin_bit_cast(v2bf, b), c, false);
}

// x * cos -/+ partner * sin for one 8-element chunk of a head (lo: the chunk is in the first
// half, its partner in the second), rounded to bf16 - the fused RoPE of the decode kernels.
__device__ __forceinline__ u16x8 rope8(u16x8 me, u16x8 ot, f32x4 ca, f32x4 cb, f32x4 sa, f32x4 sb, bool lo) {
  u16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float c = j < 4 ? ca[j] : cb[j - 4], s = j < 4 ? sa[j] : sb[j - 4];
    const float x = bf2f(me[j]), y = bf2f(ot[j]);
    r[j] = lo ? f2bf(x * c - y * s) : f2bf(x * c + y * s);
  }
  return r;
}

// The decode kernels' small geometry arguments, packed into two kernel-argument dwords so that they
// fit, with the cache / block-table / context pointers, into the 14 leading dwords that kernarg
// preload delivers in SGPRs (docs/KERNARG_PRELOAD.md): every one of them is on the address chain of
// a wave's first K / V load.
//   heads: nkv | nh << 16          geom: PS / 64 | page_log2 << 12 | NP << 17
// (PS, the context-slice length, is a multiple of 64 in every decode launcher)
constexpr int ATTN_PK_NKV_BITS = 16, ATTN_PK_NH_BITS = 16;
constexpr int ATTN_PK_PS_BITS = 12, ATTN_PK_PLOG_BITS = 5, ATTN_PK_NP_BITS = 15;
static_assert(ATTN_PK_NKV_BITS + ATTN_PK_NH_BITS == 32, "heads dword");
static_assert(ATTN_PK_PS_BITS + ATTN_PK_PLOG_BITS + ATTN_PK_NP_BITS == 32, "geom dword");
static_assert(2048 / 64 < (1 << ATTN_PK_PS_BITS), "PS <= 2048 (mp_paged_attention) fits its field");
static_assert(31 < (1 << ATTN_PK_PLOG_BITS), "any int page size's log2 fits its field");
struct AttnPacked {
  unsigned heads, geom;
};
// false when a value does not fit its field (the launcher then returns an error: never truncated)
inline bool attn_pack(int nkv, int nh, int PS, int page_log2, int NP, AttnPacked& pk) {
  auto fits = [](int v, int bits) { return v >= 0 && v < (1 << bits); };
  if (!fits(nkv, ATTN_PK_NKV_BITS) || !fits(nh, ATTN_PK_NH_BITS) || PS % 64 ||
      !fits(PS / 64, ATTN_PK_PS_BITS) || !fits(page_log2, ATTN_PK_PLOG_BITS) || !fits(NP, ATTN_PK_NP_BITS))
    return false;
  pk.heads = (unsigned)nkv | (unsigned)nh << ATTN_PK_NKV_BITS;
  pk.geom = (unsigned)(PS / 64) | (unsigned)page_log2 << ATTN_PK_PS_BITS |
            (unsigned)NP << (ATTN_PK_PS_BITS + ATTN_PK_PLOG_BITS);
  return true;
}
__device__ __forceinline__ int attn_pk_nkv(unsigned heads) { return (int)(heads & ((1u << ATTN_PK_NKV_BITS) - 1)); }
__device__ __forceinline__ int attn_pk_nh(unsigned heads) { return (int)(heads >> ATTN_PK_NKV_BITS); }
__device__ __forceinline__ int attn_pk_ps(unsigned geom) {
  return (int)(geom & ((1u << ATTN_PK_PS_BITS) - 1)) * 64;
}
__device__ __forceinline__ int attn_pk_page_log2(unsigned geom) {
  return (int)(geom >> ATTN_PK_PS_BITS & ((1u << ATTN_PK_PLOG_BITS) - 1));
}
__device__ __forceinline__ int attn_pk_np(unsigned geom) {
  return (int)(geom >> (ATTN_PK_PS_BITS + ATTN_PK_PLOG_BITS));
}

// Combine split-K partials (defined in attention.hip; launched by all three attention launchers when NP > 1)
__global__ void paged_attn_reduce_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                         bf16_t* __restrict__ out, int NP, int D, int nh, int packed_mt);

}  // namespace mp
