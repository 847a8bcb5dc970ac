// fp8 KV cache: OCP e4m3 codes [pages, nkv, page, D] + one e8m0 scale byte per (token, kv head)
// [pages, nkv, page].  The row rule (ops/reference.py quant_kv_fp8): e = mx_e8m0(amax of the D bf16
// values), code = e4m3(x * 2^(127 - e)), value = code * 2^(e - 127) - exact in bf16, so the decode
// kernel's convert (v_cvt_scalef32_pk_bf16_fp8, scale operand e << 23) hands the bf16 arithmetic
// the very operands a bf16 cache of the dequantized values would.
#pragma once
#include "mx_common.h"

namespace mp {

typedef __attribute__((ext_vector_type(2))) unsigned kvf8x8;  // 8 codes = 8 consecutive head dims

// pointers of the scale tensors (null on a bf16 cache)
struct KvF8 {
  uint8_t* ks;
  uint8_t* vs;
};

// 8 codes x 2^(e - 127) -> 8 bf16 (exact)
__device__ __forceinline__ u16x8 kvf8_dequant8(kvf8x8 raw, unsigned e) {
  typedef __attribute__((ext_vector_type(2))) unsigned short u16x2_;
  const float sc = __uint_as_float(e << 23);
  u16x8 r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u16x2_ lo = __builtin_bit_cast(u16x2_, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[h], sc, false));
    const u16x2_ hi = __builtin_bit_cast(u16x2_, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[h], sc, true));
    r[4 * h + 0] = lo[0];
    r[4 * h + 1] = lo[1];
    r[4 * h + 2] = hi[0];
    r[4 * h + 3] = hi[1];
  }
  return r;
}

// 4 floats (already scaled; |x| <= 448 by the scale rule, clamped all the same) -> 4 e4m3 bytes, RNE
__device__ __forceinline__ unsigned kvf8_pack4(float a, float b, float c, float d) {
  a = fminf(fmaxf(a, -448.f), 448.f);
  b = fminf(fmaxf(b, -448.f), 448.f);
  c = fminf(fmaxf(c, -448.f), 448.f);
  d = fminf(fmaxf(d, -448.f), 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}

// max over groups of N consecutive, N-aligned lanes (N a power of two <= 64); valid in every lane
template <int N>
__device__ __forceinline__ float kvf8_group_max(float v) {
#pragma unroll
  for (int o = 1; o < N; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float kvf8_amax8(u16x8 x) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(bf2f(x[j])));
  return a;
}

// 8 bf16 of a row whose e8m0 exponent is e -> 8 codes
__device__ __forceinline__ kvf8x8 kvf8_quant8(u16x8 x, int e) {
  const float inv = mx_inv_scale(e);
  kvf8x8 r;
  r[0] = kvf8_pack4(bf2f(x[0]) * inv, bf2f(x[1]) * inv, bf2f(x[2]) * inv, bf2f(x[3]) * inv);
  r[1] = kvf8_pack4(bf2f(x[4]) * inv, bf2f(x[5]) * inv, bf2f(x[6]) * inv, bf2f(x[7]) * inv);
  return r;
}

}  // namespace mp
