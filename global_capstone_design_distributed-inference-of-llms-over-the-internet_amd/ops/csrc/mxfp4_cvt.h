// MXFP4 weight fragment -> bf16 MFMA B operand, shared by the W4A16 decode GEMM and dequantizer
// (gemm_w4.hip) and the W4A16 GEMM above 64 rows (gemm_w4_rows.hip).  The hardware convert applies the
// block scale; every product code x 2^(e - 127) is an exact bf16 value.
#pragma once
#include "common.h"

namespace mp {

// e2m1 fragment (dword ``d``: 8 codes in k order, low nibble first) x 2^(e - 127) -> bf16 MFMA B operand
__device__ __forceinline__ u16x8 f4w_to_bf16(unsigned d, float scale) {
  u16x8 r;
  const u16x2 p0 = __builtin_bit_cast(u16x2, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0));
  const u16x2 p1 = __builtin_bit_cast(u16x2, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1));
  const u16x2 p2 = __builtin_bit_cast(u16x2, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2));
  const u16x2 p3 = __builtin_bit_cast(u16x2, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3));
  r[0] = p0[0]; r[1] = p0[1]; r[2] = p1[0]; r[3] = p1[1];
  r[4] = p2[0]; r[5] = p2[1]; r[6] = p3[0]; r[7] = p3[1];
  return r;
}
__device__ __forceinline__ float e8m0_scale(unsigned sc, int s) {
  return __uint_as_float(((sc >> (8 * s)) & 0xffu) << 23);
}

}  // namespace mp
