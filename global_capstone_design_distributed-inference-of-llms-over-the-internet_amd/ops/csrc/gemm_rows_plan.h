// What the GEMMs above 64 rows that read a quantized weight in place share (gemm_w8_rows.hip: fp8,
// gemm_w4_rows.hip: MXFP4): the workgroup LDS budget, the geometry / column-split RULE of a shape and the
// blockIdx placement.  The rule is stated in gemm_w8_rows.hip's header; it counts column tiles and row
// blocks only, so it does not depend on the weight format.
#pragma once
#include "gemm_kernels.h"

namespace mp {

constexpr int W8R_LDS_BYTES = 160 * 1024;  // gemm_t2d.h's workgroup budget

// blockIdx -> (column group, row block), gemm_t2d.h's t2d_place without a k split: the MB row blocks of one
// column group share blockIdx % 8 (one XCD under round-robin dispatch) when the grid allows it.
// Placement only - never correctness.
__device__ __forceinline__ void w8r_place(int MB, int& cg, int& mb) {
  const int b = blockIdx.x, G = gridDim.x;
  if (G % (8 * MB) == 0) {
    const int j = b >> 3;
    mb = j % MB;
    cg = (j / MB) * 8 + (b & 7);
  } else {
    mb = b % MB;
    cg = b / MB;
  }
}

// The geometry and column split of a shape (the RULE of gemm_w8_rows.hip's header).  False: not covered.
struct W8rPlan {
  int wide, MB, NB, nbig, NBB, NBS;
};
// The rule for MB row blocks of a given geometry: what a kernel whose row blocks are not ceil(T / 128)
// (gemm_moe_tiled.hip: row-block slots of the experts) shares with the dense ones.
static bool w8r_plan_blocks(int MB, int wide, int N, int K, int epi, W8rPlan& p) {
  if (epi != 0 && epi != 1) return false;
  const int step = epi == 1 ? 2 : 1;
  if (MB <= 0 || N <= 0 || K <= 0 || N % (16 * step) || K % 128) return false;
  const int units = (N / 16) / step;
  p.wide = wide;
  const int cap = (p.wide ? 16 : 4) / step;  // units a workgroup can hold
  p.MB = MB;
  int want = sk_num_cus() / p.MB;            // groups for one workgroup per CU
  const int need = (units + cap - 1) / cap;
  if (want < need) want = need;
  p.NB = units < want ? units : want;
  if (p.NB > 8 && p.NB % 8) {  // whole XCD rounds (w8r_place)
    const int up = (p.NB + 7) / 8 * 8, down = p.NB / 8 * 8;
    if (up <= units) p.NB = up; else if (down >= need) p.NB = down;
  }
  const int base = units / p.NB, rem = units % p.NB;
  p.NBB = (base + (rem ? 1 : 0)) * step;
  p.NBS = base * step;
  p.nbig = rem ? rem : p.NB;
  return (int64_t)p.NB * p.MB < (1ll << 31);
}
static bool w8r_plan(int T, int N, int K, int epi, W8rPlan& p) {
  return T >= 65 && w8r_plan_blocks((T + 127) / 128, T > 128, N, K, epi, p);
}

}  // namespace mp
