// What the tiled grouped MoE launches share (gemm_moe_tiled.hip: W8A16, gemm_moe_tiled_mx.hip: W8A8-MX): the
// shape gate, the row-block SLOTS of the experts and the blockIdx order knob.  gemm_moe_tiled.hip's header
// states the slot rule.
#pragma once
#include <cstdlib>

#include "gemm_rows_plan.h"

namespace mp {

constexpr int MT_MAX_E = 32;
constexpr int MT_MAX_PAIRS = 1 << 16;
constexpr int MT_BM = 128;  // rows of a slot

// slot -> expert e, first pair p0 and rows n (1 .. 128) of its block.  False: past the last real block.
// Every range is clamped to [0, P], so whatever off[] holds, p0 + n <= P.
__device__ __forceinline__ bool mt_slot(const int32_t* __restrict__ off, int E, int P, int slot, int& e, int& p0,
                                        int& n) {
  int first = 0;
  for (e = 0; e < E; ++e) {
    const int lo = __builtin_amdgcn_readfirstlane(max(off[e], 0));
    const int hi = __builtin_amdgcn_readfirstlane(min(off[e + 1], P));
    const int nb = hi > lo ? (hi - lo + MT_BM - 1) / MT_BM : 0;
    if (slot < first + nb) {
      p0 = lo + (slot - first) * MT_BM;
      n = min(MT_BM, hi - p0);
      return true;
    }
    first += nb;
  }
  return false;
}

static bool tiled_shape_ok(int T, int E, int k, int H, int F) {
  return T >= 65 && E > 0 && E <= MT_MAX_E && k > 0 && k <= E && (int64_t)T * k <= MT_MAX_PAIRS && H > 0 && F > 0 &&
         H % 128 == 0 && F % 128 == 0;
}

// blockIdx order of the GEMM launches (gemm_moe_tiled.hip header, Placement): a lab knob, read once
static int tiled_order() {
  static const int order = [] {
    const char* s = std::getenv("MPAMD_MOE_TILED_ORDER");
    return s != nullptr && s[0] == '1' ? 1 : 0;
  }();
  return order;
}

}  // namespace mp
