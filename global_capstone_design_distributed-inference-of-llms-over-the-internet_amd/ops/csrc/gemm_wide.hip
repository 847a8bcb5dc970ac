// Decode GEMM for 65..256 rows (the packed decode path at 96..256 sessions): split-K ring (o,
// down) and balanced ring kernels at MT = 5..8, 12 and 16 (kernels: gemm_kernels.h), and the
// two-dimensionally tiled kernel (gemm_t2d.h, GEMM_T2D), which ops picks from ops.T2D_MIN
// (129) rows up: there the ring forms measured slower than hipBLASLt (profiles/r4d) and the tiled
// form faster (profiles/r5x).
#include "gemm_t2d.h"

// The instantiation that holds 65..256 rows: MT = 5, 6, 7, 8 row tiles, then 12 (129..192 rows)
// and 16; fn(integral_constant<MT>) as with_row_tiles.  Callers pass 65 <= M <= 256 only
// (mp_gemm_bf16 and mp_gemm_rw_ok check it): on that range this switch and the ``M <= 80 / 96 / 112 /
// 128 / 192`` chains it replaces agree; below 65 rows it would pick 16 where the chains picked 5.
template <class Fn>
static inline int with_row_tiles_wide(int M, Fn&& fn) {
  switch ((M + 15) / 16) {
    case 5: return fn(std::integral_constant<int, 5>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 7: return fn(std::integral_constant<int, 7>{});
    case 8: return fn(std::integral_constant<int, 8>{});
    case 9: case 10: case 11: case 12: return fn(std::integral_constant<int, 12>{});
    default: return fn(std::integral_constant<int, 16>{});
  }
}

extern "C" int mp_gemm_bf16_wide(const mp::GemmArgs* args, const mp::EpiArgs& ep, hipStream_t stream) {
  using namespace mp;
  const GemmArgs& a = *args;
  const int M = a.M, flags = a.flags;
  int rc = 1;
  if (flags & GEMM_T2D) {  // two-dimensionally tiled form (gemm_t2d.h)
    rc = launch_gemm_t2d(a, ep, stream, gemm_t2d_split(flags));
    if (rc == 1 && gemm_t2d_split(flags)) return -7;  // a forced split this shape does not take (lab)
    if (gemm_form_done(rc)) return rc;
  }
  if ((flags & GEMM_SPLITK) && !(flags & GEMM_OUT_PACKED) && a.ws != nullptr) {  // split-K ring
    rc = with_row_tiles_wide(M, [&](auto mt) { return launch_gemm_rwk<mt()>(a, ep, stream, rwk_comb(flags)); });
    if (gemm_form_done(rc)) return rc;
  }
  rc = with_row_tiles_wide(M, [&](auto mt) { return launch_gemm_rw<mt()>(a, ep, stream); });
  if (rc != 0) return rc < 0 ? rc : -1;
  return (int)hipGetLastError();
}

// 1 if the two-dimensionally tiled form covers this shape, with and without the LDS-DMA ring (no launch).
extern "C" int mp_gemm_t2d_ok(int M, int N, int K, int epilogue, int out_packed, int with_ws) {
  using namespace mp;
  char dummy = 0;
  GemmArgs a = gemm_shape_args(M, N, K, epilogue, GEMM_A_PACKED | (out_packed ? GEMM_OUT_PACKED : 0));
  a.ws = with_ws ? &dummy : nullptr;
  const EpiArgs ep = gemm_epi(a);
  if (launch_gemm_t2d(a, ep, 0, 0, true) != 0) return 0;
  a.flags |= GEMM_T2D_DMA;
  return launch_gemm_t2d(a, ep, 0, 0, true) == 0;
}

// 1 if mp_gemm_bf16 covers a packed-activation decode GEMM of M = 65..256 rows (balanced ring
// kernel: the widths built, epilogue 0 or packed SwiGLU), else 0.  No launch.
extern "C" int mp_gemm_rw_ok(int M, int N, int K, int epilogue, int out_packed) {
  using namespace mp;
  if (M <= 64 || M > 256 || K % (32 * GU_MAX) || N % 16) return 0;
  // the fused-norm producer (residual + packed copy + row statistics) at 65..256 rows runs as
  // the split-K ring + its reduce launch (the reduce applies the epilogue): o / down widths
  if (epilogue == 3) return !out_packed && N % 2048 == 0;
  const GemmArgs a =
      gemm_shape_args(M, N, K, epilogue, GEMM_A_PACKED | (out_packed ? GEMM_OUT_PACKED : 0) | GEMM_RING);
  const int rc = with_row_tiles_wide(M, [&](auto mt) { return launch_gemm_rw<mt()>(a, gemm_epi(a), 0, true); });
  return rc == 0;
}
