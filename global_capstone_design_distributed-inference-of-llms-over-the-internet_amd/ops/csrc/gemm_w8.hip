// W8A16 decode GEMM entry point (fp8 weights dequantized into the bf16 MFMA; kernels:
// gemm_kernels.h, F8 = true instantiations).
#include "gemm_kernels.h"

// W8A16 decode GEMM: fp8 (e4m3) weights in the bf16 fragment order at 1 byte per element
// (Wq[N/16][K/32][64][8], per-output-column scales wsc[N]), packed bf16 activations, M <= 64.
// flags: GEMM_OUT_PACKED, GEMM_RING, GEMM_SPLITK (epilogue 0 / 3, needs ws), GEMM_PARTIALS, GEMM_ROT_K.
// Same epilogues / EpiArgs as mp_gemm_bf16.  Returns 1 when neither form covers the shape (nothing launched).
extern "C" int mp_gemm_w8(const mp::GemmArgs* args, hipStream_t stream) {
  (void)hipGetLastError();  // an earlier non-mpamd HIP call's stale error is not this launch's
  using namespace mp;
  const GemmArgs& a = *args;
  const int M = a.M, flags = a.flags;
  if (M == 0) return 0;
  if (M > 64 || a.K % (32 * GU_MAX) || a.N % 16 || a.wsc == nullptr) return -1;
  if (a.epilogue == 3 && (a.ap == nullptr || a.res == nullptr)) return -5;
  const EpiArgs ep = gemm_epi(a);
  int rc = 1;
  if ((flags & GEMM_SPLITK) && !(flags & GEMM_OUT_PACKED) && a.ws != nullptr) {
    rc = with_row_tiles(M, [&](auto mt) { return launch_gemm_rwk<mt(), true>(a, ep, stream, rwk_comb(flags)); });
    if (gemm_form_done(rc)) return rc;
  }
  if (flags & GEMM_PARTIALS) return -6;  // partials only: nothing else writes them
  rc = with_row_tiles(M, [&](auto mt) { return launch_gemm_rw<mt(), true>(a, ep, stream); });
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}
