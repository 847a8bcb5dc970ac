// Decode GEMM entry points, M <= 64 rows (bf16 weights), plus the weight / activation packers.
// The kernels live in gemm_kernels.h; 65..128 rows and fp8 weights are gemm_wide.hip and
// gemm_w8.hip (separate translation units: the build compiles them in parallel).
#include "gemm_kernels.h"

namespace mp {

// Pack W[N, K] (row-major) into the fragment-native layout Wp[N/16][K/32][64][8].
__global__ __launch_bounds__(256) void pack_weight_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ wp,
                                                          int N, int K) {
  const int nks = K >> 5;
  const int64_t total = (int64_t)(N >> 4) * nks * 64;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const int64_t tile = i >> 6;
    const int ks = (int)(tile % nks);
    const int64_t nt = tile / nks;
    const int c = lane & 15, q = lane >> 4;
    const u16x8 v = *reinterpret_cast<const u16x8*>(w + (nt * 16 + c) * (int64_t)K + ks * 32 + q * 8);
    *reinterpret_cast<u16x8*>(wp + i * 8) = v;
  }
}

}  // namespace mp

extern "C" int mp_gemm_ss_elems() { return mp::SS_NSH * mp::SS_ROWS; }

// byte offset / size of the split-K partial-slab region inside the GEMM workspace (shared with
// the fp8 split-K kernel, fp8.hip)
extern "C" int64_t mp_gemm_slab_offset() { return mp::RWK_SLAB_OFFSET; }
extern "C" int64_t mp_gemm_slab_bytes() { return mp::RWK_SLAB_BYTES; }

// Split count S of the split-K ring form for this shape (0: not covered): with GEMM_PARTIALS the
// GEMM leaves S fp32 partial slabs [S][M][N] at mp_gemm_slab_offset() of the workspace for a
// consumer that sums them (fixed order s = 0..S-1 from zero: the reduce launch's bits).
extern "C" int mp_gemm_rwk_split(int M, int N, int K, int f8) {
  using namespace mp;
  if (M < 1 || M > 128 || N % 2048 || K % 128) return 0;
  int nt, S;
  // the same width bound launch_gemm_rwk<MT, F8> uses, so a consumer of the partial slabs sees the
  // split count the launch picks
  const int nt_max = rwk_nt_max(M);
  // f8 == 2: the MX form (gemm_mx.hip), whose ring steps are 128 deep
  rwk_choose(N / 16, f8 == 2 ? K / 128 : K / 32, sk_num_cus(), f8 != 0, nt, S, nt_max);
  if (f8 == 2 && nt) mx_geometry(N / 16, nt, S);
  if (nt == 0 || (int64_t)S * M * N * 4 > RWK_SLAB_BYTES) return 0;
  return S;
}

extern "C" int64_t mp_gemm_workspace_bytes() { return mp::RWK_SLAB_OFFSET + mp::RWK_SLAB_BYTES; }

// bf16 weights, M <= 256 rows (flags: GemmFlags, mp_api.h).  The forms are tried in this order; one
// that does not cover the shape hands on to the next, the one-group kernel covers what is left.
extern "C" int mp_gemm_bf16(const mp::GemmArgs* args, hipStream_t stream) {
  (void)hipGetLastError();  // an earlier non-mpamd HIP call's stale error is not this launch's
  using namespace mp;
  const GemmArgs& a = *args;
  const int M = a.M;
  int flags = a.flags, rc;
  if (M == 0) return 0;
  if (a.epilogue == 3 && (a.ap == nullptr || a.res == nullptr)) return -5;
  const EpiArgs ep = gemm_epi(a);
  if (M > 256 || a.K % (32 * GU_MAX) || a.N % 16 || (!(flags & GEMM_A_PACKED) && a.x_stride % 8)) return -1;
  if (M > 64) {  // 65..256 rows: gemm_wide.hip (split-K ring / balanced ring, packed A, no gate)
    if (!(flags & GEMM_A_PACKED) || a.gate != nullptr) return -1;
    return mp_gemm_bf16_wide(args, ep, stream);
  }
  const bool apk = flags & GEMM_A_PACKED, plain = !(flags & GEMM_OUT_PACKED) && a.gate == nullptr;
  if (apk && (flags & GEMM_ROW_SPLIT) && plain) {  // row-split ring
    switch ((M + 15) / 16) {
      case 2: rc = launch_gemm_rwr<2>(a, ep, stream); break;
      case 4: rc = launch_gemm_rwr<4>(a, ep, stream); break;
      default: rc = 1; break;
    }
    if (gemm_form_done(rc)) return rc;
  }
  if (apk && (flags & GEMM_SPLITK) && plain && a.ws != nullptr) {  // split-K ring
    rc = with_row_tiles(M, [&](auto mt) { return launch_gemm_rwk<mt()>(a, ep, stream, rwk_comb(flags)); });
    if (gemm_form_done(rc)) return rc;
  }
  if (flags & GEMM_PARTIALS) return -6;  // partials only: nothing else writes them
  // gated (MoE expert) GEMMs use the one-group kernel
  if (a.gate != nullptr) flags &= ~(GEMM_STREAM_K | GEMM_SHARED_A | GEMM_RING);
  if (apk && (flags & GEMM_RING) && !(flags & GEMM_ONE_GROUP)) {  // balanced ring kernel
    rc = with_row_tiles(M, [&](auto mt) { return launch_gemm_rw<mt()>(a, ep, stream); });
    if (gemm_form_done(rc)) return rc;
  }
  if (apk && (flags & GEMM_SHARED_A) && !(flags & GEMM_ONE_GROUP)) {  // shared-A kernel
    rc = with_row_tiles(M, [&](auto mt) { return launch_gemm_lds<mt()>(a, ep, stream); });
    if (gemm_form_done(rc)) return rc;
  }
  if (apk && (flags & GEMM_STREAM_K) && !(flags & GEMM_ONE_GROUP) && a.ws != nullptr) {  // stream-K
    rc = with_row_tiles(M, [&](auto mt) { return launch_gemm_sk<mt()>(a, ep, stream); });
    if (gemm_form_done(rc)) return rc;
  }
  rc = with_row_tiles(M, [&](auto mt) { return launch_gemm<mt()>(a, ep, stream); });
  if (rc) return rc;
  return (int)hipGetLastError();
}

namespace mp {
// Pack row-major x[M, K] into Ap[K/32][ceil(M/16)][64][8] (rows >= M left untouched).
__global__ __launch_bounds__(256) void pack_act_kernel(const bf16_t* __restrict__ x, int64_t xs, bf16_t* __restrict__ ap,
                                                       int M, int K, int MT) {
  const int nch = K >> 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M * nch; i += gridDim.x * blockDim.x) {
    const int row = i / nch, col = (i - row * nch) * 8;
    *reinterpret_cast<u16x8*>(ap + apk_off(row, col, MT)) = *reinterpret_cast<const u16x8*>(x + row * xs + col);
  }
}
}  // namespace mp

extern "C" int mp_pack_act(const void* x, int64_t xs, void* ap, int M, int K, hipStream_t stream) {
  using namespace mp;
  if (K % 32 || xs % 8) return -1;
  if (M == 0) return 0;
  const int MT = (M + 15) / 16;
  const int n = M * (K / 8);
  hipLaunchKernelGGL(pack_act_kernel, dim3(min((n + 255) / 256, 4096)), dim3(256), 0, stream, (const bf16_t*)x, xs,
                     (bf16_t*)ap, M, K, MT);
  return (int)hipGetLastError();
}

extern "C" int mp_pack_weight(const void* w, void* wp, int N, int K, hipStream_t stream) {
  using namespace mp;
  if (N % 16 || K % 32) return -1;
  const int64_t total = (int64_t)(N / 16) * (K / 32) * 64;
  int64_t g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(pack_weight_kernel, dim3((int)g), dim3(256), 0, stream, (const bf16_t*)w, (bf16_t*)wp, N, K);
  return (int)hipGetLastError();
}
