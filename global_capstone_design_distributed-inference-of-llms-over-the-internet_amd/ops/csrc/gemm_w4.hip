// W4A16 decode GEMM and dequantizer for OCP MXFP4 weights (e2m1 codes, one e8m0 scale per 32
// weights along K: 4.25 bits per weight).  The GEMM is the balanced ring form of gemm_kernels.h
// ("rw": one workgroup of 4 waves per CU owning a contiguous run of column tiles and all of K, one
// launch, partial tiles summed through LDS, the shared fused-norm epilogues) with the weight
// operand dequantized in registers into the bf16 MFMA:
//
//   W4[N/16][K/128][64][16]  lane = 16 q + c: byte 4 s + b = codes of W[16 nt + c][128 kb + 32 s + 8 q + 2 b]
//                            (low nibble) and ... + 2 b + 1 (high nibble), s = 0..3: a lane's 16 bytes are
//                            its bf16-fragment elements (8 weights) of four consecutive 32-deep k-slices
//   S4[N/16][K/128][16][4]   column c, one e8m0 byte per k-slice s (its four q groups share it)
//
// so a ring step is 128 deep: one 16-byte weight load and one 4-byte scale load per column tile,
// four 16-byte activation loads per row tile, and per k-slice four v_cvt_scalef32_pk_bf16_fp4
// (dword s, byte select 0..3, scale operand uint(e) << 23 = 2^(e - 127), built once per
// fragment) feeding v_mfma_f32_16x16x32_bf16 - the VALU count of the W8A16 form.  Every product
// code x 2^(e - 127) is an exact bf16 value and the block scale is applied by the convert, so
// there is no per-column accumulator scale.
//
// Not built for 4-bit weights (ops.linear_w4 docstring): the split-K ring, partial slabs / the
// qkv fold, a start-up autotuner, W4A8 / W4A4 on the block-scaled MFMA.
#include "gemm_kernels.h"

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

// Ring slot of a 128-deep step: 16 MT (A) + 4 NT (codes) + NT (scales) VGPRs beside 4 MT NT
// accumulators (one wave per SIMD: 512 registers).  K = 4096 is 8 steps per wave.
template <int MT, int NT>
constexpr int w4_depth() {
  if (MT + NT <= 2) return 8;
  return (400 - 4 * MT * NT) / (16 * MT + 5 * NT) >= 4 ? 4 : 2;
}

template <int MT, int NT, int EPI, bool OPK>
__device__ __forceinline__ void rw4_body(const bf16_t* __restrict__ x, const uint8_t* __restrict__ w4,
                                         const uint8_t* __restrict__ s4, bf16_t* __restrict__ y, int64_t ys,
                                         const bf16_t* __restrict__ res, int64_t rs, int M, int K, int tile0,
                                         const EpiArgs& ep, f32x4* red, u64 (*rs_part)[SS_ROWS], float* rs_lds) {
  constexpr int R = w4_depth<MT, NT>();
  constexpr int Q = MT * NT;
  constexpr int NQ = (Q + RW_WAVES - 1) / RW_WAVES;  // epilogue quads per wave
  RowScale<EPI < 2, RW_WAVES> rsc;
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nkb = K >> 7;                             // 128-deep steps
  const int cnt = (nkb + RW_WAVES - 1) / RW_WAVES;    // ring steps of the busiest wave
  const uint8_t* wb = w4 + ((int64_t)tile0 * nkb) * 1024 + lane * 16;
  const uint8_t* sb = s4 + ((int64_t)tile0 * nkb) * 64 + (lane & 15) * 4;
  const bf16_t* xl = x + lane * 8;
  const int mta = ep.mt_out;

  // EPI 3: the residual quads this wave finalises, in flight during the main loop
  u16x4 rpre[NQ];
  if constexpr (EPI == 3) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int qd = min(wid + RW_WAVES * j, Q - 1), mt = qd / NT, t = qd % NT;
      const int col = (tile0 + t) * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) rpre[j][r] = res[(int64_t)min(mt * 16 + (lane >> 4) * 4 + r, M - 1) * rs + col];
    }
  }

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mt][t] = (f32x4)(0.f);
  u16x8 ra[R][MT][4];
  u32x4 rb[R][NT];
  unsigned rsx[R][NT];
  // loads past the wave's last step are clamped to a valid one and their MFMAs skipped
#define RW4_LOAD(s, i)                                                                                       \
  {                                                                                                          \
    const int k_ = min(wid + RW_WAVES * (i), nkb - 1);                                                       \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                                         \
      rb[s][t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wb + (((int64_t)t * nkb + k_) << 10))); \
      rsx[s][t] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(sb + (((int64_t)t * nkb + k_) << 6))); \
    }                                                                                                        \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int u = 0; u < 4; ++u)          \
        ra[s][mt][u] = load_a_rows(xl + (((int64_t)(4 * k_ + u) * mta + min(mt, mta - 1)) << 9), lane,      \
                                   mt * 16 + (lane & 15) < M);                                               \
  }
#pragma unroll
  for (int s = 0; s < R; ++s) RW4_LOAD(s, s)
  rsc.load(ep, w4);
  for (int i0 = 0; i0 < cnt; i0 += R) {
#pragma unroll
    for (int s = 0; s < R; ++s) {
      if (wid + RW_WAVES * (i0 + s) < nkb) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const u16x8 b = f4w_to_bf16(rb[s][t][u], e8m0_scale(rsx[s][t], u));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][t] = mfma16(ra[s][mt][u], b, acc[mt][t]);
          }
        }
      }
      RW4_LOAD(s, i0 + s + R)
    }
  }
#undef RW4_LOAD
  // ---- sum the 4 waves' partial tiles through LDS, then the shared epilogues (as rw_body) ----
  rsc.finish(ep, rs_part, rs_lds);
  static_assert(Q <= RW_QC, "one combine pass");
#pragma unroll
  for (int qd = 0; qd < Q; ++qd) red[(wid * Q + qd) * 64 + lane] = acc[qd / NT][qd % NT];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int qd = wid + RW_WAVES * j;
    if (qd >= Q) break;
    if (EPI == 1 && (qd % NT) & 1) continue;  // up tile: consumed with its gate tile
    f32x4 v = red[qd * 64 + lane], up = (f32x4)(0.f);
#pragma unroll
    for (int w = 1; w < RW_WAVES; ++w) v += red[(w * Q + qd) * 64 + lane];
    if constexpr (EPI == 1) {
#pragma unroll
      for (int w = 0; w < RW_WAVES; ++w) up += red[(w * Q + qd + 1) * 64 + lane];
    }
    tile_epilogue<MT, EPI, OPK>(qd / NT, tile0 + qd % NT, v, up, y, ys, res, rs, M, lane, ep, rs_lds,
                                EPI == 3 ? &rpre[j] : nullptr);
  }
}

template <int MT, int NTB, int NTS, int EPI, bool OPK>
__global__ __launch_bounds__(RW_WAVES * 64) void gemm_rw4_kernel(const bf16_t* __restrict__ x,
                                                                 const uint8_t* __restrict__ w4,
                                                                 const uint8_t* __restrict__ s4, bf16_t* __restrict__ y,
                                                                 int64_t ys, const bf16_t* __restrict__ res, int64_t rs,
                                                                 int M, int K, int n_big, const EpiArgs ep) {
  clear_other(ep);
  __shared__ u64 rs_part[SS_PG][SS_ROWS];
  __shared__ float rs_lds[SS_ROWS];
  __shared__ __attribute__((aligned(16))) f32x4 red[RW_WAVES * MT * NTB * 64];
  const int b = blockIdx.x;
  if (b < n_big) {
    rw4_body<MT, NTB, EPI, OPK>(x, w4, s4, y, ys, res, rs, M, K, b * NTB, ep, red, rs_part, rs_lds);
  } else {
    rw4_body<MT, NTS, EPI, OPK>(x, w4, s4, y, ys, res, rs, M, K, n_big * NTB + (b - n_big) * NTS, ep, red, rs_part,
                                rs_lds);
  }
}

// GU: a gate/up width (even tile counts, packed SwiGLU epilogue only); otherwise epilogues 0 / 3
template <int MT, int NTB, int NTS, bool GU>
static int launch_gemm_rw4_cfg(const GemmArgs& a, const EpiArgs& ep, hipStream_t stream, int G, int n_big, bool dry) {
  if (dry) return 0;
  const int epi = a.epilogue;
#define MP_RW4(EPI_, OPK_)                                                                                     \
  hipLaunchKernelGGL((gemm_rw4_kernel<MT, NTB, NTS, EPI_, OPK_>), dim3(G), dim3(RW_WAVES * 64), 0, stream,     \
                     (const bf16_t*)a.x, (const uint8_t*)a.w, (const uint8_t*)a.wsc, (bf16_t*)a.y, a.y_stride, \
                     (const bf16_t*)a.res, a.res_stride, a.M, a.K, n_big, ep)
  if constexpr (GU) {
    static_assert(NTB % 2 == 0 && NTS % 2 == 0, "gate/up tile pairs");
    if (epi != 1) return 1;
    MP_RW4(1, true);
  } else {
    if (epi == 3) {
      MP_RW4(3, false);
    } else if (epi == 0) {
      MP_RW4(0, false);
    } else {
      return 1;
    }
  }
#undef MP_RW4
  return 0;
}

// Column units (tiles, or gate/up tile pairs) over G workgroups as launch_gemm_rw splits them:
// n_big take ceil, the rest floor.  G = min(#CUs, units), raised until a workgroup owns at most
// 4 units (the widths built: up to 4 tiles, or 8 = 4 gate/up pairs).
template <int MT>
static int launch_gemm_rw4(const GemmArgs& a, const EpiArgs& ep, hipStream_t stream, bool dry = false) {
  const int epi = a.epilogue, N = a.N;
  const bool opk = a.flags & GEMM_OUT_PACKED;
  if (!(epi == 0 || epi == 3 || (epi == 1 && opk)) || (epi != 1 && opk)) return 1;
  const int step = epi == 1 ? 2 : 1;
  const int units = (N / 16) / step;
  if ((N / 16) % step || units == 0) return 1;
  int G = units < sk_num_cus() ? units : sk_num_cus();
  if ((units + 3) / 4 > G) G = (units + 3) / 4;
  const int base = units / G, rem = units % G;
  const int ntb = (base + (rem ? 1 : 0)) * step;
  const int n_big = rem ? rem : G;
#define MP_RW4C(B_, S_, GU_) return launch_gemm_rw4_cfg<MT, B_, S_, GU_>(a, ep, stream, G, n_big, dry)
  if (epi == 1) {
    switch (ntb) {
      case 2: MP_RW4C(2, 2, true);
      case 4: MP_RW4C(4, 2, true);
      case 6: MP_RW4C(6, 4, true);
      case 8: MP_RW4C(8, 6, true);
      default: return 1;
    }
  }
  switch (ntb) {
    case 1: MP_RW4C(1, 1, false);
    case 2: MP_RW4C(2, 1, false);
    case 3: MP_RW4C(3, 2, false);
    case 4: MP_RW4C(4, 3, false);
    default: return 1;
  }
#undef MP_RW4C
}

static int gemm_w4_dispatch(const GemmArgs& a, const EpiArgs& ep, hipStream_t stream, bool dry) {
  return with_row_tiles(a.M, [&](auto mt) { return launch_gemm_rw4<mt()>(a, ep, stream, dry); });
}

// One thread per 16-byte lane chunk: 32 weights (8 of each of 4 k-slices) -> 4 x 16 B of row-major bf16
__global__ __launch_bounds__(256) void dequant_w4_kernel(const uint8_t* __restrict__ w4, const uint8_t* __restrict__ s4,
                                                         bf16_t* __restrict__ w, int64_t total, int nkb, int K) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (nt * nkb + kb) * 64 + lane
  if (i >= total) return;
  const int lane = (int)(i & 63), c = lane & 15, q = lane >> 4;
  const int64_t blk = i >> 6;
  const int kb = (int)(blk % nkb);
  const int64_t nt = blk / nkb;
  const u32x4 d = *reinterpret_cast<const u32x4*>(w4 + i * 16);
  const unsigned sc = *reinterpret_cast<const unsigned*>(s4 + blk * 64 + c * 4);
  bf16_t* o = w + (nt * 16 + c) * (int64_t)K + kb * 128 + q * 8;
#pragma unroll
  for (int s = 0; s < 4; ++s) *reinterpret_cast<u16x8*>(o + 32 * s) = f4w_to_bf16(d[s], e8m0_scale(sc, s));
}

}  // namespace mp

// W4A16 decode GEMM: MXFP4 weights (layout above; a.w the codes, a.wsc the block scales), packed bf16
// activations, M <= 64, epilogues 0 (optional ss_in row scale), 1 (packed SwiGLU output:
// GEMM_OUT_PACKED, the only flag read) and 3 (residual-stream producer).  Returns 1 when the shape is
// not covered (nothing launched), < 0 for a bad call.
extern "C" int mp_gemm_w4(const mp::GemmArgs* args, hipStream_t stream) {
  (void)hipGetLastError();  // an earlier non-mpamd HIP call's stale error is not this launch's
  using namespace mp;
  const GemmArgs& a = *args;
  if (a.M == 0) return 0;
  if (a.M < 0 || a.M > 64 || a.K <= 0 || a.K % 128 || a.N <= 0 || a.N % 16) return 1;
  if (a.epilogue == 3 && (a.ap == nullptr || a.res == nullptr)) return -5;
  EpiArgs ep = gemm_epi(a);
  ep.wsc = nullptr;  // the block scales are a kernel parameter of their own, and the k walk is never
  ep.rot = 0;        // rotated: these kernels read neither field
  const int rc = gemm_w4_dispatch(a, ep, stream, false);
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

extern "C" int mp_gemm_w4_ok(int M, int N, int K, int epilogue) {
  using namespace mp;
  if (M <= 0 || M > 64 || K <= 0 || K % 128 || N <= 0 || N % 16) return 0;
  const GemmArgs a = gemm_shape_args(M, N, K, epilogue, epilogue == 1 ? GEMM_OUT_PACKED : 0);
  return gemm_w4_dispatch(a, gemm_epi(a), 0, true) == 0;
}

// MXFP4 -> row-major bf16 W[N, K] (exact: code x 2^(e - 127)), one launch
extern "C" int mp_dequant_w4(const void* w4, const void* s4, void* w, int N, int K, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (N <= 0 || K <= 0 || N % 16 || K % 128) return -1;
  const int nkb = K / 128;
  const int64_t total = (int64_t)(N / 16) * nkb * 64;
  hipLaunchKernelGGL(dequant_w4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                     (const uint8_t*)w4, (const uint8_t*)s4, (bf16_t*)w, total, nkb, K);
  return (int)hipGetLastError();
}
