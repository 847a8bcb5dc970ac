// Grouped W8A16 decode GEMMs of a sparse-MoE (Mixtral) MLP: all E experts of a layer in TWO launches
// (kernels built on gemm_kernels.h's fp8-weight ring body; nothing there changes).
//
//   mp_moe_gate_up_w8   act[e] = SwiGLU(x . gate_up[e]^T)      grid (G, E), one expert per blockIdx.y
//   mp_moe_down_w8      y = bf16( sum_e wd[:, e] * (act[e] . down[e]^T) )   grid (G)
//
// Weights are the stacked W8A16 layout (ops.w8_from_fp8 per expert): e4m3 codes uint8
// [E][N/16][K/32][64][8] in the bf16 fragment order + fp32 per-output-channel scales [E][N]; the fp8
// fragments are converted into the bf16 MFMA and the scales multiply the accumulators (rw_body, F8).
// Activations are packed bf16 (common.h apk_off), M <= 64 rows; ``act`` is E consecutive packed
// activations of packed_numel(M, F) elements.  ``cnt`` int32 [E] (device) holds the tokens routed to
// each expert: an expert with cnt == 0 is skipped ON THE DEVICE - none of its weights, scales or its
// activation slab is read - so a one-session top-2-of-8 step streams 2/8 of the expert bytes and the
// step has no data-dependent launch: it stays inside one hipGraph.
//
// Inside an expert the column split (G workgroups, n_big wide ones, wide / narrow tile counts) is the
// one launch_gemm_rw<MT, true> picks for the same (N, epilogue), so
//   * a routed expert's gate/up slab is bit for bit what mp_gemm_w8's ring form stores for that
//     expert alone (the workgroup body IS rw_body<MT, NT, 1, true, true>);
//   * the down kernel with one routed expert and weight 1 is bit for bit mp_gemm_w8's ring form
//     (same k-slices per wave in the same order, the scale applied per wave before the four waves
//     are summed in wave order, one bf16 rounding).
#include "gemm_kernels.h"

namespace mp {

constexpr int MOE_MAX_E = 32;  // routed experts travel as a 32-bit mask; wd / scales staged in LDS

// The column split of launch_gemm_rw<MT, true>(N, epilogue): units (tiles, or gate/up tile pairs)
// over G = min(#CUs, units) workgroups, n_big of them ntb tiles wide, the rest nts.  False for the
// widths this file does not build (the caller then reports the shape as not covered).
struct MoeSplit {
  int G, n_big, ntb, nts;
};
static bool moe_split(int N, int epi, MoeSplit& s) {
  const int step = epi == 1 ? 2 : 1;
  const int units = (N / 16) / step;
  if (N <= 0 || N % 16 || (N / 16) % step || units == 0) return false;
  s.G = units < sk_num_cus() ? units : sk_num_cus();
  const int base = units / s.G, rem = units % s.G;
  s.ntb = (base + (rem ? 1 : 0)) * step;
  s.n_big = rem ? rem : s.G;
  s.nts = rem ? s.ntb - step : s.ntb;
  if (epi == 1) return s.ntb == 2 || s.ntb == 4 || s.ntb == 6 || s.ntb == 8;
  return s.ntb >= 1 && s.ntb <= 4;
}

// ---------------------------------------------------------------------------------------
// Grouped gate/up + SwiGLU: workgroup (b, e) is workgroup b of the ring GEMM of expert e.
template <int MT, int NTB, int NTS>
__global__ __launch_bounds__(RW_WAVES * 64) void moe_gate_up_kernel(const bf16_t* __restrict__ x,
                                                                    const uint8_t* __restrict__ w8,
                                                                    bf16_t* __restrict__ act,
                                                                    const int32_t* __restrict__ cnt, int M, int N,
                                                                    int K, int n_big, const EpiArgs ep) {
  const int e = blockIdx.y;
  if (cnt[e] <= 0) return;  // unrouted: nothing else is loaded, the slab stays as it was
  __shared__ u64 rs_part[SS_PG][SS_ROWS];
  __shared__ float rs_lds[SS_ROWS];
  __shared__ __attribute__((aligned(16))) f32x4 red[RW_WAVES * (MT * NTB < RW_QC ? MT * NTB : RW_QC) * 64];
  EpiArgs epe = ep;
  epe.wsc = ep.wsc + (int64_t)e * N;
  const bf16_t* wp = reinterpret_cast<const bf16_t*>(w8 + (int64_t)e * N * K);
  bf16_t* ye = act + (int64_t)e * MT * 16 * (N / 2);
  const int b = blockIdx.x;
  if (b < n_big) {
    rw_body<MT, NTB, 1, true, true>(x, wp, ye, 0, nullptr, 0, M, K, b * NTB, ep.rot, epe, red, rs_part, rs_lds, 0,
                                    MT);
  } else {
    rw_body<MT, NTS, 1, true, true>(x, wp, ye, 0, nullptr, 0, M, K, n_big * NTB + (b - n_big) * NTS, ep.rot, epe,
                                    red, rs_part, rs_lds, 0, MT);
  }
}

// ---------------------------------------------------------------------------------------
// Grouped down + combine.  Ring slots: 4 MT + 2 NT VGPRs each (as rw_depth2's fp8 form), beside
// 2 x 4 MT NT accumulator registers (acc of the running expert, tot of the combine): 4 slots while
// the sum stays under 200 registers a lane (one wave per SIMD: 512 are there), else 2.
template <int MT, int NT>
constexpr int moe_depth() {
  return 4 * (4 * MT + 2 * NT) + 8 * MT * NT <= 200 ? 4 : 2;
}

template <int MT, int NT>
__device__ __forceinline__ void moe_down_body(const bf16_t* __restrict__ act, const uint8_t* __restrict__ w8,
                                              const float* __restrict__ wsc, const float* __restrict__ wd,
                                              bf16_t* __restrict__ y, int64_t ys, int M, int E, int N, int K,
                                              int tile0, unsigned mask, const EpiArgs& ep, f32x4* red, float* wd_l,
                                              float* ws_l) {
  constexpr int R = moe_depth<MT, NT>();
  constexpr int Q = MT * NT;
  constexpr int NQ = (Q + RW_WAVES - 1) / RW_WAVES;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nks = K >> 5;
  const int spw = (nks + RW_WAVES - 1) / RW_WAVES;  // ring steps per expert of the busiest wave
  const int total = __builtin_popcount(mask) * spw;  // this wave's flattened (routed expert, k-slice) steps
  const int64_t wstride = (int64_t)N * K;            // bytes per expert
  const int64_t astride = (int64_t)MT * 16 * K;      // elements per activation slab
  const uint8_t* wb = w8 + ((int64_t)tile0 * nks) * 512 + lane * 8;
  const bf16_t* xl = act + lane * 8;

  f32x4 acc[MT][NT], tot[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mt][t] = tot[mt][t] = (f32x4)(0.f);
  u16x8 ra[R][MT];
  u32x2 rb[R][NT];
  // load cursor: (lowest set bit of lmask, li) is the next step to fetch; past the last step it stays
  // on the last routed expert's last slice (in-order vmcnt needs every slot loaded; its MFMAs never run)
  unsigned lmask = mask;
  int li = 0;
#define MOE_LOAD(s)                                                                                         \
  {                                                                                                         \
    const int e_ = __builtin_ctz(lmask);                                                                    \
    const int k_ = min(wid + RW_WAVES * li, nks - 1);                                                       \
    const uint8_t* we_ = wb + e_ * wstride;                                                                 \
    const bf16_t* xe_ = xl + e_ * astride;                                                                  \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) rb[s][t] =                                               \
        __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(we_ + (((int64_t)t * nks + k_) << 9)));  \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) ra[s][mt] =                                           \
        load_a_rows(xe_ + (((int64_t)k_ * MT + mt) << 9), lane, mt * 16 + (lane & 15) < M);                 \
    if (li + 1 < spw) {                                                                                     \
      ++li;                                                                                                 \
    } else if (lmask & (lmask - 1)) {                                                                       \
      lmask &= lmask - 1;                                                                                   \
      li = 0;                                                                                               \
    }                                                                                                       \
  }
  if (mask != 0) {
#pragma unroll
    for (int s = 0; s < R; ++s) MOE_LOAD(s)
  }
  // routing weights of the real rows and the routed experts' channel scales of this workgroup's
  // columns -> LDS (read at every expert boundary: an LDS read does not wait for the ring's loads)
  for (int i = tid; i < M * E; i += RW_WAVES * 64) wd_l[i] = wd[i];
  for (int i = tid; i < E * NT * 16; i += RW_WAVES * 64) {
    const int e_ = i / (NT * 16), c_ = i % (NT * 16);
    ws_l[i] = ((mask >> e_) & 1) ? wsc[(int64_t)e_ * N + tile0 * 16 + c_] : 0.f;
  }
  lds_wait_barrier();

  unsigned cmask = mask;
  int ci = 0;
  bool first = true;
  for (int s0 = 0; s0 < total; s0 += R) {
#pragma unroll
    for (int s = 0; s < R; ++s) {
      if (s0 + s < total) {
        if (wid + RW_WAVES * ci < nks) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const u16x8 b = f8w_to_bf16(rb[s][t]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][t] = mfma16(ra[s][mt], b, acc[mt][t]);
          }
        }
        if (++ci == spw) {
          // this wave has finished an expert: tot += (acc * channel scale) * routing weight, in fp32
          const int e_ = __builtin_ctz(cmask);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              const float sc = ws_l[(e_ * NT + t) * 16 + (lane & 15)];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + (lane >> 4) * 4 + r;
                const float wv = row < M ? wd_l[row * E + e_] : 0.f;  // padding rows: never stored
                const float v = (acc[mt][t][r] * sc) * wv;
                tot[mt][t][r] = first ? v : tot[mt][t][r] + v;
              }
              acc[mt][t] = (f32x4)(0.f);
            }
          cmask &= cmask - 1;
          ci = 0;
          first = false;
        }
      }
      MOE_LOAD(s)
    }
  }
#undef MOE_LOAD
  // ---- sum the 4 waves' totals through LDS in wave order (as rw_body), one bf16 store ----
#pragma unroll
  for (int qd = 0; qd < Q; ++qd) red[(wid * Q + qd) * 64 + lane] = tot[qd / NT][qd % NT];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int qd = wid + RW_WAVES * j;
    if (qd >= Q) break;
    f32x4 v = red[qd * 64 + lane];
#pragma unroll
    for (int w = 1; w < RW_WAVES; ++w) v += red[(w * Q + qd) * 64 + lane];
    tile_epilogue<MT, 0, false>(qd / NT, tile0 + qd % NT, v, (f32x4)(0.f), y, ys, nullptr, 0, M, lane, ep, nullptr,
                                nullptr);
  }
}

template <int MT, int NTB, int NTS>
__global__ __launch_bounds__(RW_WAVES * 64) void moe_down_kernel(const bf16_t* __restrict__ act,
                                                                 const uint8_t* __restrict__ w8,
                                                                 const float* __restrict__ wsc,
                                                                 const int32_t* __restrict__ cnt,
                                                                 const float* __restrict__ wd, bf16_t* __restrict__ y,
                                                                 int64_t ys, int M, int E, int N, int K, int n_big,
                                                                 const EpiArgs ep) {
  __shared__ __attribute__((aligned(16))) f32x4 red[RW_WAVES * MT * NTB * 64];
  __shared__ float wd_l[64 * MOE_MAX_E];
  __shared__ float ws_l[MOE_MAX_E * NTB * 16];
  // the routed experts, once: lane e of every wave reads cnt[e], the ballot is the list (ascending)
  const int lane = threadIdx.x & 63;
  const int c = lane < E ? cnt[lane] : 0;
  const unsigned mask = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)__ballot(c > 0));
  const int b = blockIdx.x;
  if (b < n_big) {
    moe_down_body<MT, NTB>(act, w8, wsc, wd, y, ys, M, E, N, K, b * NTB, mask, ep, red, wd_l, ws_l);
  } else {
    moe_down_body<MT, NTS>(act, w8, wsc, wd, y, ys, M, E, N, K, n_big * NTB + (b - n_big) * NTS, mask, ep, red, wd_l,
                           ws_l);
  }
}

// ---------------------------------------------------------------------------------------
template <int MT>
static int launch_moe_gate_up(const void* x, const void* w8, const float* wsc, const int32_t* cnt, void* act, int M,
                              int E, int H, int F, hipStream_t stream, bool dry) {
  const int N = 2 * F, K = H;
  EpiArgs ep{};
  ep.mt_out = MT;
  ep.wsc = wsc;
  MoeSplit s;
  if (!moe_split(N, 1, s)) return 1;
  // the single-expert ring form must cover (and so split) the shape the same way
  if (launch_gemm_rw<MT, true>(gemm_shape_args(M, N, K, 1, GEMM_OUT_PACKED), ep, stream, true) != 0) return 1;
  if (dry) return 0;
#define MP_MGU(B_, S_)                                                                                           \
  hipLaunchKernelGGL((moe_gate_up_kernel<MT, B_, S_>), dim3(s.G, E), dim3(RW_WAVES * 64), 0, stream,            \
                     (const bf16_t*)x, (const uint8_t*)w8, (bf16_t*)act, cnt, M, N, K, s.n_big, ep);           \
  return 0
  switch (s.ntb) {
    case 2: MP_MGU(2, 2);
    case 4: MP_MGU(4, 2);
    case 6: MP_MGU(6, 4);
    case 8: MP_MGU(8, 6);
    default: return 1;
  }
#undef MP_MGU
}

template <int MT>
static int launch_moe_down(const void* act, const void* w8, const float* wsc, const int32_t* cnt, const float* wd,
                           void* y, int64_t ys, int M, int E, int H, int F, hipStream_t stream, bool dry) {
  const int N = H, K = F;
  EpiArgs ep{};
  ep.mt_out = MT;
  MoeSplit s;
  if (!moe_split(N, 0, s)) return 1;
  if (launch_gemm_rw<MT, true>(gemm_shape_args(M, N, K, 0, 0), ep, stream, true) != 0) return 1;
  if (dry) return 0;
#define MP_MDN(B_, S_)                                                                                           \
  hipLaunchKernelGGL((moe_down_kernel<MT, B_, S_>), dim3(s.G), dim3(RW_WAVES * 64), 0, stream,                  \
                     (const bf16_t*)act, (const uint8_t*)w8, wsc, cnt, wd, (bf16_t*)y, ys, M, E, N, K, s.n_big, \
                     ep);                                                                                        \
  return 0
  switch (s.ntb) {
    case 1: MP_MDN(1, 1);
    case 2: MP_MDN(2, 1);
    case 3: MP_MDN(3, 2);
    case 4: MP_MDN(4, 3);
    default: return 1;
  }
#undef MP_MDN
}

// shapes both kernels take: M <= 64 rows, E <= MOE_MAX_E experts, K of each GEMM a multiple of 128
static bool moe_shape_ok(int M, int E, int H, int F) {
  return M > 0 && M <= 64 && E > 0 && E <= MOE_MAX_E && H > 0 && F > 0 && H % 128 == 0 && F % 128 == 0;
}

}  // namespace mp

// Grouped gate/up + SwiGLU of E experts: x packed bf16 (M rows x H), w8 [E][2F/16][H/32][64][8], wsc
// [E][2F], cnt int32 [E], act E packed activations of packed_numel(M, F) elements each.  Returns 1 when
// the shape is not covered (nothing launched), < 0 for a bad call.
extern "C" int mp_moe_gate_up_w8(const void* x, const void* w8, const float* wsc, const int32_t* cnt, void* act, int M,
                                 int E, int H, int F, hipStream_t stream) {
  (void)hipGetLastError();  // an earlier non-mpamd HIP call's stale error is not this launch's
  using namespace mp;
  if (M == 0) return 0;
  if (M < 0 || x == nullptr || w8 == nullptr || wsc == nullptr || cnt == nullptr || act == nullptr) return -1;
  if (!moe_shape_ok(M, E, H, F)) return 1;
  const int rc = with_row_tiles(M, [&](auto mt) {
    return launch_moe_gate_up<mt()>(x, w8, wsc, cnt, act, M, E, H, F, stream, false);
  });
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

// Grouped down + combine: act as mp_moe_gate_up_w8 leaves it, w8 [E][H/16][F/32][64][8], wsc [E][H],
// wd fp32 [M][E] dense routing weights, y bf16 row-major [M][H] (row stride y_stride).
extern "C" int mp_moe_down_w8(const void* act, const void* w8, const float* wsc, const int32_t* cnt, const float* wd,
                              void* y, int64_t y_stride, int M, int E, int H, int F, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (M == 0) return 0;
  if (M < 0 || act == nullptr || w8 == nullptr || wsc == nullptr || cnt == nullptr || wd == nullptr || y == nullptr ||
      y_stride < H)
    return -1;
  if (!moe_shape_ok(M, E, H, F)) return 1;
  const int rc = with_row_tiles(M, [&](auto mt) {
    return launch_moe_down<mt()>(act, w8, wsc, cnt, wd, y, y_stride, M, E, H, F, stream, false);
  });
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

// dry dispatch of both launches
extern "C" int mp_moe_w8_ok(int M, int E, int H, int F) {
  using namespace mp;
  if (!moe_shape_ok(M, E, H, F)) return 0;
  return with_row_tiles(M, [&](auto mt) {
    const int a = launch_moe_gate_up<mt()>(nullptr, nullptr, nullptr, nullptr, nullptr, M, E, H, F, 0, true);
    const int b = launch_moe_down<mt()>(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, M, E, H, F, 0, true);
    return (a == 0 && b == 0) ? 0 : 1;
  }) == 0;
}
