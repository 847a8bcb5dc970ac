// Grouped bf16 decode GEMMs of a sparse-MoE (Mixtral) MLP: all E experts of a layer in TWO launches -
// the bf16 counterpart of gemm_moe.hip (which, like gemm_kernels.h, does not change).
//
//   mp_moe_gate_up   act[e] = SwiGLU(x . gate_up[e]^T)      grid (G, E), one expert per blockIdx.y
//   mp_moe_down      y = bf16( sum_e wd[:, e] * (act[e] . down[e]^T) )   grid (G)
//
// Weights are the stacks an unquantized stage already holds: ops.pack_weight per expert, bf16
// [E][N/16][K/32][64][8] in the MFMA fragment order (a B fragment is one contiguous 1 KiB read of
// 16 B per lane, straight into v_mfma_f32_16x16x32_bf16 - no conversion, no channel scale).
// Activations are packed bf16 (common.h apk_off), M <= 64 rows; ``act`` is E consecutive packed
// activations of packed_numel(M, F) elements.  ``cnt`` int32 [E] (device) holds the rows routed to each
// expert: an expert with cnt <= 0 is skipped ON THE DEVICE - neither its weights nor its activation
// slab is read - so a one-session top-2-of-8 step streams 2/8 of the expert bytes, and the step has no
// data-dependent launch and no host sync: it stays inside one hipGraph.  No atomics, no k split across
// workgroups, a grid that depends on the shape alone: the same bits on every run.
//
// Inside an expert the column split (G workgroups, n_big wide ones) is the one launch_gemm_rw<MT, false>
// picks for the same (N, epilogue), so
//   * a routed expert's gate/up slab is bit for bit what mp_gemm_bf16's ring form (GEMM_RING, no k
//     rotation) stores for that expert alone: the workgroup body IS rw_body<MT, NT, 1, true, false>;
//   * the down kernel with one routed expert and weight 1 is bit for bit that ring form too: the same
//     k-slices per wave in the same order, acc * 1.0f exact, the four waves summed in wave order, one
//     bf16 rounding.
// Padding rows past M load their tile's row 0 (load_a_rows) and are never stored or combined.
#include "gemm_kernels.h"

namespace mp {

constexpr int MOEB_MAX_E = 32;  // routed experts travel as a 32-bit mask; wd staged in LDS

// The column split of launch_gemm_rw<MT, false>(N, epilogue): units (tiles, or gate/up tile pairs)
// over G = min(#CUs, units) workgroups, n_big of them ntb tiles wide, the rest nts.  False for the
// widths this file does not build (the caller then reports the shape as not covered).
struct MoeBSplit {
  int G, n_big, ntb, nts;
};
static bool moeb_split(int N, int epi, MoeBSplit& s) {
  const int step = epi == 1 ? 2 : 1;
  if (N <= 0 || N % 16 || (N / 16) % step) return false;
  const int units = (N / 16) / step;
  s.G = units < sk_num_cus() ? units : sk_num_cus();
  const int base = units / s.G, rem = units % s.G;
  s.ntb = (base + (rem ? 1 : 0)) * step;
  s.n_big = rem ? rem : s.G;
  s.nts = rem ? s.ntb - step : s.ntb;
  if (epi == 1) return (s.ntb == 2 && !rem) || s.ntb == 4 || s.ntb == 6 || s.ntb == 8;
  return s.ntb >= 1 && s.ntb <= 4;
}

// ---------------------------------------------------------------------------------------
// Grouped gate/up + SwiGLU: workgroup (b, e) is workgroup b of the bf16 ring GEMM of expert e.
template <int MT, int NTB, int NTS>
__global__ __launch_bounds__(RW_WAVES * 64) void moe_gate_up_bf16_kernel(const bf16_t* __restrict__ x,
                                                                         const bf16_t* __restrict__ wp,
                                                                         bf16_t* __restrict__ act,
                                                                         const int32_t* __restrict__ cnt, int M,
                                                                         int N, int K, int n_big, const EpiArgs ep) {
  const int e = blockIdx.y;
  if (cnt[e] <= 0) return;  // unrouted: nothing else is loaded, the slab stays as it was
  __shared__ u64 rs_part[SS_PG][SS_ROWS];
  __shared__ float rs_lds[SS_ROWS];
  __shared__ __attribute__((aligned(16))) f32x4 red[RW_WAVES * (MT * NTB < RW_QC ? MT * NTB : RW_QC) * 64];
  const bf16_t* we = wp + (int64_t)e * N * K;
  bf16_t* ye = act + (int64_t)e * MT * 16 * (N / 2);
  const int b = blockIdx.x;
  if (b < n_big) {
    rw_body<MT, NTB, 1, true, false>(x, we, ye, 0, nullptr, 0, M, K, b * NTB, 0, ep, red, rs_part, rs_lds, 0, MT);
  } else {
    rw_body<MT, NTS, 1, true, false>(x, we, ye, 0, nullptr, 0, M, K, n_big * NTB + (b - n_big) * NTS, 0, ep, red,
                                     rs_part, rs_lds, 0, MT);
  }
}

// ---------------------------------------------------------------------------------------
// Grouped down + combine.  A workgroup owns NT column tiles for EVERY routed expert; each of its four
// waves walks one flattened sequence of (routed expert, k-slice) steps through a register ring, so the
// weight stream never drains at an expert boundary.
//
// Ring depth.  One wave per SIMD (256 threads, one workgroup per CU): 256 VGPRs + 256 AGPRs a lane.
// The MFMA accumulators of the running expert (4 MT NT) live in AGPRs; everything the VALU touches is
// in VGPRs: a ring slot is 4 MT (A fragments) + 4 NT (16-byte bf16 B fragments) registers, the combine
// total ``tot`` 4 MT NT, and ~48 go to addresses, cursors and the boundary's routing weights.  The
// depth is the largest of 8 / 4 / 2 slots whose sum stays within the 256 VGPRs, and 8 only for NT <= 2:
// a slot of a narrow form holds NT KiB of weights, four waves x 4 slots x 1 KiB = 16 KiB in flight per
// CU is under the ~24 GB/s x 2 us a CU's share of the HBM stream needs, while at NT >= 3 four slots
// already hold 48 KiB.  (gemm_moe.hip's moe_depth counts both accumulator sets against one 200-register
// budget and 2 NT per slot: with 4 NT it would leave the widest forms 2 slots.)
template <int MT, int NT>
constexpr int moeb_depth() {
  constexpr int slot = 4 * MT + 4 * NT, fixed = 4 * MT * NT + 48;
  if (NT <= 2 && 8 * slot + fixed <= 256) return 8;
  return 4 * slot + fixed <= 256 ? 4 : 2;
}

template <int MT, int NT>
__device__ __forceinline__ void moe_down_bf16_body(const bf16_t* __restrict__ act, const bf16_t* __restrict__ wp,
                                                   const float* __restrict__ wd, bf16_t* __restrict__ y, int64_t ys,
                                                   int M, int E, int N, int K, int tile0, unsigned mask,
                                                   const EpiArgs& ep, f32x4* red, float* wd_l) {
  constexpr int R = moeb_depth<MT, NT>();
  constexpr int Q = MT * NT;
  constexpr int NQ = (Q + RW_WAVES - 1) / RW_WAVES;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nks = K >> 5;
  const int spw = (nks + RW_WAVES - 1) / RW_WAVES;   // ring steps per expert of the busiest wave
  const int total = __builtin_popcount(mask) * spw;  // this wave's flattened (routed expert, k-slice) steps
  const int64_t wstride = (int64_t)N * K;            // elements per expert
  const int64_t astride = (int64_t)MT * 16 * K;      // elements per activation slab
  const bf16_t* wb = wp + ((int64_t)tile0 * nks) * 512 + lane * 8;
  const bf16_t* xl = act + lane * 8;

  f32x4 acc[MT][NT], tot[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mt][t] = tot[mt][t] = (f32x4)(0.f);
  u16x8 ra[R][MT], rb[R][NT];
  // load cursor: (lowest set bit of lmask, li) is the next step to fetch; past the last step it stays
  // on the last routed expert's last slice (in-order vmcnt needs every slot loaded; its MFMAs never run)
  unsigned lmask = mask;
  int li = 0;
#define MOEB_LOAD(s)                                                                                        \
  {                                                                                                         \
    const int e_ = __builtin_ctz(lmask);                                                                    \
    const int k_ = min(wid + RW_WAVES * li, nks - 1);                                                       \
    const bf16_t* we_ = wb + e_ * wstride;                                                                  \
    const bf16_t* xe_ = xl + e_ * astride;                                                                  \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) rb[s][t] =                                               \
        __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(we_ + (((int64_t)t * nks + k_) << 9)));  \
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
    for (int s = 0; s < R; ++s) MOEB_LOAD(s)
  }
  // routing weights of the real rows -> LDS (read at every expert boundary: an LDS read does not wait
  // for the ring's loads)
  for (int i = tid; i < M * E; i += RW_WAVES * 64) wd_l[i] = wd[i];
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
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[mt][t] = mfma16(ra[s][mt], rb[s][t], acc[mt][t]);
        }
        if (++ci == spw) {
          // this wave has finished an expert: tot += acc * routing weight, in fp32
          const int e_ = __builtin_ctz(cmask);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            float wv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = mt * 16 + (lane >> 4) * 4 + r;
              wv[r] = row < M ? wd_l[row * E + e_] : 0.f;  // padding rows: never stored
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float v = acc[mt][t][r] * wv[r];
                tot[mt][t][r] = first ? v : tot[mt][t][r] + v;
              }
              acc[mt][t] = (f32x4)(0.f);
            }
          }
          cmask &= cmask - 1;
          ci = 0;
          first = false;
        }
      }
      MOEB_LOAD(s)
    }
  }
#undef MOEB_LOAD
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
__global__ __launch_bounds__(RW_WAVES * 64) void moe_down_bf16_kernel(const bf16_t* __restrict__ act,
                                                                      const bf16_t* __restrict__ wp,
                                                                      const int32_t* __restrict__ cnt,
                                                                      const float* __restrict__ wd,
                                                                      bf16_t* __restrict__ y, int64_t ys, int M, int E,
                                                                      int N, int K, int n_big, const EpiArgs ep) {
  __shared__ __attribute__((aligned(16))) f32x4 red[RW_WAVES * MT * NTB * 64];
  __shared__ float wd_l[64 * MOEB_MAX_E];
  // the routed experts, once: lane e of every wave reads cnt[e], the ballot is the list (ascending)
  const int lane = threadIdx.x & 63;
  const int c = lane < E ? cnt[lane] : 0;
  const unsigned mask = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)__ballot(c > 0));
  const int b = blockIdx.x;
  if (b < n_big) {
    moe_down_bf16_body<MT, NTB>(act, wp, wd, y, ys, M, E, N, K, b * NTB, mask, ep, red, wd_l);
  } else {
    moe_down_bf16_body<MT, NTS>(act, wp, wd, y, ys, M, E, N, K, n_big * NTB + (b - n_big) * NTS, mask, ep, red,
                                wd_l);
  }
}

// ---------------------------------------------------------------------------------------
template <int MT>
static int launch_moe_gate_up_bf16(const void* x, const void* wp, const int32_t* cnt, void* act, int M, int E, int H,
                                   int F, hipStream_t stream, bool dry) {
  const int N = 2 * F, K = H;
  EpiArgs ep{};
  ep.mt_out = MT;
  MoeBSplit s;
  if (!moeb_split(N, 1, s)) return 1;
  if (dry) return 0;
#define MP_MGU(B_, S_)                                                                                        \
  hipLaunchKernelGGL((moe_gate_up_bf16_kernel<MT, B_, S_>), dim3(s.G, E), dim3(RW_WAVES * 64), 0, stream,    \
                     (const bf16_t*)x, (const bf16_t*)wp, (bf16_t*)act, cnt, M, N, K, s.n_big, ep);          \
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
static int launch_moe_down_bf16(const void* act, const void* wp, const int32_t* cnt, const float* wd, void* y,
                                int64_t ys, int M, int E, int H, int F, hipStream_t stream, bool dry) {
  const int N = H, K = F;
  EpiArgs ep{};
  ep.mt_out = MT;
  MoeBSplit s;
  if (!moeb_split(N, 0, s)) return 1;
  if (dry) return 0;
#define MP_MDN(B_, S_)                                                                                        \
  hipLaunchKernelGGL((moe_down_bf16_kernel<MT, B_, S_>), dim3(s.G), dim3(RW_WAVES * 64), 0, stream,          \
                     (const bf16_t*)act, (const bf16_t*)wp, cnt, wd, (bf16_t*)y, ys, M, E, N, K, s.n_big, ep); \
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

// shapes both kernels take: M <= 64 rows, E <= MOEB_MAX_E experts, K of each GEMM a multiple of 128
static bool moeb_shape_ok(int M, int E, int H, int F) {
  return M > 0 && M <= 64 && E > 0 && E <= MOEB_MAX_E && H > 0 && F > 0 && H % 128 == 0 && F % 128 == 0;
}

}  // namespace mp

// Grouped gate/up + SwiGLU of E bf16 experts: x packed bf16 (M rows x H), wp [E][2F/16][H/32][64][8], cnt
// int32 [E], act E packed activations of packed_numel(M, F) elements each.  Returns 1 when the shape is
// not covered (nothing launched), < 0 for a bad call.
extern "C" int mp_moe_gate_up(const void* x, const void* wp, const int32_t* cnt, void* act, int M, int E, int H, int F,
                              hipStream_t stream) {
  (void)hipGetLastError();  // an earlier non-mpamd HIP call's stale error is not this launch's
  using namespace mp;
  if (M == 0) return 0;
  if (M < 0 || x == nullptr || wp == nullptr || cnt == nullptr || act == nullptr) return -1;
  if (!mp_moe_ok(M, E, H, F)) return 1;
  const int rc = with_row_tiles(M, [&](auto mt) {
    return launch_moe_gate_up_bf16<mt()>(x, wp, cnt, act, M, E, H, F, stream, false);
  });
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

// Grouped down + combine: act as mp_moe_gate_up leaves it, wp [E][H/16][F/32][64][8], wd fp32 [M][E] dense
// routing weights, y bf16 row-major [M][H] (row stride y_stride).
extern "C" int mp_moe_down(const void* act, const void* wp, const int32_t* cnt, const float* wd, void* y,
                           int64_t y_stride, int M, int E, int H, int F, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (M == 0) return 0;
  if (M < 0 || act == nullptr || wp == nullptr || cnt == nullptr || wd == nullptr || y == nullptr || y_stride < H)
    return -1;
  if (!mp_moe_ok(M, E, H, F)) return 1;
  const int rc = with_row_tiles(M, [&](auto mt) {
    return launch_moe_down_bf16<mt()>(act, wp, cnt, wd, y, y_stride, M, E, H, F, stream, false);
  });
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

// dry dispatch of both launches: a shape is covered only when BOTH kernels take it
extern "C" int mp_moe_ok(int M, int E, int H, int F) {
  using namespace mp;
  if (!moeb_shape_ok(M, E, H, F)) return 0;
  return with_row_tiles(M, [&](auto mt) {
    const int a = launch_moe_gate_up_bf16<mt()>(nullptr, nullptr, nullptr, nullptr, M, E, H, F, 0, true);
    const int b = launch_moe_down_bf16<mt()>(nullptr, nullptr, nullptr, nullptr, nullptr, 0, M, E, H, F, 0, true);
    return (a == 0 && b == 0) ? 0 : 1;
  }) == 0;
}
