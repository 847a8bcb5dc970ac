// Row-gathered grouped W8A16 GEMMs of a sparse-MoE (Mixtral) MLP for steps ABOVE 64 rows: prefill,
// chunked prefill and decode steps of 65+ sessions.  gemm_moe.hip runs every routed expert over all
// M <= 64 rows; here each expert sees only the rows routed to it (the sparse schedule), in three
// launches with no host sync:
//
//   mp_moe_group          (idx, w) [T, k] -> off [E + 1], tok [T k], wsel [T k]: the (token, expert)
//                         pairs in (expert, token) order - a stable counting sort, one workgroup,
//                         counts and scan in LDS
//   mp_moe_gate_up_w8_rows  out[p] = SwiGLU(x[tok[p]] . gate_up[e(p)]^T)     grid (G, E)
//   mp_moe_down_w8_rows     y[t] = bf16( sum over t's pairs p, ascending expert, of
//                                        wsel[p] * ((act[p] . down[e]^T) * ws[e]) )   grid (G)
//
// Weights are gemm_moe.hip's stacked W8A16 layout (uint8 [E][N/16][K/32][64][8] + fp32 [E][N]) and the
// column split is the same (G workgroups, n_big wide ones).  Activations are ROW-MAJOR bf16: a lane
// (row c = lane & 15, quad q = lane >> 4) reads its A fragment of k-slice ks as the 16 bytes at
// row[32 ks + 8 q] - for gate/up the row is x[tok[p]] (the gather costs nothing extra: one row pointer
// per lane and row tile, loaded once per block), for down it is act[p] (contiguous).
//
// An expert's rows are walked in blocks of up to 64; a block of r rows runs the body built for
// ceil(r / 16) row tiles, lanes past row r read row r - 1 (no further memory touched) and store
// nothing.  Inside a block the four waves take interleaved k-slices through the fp8 register ring of
// rw_body (same depth rule, loads issued R slices ahead, the tail clamped), apply the channel scales
// to their partial tiles and sum them through LDS in wave order.
//
// Down combines without atomics: a workgroup owns its columns for EVERY expert, zeroes them in an fp32
// [T][H] workspace, then takes the routed experts in ascending order and adds wsel * tile into the
// rows tok names with plain loads and stores (a token meets an expert at most once, blocks are
// separated by workgroup barriers, nobody else touches these columns), and rounds its columns to bf16
// once at the end: a fixed summation order, the same bits on every run.
#include "gemm_kernels.h"

namespace mp {

constexpr int MR_MAX_E = 32;       // experts: the grouping kernel's LDS histogram is [E][MR_THREADS]
constexpr int MR_THREADS = RW_WAVES * 64;
constexpr int MR_QC = 16;          // quads per LDS combine pass (waves x 16 x 1 KiB = 64 KiB: two workgroups a CU)
constexpr int MR_MAX_PAIRS = 1 << 16;

// gemm_moe.hip's column split (launch_gemm_rw<MT, true>): units (tiles, or gate/up tile pairs) over
// G = min(#CUs, units) workgroups, n_big of them ntb tiles wide, the rest nts.
struct RowsSplit {
  int G, n_big, ntb, nts;
};
static bool rows_split(int N, int epi, RowsSplit& s) {
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
// Grouping.  Thread i owns the contiguous pairs [i C, (i + 1) C) of the flat [T k] list and counts
// them per expert into hist[e][i]; an exclusive scan over hist in (expert, thread) order is each
// thread's first output slot per expert, so the second walk places pairs in (expert, flat index)
// order: the stable counting sort.  Expert ids outside [0, E) are dropped (off[E] < T k then).
__global__ __launch_bounds__(MR_THREADS) void moe_group_kernel(const int64_t* __restrict__ idx,
                                                               const float* __restrict__ w,
                                                               int32_t* __restrict__ off, int32_t* __restrict__ tok,
                                                               float* __restrict__ wsel, int P, int k, int E) {
  __shared__ int hist[MR_MAX_E * MR_THREADS];
  __shared__ int wave_sum[RW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int C = (P + MR_THREADS - 1) / MR_THREADS;
  const int lo = min(tid * C, P), hi = min(lo + C, P);
  for (int e = 0; e < E; ++e) hist[e * MR_THREADS + tid] = 0;
  for (int p = lo; p < hi; ++p) {
    const int64_t e = idx[p];
    if (e >= 0 && e < E) ++hist[(int)e * MR_THREADS + tid];
  }
  __syncthreads();
  // scan of the E * MR_THREADS counts: thread j sums flat[j E .. j E + E), a block scan of the sums
  int s = 0;
  for (int i = 0; i < E; ++i) s += hist[tid * E + i];
  int inc = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_sum[wid] = inc;
  __syncthreads();
  int base = inc - s;
  for (int v = 0; v < wid; ++v) base += wave_sum[v];
  for (int i = 0; i < E; ++i) {
    const int c = hist[tid * E + i];
    hist[tid * E + i] = base;
    base += c;
  }
  __syncthreads();
  if (tid < E) off[tid] = hist[tid * MR_THREADS];
  if (tid == MR_THREADS - 1) off[E] = base;
  for (int p = lo; p < hi; ++p) {
    const int64_t e = idx[p];
    if (e >= 0 && e < E) {
      const int pos = hist[(int)e * MR_THREADS + tid]++;
      tok[pos] = p / k;
      wsel[pos] = w[p];
    }
  }
}

// ---------------------------------------------------------------------------------------
// One block's K loop: acc[mt][t] += A rows (xr[mt]: this lane's row + 8 q) x fp8 tiles at wb.
template <int MT, int NT>
__device__ __forceinline__ void rows_mainloop(const bf16_t* (&xr)[MT], const uint8_t* __restrict__ wb, int nks,
                                              int wid, f32x4 (&acc)[MT][NT]) {
  constexpr int R = rw_depth2<MT, NT, true>();
  const int cnt = (nks + RW_WAVES - 1) / RW_WAVES;  // ring steps of the busiest wave
  u16x8 ra[R][MT];
  u32x2 rb[R][NT];
#define MR_LOAD(s, i)                                                                                        \
  {                                                                                                          \
    const int k_ = min(wid + RW_WAVES * (i), nks - 1);                                                     \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) rb[s][t] =                                                \
        __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(wb + (((int64_t)t * nks + k_) << 9)));    \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) ra[s][mt] = MP_LOAD_A_FRAG(xr[mt] + (k_ << 5));        \
  }
#pragma unroll
  for (int s = 0; s < R; ++s) MR_LOAD(s, s)
  for (int i0 = 0; i0 < cnt; i0 += R) {
#pragma unroll
    for (int s = 0; s < R; ++s) {
      if (wid + RW_WAVES * (i0 + s) < nks) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const u16x8 b = f8w_to_bf16(rb[s][t]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][t] = mfma16(ra[s][mt], b, acc[mt][t]);
        }
      }
      MR_LOAD(s, i0 + s + R)
    }
  }
#undef MR_LOAD
}

// Sum the four waves' partial tiles through LDS in wave order, in passes of MR_QC quads; wave w
// finishes units w, w + 4, ... of a pass, a unit being STEP consecutive quads (2: a gate tile and its
// up tile): fn(mt, t, v[STEP]).  Starts with a barrier: the previous block has finished reading red.
template <int MT, int NT, int STEP, class Fn>
__device__ __forceinline__ void rows_reduce(const f32x4 (&acc)[MT][NT], f32x4* red, int wid, int lane, Fn&& fn) {
  constexpr int Q = MT * NT;
  constexpr int QC = Q < MR_QC ? Q : MR_QC;
  static_assert(QC % STEP == 0 && NT % STEP == 0, "a unit stays inside one pass and one row tile");
#pragma unroll
  for (int p0 = 0; p0 < Q; p0 += QC) {
    __syncthreads();
#pragma unroll
    for (int qd = p0; qd < p0 + QC && qd < Q; ++qd) red[(wid * QC + qd - p0) * 64 + lane] = acc[qd / NT][qd % NT];
    __syncthreads();
    for (int u = wid; u < QC / STEP; u += RW_WAVES) {
      const int qd = p0 + u * STEP;
      if (qd >= Q) break;
      f32x4 v[STEP];
#pragma unroll
      for (int s = 0; s < STEP; ++s) {
        v[s] = red[(qd + s - p0) * 64 + lane];
#pragma unroll
        for (int wv = 1; wv < RW_WAVES; ++wv) v[s] += red[(wv * QC + qd + s - p0) * 64 + lane];
      }
      fn(qd / NT, qd % NT, v);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Gate/up + SwiGLU of one block: pairs [pb, pb + r) of expert e, r <= 16 MT.
template <int MT, int NT>
__device__ __forceinline__ void gate_up_block(const bf16_t* __restrict__ x, const int32_t* __restrict__ tok,
                                              const uint8_t* __restrict__ wb, const float (&sc)[NT],
                                              bf16_t* __restrict__ out, int T, int H, int F, int tile0, int pb,
                                              int r, f32x4* red) {
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;
  const bf16_t* xr[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int t = min(max(tok[pb + min(mt * 16 + c, r - 1)], 0), T - 1);
    xr[mt] = x + (int64_t)t * H + 8 * q;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mt][t] = (f32x4)(0.f);
  rows_mainloop<MT, NT>(xr, wb, H >> 5, wid, acc);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[mt][t][j] *= sc[t];
  rows_reduce<MT, NT, 2>(acc, red, wid, lane, [&](int mt, int t, const f32x4(&v)[2]) {
    const int col = ((tile0 + t) >> 1) * 16 + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = mt * 16 + q * 4 + j;
      if (row >= r) continue;
      const float g = v[0][j];
      out[(int64_t)(pb + row) * F + col] = f2bf(g / (1.f + __expf(-g)) * v[1][j]);  // fp32 SwiGLU, one rounding
    }
  });
}

template <int NT>
__device__ __forceinline__ void gate_up_expert(const bf16_t* __restrict__ x, const uint8_t* __restrict__ w8,
                                               const float* __restrict__ wsc, const int32_t* __restrict__ tok,
                                               bf16_t* __restrict__ out, int T, int H, int F, int e, int tile0,
                                               int p0, int p1, f32x4* red) {
  const int lane = threadIdx.x & 63, N = 2 * F;
  const uint8_t* wb = w8 + (int64_t)e * N * H + ((int64_t)tile0 * (H >> 5)) * 512 + lane * 8;
  float sc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) sc[t] = wsc[(int64_t)e * N + (tile0 + t) * 16 + (lane & 15)];
  for (int pb = p0; pb < p1; pb += 64) {
    const int r = min(64, p1 - pb);
    switch ((r + 15) >> 4) {
      case 1: gate_up_block<1, NT>(x, tok, wb, sc, out, T, H, F, tile0, pb, r, red); break;
      case 2: gate_up_block<2, NT>(x, tok, wb, sc, out, T, H, F, tile0, pb, r, red); break;
      case 3: gate_up_block<3, NT>(x, tok, wb, sc, out, T, H, F, tile0, pb, r, red); break;
      default: gate_up_block<4, NT>(x, tok, wb, sc, out, T, H, F, tile0, pb, r, red); break;
    }
  }
}

// Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER): off, then what the first loads need.
template <int NTB, int NTS>
__global__ __launch_bounds__(MR_THREADS) void moe_rows_gate_up_kernel(const int32_t* __restrict__ off,
                                                                      const int32_t* __restrict__ tok,
                                                                      const bf16_t* __restrict__ x,
                                                                      const uint8_t* __restrict__ w8, int T, int P,
                                                                      int H, int F, int n_big,
                                                                      const float* __restrict__ wsc,
                                                                      bf16_t* __restrict__ out) {
  const int e = blockIdx.y;
  const int p0 = __builtin_amdgcn_readfirstlane(max(off[e], 0));
  const int p1 = __builtin_amdgcn_readfirstlane(min(off[e + 1], P));
  if (p1 <= p0) return;  // unrouted: none of this expert's weights or scales is read
  __shared__ __attribute__((aligned(16))) f32x4 red[RW_WAVES * (4 * NTB < MR_QC ? 4 * NTB : MR_QC) * 64];
  const int b = blockIdx.x;
  if (b < n_big) {
    gate_up_expert<NTB>(x, w8, wsc, tok, out, T, H, F, e, b * NTB, p0, p1, red);
  } else {
    gate_up_expert<NTS>(x, w8, wsc, tok, out, T, H, F, e, n_big * NTB + (b - n_big) * NTS, p0, p1, red);
  }
}

// ---------------------------------------------------------------------------------------
// Down + combine of one block into the workgroup's columns of the fp32 workspace.
template <int MT, int NT>
__device__ __forceinline__ void down_block(const bf16_t* __restrict__ act, const int32_t* __restrict__ tok,
                                           const float* __restrict__ wsel, const uint8_t* __restrict__ wb,
                                           const float (&sc)[NT], float* __restrict__ ws, int T, int H, int F,
                                           int tile0, int pb, int r, f32x4* red) {
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;
  const bf16_t* xr[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xr[mt] = act + (int64_t)(pb + min(mt * 16 + c, r - 1)) * F + 8 * q;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mt][t] = (f32x4)(0.f);
  rows_mainloop<MT, NT>(xr, wb, F >> 5, wid, acc);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[mt][t][j] *= sc[t];
  rows_reduce<MT, NT, 1>(acc, red, wid, lane, [&](int mt, int t, const f32x4(&v)[1]) {
    const int col = (tile0 + t) * 16 + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = mt * 16 + q * 4 + j;
      if (row >= r) continue;
      float* dst = ws + (int64_t)min(max(tok[pb + row], 0), T - 1) * H + col;
      *dst += wsel[pb + row] * v[0][j];
    }
  });
}

template <int NT>
__device__ __forceinline__ void down_body(const bf16_t* __restrict__ act, const uint8_t* __restrict__ w8,
                                          const float* __restrict__ wsc, const int32_t* __restrict__ off,
                                          const int32_t* __restrict__ tok, const float* __restrict__ wsel,
                                          float* __restrict__ ws, bf16_t* __restrict__ y, int64_t ys, int T, int P,
                                          int E, int H, int F, int tile0, f32x4* red) {
  const int tid = threadIdx.x, lane = tid & 63;
  // this workgroup's columns of the workspace start at zero (16-byte chunks: NT * 4 per row)
  for (int i = tid; i < T * NT * 4; i += MR_THREADS) {
    float* p = ws + (int64_t)(i / (NT * 4)) * H + tile0 * 16 + (i % (NT * 4)) * 4;
    *reinterpret_cast<f32x4*>(p) = (f32x4)(0.f);
  }
  for (int e = 0; e < E; ++e) {
    const int p0 = __builtin_amdgcn_readfirstlane(max(off[e], 0));
    const int p1 = __builtin_amdgcn_readfirstlane(min(off[e + 1], P));
    if (p1 <= p0) continue;  // unrouted: nothing of this expert is read
    const uint8_t* wb = w8 + (int64_t)e * H * F + ((int64_t)tile0 * (F >> 5)) * 512 + lane * 8;
    float sc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sc[t] = wsc[(int64_t)e * H + (tile0 + t) * 16 + (lane & 15)];
    for (int pb = p0; pb < p1; pb += 64) {
      const int r = min(64, p1 - pb);
      switch ((r + 15) >> 4) {
        case 1: down_block<1, NT>(act, tok, wsel, wb, sc, ws, T, H, F, tile0, pb, r, red); break;
        case 2: down_block<2, NT>(act, tok, wsel, wb, sc, ws, T, H, F, tile0, pb, r, red); break;
        case 3: down_block<3, NT>(act, tok, wsel, wb, sc, ws, T, H, F, tile0, pb, r, red); break;
        default: down_block<4, NT>(act, tok, wsel, wb, sc, ws, T, H, F, tile0, pb, r, red); break;
      }
    }
  }
  __syncthreads();  // every wave's adds are done (and, with no routed expert, the zeroes written)
  for (int i = tid; i < T * NT * 4; i += MR_THREADS) {
    const int row = i / (NT * 4), col = tile0 * 16 + (i % (NT * 4)) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(ws + (int64_t)row * H + col);
    u16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = f2bf(v[j]);
    *reinterpret_cast<u16x4*>(y + (int64_t)row * ys + col) = o;
  }
}

template <int NTB, int NTS>
__global__ __launch_bounds__(MR_THREADS) void moe_rows_down_kernel(const int32_t* __restrict__ off,
                                                                   const bf16_t* __restrict__ act,
                                                                   const uint8_t* __restrict__ w8, int T, int P, int E,
                                                                   int H, int F, int n_big,
                                                                   const int32_t* __restrict__ tok,
                                                                   const float* __restrict__ wsel,
                                                                   const float* __restrict__ wsc,
                                                                   float* __restrict__ ws, bf16_t* __restrict__ y,
                                                                   int64_t ys) {
  __shared__ __attribute__((aligned(16))) f32x4 red[RW_WAVES * 4 * NTB * 64];
  const int b = blockIdx.x;
  if (b < n_big) {
    down_body<NTB>(act, w8, wsc, off, tok, wsel, ws, y, ys, T, P, E, H, F, b * NTB, red);
  } else {
    down_body<NTS>(act, w8, wsc, off, tok, wsel, ws, y, ys, T, P, E, H, F, n_big * NTB + (b - n_big) * NTS, red);
  }
}

// ---------------------------------------------------------------------------------------
// Shapes the three launches take: any T > 0 whose pairs fit the grouping kernel, 1 <= k <= E <=
// MR_MAX_E, K of each GEMM a multiple of 128 (whole ring turns of the four waves), 32-bit row offsets.
static bool rows_shape_ok(int T, int E, int k, int H, int F) {
  return T > 0 && E > 0 && E <= MR_MAX_E && k > 0 && k <= E && (int64_t)T * k <= MR_MAX_PAIRS && H > 0 && F > 0 &&
         H % 128 == 0 && F % 128 == 0;
}

static int launch_rows_gate_up(const void* x, const void* w8, const float* wsc, const int32_t* off, const int32_t* tok,
                               void* out, int T, int P, int E, int H, int F, hipStream_t stream, bool dry) {
  RowsSplit s;
  if (!rows_split(2 * F, 1, s)) return 1;
  if (dry) return 0;
#define MP_RGU(B_, S_)                                                                                          \
  hipLaunchKernelGGL((moe_rows_gate_up_kernel<B_, S_>), dim3(s.G, E), dim3(MR_THREADS), 0, stream, off, tok,    \
                     (const bf16_t*)x, (const uint8_t*)w8, T, P, H, F, s.n_big, wsc, (bf16_t*)out);             \
  return 0
  switch (s.ntb) {
    case 2: MP_RGU(2, 2);
    case 4: MP_RGU(4, 2);
    case 6: MP_RGU(6, 4);
    case 8: MP_RGU(8, 6);
    default: return 1;
  }
#undef MP_RGU
}

static int launch_rows_down(const void* act, const void* w8, const float* wsc, const int32_t* off, const int32_t* tok,
                            const float* wsel, float* ws, void* y, int64_t ys, int T, int P, int E, int H, int F,
                            hipStream_t stream, bool dry) {
  RowsSplit s;
  if (!rows_split(H, 0, s)) return 1;
  if (dry) return 0;
#define MP_RDN(B_, S_)                                                                                          \
  hipLaunchKernelGGL((moe_rows_down_kernel<B_, S_>), dim3(s.G), dim3(MR_THREADS), 0, stream, off,               \
                     (const bf16_t*)act, (const uint8_t*)w8, T, P, E, H, F, s.n_big, tok, wsel, wsc, ws,        \
                     (bf16_t*)y, ys);                                                                           \
  return 0
  switch (s.ntb) {
    case 1: MP_RDN(1, 1);
    case 2: MP_RDN(2, 1);
    case 3: MP_RDN(3, 2);
    case 4: MP_RDN(4, 3);
    default: return 1;
  }
#undef MP_RDN
}

}  // namespace mp

// Group the T x k routed (token, expert) pairs by expert: idx int64 [T][k], w fp32 [T][k] -> off int32
// [E + 1] (exclusive prefix sums of the per-expert counts), tok int32 [T k], wsel fp32 [T k], pairs in
// (expert, token) order.  Returns 1 when the shape is not covered (nothing launched), < 0 for a bad call.
extern "C" int mp_moe_group(const int64_t* idx, const float* w, int32_t* off, int32_t* tok, float* wsel, int T, int k,
                            int E, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (idx == nullptr || w == nullptr || off == nullptr || tok == nullptr || wsel == nullptr) return -1;
  if (T <= 0 || E <= 0 || E > MR_MAX_E || k <= 0 || k > E || (int64_t)T * k > MR_MAX_PAIRS) return 1;
  hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(MR_THREADS), 0, stream, idx, w, off, tok, wsel, T * k, k, E);
  return (int)hipGetLastError();
}

// Gate/up + SwiGLU on gathered rows: x bf16 row-major [T][H] (contiguous), w8 [E][2F/16][H/32][64][8],
// wsc [E][2F], off / tok as mp_moe_group leaves them (P = T k pairs), out bf16 row-major [P][F].
extern "C" int mp_moe_gate_up_w8_rows(const void* x, const void* w8, const float* wsc, const int32_t* off,
                                      const int32_t* tok, void* out, int T, int P, int E, int H, int F,
                                      hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (x == nullptr || w8 == nullptr || wsc == nullptr || off == nullptr || tok == nullptr || out == nullptr || P < T ||
      (T > 0 && P % T))
    return -1;
  if (!rows_shape_ok(T, E, P / T, H, F)) return 1;
  const int rc = launch_rows_gate_up(x, w8, wsc, off, tok, out, T, P, E, H, F, stream, false);
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

// Down + combine: act bf16 row-major [P][F] as mp_moe_gate_up_w8_rows leaves it, w8 [E][H/16][F/32][64][8],
// wsc [E][H], wsel fp32 [P], ws fp32 [T][H] scratch, y bf16 row-major [T][H] (row stride y_stride, a
// multiple of 4 elements).
extern "C" int mp_moe_down_w8_rows(const void* act, const void* w8, const float* wsc, const int32_t* off,
                                   const int32_t* tok, const float* wsel, float* ws, void* y, int64_t y_stride, int T,
                                   int P, int E, int H, int F, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (act == nullptr || w8 == nullptr || wsc == nullptr || off == nullptr || tok == nullptr || wsel == nullptr ||
      ws == nullptr || y == nullptr || y_stride < H || y_stride % 4 || P < T || (T > 0 && P % T))
    return -1;
  if (!rows_shape_ok(T, E, P / T, H, F)) return 1;
  const int rc = launch_rows_down(act, w8, wsc, off, tok, wsel, ws, y, y_stride, T, P, E, H, F, stream, false);
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

// dry dispatch of the three launches
extern "C" int mp_moe_rows_ok(int T, int E, int k, int H, int F) {
  using namespace mp;
  if (!rows_shape_ok(T, E, k, H, F)) return 0;
  const int a = launch_rows_gate_up(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, T, T * k, E, H, F, 0, true);
  const int b = launch_rows_down(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, T, T * k,
                                 E, H, F, 0, true);
  return a == 0 && b == 0;
}
