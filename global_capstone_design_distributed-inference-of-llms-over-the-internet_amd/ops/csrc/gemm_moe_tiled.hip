// Tiled grouped W8A16 GEMMs of a sparse-MoE (Mixtral) MLP for LARGE steps (prefill rounds of hundreds to
// thousands of rows).  gemm_moe_rows.hip walks an expert's rows in 64-row blocks and every block streams the
// expert's whole weight again; here the work is cut in two dimensions, gemm_w8_rows.hip's way, so a weight
// byte is taken in once per 128-ROW block (from L2 after the first) and feeds four row tiles per convert.
// Three launches after mp_moe_group (gemm_moe_rows.hip; untouched), no host sync:
//
//   mp_moe_gate_up_w8_tiled  act[p] = SwiGLU(x[tok[p]] . gate_up[e(p)]^T)          bf16 [P][F]
//   mp_moe_down_w8_tiled     ws[tok[p]][j(p)] = wsel[p] * ((act[p] . down[e(p)]^T) * ws[e])   fp32 [T][k][H]
//   mp_moe_combine_tiled     y[t] = bf16(ws[t][0] + ws[t][1] + ...)                 bf16 [T][H], row stride
//
// Weights: gemm_moe.hip's stacked W8A16 layout (uint8 [E][N/16][K/32][64][8] + fp32 [E][N]).  P = T k pairs.
//
// Slots.  The host knows the shape, not the per-expert counts n_e, so the grid has S = floor(P / 128) + E
// row-block SLOTS, at least sum_e ceil(n_e / 128).  A workgroup turns its slot into (expert e, block b of e)
// by walking off[] (wave-uniform loads, E <= 32); a slot past the last real block returns before any other
// load, and an unrouted expert has no slot: none of its weights or scales is read.
// Split.  A workgroup owns up to 128 of e's pair rows x a group of column tiles: gemm_w8_rows.hip's wide
// geometry (2 x 4 waves of 4 x 4 tiles, 512 threads, k-stages of KU = 2 slices - 4 spill there and here) and
// its column rule for S row blocks (gemm_rows_plan.h w8r_plan_blocks): a function of (P, E, H, F) only.
// A operand.  Gate/up GATHERS: a lane's 16-byte load is x[tok[p]][32 ks + 8 q ..]; the row pointers are
// formed once per block, tok clamped to [0, T - 1]; down reads act[p], contiguous.  Wave w loads fragments
// w, w + 8 of a stage, holds them for one stage and writes them lane-linear into one of two LDS buffers that
// the column waves share.  Rows past the expert's last pair read its last real row and store nothing.
// B operand.  The fp8 fragments of the wave's column tiles in a two-stage register ring, f8w_to_bf16 right
// before the four MFMAs (v_mfma_f32_16x16x32_bf16) of the wave's row tiles.  Pipeline order: gemm_w8_rows.hip.
// Epilogues.  Channel scales multiply the fp32 accumulators.  Gate/up: fp32 SwiGLU over the 16-row gate/up
// interleave, one rounding.  Down: row p goes, in fp32, to slot j = #{i : 0 <= idx[t][i] < e} of its token
// t = tok[p] - the pair's rank among the token's valid experts, so every (t, j) has one writer (a token meets
// an expert at most once) and combine adds a token's slots in ascending expert order over its valid ids only:
// slots never written are never read.  No atomics, no k split, every wave walks K upwards, nobody reads what
// another workgroup of the same launch wrote: the same bits on every run.
//
// Placement (never correctness).  order 0, the default: column groups fastest - the workgroups of one slot are
// dispatched together and a column group stays on one XCD when their number is a multiple of 8 (the rule
// rounds to one where it can), so an expert's consecutive slots meet a group's weights on the same XCD.
// order 1 (lab knob MPAMD_MOE_TILED_ORDER=1): w8r_place over the S slots, where an XCD takes ONE column group
// through all slots in turn.  Layer A/B at Mixtral-8x7B shapes, same routing (profiles/moe_tiled/README.md):
// order 0 is ahead by 6 % at 512 rows, 3 % at 2048, 4 % at 4096 and 2 % at 8192 and level below 512, so it
// is the default; why was not analysed.
//
// Packed fp32.  Built WITHOUT ops/build.py's _NO_PK_F32 file flag: the only fp32 VALU work is the epilogues'
// independent multiplies and combine's adds, v_pk_mul_f32 / v_pk_add_f32 round each half as the scalar forms
// do, nothing here can contract to an fma, and no other kernel has to match these outputs bit for bit (the
// route is opt-in because its summation order is its own).  Registers / LDS / scratch: profiles/moe_tiled.
#include "moe_tiled_common.h"

namespace mp {

// DOWN = false: gate/up (x gathered through tok, SwiGLU, bf16 rows of out).  DOWN = true: act rows in place,
// fp32 rows of the per-pair workspace.  Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER).
template <bool DOWN>
__global__ __launch_bounds__(512) void moe_tiled_kernel(const int32_t* __restrict__ off,
                                                        const int32_t* __restrict__ tok,
                                                        const bf16_t* __restrict__ x,
                                                        const uint8_t* __restrict__ w8, int T, int P, int E, int N,
                                                        int K, int S, int nbig, int NBB, int NBS, int order,
                                                        const float* __restrict__ wsc, bf16_t* __restrict__ out,
                                                        const float* __restrict__ wsel,
                                                        const int64_t* __restrict__ idx, float* __restrict__ ws,
                                                        int k) {
  constexpr int MW = 4, NW = 4, WM = 2, WN = 4, KU = 2;
  constexpr int WAVES = WM * WN, BMT = WM * MW, FA = BMT * KU, J = FA / WAVES, SB = FA * 1024;
  constexpr int STEP = DOWN ? 1 : 2;
  static_assert(16 * BMT == MT_BM && 2 * SB <= W8R_LDS_BYTES && FA % WAVES == 0, "the wide geometry");
  int cg, slot;
  if (order == 0) {
    const int NB = gridDim.x / S;
    cg = blockIdx.x % NB;
    slot = blockIdx.x / NB;
  } else {
    w8r_place(S, cg, slot);
  }
  int e, p0, n;
  if (!mt_slot(off, E, P, slot, e, p0, n)) return;

  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * SB];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wid % WM, wn = wid / WM;
  const int c = lane & 15, q = lane >> 4;
  const int tile0 = cg < nbig ? cg * NBB : nbig * NBB + (cg - nbig) * NBS;
  const int ug = (cg < nbig ? NBB : NBS) / STEP;            // units of this column group (>= 1)
  const int u0 = wn * ug / WN, u1 = (wn + 1) * ug / WN;     // ... of this wave
  const int ntw = (u1 - u0) * STEP;                         // its column tiles: 0 .. NW (wave-uniform)
  const int tw0 = tile0 + u0 * STEP;                        // its first (u0 < ug: inside the group)
  const int nks = K >> 5, nst = nks / KU;

  // this wave's J activation fragments of a stage: f = wid + WAVES j is k-slice f / BMT, row tile f % BMT
  const bf16_t* xp[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int f = wid + WAVES * j;
    const int p = p0 + min((f % BMT) * 16 + c, n - 1);
    const int row = DOWN ? p : min(max(tok[p], 0), T - 1);
    xp[j] = x + (int64_t)row * K + (f / BMT) * 32 + 8 * q;
  }
  // its weight stream: tile t at wb + t * nks * 512; tiles past ntw repeat a real one (never used)
  const uint8_t* wb = w8 + ((int64_t)e * (N >> 4) + tw0) * nks * 512 + lane * 8;
  int tc[NW];
  float sc[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t) {
    tc[t] = max(min(t, ntw - 1), 0);
    sc[t] = wsc[(int64_t)e * N + (tw0 + tc[t]) * 16 + c];
  }

  f32x4 acc[MW][NW];
#pragma unroll
  for (int mt = 0; mt < MW; ++mt)
#pragma unroll
    for (int t = 0; t < NW; ++t) acc[mt][t] = (f32x4)(0.f);

  u16x8 stg[J];
  u32x2 rb[2][KU][NW];
#define MT_LOAD_A(st)                                                                                   \
  {                                                                                                     \
    const int s_ = min(st, nst - 1);                                                                    \
    _Pragma("unroll") for (int j = 0; j < J; ++j) stg[j] = MP_LOAD_A_FRAG(xp[j] + (int64_t)s_ * (KU * 32)); \
  }
#define MT_STORE_A(buf)                                                                                 \
  _Pragma("unroll") for (int j = 0; j < J; ++j) *reinterpret_cast<u16x8*>(                             \
      smem + (buf) * SB + (wid + WAVES * j) * 1024 + lane * 16) = stg[j];
#define MT_LOAD_B(d, st)                                                                                \
  {                                                                                                     \
    const int s_ = min(st, nst - 1);                                                                    \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) _Pragma("unroll") for (int t = 0; t < NW; ++t)       \
        rb[d][u][t] = *reinterpret_cast<const u32x2*>(wb + (((int64_t)tc[t] * nks + s_ * KU + u) << 9)); \
  }
#define MT_MMA(d)                                                                                       \
  {                                                                                                     \
    const unsigned char* sb_ = smem + (d) * SB + lane * 16;                                             \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                                    \
      u16x8 a_[MW];                                                                                     \
      _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) a_[mt] =                                        \
          *reinterpret_cast<const u16x8*>(sb_ + (u * BMT + wm * MW + mt) * 1024);                       \
      _Pragma("unroll") for (int t = 0; t < NW; ++t) {                                                  \
        if (t < ntw) {                                                                                  \
          const u16x8 b_ = f8w_to_bf16(rb[d][u][t]);                                                    \
          _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) acc[mt][t] = mfma16(a_[mt], b_, acc[mt][t]); \
        }                                                                                               \
      }                                                                                                 \
    }                                                                                                   \
  }

  MT_LOAD_A(0)
  MT_LOAD_B(0, 0)
  MT_STORE_A(0)
  MT_LOAD_A(1)
  lds_barrier();
  // at the top of step s: LDS buffer s & 1 holds stage s of A, stg stage s + 1 (in flight), ring slot
  // s & 1 stage s of B
  for (int s0 = 0; s0 < nst; s0 += 2) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int s = s0 + d;
      if (s >= nst) break;
      MT_LOAD_B(d ^ 1, s + 1)
      MT_MMA(d)
      MT_STORE_A(d ^ 1)  // (at s = nst - 1 a clamped copy nobody reads: no branch around the pipeline)
      MT_LOAD_A(s + 2)
      lds_barrier();
    }
  }
#undef MT_MMA
#undef MT_LOAD_B
#undef MT_STORE_A
#undef MT_LOAD_A

  // epilogue: scales in fp32; rows past n and tiles past ntw store nothing
  if (ntw == 0) return;
#pragma unroll
  for (int mt = 0; mt < MW; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = (wm * MW + mt) * 16 + q * 4 + j;
      if (row >= n) continue;
      const int p = p0 + row;
      if constexpr (DOWN) {
        const int t = min(max(tok[p], 0), T - 1);
        int rank = 0;  // the pair's slot in its token: valid expert ids below e
        for (int i = 0; i < k; ++i) {
          const int64_t id = idx[(int64_t)t * k + i];
          rank += (id >= 0 && id < e) ? 1 : 0;
        }
        const float wv = wsel[p];
        float* dst = ws + ((int64_t)t * k + rank) * N;
#pragma unroll
        for (int tt = 0; tt < NW; ++tt)
          if (tt < ntw) dst[(tw0 + tt) * 16 + c] = wv * (acc[mt][tt][j] * sc[tt]);
      } else {
        bf16_t* dst = out + (int64_t)p * (N >> 1);
#pragma unroll
        for (int tt = 0; tt < NW; tt += 2) {
          if (tt >= ntw) continue;
          const float g = acc[mt][tt][j] * sc[tt];
          dst[((tw0 + tt) >> 1) * 16 + c] = f2bf(g / (1.f + __expf(-g)) * (acc[mt][tt + 1][j] * sc[tt + 1]));
        }
      }
    }
}

// y[t] = bf16(ws[t][0] + ... + ws[t][v - 1]), v = the token's valid expert ids: one thread per 4 columns.
constexpr int MT_CB = 256;
__global__ __launch_bounds__(MT_CB) void moe_combine_tiled_kernel(const float* __restrict__ ws,
                                                                  const int64_t* __restrict__ idx,
                                                                  bf16_t* __restrict__ y, int64_t ys, int T, int k,
                                                                  int E, int H) {
  const int h4 = H >> 2;
  const int64_t i = (int64_t)blockIdx.x * MT_CB + threadIdx.x;
  if (i >= (int64_t)T * h4) return;
  const int t = (int)(i / h4), col = (int)(i % h4) * 4;
  int v = 0;
  for (int j = 0; j < k; ++j) {
    const int64_t id = idx[(int64_t)t * k + j];
    v += (id >= 0 && id < E) ? 1 : 0;
  }
  const float* src = ws + (int64_t)t * k * H + col;
  f32x4 s = (f32x4)(0.f);
  if (v > 0) s = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src));
  for (int j = 1; j < v; ++j) s += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (int64_t)j * H));
  u16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f2bf(s[j]);
  *reinterpret_cast<u16x4*>(y + (int64_t)t * ys + col) = o;
}

// One GEMM launch: N output channels (gate/up: 2F, SwiGLU pairs), depth K, over S = P / 128 + E slots.
template <bool DOWN>
static int launch_tiled(const int32_t* off, const int32_t* tok, const void* x, const void* w8, const float* wsc,
                        void* out, const float* wsel, const int64_t* idx, float* ws, int T, int P, int E, int N, int K,
                        hipStream_t stream, bool dry) {
  const int S = P / MT_BM + E;
  W8rPlan p;
  if (!w8r_plan_blocks(S, 1, N, K, DOWN ? 0 : 1, p)) return 1;
  if (dry) return 0;
  hipLaunchKernelGGL((moe_tiled_kernel<DOWN>), dim3(p.NB * S), dim3(512), 0, stream, off, tok, (const bf16_t*)x,
                     (const uint8_t*)w8, T, P, E, N, K, S, p.nbig, p.NBB, p.NBS, tiled_order(), wsc, (bf16_t*)out,
                     wsel, idx, ws, P / T);
  return 0;
}

}  // namespace mp

// Gate/up + SwiGLU: x bf16 row-major [T][H] (contiguous), w8 [E][2F/16][H/32][64][8], wsc [E][2F], off / tok
// as mp_moe_group leaves them (P = T k pairs), out bf16 row-major [P][F].  Returns 0, 1 when the shape is not
// covered (nothing launched), < 0 for a bad call, else the HIP error.
extern "C" int mp_moe_gate_up_w8_tiled(const void* x, const void* w8, const float* wsc, const int32_t* off,
                                       const int32_t* tok, void* out, int T, int P, int E, int H, int F,
                                       hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (x == nullptr || w8 == nullptr || wsc == nullptr || off == nullptr || tok == nullptr || out == nullptr || P < T ||
      (T > 0 && P % T))
    return -1;
  if (!tiled_shape_ok(T, E, P / T, H, F)) return 1;
  const int rc = launch_tiled<false>(off, tok, x, w8, wsc, out, nullptr, nullptr, nullptr, T, P, E, 2 * F, H, stream,
                                     false);
  return rc != 0 ? rc : (int)hipGetLastError();
}

// Down: act bf16 row-major [P][F], w8 [E][H/16][F/32][64][8], wsc [E][H], wsel fp32 [P], idx int64 [T][k] (the
// routing mp_moe_group sorted), ws fp32 [T][k][H]: row (t, j) = token t's j-th valid expert in ascending order.
extern "C" int mp_moe_down_w8_tiled(const void* act, const void* w8, const float* wsc, const int32_t* off,
                                    const int32_t* tok, const float* wsel, const int64_t* idx, float* ws, int T, int P,
                                    int E, int H, int F, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (act == nullptr || w8 == nullptr || wsc == nullptr || off == nullptr || tok == nullptr || wsel == nullptr ||
      idx == nullptr || ws == nullptr || P < T || (T > 0 && P % T))
    return -1;
  if (!tiled_shape_ok(T, E, P / T, H, F)) return 1;
  const int rc = launch_tiled<true>(off, tok, act, w8, wsc, nullptr, wsel, idx, ws, T, P, E, H, F, stream, false);
  return rc != 0 ? rc : (int)hipGetLastError();
}

// Combine: y bf16 [T][H] (row stride y_stride, a multiple of 4 elements) from ws as mp_moe_down_w8_tiled
// leaves it; only a token's valid ids (0 <= idx < E) are summed.
extern "C" int mp_moe_combine_tiled(const float* ws, const int64_t* idx, void* y, int64_t y_stride, int T, int k, int E,
                                    int H, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (ws == nullptr || idx == nullptr || y == nullptr || y_stride < H || y_stride % 4) return -1;
  if (T <= 0 || k <= 0 || E <= 0 || H <= 0 || H % 4 || (int64_t)T * k > MT_MAX_PAIRS) return 1;
  const int64_t blocks = ((int64_t)T * (H >> 2) + MT_CB - 1) / MT_CB;
  if (blocks >= (1ll << 31)) return 1;
  hipLaunchKernelGGL(moe_combine_tiled_kernel, dim3((unsigned)blocks), dim3(MT_CB), 0, stream, ws, idx, (bf16_t*)y,
                     y_stride, T, k, E, H);
  return (int)hipGetLastError();
}

// dry dispatch of the launches
extern "C" int mp_moe_tiled_ok(int T, int E, int k, int H, int F) {
  using namespace mp;
  if (!tiled_shape_ok(T, E, k, H, F)) return 0;
  const int a = launch_tiled<false>(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, T,
                                    T * k, E, 2 * F, H, 0, true);
  const int b = launch_tiled<true>(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, T,
                                   T * k, E, H, F, 0, true);
  return a == 0 && b == 0;
}
