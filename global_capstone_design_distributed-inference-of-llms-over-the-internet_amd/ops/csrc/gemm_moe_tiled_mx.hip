// Tiled grouped W8A8-MX GEMMs of a sparse-MoE (Mixtral) MLP for LARGE steps: gemm_moe_tiled.hip's slots, split,
// down workspace and combine with gemm_mx_rows.hip's operand formats - the fp8 expert weights go to gfx950's
// block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 as they are (no fp8 -> bf16 convert, half the matrix passes
// per k of the bf16 form) and the activations are e4m3 with one e8m0 scale per 32-element block.  Five launches
// after mp_moe_group (gemm_moe_rows.hip; untouched), no host sync:
//
//   mp_moe_quant_mx_tiled    ax, as = quant(x[tok[p]])          gather form, slot order
//   mp_moe_gate_up_mx_tiled  act[p] = SwiGLU(dequant(ax, as)[p] . gate_up[e(p)]^T)                bf16 [P][F]
//   mp_moe_quant_mx_tiled    ax, as = quant(act[p])             in-place form, slot order
//   mp_moe_down_mx_tiled     ws[tok[p]][j(p)] = wsel[p] * ((dequant(ax, as)[p] . down[e(p)]^T) * ws[e])  fp32
//   mp_moe_combine_tiled     (gemm_moe_tiled.hip, unchanged)
//
// Weights: the stacked W8A16 layout in place (uint8 [E][N/16][K/32][64][8] + fp32 [E][N]).  P = T k pairs.
// Slots: moe_tiled_common.h mt_slot, S = floor(P / 128) + E; a slot past the last real block returns before any
// other load and an unrouted expert has no slot: none of its weights, scales or activations is read.
//
// Format.  gemm_mx_rows.hip's fragment and scale map, indexed by SLOT instead of row block - a slot is the 128
// rows p0 .. p0 + 127 of ONE expert, its rows past the expert's last pair zero bytes with scale 127:
//   ax uint8 [S][8][K/128][2][64][16]    row tile mt of the slot, half h of lane l = 16 q + r
//   as uint8 [S][2][K/128][64][4]        byte i of lane 16 b + r: block b of row r of row tile 4 g + i
// so quant_mx_rows of the slot-order matrix [S * 128][K] writes the same bytes.  Dead slots are not written
// and not read.
//
// Quantizer.  A 512-thread workgroup takes one slot and one 128-deep k-step, one row tile a wave; per wave it
// is quant_mx_rows_kernel's read (lane l: 16 bytes at chunk l & 15 of row 4 p + (l >> 4): a row's k-step is 256
// contiguous bytes over sixteen lanes), block rule (mx_quant_chunk below) and 2 KiB LDS transpose
// into two lane-linear 16-byte stores.  Row r of the slot is x[tok[p0 + r]] (gather, tok clamped to [0, T - 1]
// as the tiled gate/up clamps it) or x[p0 + r] (in place); r >= n reads nothing.  Every byte of a live slot is
// written once.
//
// GEMMs.  Grid: column groups x S slots, gemm_rows_plan.h w8r_plan_blocks' column rule, the tiled kernel's
// blockIdx order 0 by default (MPAMD_MOE_TILED_ORDER=1: w8r_place).  The wide geometry (2 x 4 waves of 4 x 4
// tiles, 512 threads).  A stage, B ring, MFMA step and their order are mx_rows_stage.h's: one 128-deep step =
// 8 row tiles x 2 KiB + 2 x 256 B of scale dwords through registers into double-buffered LDS (33 KiB), the
// barrier on lgkmcnt only; all 8 row tiles of a live slot exist, so no clamp and no gather here.  B: the
// expert's 32 bytes per lane and step, two-stage register ring, weight scale 127.
// Epilogues: gemm_moe_tiled.hip's.  Channel scales multiply the fp32 accumulators; gate/up: fp32 SwiGLU over
// the 16-row gate/up interleave, one rounding, row p0 + r of act for r < n; down: row p in fp32 into slot
// j = #{i : 0 <= idx[t][i] < e} of token t = tok[p].  No atomics, no k split: the same bits on every run.
//
// Packed fp32: built without ops/build.py's _NO_PK_F32, as gemm_moe_tiled.hip is and for its reasons.
// Registers / LDS / scratch: profiles/moe_tiled_mx/README.md.
#include "moe_tiled_common.h"
#include "mx_common.h"
#include "mx_rows_stage.h"

namespace mp {

// quant_mx_rows_kernel's block rule on one lane's 16-byte chunk (kept there in line: that file compiles to what
// it did): 8 values of chunk ch = 4 s + q of a row's 128-deep step, the row's sixteen chunks in sixteen
// consecutive lanes.  The block's four chunks sit in lanes ch ^ 1, ch ^ 4, ch ^ 5: two shuffles give the block
// maximum (all lanes active).  Returns the 8 e4m3 bytes; e: the block's e8m0 scale.
__device__ __forceinline__ u32x2 mx_quant_chunk(const u16x8 v, int& e) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf2f(v[j])));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 4));
  e = mx_e8m0(amax);
  const float sc = mx_inv_scale(e);
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(bf2f(v[j]) * sc, -448.f), 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return (u32x2){(unsigned)lo, (unsigned)hi};
}

// GATHER: row r of the slot is x[tok[p0 + r]], else x[p0 + r].  Addresses first (gemm_kernels.h KERNARG ORDER).
template <bool GATHER>
__global__ __launch_bounds__(512) void moe_quant_mx_kernel(const int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ tok,
                                                           const bf16_t* __restrict__ x, uint8_t* __restrict__ ax,
                                                           uint8_t* __restrict__ as, int T, int P, int E, int nkb) {
  const int slot = blockIdx.x / nkb, kb = blockIdx.x - slot * nkb;
  int e, p0, n;
  if (!mt_slot(off, E, P, slot, e, p0, n)) return;

  __shared__ __attribute__((aligned(16))) unsigned char smem[8 * 2048];
  const int lane = threadIdx.x & 63, mt = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // row tile 0 .. 7
  const int ch = lane & 15, rr = lane >> 4, s = ch >> 2, q = ch & 3;
  unsigned char* sw = smem + mt * 2048;
  const int64_t K = (int64_t)nkb * 128;
  u16x8 v[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = mt * 16 + 4 * p + rr;
    v[p] = (u16x8)(0);
    if (r < n) {
      const int row = GATHER ? min(max(tok[p0 + r], 0), T - 1) : p0 + r;
      v[p] = *reinterpret_cast<const u16x8*>(x + row * K + 128 * kb + 8 * ch);
    }
  }
  uint8_t* sd = as + (((int64_t)(2 * slot + (mt >> 2)) * nkb + kb) << 8) + (mt & 3);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = 4 * p + rr;
    int sc;
    *reinterpret_cast<u32x2*>(sw + (s >> 1) * 1024 + (16 * q + r) * 16 + 8 * (s & 1)) = mx_quant_chunk(v[p], sc);
    if ((ch & 5) == 0) sd[(16 * (2 * (s >> 1) + (q >> 1)) + r) * 4] = (uint8_t)sc;
  }
  __syncthreads();
  uint8_t* dst = ax + (((int64_t)(8 * slot + mt) * nkb + kb) << 11) + lane * 16;
  *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(sw + lane * 16);
  *reinterpret_cast<u32x4*>(dst + 1024) = *reinterpret_cast<const u32x4*>(sw + 1024 + lane * 16);
}

// DOWN = false: gate/up (SwiGLU, bf16 rows of out).  DOWN = true: fp32 rows of the per-pair workspace.
// Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER).
template <bool DOWN>
__global__ __launch_bounds__(512) void moe_tiled_mx_kernel(const int32_t* __restrict__ off,
                                                           const uint8_t* __restrict__ ax,
                                                           const uint8_t* __restrict__ as,
                                                           const uint8_t* __restrict__ w8, int P, int E, int N, int K,
                                                           int S, int nbig, int NBB, int NBS, int order,
                                                           const float* __restrict__ wsc, bf16_t* __restrict__ out,
                                                           const int32_t* __restrict__ tok,
                                                           const float* __restrict__ wsel,
                                                           const int64_t* __restrict__ idx, float* __restrict__ ws,
                                                           int T, int k) {
  constexpr int MW = 4, NW = 4, WM = 2, WN = 4;
  using G = MxrGeom<MW, NW, WM, WN>;
  constexpr int BMT = G::BMT, J = G::J, SB = G::STAGE_BYTES, WAVES = G::WAVES, SOFF = G::FA * 1024;
  constexpr int STEP = DOWN ? 1 : 2;
  static_assert(G::BM == MT_BM && G::THREADS == 512, "the wide geometry: a slot is one row block");
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

  __shared__ __attribute__((aligned(16))) unsigned char smem[G::LDS_BYTES];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wid % WM, wn = wid / WM;
  const int c = lane & 15, q = lane >> 4;
  const int tile0 = cg < nbig ? cg * NBB : nbig * NBB + (cg - nbig) * NBS;
  const int ug = (cg < nbig ? NBB : NBS) / STEP;            // units of this column group (>= 1)
  const int u0 = wn * ug / WN, u1 = (wn + 1) * ug / WN;     // ... of this wave
  const int ntw = (u1 - u0) * STEP;                         // its column tiles: 0 .. NW (wave-uniform)
  const int tw0 = tile0 + u0 * STEP;                        // its first (u0 < ug: inside the group)
  const int nks = K >> 5, nst = K >> 7;

  // this wave's J activation fragments of a stage: f = wid + WAVES j is row tile f / 2 of the slot, half f % 2.
  // Wave wid < WM also stages row wave wid's scale dwords
  const uint8_t* xp[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int f = wid + WAVES * j;
    xp[j] = ax + (((int64_t)(slot * BMT + (f >> 1)) * nst) << 11) + (f & 1) * 1024 + lane * 16;
  }
  const uint8_t* sp = as + (((int64_t)(slot * WM + min(wid, WM - 1)) * nst) << 8) + lane * 4;
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

  u32x4 stg[J];
  unsigned stgs = 0;
  u32x8 rb[2][NW];
  MXR_PIPELINE()

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

// One GEMM launch: N output channels (gate/up: 2F, SwiGLU pairs), depth K, over S = P / 128 + E slots.
template <bool DOWN>
static int launch_tiled_mx(const int32_t* off, const void* ax, const void* as, const void* w8, const float* wsc,
                           void* out, const int32_t* tok, const float* wsel, const int64_t* idx, float* ws, int T,
                           int P, int E, int N, int K, hipStream_t stream) {
  const int S = P / MT_BM + E;
  W8rPlan p;
  if (!w8r_plan_blocks(S, 1, N, K, DOWN ? 0 : 1, p)) return 1;
  hipLaunchKernelGGL((moe_tiled_mx_kernel<DOWN>), dim3(p.NB * S), dim3(512), 0, stream, off, (const uint8_t*)ax,
                     (const uint8_t*)as, (const uint8_t*)w8, P, E, N, K, S, p.nbig, p.NBB, p.NBS, tiled_order(), wsc,
                     (bf16_t*)out, tok, wsel, idx, ws, T, P / T);
  return 0;
}

}  // namespace mp

// Slot-order MX quantizer: x bf16 row-major, contiguous - [T][K] with tok (gather: row p of the pair order is
// x[tok[p]]) or [P][K] with tok null (in place) - into ax [S][8][K/128][2][64][16] and as [S][2][K/128][64][4],
// S = P / 128 + E, live slots only.  Returns 0, 1 when the shape is not covered (nothing launched), < 0 for a
// bad call, else the HIP error.
extern "C" int mp_moe_quant_mx_tiled(const void* x, const int32_t* off, const int32_t* tok, void* ax, void* as, int T,
                                     int P, int E, int K, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (x == nullptr || off == nullptr || ax == nullptr || as == nullptr || T <= 0 || P < T) return -1;
  if (E <= 0 || E > MT_MAX_E || P > MT_MAX_PAIRS || K <= 0 || K % 128) return 1;
  const int S = P / MT_BM + E, nkb = K / 128;
  if (tok != nullptr)
    hipLaunchKernelGGL((moe_quant_mx_kernel<true>), dim3(S * nkb), dim3(512), 0, stream, off, tok, (const bf16_t*)x,
                       (uint8_t*)ax, (uint8_t*)as, T, P, E, nkb);
  else
    hipLaunchKernelGGL((moe_quant_mx_kernel<false>), dim3(S * nkb), dim3(512), 0, stream, off, tok, (const bf16_t*)x,
                       (uint8_t*)ax, (uint8_t*)as, T, P, E, nkb);
  return (int)hipGetLastError();
}

// Gate/up + SwiGLU over ax / as of the gather form (K = H): w8 [E][2F/16][H/32][64][8], wsc [E][2F], out bf16
// row-major [P][F].  The return codes of mp_moe_gate_up_w8_tiled.
extern "C" int mp_moe_gate_up_mx_tiled(const void* ax, const void* as, const void* w8, const float* wsc,
                                       const int32_t* off, void* out, int T, int P, int E, int H, int F,
                                       hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (ax == nullptr || as == nullptr || w8 == nullptr || wsc == nullptr || off == nullptr || out == nullptr || P < T ||
      (T > 0 && P % T))
    return -1;
  if (!tiled_shape_ok(T, E, P / T, H, F)) return 1;
  const int rc = launch_tiled_mx<false>(off, ax, as, w8, wsc, out, nullptr, nullptr, nullptr, nullptr, T, P, E, 2 * F,
                                        H, stream);
  return rc != 0 ? rc : (int)hipGetLastError();
}

// Down over ax / as of the in-place form of act (K = F): w8 [E][H/16][F/32][64][8], wsc [E][H], tok / wsel / idx
// / ws as mp_moe_down_w8_tiled takes them; mp_moe_combine_tiled follows.
extern "C" int mp_moe_down_mx_tiled(const void* ax, const void* as, const void* w8, const float* wsc,
                                    const int32_t* off, const int32_t* tok, const float* wsel, const int64_t* idx,
                                    float* ws, int T, int P, int E, int H, int F, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (ax == nullptr || as == nullptr || w8 == nullptr || wsc == nullptr || off == nullptr || tok == nullptr ||
      wsel == nullptr || idx == nullptr || ws == nullptr || P < T || (T > 0 && P % T))
    return -1;
  if (!tiled_shape_ok(T, E, P / T, H, F)) return 1;
  const int rc = launch_tiled_mx<true>(off, ax, as, w8, wsc, nullptr, tok, wsel, idx, ws, T, P, E, H, F, stream);
  return rc != 0 ? rc : (int)hipGetLastError();
}
