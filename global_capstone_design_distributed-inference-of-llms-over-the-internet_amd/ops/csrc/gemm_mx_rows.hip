// W8A8-MX GEMM for steps ABOVE 64 rows (prefill, chunked prefill, mixed and verify steps) of an fp8 stage
// in MX mode: the e4m3 weights are read in place, as gemm_w8_rows.hip reads them, but the activations are
// e4m3 with one e8m0 scale per 32-element block and the product runs on gfx950's block-scaled matrix
// instruction v_mfma_scale_f32_16x16x128_f8f6f4 - no fp8 -> bf16 convert of the weight fragments and half
// the matrix passes per k of the bf16 form.  Two launches: the quantizer, then the GEMM.
//
//   ax, as = quant(x[T, K])                       mp_quant_mx_rows
//   y[T, N'] = epilogue( dequant(ax, as) . W^T )  mp_gemm_mx_rows
//   W = codes uint8 [N/16][K/32][64][8] (ops.w8_from_fp8) * ws fp32 [N]
//
// Format.  The instruction's fragment and scale map is gemm_mx.hip's (measured by lab/hip/mx_probe*): lane
// l = 16 q + r of a 128-deep k-step kb holds row r's 32 bytes, byte 8 s + j = k 128 kb + 32 s + 8 q + j (the
// W8A16 byte order the weights already have: A and B permute k identically), the hardware's 32-block b of
// row r takes its scale from lane 16 b + r and covers (s >> 1, q >> 1) = (b >> 1, b & 1).  Row-major layouts
// for any T, row tiles outermost so that a row block's k walk is one contiguous run per row tile:
//   ax uint8 [ceil(T/16)][K/128][2][64][16]  half h of lane l: its bytes 16 h .. 16 h + 15 (lane-linear KiB)
//   as uint8 [ceil(T/64)][K/128][64][4]      byte i of lane 16 b + r: block b of row r of row tile 4 g + i
// Rows >= T are zero bytes with scale 127 (= 1.0).  The block rule is gemm_mx.hip's and ops.mx_block_quant's:
// e = mx_e8m0(amax), value * 2^(127 - e) clamped to +-448, cvt_pk_fp8_f32 (round to nearest even).
//
// Quantizer.  A 256-thread workgroup takes one row tile (16 rows) and four k-steps, one k-step a wave.  Lane
// l of a wave reads 16 bytes (8 values) at chunk ch = l & 15 of row 4 p + (l >> 4), p = 0 .. 3: sixteen
// consecutive lanes read the 256 contiguous bytes of a row's k-step, so x is read once, coalesced along K.
// Chunk ch is (s, q) = (ch >> 2, ch & 3); its block's four chunks sit in lanes ch ^ 1, ch ^ 4, ch ^ 5: two
// shuffles give the block maximum.  The lane's 8 e4m3 bytes go to the wave's 2 KiB of LDS in fragment order
// and leave as two lane-linear 16-byte stores per lane; the lane of a block with (ch & 5) == 0 stores its
// scale byte.  Every byte is written once, no atomics.  Row tiles past ceil(T/16) of the last group of four
// write their scale bytes (127) only.
//
// GEMM.  Split, geometries and placement are gemm_w8_rows.hip's (gemm_rows_plan.h: w8r_plan, w8r_place,
// counting tiles only): a workgroup owns 128 rows x a group of column tiles, narrow 2 x 2 waves of 4 x 2
// tiles at 65 .. 128 rows, wide 2 x 4 waves of 4 x 4 tiles above; a group narrower than the geometry spreads
// its units over the column waves and a wave issues MFMAs for its real tiles only.
// A operand.  A k-stage is ONE 128-deep step of the row block: 8 row tiles x 2 KiB of e4m3 bytes (16
// lane-linear fragments of 1 KiB) + 2 x 256 B of scale dwords (one per group of four row tiles = per row
// wave): 16.5 KiB, double-buffered in 33 KiB of LDS, shared by the waves that differ only in columns.  It is
// staged THROUGH REGISTERS (global_load_dwordx4, ds_write_b128), as gemm_w8_rows.hip stages its bf16 rows,
// not with gemm_t2d.h's LDS-DMA ring: the stage is 2 (wide) or 4 (narrow) 16-byte loads a lane, which costs 8
// or 16 VGPRs where the bf16 form's convert-free ring has left room, and it keeps the one pipeline and the
// lgkmcnt-only barrier of the sibling kernels (the DMA ring needs vmcnt waits at the barrier, which would also
// wait for the weight loads in flight).  Row tiles past ceil(T/16) are clamped to the last real one when the
// pointers are formed (their rows are never stored); rows past T inside a tile are zero in ax: no clamp in
// the loop.  One stage per barrier is 16 (wide) or 8 (narrow) MFMAs of 8 passes a wave; a deeper stage was
// not built (K / 128 may be odd, and the narrow geometry is bound by the weight stream).
// B operand.  Per column tile and step a lane's 32 bytes are the four 8-byte fragments of k-slices 4 kb ..
// 4 kb + 3 (2 KiB contiguous a tile), loaded into a two-stage register ring with the default cache policy
// (the next row block reads them from L2) and fed to the MFMA as they are, weight scale 127.
// Compute per wave and step: MW x NW MFMAs; the A scale of row tile mt is byte mt of the lane's scale dword.
// Order per step s: issue B(s + 1); compute stage s from LDS buffer s & 1 and ring slot s & 1; write
// A(s + 1) to the other buffer; issue A(s + 2); barrier (lgkmcnt only: the loads stay in flight).
//
// Deterministic: no atomics, no k split, every wave walks K upwards.  Nothing outside ax, as, the weight, the
// scales and y[0:T, 0:N'] is touched.  Registers / LDS / scratch: profiles/mx_rows/README.md.
#include "mx_common.h"
#include "mx_rows_stage.h"

namespace mp {

__global__ __launch_bounds__(256) void quant_mx_rows_kernel(const bf16_t* __restrict__ x, int64_t xs,
                                                            uint8_t* __restrict__ ax, uint8_t* __restrict__ as,
                                                            int T, int MT, int nkb, int nkg) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 2048];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int mt = blockIdx.x / nkg, kb = (blockIdx.x - mt * nkg) * 4 + wid;
  const bool live = kb < nkb;                       // wave-uniform; no early return: the barrier below
  const int ch = lane & 15, rr = lane >> 4, s = ch >> 2, q = ch & 3;
  unsigned char* sw = smem + wid * 2048;
  u16x8 v[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int row = mt * 16 + 4 * p + rr;
    v[p] = live && row < T ? *reinterpret_cast<const u16x8*>(x + (int64_t)row * xs + 128 * kb + 8 * ch) : (u16x8)(0);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = 4 * p + rr;
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf2f(v[p][j])));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 4));
    const int e = mx_e8m0(amax);
    const float sc = mx_inv_scale(e);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(bf2f(v[p][j]) * sc, -448.f), 448.f);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    *reinterpret_cast<u32x2*>(sw + (s >> 1) * 1024 + (16 * q + r) * 16 + 8 * (s & 1)) = (u32x2){(unsigned)lo, (unsigned)hi};
    if (live && (ch & 5) == 0)
      as[(((int64_t)(mt >> 2) * nkb + kb) * 64 + 16 * (2 * (s >> 1) + (q >> 1)) + r) * 4 + (mt & 3)] = (uint8_t)e;
  }
  __syncthreads();
  if (live && mt < MT) {
    uint8_t* dst = ax + (((int64_t)mt * nkb + kb) << 11) + lane * 16;
    *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(sw + lane * 16);
    *reinterpret_cast<u32x4*>(dst + 1024) = *reinterpret_cast<const u32x4*>(sw + 1024 + lane * 16);
  }
}

// MxrGeom and the stage macros (MXR_*): mx_rows_stage.h, shared with gemm_moe_tiled_mx.hip.
// Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER).
template <int MW, int NW, int WM, int WN, int EPI>
__global__ __launch_bounds__(WM* WN * 64) void gemm_mx_rows_kernel(const uint8_t* __restrict__ ax,
                                                                   const uint8_t* __restrict__ as,
                                                                   const uint8_t* __restrict__ w8, int T, int K,
                                                                   int MB, int nbig, int NBB, int NBS,
                                                                   const float* __restrict__ wsc,
                                                                   bf16_t* __restrict__ y, int64_t ys) {
  using G = MxrGeom<MW, NW, WM, WN>;
  constexpr int BMT = G::BMT, J = G::J, SB = G::STAGE_BYTES, WAVES = G::WAVES, SOFF = G::FA * 1024;
  constexpr int STEP = EPI == 1 ? 2 : 1;
  static_assert(NW % STEP == 0, "a gate tile and its up tile belong to one wave");
  __shared__ __attribute__((aligned(16))) unsigned char smem[G::LDS_BYTES];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wid % WM, wn = wid / WM;
  const int c = lane & 15, q = lane >> 4;
  int cg, mb;
  w8r_place(MB, cg, mb);
  const int tile0 = cg < nbig ? cg * NBB : nbig * NBB + (cg - nbig) * NBS;
  const int ug = (cg < nbig ? NBB : NBS) / STEP;            // units of this column group (>= 1)
  const int u0 = wn * ug / WN, u1 = (wn + 1) * ug / WN;     // ... of this wave
  const int ntw = (u1 - u0) * STEP;                         // its column tiles: 0 .. NW (wave-uniform)
  const int tw0 = tile0 + u0 * STEP;                        // its first (u0 < ug: inside the group)
  const int nks = K >> 5, nst = K >> 7;
  const int row0 = mb * G::BM;
  const int MT = (T + 15) >> 4, MG = (T + 63) >> 6;         // row tiles of ax, groups of four of as

  // this wave's J activation fragments of a stage: f = wid + WAVES j is row tile f / 2, half f % 2; a row
  // tile past the last one repeats it (never stored).  Wave wid < WM also stages row wave wid's scale dwords
  const uint8_t* xp[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int f = wid + WAVES * j;
    xp[j] = ax + (((int64_t)min(mb * BMT + (f >> 1), MT - 1) * nst) << 11) + (f & 1) * 1024 + lane * 16;
  }
  const uint8_t* sp = as + (((int64_t)min(mb * WM + min(wid, WM - 1), MG - 1) * nst) << 8) + lane * 4;
  // its weight stream: tile t at wb + t * nks * 512; tiles past ntw repeat a real one (never used)
  const uint8_t* wb = w8 + (int64_t)tw0 * nks * 512 + lane * 8;
  int tc[NW];
  float sc[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t) {
    tc[t] = max(min(t, ntw - 1), 0);
    sc[t] = wsc[(tw0 + tc[t]) * 16 + c];
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

  // epilogue: scales in fp32, one rounding; rows past T and tiles past ntw store nothing
#pragma unroll
  for (int mt = 0; mt < MW; ++mt)
#pragma unroll
    for (int t = 0; t < NW; t += STEP) {
      if (t >= ntw) continue;
      const int col = EPI == 1 ? ((tw0 + t) >> 1) * 16 + c : (tw0 + t) * 16 + c;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = row0 + (wm * MW + mt) * 16 + q * 4 + j;
        if (row >= T) continue;
        float v = acc[mt][t][j] * sc[t];
        if constexpr (EPI == 1) v = v / (1.f + __expf(-v)) * (acc[mt][t + 1][j] * sc[t + 1]);  // fp32 SwiGLU
        y[(int64_t)row * ys + col] = f2bf(v);
      }
    }
}

template <int MW, int NW, int WM, int WN>
static void mxr_launch(const GemmArgs& a, const W8rPlan& p, hipStream_t stream) {
#define MXR_L(EPI_)                                                                                          \
  hipLaunchKernelGGL((gemm_mx_rows_kernel<MW, NW, WM, WN, EPI_>), dim3(p.NB* p.MB), dim3(WM* WN * 64), 0,    \
                     stream, (const uint8_t*)a.x, (const uint8_t*)a.as, (const uint8_t*)a.w, a.M, a.K, p.MB, \
                     p.nbig, p.NBB, p.NBS, (const float*)a.wsc, (bf16_t*)a.y, a.y_stride)
  if (a.epilogue == 1) MXR_L(1); else MXR_L(0);
#undef MXR_L
}

}  // namespace mp

// x bf16 rows [T, K] (xs elements a row, a multiple of 8) -> ax [ceil(T/16)][K/128][2][64][16] and as
// [ceil(T/64)][K/128][64][4].  Returns 0, < 0 for a bad call, else the HIP error.
extern "C" int mp_quant_mx_rows(const void* x, int64_t xs, void* ax, void* as, int T, int K, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (x == nullptr || ax == nullptr || as == nullptr || T <= 0 || K <= 0 || K % 128 || xs < K || xs % 8) return -1;
  const int MT = (T + 15) / 16, nkb = K / 128, nkg = (nkb + 3) / 4;
  const int64_t blocks = (int64_t)((T + 63) / 64) * 4 * nkg;  // whole groups of four row tiles: their scale bytes
  if (blocks >= (1ll << 31)) return -1;
  hipLaunchKernelGGL(quant_mx_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16_t*)x, xs,
                     (uint8_t*)ax, (uint8_t*)as, T, MT, nkb, nkg);
  return (int)hipGetLastError();
}

// a.x = ax, a.as = as (mp_quant_mx_rows of M = T rows), w the W8A16 codes, wsc fp32 [N], y bf16 rows [T, N']
// (y_stride elements); epilogue 0 / 1.  Returns 0, 1 when the shape is not covered (nothing launched), < 0
// for a bad call, else the HIP error.
extern "C" int mp_gemm_mx_rows(const mp::GemmArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (a == nullptr || a->x == nullptr || a->as == nullptr || a->w == nullptr || a->wsc == nullptr || a->y == nullptr)
    return -1;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->y_stride < (a->epilogue == 1 ? a->N / 2 : a->N)) return -1;
  W8rPlan p;
  if (!w8r_plan(a->M, a->N, a->K, a->epilogue, p)) return 1;
  if (p.wide) mxr_launch<4, 4, 2, 4>(*a, p, stream); else mxr_launch<4, 2, 2, 2>(*a, p, stream);
  return (int)hipGetLastError();
}

// dry dispatch
extern "C" int mp_gemm_mx_rows_ok(int T, int N, int K, int epilogue) {
  mp::W8rPlan p;
  return mp::w8r_plan(T, N, K, epilogue, p) ? 1 : 0;
}
