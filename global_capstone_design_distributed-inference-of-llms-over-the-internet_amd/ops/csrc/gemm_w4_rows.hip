// W4A16 GEMM for steps ABOVE 64 rows (prefill, chunked prefill, mixed and verify steps) of an MXFP4
// stage: the e2m1 codes and e8m0 block scales are read IN PLACE, in the fragment order and at the 0.53 bytes
// per weight the decode kernel streams them, instead of being rewritten as a row-major bf16 copy
// (mp_dequant_w4) for the library GEMM.  The 4-bit counterpart of gemm_w8_rows.hip.
//
//   y[T, N'] = epilogue( x[T, K] . W^T ),   W = w4 uint8 [N/16][K/128][64][16], s4 uint8 [N/16][K/128][16][4]
//                                           (gemm_w4.hip's header, ops.pack_weight_w4)
//
// x is row-major bf16 with a row stride (a multiple of 8 elements), T >= 65 without an upper limit,
// N % 16 == 0 (SwiGLU: % 32), K % 128 == 0.  Epilogue 0 stores N' = N columns, epilogue 1 is SwiGLU in fp32
// over the 16-row gate/up interleave (tile 2u = gate, 2u + 1 = up, N' = N / 2).  Every dequantized value
// code x 2^(e - 127) is an exact bf16 number and the convert applies the block scale, so there is no
// accumulator scale: the fp32 accumulators go straight to the epilogue, one rounding to bf16.
//
// Split, geometries and placement are gemm_w8_rows.hip's (gemm_rows_plan.h: w8r_plan, w8r_place): a
// workgroup owns 128 rows by a group of column tiles,
//   narrow  2 x 2 waves, 4 x 2 tiles: 128 rows x up to  64 columns, 256 threads      65 <= T <= 128
//   wide    2 x 4 waves, 4 x 4 tiles: 128 rows x up to 256 columns, 512 threads      T > 128
// (4-bit bytes would ask for wider column blocks than the accumulator registers allow: the fp8 rule is
// taken as it is).
//
// Stage.  The weight layout's own unit: one 128-deep k-block = four 32-deep k-slices, nst = K / 128 stages.
// B operand.  Per column tile a stage is ONE 16-byte code load per lane (the lane's 8 weights of each of the
// four k-slices, dword u = slice u) and ONE 4-byte scale load (lanes of equal c = lane & 15 read the same
// dword, byte u = slice u), straight into a two-stage register ring of NW u32x4 + NW dwords per slot: 40
// registers in the wide geometry for four slices, where the fp8 ring needs 64 for two - so both geometries
// take the 4-slice stage.  Default cache policy (the next row block reads the weights again, unlike the
// decode kernel's non-temporal stream).  Slice u of tile t becomes a B fragment right before use,
// f4w_to_bf16(codes[u], e8m0_scale(scales, u)): four v_cvt_scalef32_pk_bf16_fp4 and no permutes, feeding
// v_mfma_f32_16x16x32_bf16 for the wave's MW = 4 row tiles - four MFMAs per convert.  Tiles past the wave's
// ntw are never converted or multiplied.
// A operand.  A stage is 8 row tiles x 4 slices = 32 fragments of 1 KiB in A-fragment order, double-buffered
// in LDS: 64 KiB per workgroup in both geometries (two workgroups inside the 160 KB budget; the wide
// geometry's 152 registers keep it to one 512-thread workgroup a CU all the same).  Wave w loads
// fragments w, w + WAVES, ... (a lane's load is the 16 bytes at row[128 s + 32 u + 8 q]: the row-gather
// access of gemm_moe_rows.hip; rows past T read row T - 1), holds them in registers for one stage and writes
// them lane-linear (ds_write_b128); the waves that differ only in columns share them (ds_read_b128).
// Order per step s (the fp8 kernel's): issue B(s + 1); compute stage s from LDS buffer s & 1 and ring slot
// s & 1; write A(s + 1) to the other buffer; issue A(s + 2); barrier (lgkmcnt only: the loads stay in
// flight).  Stages past the last are clamped to it (loaded, never used), so nst = 1 - the prologue and one
// step - and odd nst need no branch around the pipeline.
//
// Deterministic: no atomics, no k split, every wave walks K upwards.  Nothing outside x[0:T, 0:K], w4, s4
// and y[0:T, 0:N'] is touched.  Registers / LDS / scratch: profiles/w4_rows/README.md.
#include "gemm_rows_plan.h"
#include "mxfp4_cvt.h"

namespace mp {

template <int MW, int NW, int WM, int WN>
struct W4rGeom {
  static constexpr int WAVES = WM * WN, THREADS = WAVES * 64;
  static constexpr int BMT = WM * MW, BM = 16 * BMT;     // row tiles / rows per block
  static constexpr int FA = BMT * 4;                     // activation fragments per stage (4 k-slices)
  static constexpr int J = FA / WAVES;                   // fragment loads per wave per stage
  static constexpr int STAGE_BYTES = FA * 1024;
  static constexpr int LDS_BYTES = 2 * STAGE_BYTES;
  static_assert(BM == 128, "w8r_plan cuts the rows into blocks of 128");
  static_assert(FA % WAVES == 0, "every wave loads the same number of fragments");
  static_assert(2 * LDS_BYTES <= W8R_LDS_BYTES, "two workgroups inside the LDS budget of gemm_t2d.h");
};

// Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER).
template <int MW, int NW, int WM, int WN, int EPI>
__global__ __launch_bounds__(WM* WN * 64) void gemm_w4_rows_kernel(const bf16_t* __restrict__ x,
                                                                   const uint8_t* __restrict__ w4,
                                                                   const uint8_t* __restrict__ s4, int T, int K,
                                                                   int64_t xs, int MB, int nbig, int NBB, int NBS,
                                                                   bf16_t* __restrict__ y, int64_t ys) {
  using G = W4rGeom<MW, NW, WM, WN>;
  constexpr int BMT = G::BMT, J = G::J, SB = G::STAGE_BYTES, WAVES = G::WAVES;
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
  const int nst = K >> 7;                                   // stages: 128-deep k-blocks
  const int row0 = mb * G::BM;

  // this wave's J activation fragments of a stage: f = wid + WAVES j is k-slice f / BMT, row tile f % BMT
  const bf16_t* xp[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int f = wid + WAVES * j;
    const int row = min(row0 + (f % BMT) * 16 + c, T - 1);
    xp[j] = x + (int64_t)row * xs + (f / BMT) * 32 + 8 * q;
  }
  // its weight stream: k-block s of tile t is 1 KiB of codes at wb + (t nst + s) * 1024 and 64 scale bytes at
  // sb + (t nst + s) * 64; tiles past ntw repeat a real one (never used)
  const uint8_t* wb = w4 + (int64_t)tw0 * nst * 1024 + lane * 16;
  const uint8_t* sb = s4 + (int64_t)tw0 * nst * 64 + c * 4;
  int tc[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t) tc[t] = max(min(t, ntw - 1), 0);

  f32x4 acc[MW][NW];
#pragma unroll
  for (int mt = 0; mt < MW; ++mt)
#pragma unroll
    for (int t = 0; t < NW; ++t) acc[mt][t] = (f32x4)(0.f);

  u16x8 stg[J];
  u32x4 rb[2][NW];
  unsigned rs[2][NW];
#define W4R_LOAD_A(st)                                                                                \
  {                                                                                                   \
    const int s_ = min(st, nst - 1);                                                                  \
    _Pragma("unroll") for (int j = 0; j < J; ++j) stg[j] = MP_LOAD_A_FRAG(xp[j] + (int64_t)s_ * 128); \
  }
#define W4R_STORE_A(buf)                                                                              \
  _Pragma("unroll") for (int j = 0; j < J; ++j) *reinterpret_cast<u16x8*>(                           \
      smem + (buf) * SB + (wid + WAVES * j) * 1024 + lane * 16) = stg[j];
#define W4R_LOAD_B(d, st)                                                                             \
  {                                                                                                   \
    const int s_ = min(st, nst - 1);                                                                  \
    _Pragma("unroll") for (int t = 0; t < NW; ++t) {                                                  \
      const int64_t blk_ = (int64_t)tc[t] * nst + s_;                                                 \
      rb[d][t] = *reinterpret_cast<const u32x4*>(wb + (blk_ << 10));                                  \
      rs[d][t] = *reinterpret_cast<const unsigned*>(sb + (blk_ << 6));                                \
    }                                                                                                 \
  }
#define W4R_MMA(d)                                                                                       \
  {                                                                                                      \
    const unsigned char* sb_ = smem + (d) * SB + lane * 16;                                              \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                      \
      u16x8 a_[MW];                                                                                      \
      _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) a_[mt] =                                         \
          *reinterpret_cast<const u16x8*>(sb_ + (u * BMT + wm * MW + mt) * 1024);                        \
      _Pragma("unroll") for (int t = 0; t < NW; ++t) {                                                   \
        if (t < ntw) {                                                                                   \
          const u16x8 b_ = f4w_to_bf16(rb[d][t][u], e8m0_scale(rs[d][t], u));                            \
          _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) acc[mt][t] = mfma16(a_[mt], b_, acc[mt][t]); \
        }                                                                                                \
      }                                                                                                  \
    }                                                                                                    \
  }

  W4R_LOAD_A(0)
  W4R_LOAD_B(0, 0)
  W4R_STORE_A(0)
  W4R_LOAD_A(1)
  lds_barrier();
  // at the top of step s: LDS buffer s & 1 holds stage s of A, stg stage s + 1 (in flight), ring slot
  // s & 1 stage s of B
  for (int s0 = 0; s0 < nst; s0 += 2) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int s = s0 + d;
      if (s >= nst) break;
      W4R_LOAD_B(d ^ 1, s + 1)
      W4R_MMA(d)
      W4R_STORE_A(d ^ 1)  // (at s = nst - 1 a clamped copy nobody reads: no branch around the pipeline)
      W4R_LOAD_A(s + 2)
      lds_barrier();
    }
  }
#undef W4R_MMA
#undef W4R_LOAD_B
#undef W4R_STORE_A
#undef W4R_LOAD_A

  // epilogue: the accumulators as they are, one rounding; rows past T and tiles past ntw store nothing
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
        float v = acc[mt][t][j];
        if constexpr (EPI == 1) v = v / (1.f + __expf(-v)) * acc[mt][t + 1][j];  // fp32 SwiGLU
        y[(int64_t)row * ys + col] = f2bf(v);
      }
    }
}

template <int MW, int NW, int WM, int WN>
static void w4r_launch(const GemmArgs& a, const W8rPlan& p, hipStream_t stream) {
#define W4R_L(EPI_)                                                                                           \
  hipLaunchKernelGGL((gemm_w4_rows_kernel<MW, NW, WM, WN, EPI_>), dim3(p.NB* p.MB), dim3(WM* WN * 64), 0,     \
                     stream, (const bf16_t*)a.x, (const uint8_t*)a.w, (const uint8_t*)a.wsc, a.M, a.K,        \
                     a.x_stride, p.MB, p.nbig, p.NBB, p.NBS, (bf16_t*)a.y, a.y_stride)
  if (a.epilogue == 1) W4R_L(1); else W4R_L(0);
#undef W4R_L
}

}  // namespace mp

// x bf16 rows [M = T, K] (x_stride elements, a multiple of 8), w the MXFP4 codes, wsc the e8m0 block scales
// s4 (the field mp_gemm_w4 reads them from), y bf16 rows [T, N'] (y_stride elements); epilogue 0 / 1.
// Returns 0, 1 when the shape is not covered (nothing launched), < 0 for a bad call, else the HIP error.
extern "C" int mp_gemm_w4_rows(const mp::GemmArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (a == nullptr || a->x == nullptr || a->w == nullptr || a->wsc == nullptr || a->y == nullptr) return -1;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->x_stride < a->K || a->x_stride % 8 ||
      a->y_stride < (a->epilogue == 1 ? a->N / 2 : a->N))
    return -1;
  W8rPlan p;
  if (!w8r_plan(a->M, a->N, a->K, a->epilogue, p)) return 1;
  if (p.wide) w4r_launch<4, 4, 2, 4>(*a, p, stream); else w4r_launch<4, 2, 2, 2>(*a, p, stream);
  return (int)hipGetLastError();
}

// dry dispatch
extern "C" int mp_gemm_w4_rows_ok(int T, int N, int K, int epilogue) {
  mp::W8rPlan p;
  return mp::w8r_plan(T, N, K, epilogue, p) ? 1 : 0;
}
