// W8A16 GEMM for steps ABOVE 64 rows (prefill, chunked prefill, mixed and verify steps) of an fp8
// stage: the e4m3 weights are read IN PLACE, in the fragment order and at the 1 byte per weight the
// decode kernels stream them, instead of being rewritten as a row-major bf16 copy for the library GEMM.
//
//   y[T, N'] = epilogue( x[T, K] . W^T ),   W = codes uint8 [N/16][K/32][64][8] (ops.w8_from_fp8) * ws fp32 [N]
//
// x is row-major bf16 with a row stride (a multiple of 8 elements), T >= 65 without an upper limit.
// Epilogue 0 stores N' = N columns, epilogue 1 is SwiGLU over the 16-row gate/up interleave (tile 2u =
// gate, 2u + 1 = up, N' = N / 2).  The channel scales multiply the fp32 accumulators; one rounding to bf16.
//
// Split.  Two-dimensional, for gemm_t2d.h's reason: a workgroup that took all rows of its columns would
// make every CU take in all of x.  A workgroup owns a block of 128 rows by a group of column tiles.  When
// the number of column groups is a multiple of 8 (the rule below rounds it to one where it can), the row
// blocks of one column group sit on one XCD (w8r_place) and are dispatched together, so the group's weights
// come from HBM once and from that XCD's L2 for the other row blocks; otherwise consecutive row blocks of a
// group go round the XCDs and its weights may come from HBM up to MB times.  Weights are 1 byte and
// activations 2, so the intake per output, 2 / BN + 1 / BM bytes per k, asks for BN = 2 BM: the wide
// geometry is 128 rows x 256 columns.  (A 256-row block needs 128 accumulator registers per lane at that
// width, or is no better than 128 x 256 at half of it: not built.)
//
// Geometries (WM x WN waves, each MW x NW 16 x 16 tiles), both epilogues:
//   narrow  2 x 2 waves, 4 x 2 tiles: 128 rows x up to  64 columns, 256 threads      65 <= T <= 128
//   wide    2 x 4 waves, 4 x 4 tiles: 128 rows x up to 256 columns, 512 threads      T > 128
// RULE (w8r_plan): MB = ceil(T / 128) row blocks.  The N / 16 column tiles (SwiGLU: gate/up pairs) are cut
// into NB = min(units, max(ceil(units / capacity), #CUs / MB)) groups, as evenly as whole units allow: the
// fewest groups the geometry can hold, but enough that every CU has a workgroup where N / 16 allows it.
// NB above 8 is then rounded up to a multiple of 8 (down, if there are too few units and the capacity
// allows), for the XCD placement.  At 65 .. 128 rows the weight stream sets the time and the narrow
// geometry's 64-column capacity keeps two workgroups (64 KB of LDS each) on a CU; the wide geometry uses
// 32 KB.  A group narrower than the geometry spreads its units over the WN column waves; a wave runs
// converts and MFMAs for its real tiles only.
//
// A operand.  A k-stage is KU k-slices of the row block in A-fragment order: 4 slices (32 fragments of
// 1 KiB) in the narrow geometry, 2 (16 fragments) in the wide one, whose 4-tile waves spill with a 4-slice
// fp8 ring.  Wave w loads fragments w, w + WAVES, ... (a lane's load is the 16 bytes at row[32 ks + 8 q]:
// gemm_moe_rows.hip's access), holds them in registers for one stage and writes them lane-linear
// (ds_write_b128) into one of two LDS buffers; the waves that differ only in columns share them
// (ds_read_b128).  Lanes of rows past T read row T - 1.
// B operand.  A wave loads the 512-byte fp8 fragments of its own column tiles straight into a two-stage
// register ring with the default cache policy (the next row block reads them again), converts one with
// f8w_to_bf16 right before use and feeds it to v_mfma_f32_16x16x32_bf16 for its MW = 4 row tiles: FOUR
// MFMAs (64 issue cycles) per convert (4 cvt + 4 permutes, about 32).  The converts of one wave run under
// the MFMAs of the other wave on its SIMD: the wide geometry has two waves a SIMD, the narrow one has one
// per workgroup and a second only while two workgroups share the CU.
// Order per step s: issue B(s + 1); compute stage s from LDS buffer s & 1 and ring slot s & 1; write
// A(s + 1) to the other buffer; issue A(s + 2); barrier (lgkmcnt only: the loads stay in flight).
//
// Deterministic: no atomics, no k split, every wave walks K upwards.  Nothing outside x[0:T, 0:K], the
// weight, the scales and y[0:T, 0:N'] is touched.  Registers / LDS / scratch: profiles/w8_rows/README.md.
#include "gemm_rows_plan.h"  // W8R_LDS_BYTES, w8r_place, W8rPlan, w8r_plan: shared with gemm_w4_rows.hip

namespace mp {

template <int MW, int NW, int WM, int WN, int KU>
struct W8rGeom {
  static constexpr int WAVES = WM * WN, THREADS = WAVES * 64;
  static constexpr int BMT = WM * MW, BM = 16 * BMT;     // row tiles / rows per block
  static constexpr int NBMAX = WN * NW;                  // column tiles per block (at most)
  static constexpr int FA = BMT * KU;                    // activation fragments per stage
  static constexpr int J = FA / WAVES;                   // fragment loads per wave per stage
  static constexpr int STAGE_BYTES = FA * 1024;
  static constexpr int LDS_BYTES = 2 * STAGE_BYTES;
  static_assert(FA % WAVES == 0, "every wave loads the same number of fragments");
  static_assert(LDS_BYTES <= W8R_LDS_BYTES, "LDS budget of gemm_t2d.h");
};

// Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER).
template <int MW, int NW, int WM, int WN, int KU, int EPI>
__global__ __launch_bounds__(WM* WN * 64) void gemm_w8_rows_kernel(const bf16_t* __restrict__ x,
                                                                   const uint8_t* __restrict__ w8, int T, int K,
                                                                   int64_t xs, int MB, int nbig, int NBB, int NBS,
                                                                   const float* __restrict__ wsc,
                                                                   bf16_t* __restrict__ y, int64_t ys) {
  using G = W8rGeom<MW, NW, WM, WN, KU>;
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
  const int nks = K >> 5, nst = nks / KU;
  const int row0 = mb * G::BM;

  // this wave's J activation fragments of a stage: f = wid + WAVES j is k-slice f / BMT, row tile f % BMT
  const bf16_t* xp[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int f = wid + WAVES * j;
    const int row = min(row0 + (f % BMT) * 16 + c, T - 1);
    xp[j] = x + (int64_t)row * xs + (f / BMT) * 32 + 8 * q;
  }
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

  u16x8 stg[J];
  u32x2 rb[2][KU][NW];
#define W8R_LOAD_A(st)                                                                                   \
  {                                                                                                      \
    const int s_ = min(st, nst - 1);                                                                     \
    _Pragma("unroll") for (int j = 0; j < J; ++j) stg[j] = MP_LOAD_A_FRAG(xp[j] + (int64_t)s_ * (KU * 32)); \
  }
#define W8R_STORE_A(buf)                                                                                 \
  _Pragma("unroll") for (int j = 0; j < J; ++j) *reinterpret_cast<u16x8*>(                              \
      smem + (buf) * SB + (wid + WAVES * j) * 1024 + lane * 16) = stg[j];
#define W8R_LOAD_B(d, st)                                                                                \
  {                                                                                                      \
    const int s_ = min(st, nst - 1);                                                                     \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) _Pragma("unroll") for (int t = 0; t < NW; ++t)        \
        rb[d][u][t] = *reinterpret_cast<const u32x2*>(wb + (((int64_t)tc[t] * nks + s_ * KU + u) << 9)); \
  }
#define W8R_MMA(d)                                                                                       \
  {                                                                                                      \
    const unsigned char* sb_ = smem + (d) * SB + lane * 16;                                              \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                                     \
      u16x8 a_[MW];                                                                                      \
      _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) a_[mt] =                                         \
          *reinterpret_cast<const u16x8*>(sb_ + (u * BMT + wm * MW + mt) * 1024);                        \
      _Pragma("unroll") for (int t = 0; t < NW; ++t) {                                                   \
        if (t < ntw) {                                                                                   \
          const u16x8 b_ = f8w_to_bf16(rb[d][u][t]);                                                     \
          _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) acc[mt][t] = mfma16(a_[mt], b_, acc[mt][t]); \
        }                                                                                                \
      }                                                                                                  \
    }                                                                                                    \
  }

  W8R_LOAD_A(0)
  W8R_LOAD_B(0, 0)
  W8R_STORE_A(0)
  W8R_LOAD_A(1)
  lds_barrier();
  // at the top of step s: LDS buffer s & 1 holds stage s of A, stg stage s + 1 (in flight), ring slot
  // s & 1 stage s of B
  for (int s0 = 0; s0 < nst; s0 += 2) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int s = s0 + d;
      if (s >= nst) break;
      W8R_LOAD_B(d ^ 1, s + 1)
      W8R_MMA(d)
      W8R_STORE_A(d ^ 1)  // (at s = nst - 1 a clamped copy nobody reads: no branch around the pipeline)
      W8R_LOAD_A(s + 2)
      lds_barrier();
    }
  }
#undef W8R_MMA
#undef W8R_LOAD_B
#undef W8R_STORE_A
#undef W8R_LOAD_A

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

template <int MW, int NW, int WM, int WN, int KU>
static void w8r_launch(const GemmArgs& a, const W8rPlan& p, hipStream_t stream) {
#define W8R_L(EPI_)                                                                                            \
  hipLaunchKernelGGL((gemm_w8_rows_kernel<MW, NW, WM, WN, KU, EPI_>), dim3(p.NB* p.MB), dim3(WM* WN * 64), 0,  \
                     stream, (const bf16_t*)a.x, (const uint8_t*)a.w, a.M, a.K, a.x_stride, p.MB, p.nbig, p.NBB, \
                     p.NBS, (const float*)a.wsc, (bf16_t*)a.y, a.y_stride)
  if (a.epilogue == 1) W8R_L(1); else W8R_L(0);
#undef W8R_L
}

}  // namespace mp

// x bf16 rows [M = T, K] (x_stride elements, a multiple of 8), w the W8A16 codes, wsc fp32 [N], y bf16 rows
// [T, N'] (y_stride elements); epilogue 0 / 1.  Returns 0, 1 when the shape is not covered (nothing
// launched), < 0 for a bad call, else the HIP error.
extern "C" int mp_gemm_w8_rows(const mp::GemmArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (a == nullptr || a->x == nullptr || a->w == nullptr || a->wsc == nullptr || a->y == nullptr) return -1;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->x_stride < a->K || a->x_stride % 8 ||
      a->y_stride < (a->epilogue == 1 ? a->N / 2 : a->N))
    return -1;
  W8rPlan p;
  if (!w8r_plan(a->M, a->N, a->K, a->epilogue, p)) return 1;
  if (p.wide) w8r_launch<4, 4, 2, 4, 2>(*a, p, stream); else w8r_launch<4, 2, 2, 2, 4>(*a, p, stream);
  return (int)hipGetLastError();
}

// dry dispatch
extern "C" int mp_gemm_w8_rows_ok(int T, int N, int K, int epilogue) {
  mp::W8rPlan p;
  return mp::w8r_plan(T, N, K, epilogue, p) ? 1 : 0;
}
