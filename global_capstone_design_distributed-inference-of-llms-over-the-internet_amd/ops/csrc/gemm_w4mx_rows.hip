// W4A8-MX GEMM for steps ABOVE 64 rows (prefill, chunked prefill, mixed and verify steps) of an MXFP4 stage:
// the e2m1 codes and e8m0 block scales are read IN PLACE, as gemm_w4_rows.hip reads them, but they are never
// converted - gfx950's block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 takes them as its B
// operand (blgp 4) against e4m3 activations with one e8m0 scale per 32 CONTIGUOUS k (cbsz 0), and applies
// both block scales itself.  Per column tile and 128-deep step that is 4 lane swaps, 1 shift and 1 MFMA
// where the W4A16 form has 16 v_cvt_scalef32_pk_bf16_fp4 and 4 bf16 MFMAs.  Two launches: the quantizer,
// then the GEMM.
//
//   axn, asn = quant(x[T, K])                       mp_quant_mxn_rows
//   y[T, N'] = epilogue( dequant(axn, asn) . W^T )  mp_gemm_w4mx_rows
//   W = w4 uint8 [N/16][K/128][64][16], s4 uint8 [N/16][K/128][16][4]  (gemm_w4.hip's header)
//
// T >= 65 without an upper limit, N % 16 == 0 (SwiGLU: % 32), K % 128 == 0.  Epilogue 0 stores N' = N
// columns, epilogue 1 is SwiGLU in fp32 over the 16-row gate/up interleave (N' = N / 2).  No accumulator
// scale: the fp32 accumulators go straight to the epilogue, one rounding to bf16.
//
// Operand map, MEASURED by lab/hip/mx_probe4.hip (profiles/w4mx_rows/mx_probe4.txt; it is the map the MX
// specification's contiguous blocks suggest, nothing had to be adapted):
//   B (e2m1, 4 VGPRs)  lane 16 b + c holds column c's k 32 b .. 32 b + 31 of the step in ascending nibble
//                      order: k 32 b + p is nibble p & 7 of dword p >> 3, low nibble first; code values 0,
//                      .5, 1, 1.5, 2, 3, 4, 6 and their negatives (bit 3).  The lane's own scale byte (byte 0
//                      under opsel 0) covers exactly those 32.
//   A (e4m3, 8 VGPRs)  byte i of half h (VGPRs 4 h .. 4 h + 3) of lane 16 q + r is k 64 h + 16 q + i of row
//                      r; k-block bl = 2 h + (q >> 1) takes its scale from lane 16 bl + r - gemm_mx_rows.hip's
//                      map in hardware terms, unchanged beside an fp4 B.
//   C                  row 4 (l >> 4) + i, column l & 15, as every 16x16 MFMA.
//
// Activation format: blocks are the MX specification's, block b of step kb = k 128 kb + 32 b .. + 31 (the
// "natural" order; mp_quant_mx_rows' blocks follow the W8A16 byte order instead and are not contiguous in k,
// so they cannot share a step with MXFP4's blocks):
//   axn uint8 [ceil(T/16)][K/128][2][64][16]  half h, lane 16 q + r, byte i = x[16 mt + r][128 kb + 64 h + 16 q + i]
//   asn uint8 [ceil(T/64)][K/128][64][4]      byte i of lane 16 b + r: block b of row r of row tile 4 g + i
// Rows >= T are zero bytes with scale 127 (= 1.0).  The block rule is gemm_mx.hip's and ops.mx_block_quant's:
// e = mx_e8m0(amax), value * 2^(127 - e) clamped to +-448, cvt_pk_fp8_f32 (round to nearest even).
//
// Quantizer.  gemm_mx_rows.hip's split: a 256-thread workgroup takes one row tile (16 rows) and four k-steps,
// one k-step a wave; lane l reads 16 bytes (8 values) at chunk ch = l & 15 of row 4 p + (l >> 4), p = 0 .. 3,
// so sixteen consecutive lanes read the 256 contiguous bytes of a row's k-step: x is read once, coalesced
// along K.  Chunk ch is k 8 ch .. 8 ch + 7: block ch >> 2, whose four chunks sit in lanes ch ^ 1, ch ^ 2,
// ch ^ 3 - two shuffles give the block maximum - and half ch >> 3, lane group (ch >> 1) & 3, bytes 8 (ch & 1)
// .. + 7 of the fragment.  The bytes go to the wave's 2 KiB of LDS in fragment order and leave as two
// lane-linear 16-byte stores per lane; the lane with (ch & 3) == 0 stores the block's scale byte.  Every byte
// is written once, no atomics.  Row tiles past ceil(T/16) of the last group of four write their scale bytes
// (127) only.
//
// GEMM.  Split, geometries and placement are gemm_w8_rows.hip's (gemm_rows_plan.h: w8r_plan, w8r_place): a
// workgroup owns 128 rows x a group of column tiles, narrow 2 x 2 waves of 4 x 2 tiles at 65 .. 128 rows, wide
// 2 x 4 waves of 4 x 4 tiles above; a wave issues MFMAs for its real tiles only.
// A operand.  gemm_mx_rows.hip's stage: ONE 128-deep step of the row block = 8 row tiles x 2 KiB of e4m3
// bytes + 2 x 256 B of scale dwords (one per lane and row wave), 16.5 KiB, double-buffered in 33 KiB of LDS,
// staged through registers (global_load_dwordx4, ds_write_b128) behind an lgkmcnt-only barrier.  Row tiles
// past ceil(T/16) are clamped to the last real one (their rows are never stored).
// B operand.  A lane's 16-byte load is the weight layout's own unit: lane 16 q + c, dword s = the 8 codes of
// k 32 s + 8 q .. + 7 of column c; its 4-byte scale load is column c's four block bytes.  The raw loads sit in
// a two-stage register ring of NW x (4 + 1) dwords a slot (40 registers in the wide geometry; the fp8 ring
// needs 64).  The instruction wants lane group b to hold block b: a 4 x 4 dword transpose across the four
// 16-lane rows, done in registers right before the MFMA - v_permlane16_swap on the dword pairs (0, 1) and
// (2, 3) (odd rows of the first <-> even rows of the second), then v_permlane32_swap on (0, 2) and (1, 3)
// (upper half of the first <-> lower half of the second).  After it lane 16 s + c holds dword q = k 32 s +
// 8 q .. + 7: block s in ascending nibble order, and its scale is byte lane >> 4 of the scale dword (one
// shift; the instruction reads byte 0).
// Order per step s (the sibling kernels'): issue B(s + 1); compute stage s from LDS buffer s & 1 and ring
// slot s & 1; write A(s + 1) to the other buffer; issue A(s + 2); barrier.  Stages past the last are clamped
// to it (loaded, never used): nst = 1 and odd nst need no branch around the pipeline.
//
// Deterministic: no atomics, no k split, every wave walks K upwards.  Nothing outside axn, asn, w4, s4 and
// y[0:T, 0:N'] is touched.  Registers / LDS / scratch: profiles/w4mx_rows/README.md.
#include "gemm_rows_plan.h"
#include "mx_common.h"

namespace mp {

__global__ __launch_bounds__(256) void quant_mxn_rows_kernel(const bf16_t* __restrict__ x, int64_t xs,
                                                             uint8_t* __restrict__ ax, uint8_t* __restrict__ as,
                                                             int T, int MT, int nkb, int nkg) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 2048];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int mt = blockIdx.x / nkg, kb = (blockIdx.x - mt * nkg) * 4 + wid;
  const bool live = kb < nkb;                       // wave-uniform; no early return: the barrier below
  const int ch = lane & 15, rr = lane >> 4, h = ch >> 3, q = (ch >> 1) & 3, b = ch >> 2;
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
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const int e = mx_e8m0(amax);
    const float sc = mx_inv_scale(e);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(bf2f(v[p][j]) * sc, -448.f), 448.f);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    *reinterpret_cast<u32x2*>(sw + h * 1024 + (16 * q + r) * 16 + 8 * (ch & 1)) = (u32x2){(unsigned)lo, (unsigned)hi};
    if (live && (ch & 3) == 0)
      as[(((int64_t)(mt >> 2) * nkb + kb) * 64 + 16 * b + r) * 4 + (mt & 3)] = (uint8_t)e;
  }
  __syncthreads();
  if (live && mt < MT) {
    uint8_t* dst = ax + (((int64_t)mt * nkb + kb) << 11) + lane * 16;
    *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(sw + lane * 16);
    *reinterpret_cast<u32x4*>(dst + 1024) = *reinterpret_cast<const u32x4*>(sw + 1024 + lane * 16);
  }
}

// The 4 x 4 dword transpose across the four 16-lane rows (header, B operand): lane 16 q + c, dword s  ->
// lane 16 s + c, dword q.
__device__ __forceinline__ u32x4 w4mx_block_transpose(const u32x4& w) {
  const auto p01 = __builtin_amdgcn_permlane16_swap(w[0], w[1], false, false);
  const auto p23 = __builtin_amdgcn_permlane16_swap(w[2], w[3], false, false);
  const auto p02 = __builtin_amdgcn_permlane32_swap(p01[0], p23[0], false, false);
  const auto p13 = __builtin_amdgcn_permlane32_swap(p01[1], p23[1], false, false);
  return (u32x4){p02[0], p13[0], p02[1], p13[1]};
}

// e4m3 A (8 VGPRs) x e2m1 B (4 VGPRs), both block scales from byte 0 of sa / sb
__device__ __forceinline__ f32x4 mfma_mx4(const u32x8& a, const u32x4& b, unsigned sa, unsigned sb, f32x4 c) {
  const i32x8_t b8 = {(int)b[0], (int)b[1], (int)b[2], (int)b[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(__builtin_bit_cast(i32x8_t, a), b8, c, 0, 4, 0, (int)sa, 0,
                                                          (int)sb);
}

template <int MW, int NW, int WM, int WN>
struct W4mxGeom {
  static constexpr int WAVES = WM * WN, THREADS = WAVES * 64;
  static constexpr int BMT = WM * MW, BM = 16 * BMT;     // row tiles / rows per block
  static constexpr int FA = 2 * BMT;                     // 1 KiB activation fragments per stage
  static constexpr int J = FA / WAVES;                   // fragment loads per wave per stage
  static constexpr int STAGE_BYTES = FA * 1024 + WM * 256;  // + one scale dword per lane and row wave
  static constexpr int LDS_BYTES = 2 * STAGE_BYTES;
  static_assert(BM == 128, "w8r_plan cuts the rows into blocks of 128");
  static_assert(MW == 4, "a row wave is one group of four row tiles: one scale dword per lane");
  static_assert(FA % WAVES == 0 && WM <= WAVES, "every wave loads the same number of fragments");
  static_assert(LDS_BYTES <= W8R_LDS_BYTES, "LDS budget of gemm_t2d.h");
};

// Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER).
template <int MW, int NW, int WM, int WN, int EPI>
__global__ __launch_bounds__(WM* WN * 64) void gemm_w4mx_rows_kernel(const uint8_t* __restrict__ ax,
                                                                     const uint8_t* __restrict__ as,
                                                                     const uint8_t* __restrict__ w4,
                                                                     const uint8_t* __restrict__ s4, int T, int K,
                                                                     int MB, int nbig, int NBB, int NBS,
                                                                     bf16_t* __restrict__ y, int64_t ys) {
  using G = W4mxGeom<MW, NW, WM, WN>;
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
  const int nst = K >> 7;                                   // stages: 128-deep k-blocks
  const int row0 = mb * G::BM;
  const int MT = (T + 15) >> 4, MG = (T + 63) >> 6;         // row tiles of axn, groups of four of asn

  // this wave's J activation fragments of a stage: f = wid + WAVES j is row tile f / 2, half f % 2; a row
  // tile past the last one repeats it (never stored).  Wave wid < WM also stages row wave wid's scale dwords
  const uint8_t* xp[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int f = wid + WAVES * j;
    xp[j] = ax + (((int64_t)min(mb * BMT + (f >> 1), MT - 1) * nst) << 11) + (f & 1) * 1024 + lane * 16;
  }
  const uint8_t* sp = as + (((int64_t)min(mb * WM + min(wid, WM - 1), MG - 1) * nst) << 8) + lane * 4;
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

  u32x4 stg[J];
  unsigned stgs = 0;
  u32x4 rb[2][NW];
  unsigned rs[2][NW];
#define W4X_LOAD_A(st)                                                                                   \
  {                                                                                                      \
    const int s_ = min(st, nst - 1);                                                                     \
    _Pragma("unroll") for (int j = 0; j < J; ++j) stg[j] =                                               \
        *reinterpret_cast<const u32x4*>(xp[j] + ((int64_t)s_ << 11));                                    \
    if (wid < WM) stgs = *reinterpret_cast<const unsigned*>(sp + ((int64_t)s_ << 8));                    \
  }
#define W4X_STORE_A(buf)                                                                                 \
  {                                                                                                      \
    _Pragma("unroll") for (int j = 0; j < J; ++j) *reinterpret_cast<u32x4*>(                             \
        smem + (buf) * SB + (wid + WAVES * j) * 1024 + lane * 16) = stg[j];                              \
    if (wid < WM) *reinterpret_cast<unsigned*>(smem + (buf) * SB + SOFF + wid * 256 + lane * 4) = stgs;  \
  }
#define W4X_LOAD_B(d, st)                                                                                \
  {                                                                                                      \
    const int s_ = min(st, nst - 1);                                                                     \
    _Pragma("unroll") for (int t = 0; t < NW; ++t) {                                                     \
      const int64_t blk_ = (int64_t)tc[t] * nst + s_;                                                    \
      rb[d][t] = *reinterpret_cast<const u32x4*>(wb + (blk_ << 10));                                     \
      rs[d][t] = *reinterpret_cast<const unsigned*>(sb + (blk_ << 6));                                   \
    }                                                                                                    \
  }
#define W4X_MMA(d)                                                                                       \
  {                                                                                                      \
    const unsigned char* sb_ = smem + (d) * SB;                                                          \
    const unsigned sa_ = *reinterpret_cast<const unsigned*>(sb_ + SOFF + wm * 256 + lane * 4);           \
    u32x8 a_[MW];                                                                                        \
    _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) {                                                  \
      const unsigned char* f_ = sb_ + (wm * MW + mt) * 2048 + lane * 16;                                 \
      const u32x4 a0 = *reinterpret_cast<const u32x4*>(f_), a1 = *reinterpret_cast<const u32x4*>(f_ + 1024); \
      a_[mt] = (u32x8){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};                          \
    }                                                                                                    \
    _Pragma("unroll") for (int t = 0; t < NW; ++t) {                                                     \
      if (t < ntw) {                                                                                     \
        const u32x4 b_ = w4mx_block_transpose(rb[d][t]);                                                 \
        const unsigned sb4_ = rs[d][t] >> (8 * q);                                                       \
        _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) acc[mt][t] =                                   \
            mfma_mx4(a_[mt], b_, sa_ >> (8 * mt), sb4_, acc[mt][t]);                                     \
      }                                                                                                  \
    }                                                                                                    \
  }

  W4X_LOAD_A(0)
  W4X_LOAD_B(0, 0)
  W4X_STORE_A(0)
  W4X_LOAD_A(1)
  lds_barrier();
  // at the top of step s: LDS buffer s & 1 holds stage s of A, stg stage s + 1 (in flight), ring slot
  // s & 1 stage s of B (raw: transposed on use)
  for (int s0 = 0; s0 < nst; s0 += 2) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int s = s0 + d;
      if (s >= nst) break;
      W4X_LOAD_B(d ^ 1, s + 1)
      W4X_MMA(d)
      W4X_STORE_A(d ^ 1)  // (at s = nst - 1 a clamped copy nobody reads: no branch around the pipeline)
      W4X_LOAD_A(s + 2)
      lds_barrier();
    }
  }
#undef W4X_MMA
#undef W4X_LOAD_B
#undef W4X_STORE_A
#undef W4X_LOAD_A

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
static void w4x_launch(const GemmArgs& a, const W8rPlan& p, hipStream_t stream) {
#define W4X_L(EPI_)                                                                                           \
  hipLaunchKernelGGL((gemm_w4mx_rows_kernel<MW, NW, WM, WN, EPI_>), dim3(p.NB* p.MB), dim3(WM* WN * 64), 0,   \
                     stream, /* ax */ (const uint8_t*)a.x, /* as */ (const uint8_t*)a.as,                     \
                     /* w4 */ (const uint8_t*)a.w, /* s4 */ (const uint8_t*)a.wsc, /* T */ a.M, /* K */ a.K,  \
                     /* MB */ p.MB, /* nbig */ p.nbig, /* NBB */ p.NBB, /* NBS */ p.NBS, /* y */ (bf16_t*)a.y, \
                     /* ys */ a.y_stride)
  if (a.epilogue == 1) W4X_L(1); else W4X_L(0);
#undef W4X_L
}

}  // namespace mp

// x bf16 rows [T, K] (xs elements a row, a multiple of 8) -> axn [ceil(T/16)][K/128][2][64][16] and asn
// [ceil(T/64)][K/128][64][4] on natural 32-blocks.  Returns 0, < 0 for a bad call, else the HIP error.
extern "C" int mp_quant_mxn_rows(const void* x, int64_t xs, void* ax, void* as, int T, int K, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (x == nullptr || ax == nullptr || as == nullptr || T <= 0 || K <= 0 || K % 128 || xs < K || xs % 8) return -1;
  const int MT = (T + 15) / 16, nkb = K / 128, nkg = (nkb + 3) / 4;
  const int64_t blocks = (int64_t)((T + 63) / 64) * 4 * nkg;  // whole groups of four row tiles: their scale bytes
  if (blocks >= (1ll << 31)) return -1;
  hipLaunchKernelGGL(quant_mxn_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16_t*)x, xs,
                     (uint8_t*)ax, (uint8_t*)as, T, MT, nkb, nkg);
  return (int)hipGetLastError();
}

// a.x = axn, a.as = asn (mp_quant_mxn_rows of M = T rows), w the MXFP4 codes, wsc the e8m0 block scales s4 (the
// field mp_gemm_w4 reads them from), y bf16 rows [T, N'] (y_stride elements); epilogue 0 / 1.  Returns 0, 1
// when the shape is not covered (nothing launched), < 0 for a bad call, else the HIP error.
extern "C" int mp_gemm_w4mx_rows(const mp::GemmArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  using namespace mp;
  if (a == nullptr || a->x == nullptr || a->as == nullptr || a->w == nullptr || a->wsc == nullptr || a->y == nullptr)
    return -1;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->y_stride < (a->epilogue == 1 ? a->N / 2 : a->N)) return -1;
  W8rPlan p;
  if (!w8r_plan(a->M, a->N, a->K, a->epilogue, p)) return 1;
  if (p.wide) w4x_launch<4, 4, 2, 4>(*a, p, stream); else w4x_launch<4, 2, 2, 2>(*a, p, stream);
  return (int)hipGetLastError();
}

// dry dispatch
extern "C" int mp_gemm_w4mx_rows_ok(int T, int N, int K, int epilogue) {
  mp::W8rPlan p;
  return mp::w8r_plan(T, N, K, epilogue, p) ? 1 : 0;
}
