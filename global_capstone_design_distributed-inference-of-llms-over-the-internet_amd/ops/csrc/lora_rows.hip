// Batched LoRA for steps ABOVE 64 rows (prompts, chunked-prefill chunks, mixed and verify steps): the
// semantics of lora.hip on row-major activations of any row count, on the matrix cores.
//
//   shrink: t[m][j] = scale[s] * sum_k A[s][j][k] * x[m][k]                      (fp32, s = slots[m])
//   expand: y[m][n] = bf16( fp32(y[m][n]) + sum_j fp32(B[s][n][j]) * t[m][j] )   (in place)
//
// x bf16 [T, K] and y bf16 [T, N] are row-major with a row stride (a multiple of 8 elements, 16-B aligned);
// A bf16 [S, R, K], B bf16 [S, N, R], scale fp32 [S], slots int32 [T] on the device, t fp32 [T, R].
// T >= 1 without an upper limit, K % 32 == 0, N % 16 == 0, R % 16 == 0, R <= 192.
//
// Unit of work: a 16-row TILE, not a host-side run of equal slots.  A workgroup reads its 16 slots (rows
// past T and slots outside [0, S) count as -1), takes the ballot of the rows that have one and walks the
// DISTINCT slots of the tile in row order (lora_next_slot): a prefill tile has one or two, a tile with none
// returns before any load.  Every slot gets a pass of its own with fresh accumulators, over that slot's
// matrices only; in a pass a lane loads the activations (x, t, y) of its own row only if the row's slot is
// the pass's - a lane of another row reads the pass's first row again, so neither a base row nor a row of
// another slot is read - and at the end only the pass's rows are stored.  An MFMA output row is a function
// of its own operand row, so a row's bits depend on (K, R), its own x / y and its own slot's matrices: not on
// its neighbours' slots, nor on what another slot's matrices hold (another pass's NaN stays in accumulators
// that pass never stores).  No atomics, no k-split across workgroups, the grid is a function of the shape:
// capture-safe, same bits every run.
//
// Operand roles.  Both kernels put the ADAPTER matrix on the MFMA's row operand and the activation on its
// column operand, i.e. they compute the transposed tile: lane (m = lane & 15, q = lane >> 4) then holds four
// consecutive ranks / columns of ITS OWN row m.  (The other assignment - lane = column, four rows per lane, as
// the GEMMs of this directory have it - takes the same 16-byte / 8-byte operand loads.)  This way
//   * "store only the pass's rows" is a per-lane predicate, the one the loads already use;
//   * shrink stores t as 16-byte pieces, and expand reads and writes y as 16-byte pieces (below) without a
//     transposition through LDS.
//
// Shrink.  One 4-wave workgroup owns a row tile and all R / 16 rank tiles (at most 12 f32x4 accumulators), so
// x is read once.  Wave w takes the 32-deep k-slices w, w + 4, ...; both operands come straight from row-major
// global memory in 16-byte loads (the row gather of gemm_w8_rows.hip, no LDS staging): lane (m, q) reads
// x[m][32 ks + 8 q ..], and A[s][16 jt + (lane & 15)][32 ks + 8 q ..] for every rank tile jt.  A register ring
// of D slices keeps the loads in flight: D = 8 at one rank tile down to 2 at five and more - at 65 rows only five
// workgroups exist, and the depth of the ring is all that hides the latency of their K / 128 dependent steps.
// v_mfma_f32_16x16x32_bf16: bf16 x bf16 products are exact in fp32.  The four waves' partial tiles meet in LDS
// and are summed in wave order, ((p0 + p1) + p2) + p3 (a wave without a slice contributes zeros), wave w
// finishing rank tiles w, w + 4, ...: times scale[s], stored as fp32.  One instantiation per rank-tile count,
// 1 .. 12.
//
// Expand.  Grid (row tile, 256-column block); wave w owns 64 columns, as two 32-column pairs of MFMA tiles.
// t is NOT rounded to bf16: v_mfma_f32_16x16x4_f32.  Per 16-rank chunk c lane (i, q) loads the 8 bytes
// B[s][n(i)][16 c + 4 q ..] of each of its four tiles and widens them, lane (m, q) loads the 16 bytes
// t[m][16 c + 4 q ..]; MFMA step i pairs rank 16 c + 4 q + i on both operands.  The two tiles h = 0, 1 of a
// pair take the B rows n(i) = pair + 8 (i >> 2) + 4 h + (i & 3), so that lane (m, q) ends up with the EIGHT
// consecutive columns pair + 8 q .. + 7 of row m: one 16-byte load of y (issued before the chunk loop),
// fp32 add, one rounding, one 16-byte store.  No LDS.
//
// Registers / LDS / scratch of every instantiation and the A/B against ops.lora_update:
// profiles/lora_rows/README.md.
#include "common.h"

namespace mp {

constexpr int LR_THREADS = 256;  // 4 waves
constexpr int LR_MAX_R = 192;
constexpr int64_t LR_MAX_STRIDE = 1 << 26;  // a tile's 16 rows of x / y / A within a 32-bit byte offset

typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((ext_vector_type(8))) __bf16 lr_bf16x8;

// v_mfma_f32_16x16x32_bf16: lane (i = lane & 15, q = lane >> 4) gives row i of ``a`` and column i of ``b`` at
// k = 8 q .. 8 q + 7, and gets c[4 q + j][i] in element j
__device__ __forceinline__ f32x4 mfma16(const u16x8& a, const u16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lr_bf16x8, a), __builtin_bit_cast(lr_bf16x8, b), c,
                                                  0, 0, 0);
}
// v_mfma_f32_16x16x4_f32: the same lanes at k = q
__device__ __forceinline__ f32x4 mfma4(float a, float b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// This lane's row of the tile (row0 + (lane & 15)) and its slot, -1 for "not this launch's business".
__device__ __forceinline__ int lora_tile_slot(const int32_t* __restrict__ slots, int64_t row, int T, int S) {
  int s = -1;
  if (row < T) {
    s = slots[row];
    if (s < 0 || s >= S) s = -1;
  }
  return s;
}

// The tile's next distinct slot: ``todo`` holds the rows (bits 0 .. 15) no pass has served.  Returns the
// slot of the first of them (``first``) and clears every row that names it.  Wave-uniform, the same in all
// four waves.
__device__ __forceinline__ int lora_next_slot(int my, unsigned& todo, int& first) {
  first = __builtin_ctz(todo);
  const int s = __builtin_amdgcn_readlane(my, first);
  todo &= ~(unsigned)__ballot(my == s);
  return s;
}

// A load is (wave-uniform base) + (this lane's 32-bit byte offset): one address register per stream.
template <typename V>
__device__ __forceinline__ V lr_load(const char* base, unsigned off) {
  return *reinterpret_cast<const V*>(base + off);
}

// Addresses first (kernarg preload, gemm_kernels.h KERNARG ORDER).
template <int RT, int D>
__global__ __launch_bounds__(LR_THREADS) void lora_shrink_rows_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ A, const int32_t* __restrict__ slots,
    const float* __restrict__ scale, float* __restrict__ t, int64_t xs, int64_t a_stride, int T, int K, int S) {
  constexpr int R = 16 * RT;
  __shared__ f32x4 part[4 * RT * 64];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int nks = K >> 5;
  const int n = w < nks ? (nks - w + 3) >> 2 : 0;  // this wave's k-slices: w, w + 4, ...
  const int64_t row0 = (int64_t)blockIdx.x * 16, row = row0 + c;
  const int my = lora_tile_slot(slots, row, T, S);
  unsigned todo = (unsigned)__ballot(my >= 0) & 0xFFFFu;
  if (todo == 0) return;
  const char* xb = reinterpret_cast<const char*>(x + row0 * xs + 32 * w);  // slice i of this wave: + 256 i bytes
  const unsigned ao = (unsigned)(c * K + 8 * q) * 2u;

  while (todo != 0) {
    int first;
    const int s = lora_next_slot(my, todo, first);
    const bool mine = my == s;
    // a lane whose row is not the pass's reads the pass's first row again (results it never stores): no
    // row of another slot, and no base row, is read
    const unsigned xo = (unsigned)((mine ? c : first) * (int)xs + 8 * q) * 2u;
    const char* ab = reinterpret_cast<const char*>(A + (int64_t)s * a_stride + 32 * w);
    f32x4 acc[RT];
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) acc[jt] = (f32x4)(0.f);
    u16x8 rx[D], ra[D][RT];
    // slice i of this wave; past the last one the last one again (a cached line, never used): no branch
    // around a load, every ring slot always holds loaded registers
#define LR_LOAD(d, i)                                                                                   \
  {                                                                                                     \
    const int64_t o_ = (int64_t)min(i, n - 1) * 256;                                                    \
    rx[d] = lr_load<u16x8>(xb + o_, xo);                                                                \
    _Pragma("unroll") for (int jt = 0; jt < RT; ++jt) ra[d][jt] =                                       \
        lr_load<u16x8>(ab + (int64_t)jt * 32 * K + o_, ao);                                             \
  }
    if (n > 0) {
#pragma unroll
      for (int d = 0; d < D; ++d) LR_LOAD(d, d)
      for (int i0 = 0; i0 < n; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          if (i0 + d >= n) break;
#pragma unroll
          for (int jt = 0; jt < RT; ++jt) acc[jt] = mfma16(ra[d][jt], rx[d], acc[jt]);
          LR_LOAD(d, i0 + d + D)
        }
      }
    }
#undef LR_LOAD
    // the four partial tiles, summed in wave order; acc[jt][j] is t[row][16 jt + 4 q + j]
#pragma unroll
    for (int jt = 0; jt < RT; ++jt)
      part[(w * RT + jt) * 64 + lane] = acc[jt];
    __syncthreads();
    const float sc = scale[s];
    for (int jt = w; jt < RT; jt += 4) {
      f32x4 v = part[jt * 64 + lane] + part[(RT + jt) * 64 + lane];
      v += part[(2 * RT + jt) * 64 + lane];
      v += part[(3 * RT + jt) * 64 + lane];
      if (mine) *reinterpret_cast<f32x4*>(t + row * R + 16 * jt + 4 * q) = v * sc;
    }
    __syncthreads();  // the next pass writes part again
  }
}

__global__ __launch_bounds__(LR_THREADS) void lora_expand_rows_kernel(
    const float* __restrict__ t, const bf16_t* __restrict__ B, const int32_t* __restrict__ slots,
    bf16_t* __restrict__ y, int64_t ys, int64_t b_stride, int T, int N, int R, int S) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int colw = blockIdx.y * 256 + 64 * w;  // this wave's 64 columns
  if (colw >= N) return;                        // (no barrier in this kernel)
  const int64_t row0 = (int64_t)blockIdx.x * 16, row = row0 + c;
  const int my = lora_tile_slot(slots, row, T, S);
  unsigned todo = (unsigned)__ballot(my >= 0) & 0xFFFFu;
  if (todo == 0) return;
  const int nch = R >> 4;
  // B row of MFMA row c in tile (pair p, half h): colw + 32 p + 8 (c >> 2) + 4 h + (c & 3); a row past N
  // (whole 16-column tiles past it) reads row N - 1 instead, into columns nobody stores
  unsigned bo[2][2];
  bool yok[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    yok[p] = colw + 32 * p + 8 * q < N;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      bo[p][h] = (unsigned)(min(32 * p + 8 * (c >> 2) + 4 * h + (c & 3), N - 1 - colw) * R + 4 * q) * 2u;
  }
  const char* tb = reinterpret_cast<const char*>(t + row0 * R);
  const char* yb = reinterpret_cast<const char*>(y + row0 * ys + colw);
  bf16_t* yp = y + row * ys + colw + 8 * q;  // this lane's 8 columns of pair p: yp + 32 p

  while (todo != 0) {
    int first;
    const int s = lora_next_slot(my, todo, first);
    const bool mine = my == s;
    const int frow = mine ? c : first;  // (as in the shrink kernel: only rows of the pass are read)
    const unsigned to = (unsigned)(frow * R + 4 * q) * 4u, yo = (unsigned)(frow * (int)ys + 8 * q) * 2u;
    const char* bb = reinterpret_cast<const char*>(B + (int64_t)s * b_stride + (int64_t)colw * R);
    u16x8 yv[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      yv[p] = (u16x8)(0);
      if (yok[p]) yv[p] = lr_load<u16x8>(yb + 64 * p, yo);
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) acc[p][0] = acc[p][1] = (f32x4)(0.f);
    for (int ch = 0; ch < nch; ++ch) {
      const f32x4 tv = lr_load<f32x4>(tb + 64 * ch, to);
      u32x2_t bv[2][2];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h) bv[p][h] = lr_load<u32x2_t>(bb + 32 * ch, bo[p][h]);
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u32x2_t b = bv[p][h];  // ranks 16 ch + 4 q + 0 .. 3, widened exactly
          acc[p][h] = mfma4(__uint_as_float(b[0] << 16), tv[0], acc[p][h]);
          acc[p][h] = mfma4(__uint_as_float(b[0] & 0xFFFF0000u), tv[1], acc[p][h]);
          acc[p][h] = mfma4(__uint_as_float(b[1] << 16), tv[2], acc[p][h]);
          acc[p][h] = mfma4(__uint_as_float(b[1] & 0xFFFF0000u), tv[3], acc[p][h]);
        }
    }
    // acc[p][h][j] is the update of y[row][colw + 32 p + 8 q + 4 h + j]: fp32 add, one rounding
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (!(mine && yok[p])) continue;
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = f2bf(bf2f(yv[p][j]) + acc[p][0][j]);
        o[j + 4] = f2bf(bf2f(yv[p][j + 4]) + acc[p][1][j]);
      }
      *reinterpret_cast<u16x8*>(yp + 32 * p) = o;
    }
  }
}

// 0: covered, 1: not covered, < 0: bad call (the shape half of both entry points)
static int lora_rows_shape(const LoraArgs& a, bool shrink) {
  if (a.M < 0 || a.N < 0 || a.K < 0 || a.R < 0 || a.S < 0) return -1;
  if (a.R == 0 || a.R % 16 != 0 || a.R > LR_MAX_R) return 1;
  if (shrink ? (a.K == 0 || a.K % 32 != 0 || a.K >= LR_MAX_STRIDE)
             : (a.N == 0 || a.N % 16 != 0 || a.N > 65535 * 256))  // (grid.y)
    return 1;
  return 0;
}

// ring depth by rank tiles: 8 slices of (1 + RT) 16-byte loads at one tile, 2 at five and more
constexpr int lr_depth(int rt) { return rt == 1 ? 8 : rt == 2 ? 4 : rt <= 4 ? 3 : 2; }

template <int RT>
static void lora_shrink_rows_launch(const LoraArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL((lora_shrink_rows_kernel<RT, lr_depth(RT)>), dim3((unsigned)(((int64_t)a.M + 15) / 16)),
                     dim3(LR_THREADS), 0, stream, (const bf16_t*)a.x, (const bf16_t*)a.A, a.slots, a.scale, a.t,
                     a.x_stride, a.a_stride, a.M, a.K, a.S);
}

}  // namespace mp

extern "C" int mp_lora_rows_ok(int T, int N, int K, int R) {
  mp::LoraArgs a{};
  a.M = T, a.N = N, a.K = K, a.R = R, a.S = 1;
  return T >= 1 && mp::lora_rows_shape(a, true) == 0 && mp::lora_rows_shape(a, false) == 0;
}

extern "C" int mp_lora_shrink_rows(const mp::LoraArgs* a, hipStream_t stream) {
  using namespace mp;
  (void)hipGetLastError();
  const int rc = lora_rows_shape(*a, true);
  if (rc != 0) return rc;
  if (a->M == 0) return 0;
  if (a->x == nullptr || a->A == nullptr || a->scale == nullptr || a->slots == nullptr || a->t == nullptr || a->S < 1 ||
      a->a_stride < (int64_t)a->R * a->K || a->x_stride < a->K || a->x_stride % 8 != 0 || a->x_stride >= LR_MAX_STRIDE)
    return -2;
  switch (a->R / 16) {
#define LR_CASE(RT_) case RT_: lora_shrink_rows_launch<RT_>(*a, stream); break;
    LR_CASE(1) LR_CASE(2) LR_CASE(3) LR_CASE(4) LR_CASE(5) LR_CASE(6)
    LR_CASE(7) LR_CASE(8) LR_CASE(9) LR_CASE(10) LR_CASE(11) LR_CASE(12)
#undef LR_CASE
  }
  return (int)hipGetLastError();
}

extern "C" int mp_lora_expand_rows(const mp::LoraArgs* a, hipStream_t stream) {
  using namespace mp;
  (void)hipGetLastError();
  const int rc = lora_rows_shape(*a, false);
  if (rc != 0) return rc;
  if (a->M == 0) return 0;
  if (a->t == nullptr || a->B == nullptr || a->slots == nullptr || a->y == nullptr || a->S < 1 ||
      a->b_stride < (int64_t)a->N * a->R || a->y_stride < a->N || a->y_stride % 8 != 0 || a->y_stride >= LR_MAX_STRIDE)
    return -2;
  const dim3 grid((unsigned)(((int64_t)a->M + 15) / 16), (a->N + 255) / 256);
  hipLaunchKernelGGL(lora_expand_rows_kernel, grid, dim3(LR_THREADS), 0, stream, a->t, (const bf16_t*)a->B, a->slots,
                     (bf16_t*)a->y, a->y_stride, a->b_stride, a->M, a->N, a->R, a->S);
  return (int)hipGetLastError();
}
