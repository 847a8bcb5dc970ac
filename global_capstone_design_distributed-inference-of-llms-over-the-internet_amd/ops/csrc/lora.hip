// Batched LoRA for ragged decode steps (mp::LoraArgs, mp_api.h): every row carries the slot of
// its adapter, read on the device, so rows of different adapters - and base-model rows, slot -1 -
// share one launch whose grid depends on the shape alone (graph-safe, no host synchronisation).
//
//   shrink: t[m][j]  = scale[s] * sum_k A[s][j][k] * x[m][k]                      (fp32, s = slots[m])
//   expand: y[m][n]  = bf16( fp32(y[m][n]) + sum_j fp32(B[s][n][j]) * t[m][j] )   (in place)
//
// Both are per-row gathers: a workgroup belongs to ONE row, reads that row's slot and only that
// slot's matrices, and returns at once for a row with slot -1 (or a slot outside [0, S)): such a
// row's x, t and y are neither read nor written.  A row's sums run in an order fixed by (K, R)
// alone, so its bits do not depend on what the other rows of the launch name.  bf16 x bf16
// products are exact in fp32; all accumulation is fp32 FMA.
#include "common.h"

namespace mp {

constexpr int LORA_SHRINK_THREADS = 256;  // 4 waves, 4 ranks each: a workgroup is (row, 16 ranks)
constexpr int LORA_EXPAND_THREADS = 256;  // one column per thread: a workgroup is (row, 256 columns)
constexpr int LORA_MAX_R = 192;
constexpr int LORA_RC = 64;               // ranks of B staged in LDS per pass
constexpr int LORA_RS = LORA_RC + 8;      // LDS row pitch in elements (144 B = 9 x 16 B)

__device__ __forceinline__ int lora_slot(const int32_t* slots, int m, int S) {
  const int s = slots[m];
  return (s >= 0 && s < S) ? s : -1;
}

// x: packed bf16 (apk_off, MT = ceil(M/16)); the 8 columns [8c, 8c + 8) of a row are one 16-B piece,
// so the padding rows of a partial tile are never touched.  A: bf16 [S][R][K] (slot stride a_stride).
__global__ __launch_bounds__(LORA_SHRINK_THREADS) void lora_shrink_kernel(
    const bf16_t* __restrict__ xp, const bf16_t* __restrict__ A, int64_t a_stride, const float* __restrict__ scale,
    const int32_t* __restrict__ slots, float* __restrict__ t, int M, int K, int R, int S) {
  const int m = blockIdx.x;
  const int s = lora_slot(slots, m, S);
  if (s < 0) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int j0 = blockIdx.y * 16 + wid * 4;  // this wave's 4 ranks
  const int MT = (M + 15) >> 4;
  const bf16_t* a0 = A + (int64_t)s * a_stride + (int64_t)j0 * K;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = lane; c < (K >> 3); c += WAVE) {
    const u16x8 xv = *reinterpret_cast<const u16x8*>(xp + apk_off(m, c << 3, MT));
    u16x8 av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) av[j] = *reinterpret_cast<const u16x8*>(a0 + (int64_t)j * K + (c << 3));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j] = fmaf(bf2f(av[j][i]), bf2f(xv[i]), acc[j]);
    }
  }
  const float sc = scale[s];
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = sc * wave_sum(acc[j]);
  if (lane == 0) *reinterpret_cast<f32x4*>(t + (int64_t)m * R + j0) = r;
}

// B: bf16 [S][N][R] (slot stride b_stride); t: fp32 [M][R]; y: bf16 rows, updated in place.
// One column per thread.  A column's R weights are contiguous, so a thread reading its own column
// straight from memory would touch 64 cache lines per wave load; instead the workgroup copies its
// 256 x rc block of B (contiguous rows) into LDS with coalesced 16-B loads, LORA_RC ranks per pass,
// and every thread then reads its column from LDS (row pitch 9 x 16 B: conflict-free b128 reads).
__global__ __launch_bounds__(LORA_EXPAND_THREADS) void lora_expand_kernel(
    const float* __restrict__ t, const bf16_t* __restrict__ B, int64_t b_stride, const int32_t* __restrict__ slots,
    bf16_t* __restrict__ y, int64_t y_stride, int N, int R, int S) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[LORA_EXPAND_THREADS * LORA_RS];
  __shared__ __attribute__((aligned(16))) float ts[LORA_MAX_R];
  const int m = blockIdx.x;
  const int s = lora_slot(slots, m, S);
  if (s < 0) return;  // uniform over the workgroup: nobody waits at the barriers below
  const int tid = threadIdx.x;
  for (int j = tid; j < R; j += LORA_EXPAND_THREADS) ts[j] = t[(int64_t)m * R + j];
  const int nb0 = blockIdx.y * LORA_EXPAND_THREADS;
  const int rows = min(LORA_EXPAND_THREADS, N - nb0);  // columns of y = rows of B in this workgroup
  const bf16_t* b0 = B + (int64_t)s * b_stride + (int64_t)nb0 * R;
  float acc = 0.f;
  for (int j0 = 0; j0 < R; j0 += LORA_RC) {
    const int rc = min(LORA_RC, R - j0), cpr = rc >> 3;  // ranks of this pass, 16-B pieces per row
    __syncthreads();  // the previous pass has been read (first pass: ts is written)
    for (int q = tid; q < rows * cpr; q += LORA_EXPAND_THREADS) {
      const int row = q / cpr, ch = q - row * cpr;
      *reinterpret_cast<u16x8*>(tile + row * LORA_RS + (ch << 3)) =
          *reinterpret_cast<const u16x8*>(b0 + (int64_t)row * R + j0 + (ch << 3));
    }
    __syncthreads();
    if (tid < rows) {
      const bf16_t* tr = tile + tid * LORA_RS;
      for (int j = 0; j < rc; j += 8) {
        const u16x8 bv = *reinterpret_cast<const u16x8*>(tr + j);
        const f32x4 t0 = *reinterpret_cast<const f32x4*>(ts + j0 + j), t1 = *reinterpret_cast<const f32x4*>(ts + j0 + j + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = fmaf(bf2f(bv[i]), t0[i], acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = fmaf(bf2f(bv[i + 4]), t1[i], acc);
      }
    }
  }
  if (tid < rows) {
    bf16_t* yp = y + (int64_t)m * y_stride + nb0 + tid;
    *yp = f2bf(bf2f(*yp) + acc);
  }
}

// 0: covered, 1: not covered, < 0: bad call (the shape half of both entry points)
static int lora_shape(const LoraArgs& a, bool shrink) {
  if (a.M < 0 || a.N < 0 || a.K < 0 || a.R < 0 || a.S < 0) return -1;
  if (a.M > 64 || a.R == 0 || a.R % 16 != 0 || a.R > LORA_MAX_R) return 1;
  if (shrink ? (a.K == 0 || a.K % 32 != 0) : (a.N == 0 || a.N % 8 != 0)) return 1;
  return 0;
}

}  // namespace mp

extern "C" int mp_lora_ok(int M, int N, int K, int R) {
  mp::LoraArgs a{};
  a.M = M, a.N = N, a.K = K, a.R = R, a.S = 1;
  return mp::lora_shape(a, true) == 0 && mp::lora_shape(a, false) == 0;
}

extern "C" int mp_lora_shrink(const mp::LoraArgs* a, hipStream_t stream) {
  using namespace mp;
  const int rc = lora_shape(*a, true);
  if (rc != 0) return rc;
  if (a->M == 0) return 0;
  if (a->x == nullptr || a->A == nullptr || a->scale == nullptr || a->slots == nullptr || a->t == nullptr || a->S < 1 ||
      a->a_stride < (int64_t)a->R * a->K)
    return -2;
  hipLaunchKernelGGL(lora_shrink_kernel, dim3(a->M, a->R / 16), dim3(LORA_SHRINK_THREADS), 0, stream,
                     (const bf16_t*)a->x, (const bf16_t*)a->A, a->a_stride, a->scale, a->slots, a->t, a->M, a->K, a->R,
                     a->S);
  return (int)hipGetLastError();
}

extern "C" int mp_lora_expand(const mp::LoraArgs* a, hipStream_t stream) {
  using namespace mp;
  const int rc = lora_shape(*a, false);
  if (rc != 0) return rc;
  if (a->M == 0) return 0;
  if (a->t == nullptr || a->B == nullptr || a->slots == nullptr || a->y == nullptr || a->S < 1 ||
      a->b_stride < (int64_t)a->N * a->R || a->y_stride < a->N || a->y_stride % 8 != 0)
    return -2;
  const int per = LORA_EXPAND_THREADS;
  hipLaunchKernelGGL(lora_expand_kernel, dim3(a->M, (a->N + per - 1) / per), dim3(LORA_EXPAND_THREADS), 0, stream,
                     a->t, (const bf16_t*)a->B, a->b_stride, a->slots, (bf16_t*)a->y, a->y_stride, a->N, a->R, a->S);
  return (int)hipGetLastError();
}
