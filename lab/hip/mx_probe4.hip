// Fourth probe of v_mfma_scale_f32_16x16x128_f8f6f4: e4m3 A (cbsz 0) x e2m1 B (blgp 4, a 4-VGPR operand of
// 32 nibbles a lane).  One-hot operands answer: which (lane, dword, nibble) of B is which (column, k); which
// lane's scale byte applies to which 32 of them; which k each A byte meets.  k is named through the A map
// gemm_mx_rows.hip documents in hardware terms: byte i of half h of lane 16 q + r = k 64 h + 16 q + i of
// row r, block 2 h + (q >> 1) scaled from lane 16 (2 h + (q >> 1)) + r - the probe re-measures the block
// part with an fp4 B.  Every experiment is one 64-lane workgroup of ONE launch (problem p = blockIdx.x).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

struct Problem {
  unsigned char A[64][32], B[64][32];  // B: bytes 0 .. 15 are the fp4 operand, the rest stays zero
  unsigned SA[64], SB[64];
  float C[64][4];
};

__global__ void mx4_kernel(Problem* p) {
  Problem& P = p[blockIdx.x];
  const int l = threadIdx.x;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(*reinterpret_cast<const i32x8*>(P.A[l]),
                                                         *reinterpret_cast<const i32x8*>(P.B[l]), acc, 0, 4, 0,
                                                         (int)P.SA[l], 0, (int)P.SB[l]);
  *reinterpret_cast<f32x4*>(P.C[l]) = acc;
}

static std::vector<Problem> probs;
static Problem& fresh() {
  probs.emplace_back();
  Problem& P = probs.back();
  memset(&P, 0, sizeof(P));
  for (int l = 0; l < 64; ++l) P.SA[l] = P.SB[l] = 0x7f7f7f7fu;
  return P;
}
static void set_nib(Problem& P, int lane, int p, int code) { P.B[lane][p >> 1] |= code << (4 * (p & 1)); }
// C[row][col] sits in (lane 16 (row >> 2) + col, reg row & 3)
static float cval(const Problem& P, int row, int col) { return P.C[16 * (row >> 2) + col][row & 3]; }

int main() {
  // E1 (k map of B): B one-hot 1.0 (e2m1 code 2) at (lane 16 b, nibble p); A row 0 = 1.0 on the positions
  // a = 32 q + 16 h + i whose bit j is set: seven runs spell the A position the nibble meets.
  const int e1 = (int)probs.size();
  for (int b = 0; b < 4; ++b)
    for (int p = 0; p < 32; ++p)
      for (int j = 0; j < 7; ++j) {
        Problem& P = fresh();
        set_nib(P, 16 * b, p, 2);
        for (int a = 0; a < 128; ++a)
          if ((a >> j) & 1) P.A[16 * (a >> 5)][a & 31] = 0x38;
      }
  // E2 (column / row map): B one-hot at lane lb nibble 5, A all ones -> the nonzero column; A one-hot at lane
  // la byte 3, B all ones -> the nonzero row
  const int e2 = (int)probs.size();
  const int lanes[] = {0, 1, 7, 15, 16, 22, 37, 63};
  for (int lb : lanes) {
    Problem& P = fresh();
    memset(P.A, 0x38, sizeof(P.A));
    set_nib(P, lb, 5, 2);
  }
  for (int la : lanes) {
    Problem& P = fresh();
    P.A[la][3] = 0x38;
    for (int l = 0; l < 64; ++l) memset(P.B[l], 0x22, 16);
  }
  // E3 (scale_b): ones in B's lane group bd only, byte 0 of scale_b of lane group bs = 128 (x 2)
  const int e3 = (int)probs.size();
  for (int bs = 0; bs < 4; ++bs)
    for (int bd = 0; bd < 4; ++bd) {
      Problem& P = fresh();
      memset(P.A, 0x38, sizeof(P.A));
      for (int c = 0; c < 16; ++c) memset(P.B[16 * bd + c], 0x22, 16);
      for (int c = 0; c < 16; ++c) P.SB[16 * bs + c] = 0x7f7f7f80u;
    }
  // E4 (scale_a beside an fp4 B): ones in half h of A's lane group q only, scale_a of lane group g = 128
  const int e4 = (int)probs.size();
  for (int g = 0; g < 4; ++g)
    for (int q = 0; q < 4; ++q)
      for (int h = 0; h < 2; ++h) {
        Problem& P = fresh();
        for (int r = 0; r < 16; ++r) memset(P.A[16 * q + r] + 16 * h, 0x38, 16);
        for (int l = 0; l < 64; ++l) memset(P.B[l], 0x22, 16);
        for (int r = 0; r < 16; ++r) P.SA[16 * g + r] = 0x7f7f7f80u;
      }
  // E5 (e2m1 code values): the 16 codes at (lane 0, nibble 0) against A = 1.0
  const int e5 = (int)probs.size();
  for (int code = 0; code < 16; ++code) {
    Problem& P = fresh();
    memset(P.A, 0x38, sizeof(P.A));
    set_nib(P, 0, 0, code);
  }

  Problem* d = nullptr;
  const size_t bytes = probs.size() * sizeof(Problem);
  if (hipMalloc(&d, bytes) != hipSuccess || hipMemcpy(d, probs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    printf("allocation / copy failed\n");
    return 2;
  }
  mx4_kernel<<<(unsigned)probs.size(), 64>>>(d);
  const hipError_t err = hipMemcpy(probs.data(), d, bytes, hipMemcpyDeviceToHost);
  if (err != hipSuccess) {
    printf("run failed: %s\n", hipGetErrorString(err));
    return 2;
  }

  int bad = 0;
  printf("E1: B (lane group b, nibble p) -> A position (q, h, i) -> k = 64 h + 16 q + i; expected k = 32 b + p\n");
  for (int b = 0; b < 4; ++b) {
    printf("  b=%d:", b);
    for (int p = 0; p < 32; ++p) {
      int a = 0;
      for (int j = 0; j < 7; ++j) {
        const float v = cval(probs[e1 + (b * 32 + p) * 7 + j], 0, 0);
        if (v == 1.f) a |= 1 << j; else if (v != 0.f) { printf(" [odd value %g]", v); ++bad; }
      }
      const int q = a >> 5, h = (a >> 4) & 1, i = a & 15, k = 64 * h + 16 * q + i;
      printf(" %d", k);
      if (k != 32 * b + p) ++bad;
    }
    printf("\n");
  }
  printf("E2: nonzero outputs of a B one-hot (expect column lane & 15, all 16 rows) / an A one-hot (row lane & 15)\n");
  for (int n = 0; n < 16; ++n) {
    const Problem& P = probs[e2 + n];
    const int lane = lanes[n & 7];
    int cnt = 0, where = -1;
    for (int r = 0; r < 16; ++r)
      for (int c = 0; c < 16; ++c)
        if (cval(P, r, c) != 0.f) { ++cnt; where = n < 8 ? c : r; }
    printf("  %c lane %2d: %d nonzero, %s %d\n", n < 8 ? 'B' : 'A', lane, cnt, n < 8 ? "column" : "row", where);
    if (cnt != 16 || where != (lane & 15)) ++bad;
  }
  printf("E3: C[0][0] with B data in lane group bd, scale_b x2 on lane group bs (32 = unscaled, 64 = scaled)\n");
  for (int bs = 0; bs < 4; ++bs) {
    printf("  bs=%d:", bs);
    for (int bd = 0; bd < 4; ++bd) {
      const float v = cval(probs[e3 + bs * 4 + bd], 0, 0);
      printf(" bd%d=%g", bd, v);
      if (v != (bs == bd ? 64.f : 32.f)) ++bad;
    }
    printf("\n");
  }
  printf("E4: C[0][0] with A data in (group q, half h), scale_a x2 on lane group g (16 = unscaled, 32 = scaled)\n");
  for (int g = 0; g < 4; ++g) {
    printf("  g=%d:", g);
    for (int q = 0; q < 4; ++q)
      for (int h = 0; h < 2; ++h) {
        const float v = cval(probs[e4 + (g * 4 + q) * 2 + h], 0, 0);
        printf(" q%dh%d=%g", q, h, v);
        if (v != (g == 2 * h + (q >> 1) ? 32.f : 16.f)) ++bad;
      }
    printf("\n");
  }
  printf("E5: e2m1 code values:");
  const float want[16] = {0.f, .5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f, -0.f, -.5f, -1.f, -1.5f, -2.f, -3.f, -4.f, -6.f};
  for (int code = 0; code < 16; ++code) {
    const float v = cval(probs[e5 + code], 0, 0);
    printf(" %g", v);
    if (v != want[code]) ++bad;
  }
  printf("\n%s (%d deviations from the expected map)\n", bad ? "DIFFERS" : "MATCHES THE EXPECTED MAP", bad);
  (void)hipFree(d);
  return 0;
}
