// The k-stage pipeline of the W8A8-MX GEMMs above 64 rows (gemm_mx_rows.hip: dense, gemm_moe_tiled_mx.hip: the
// experts' row-block slots): the geometry's LDS arithmetic and the four stage steps as macros over the kernels'
// locals.  gemm_mx_rows.hip's header states the formats and the order of a step.
//
// The macros read these locals of the kernel that expands them:
//   MW NW WM WAVES J SB SOFF   constants of MxrGeom
//   smem                       the G::LDS_BYTES of LDS
//   lane wid wm ntw nks nst    lane, wave, row wave, the wave's real column tiles, K / 32, K / 128
//   xp[J] sp                   the wave's activation fragment / scale dword addresses of stage 0
//   wb tc[NW]                  its weight stream (tile t at wb + t * nks * 512) and the clamped tile of slot t
//   stg[J] stgs rb[2][NW] acc[MW][NW]
#pragma once
#include "gemm_rows_plan.h"

namespace mp {

template <int MW, int NW, int WM, int WN>
struct MxrGeom {
  static constexpr int WAVES = WM * WN, THREADS = WAVES * 64;
  static constexpr int BMT = WM * MW, BM = 16 * BMT;     // row tiles / rows per block
  static constexpr int FA = 2 * BMT;                     // 1 KiB activation fragments per stage
  static constexpr int J = FA / WAVES;                   // fragment loads per wave per stage
  static constexpr int STAGE_BYTES = FA * 1024 + WM * 256;  // + one scale dword per lane and row wave
  static constexpr int LDS_BYTES = 2 * STAGE_BYTES;
  static_assert(MW == 4, "a row wave is one group of four row tiles: one scale dword per lane");
  static_assert(FA % WAVES == 0 && WM <= WAVES, "every wave loads the same number of fragments");
  static_assert(LDS_BYTES <= W8R_LDS_BYTES, "LDS budget of gemm_t2d.h");
};

}  // namespace mp

#define MXR_LOAD_A(st)                                                                                   \
  {                                                                                                      \
    const int s_ = min(st, nst - 1);                                                                     \
    _Pragma("unroll") for (int j = 0; j < J; ++j) stg[j] =                                               \
        *reinterpret_cast<const u32x4*>(xp[j] + ((int64_t)s_ << 11));                                    \
    if (wid < WM) stgs = *reinterpret_cast<const unsigned*>(sp + ((int64_t)s_ << 8));                    \
  }
#define MXR_STORE_A(buf)                                                                                 \
  {                                                                                                      \
    _Pragma("unroll") for (int j = 0; j < J; ++j) *reinterpret_cast<u32x4*>(                             \
        smem + (buf) * SB + (wid + WAVES * j) * 1024 + lane * 16) = stg[j];                              \
    if (wid < WM) *reinterpret_cast<unsigned*>(smem + (buf) * SB + SOFF + wid * 256 + lane * 4) = stgs;  \
  }
#define MXR_LOAD_B(d, st)                                                                                \
  {                                                                                                      \
    const int s_ = min(st, nst - 1);                                                                     \
    _Pragma("unroll") for (int t = 0; t < NW; ++t) {                                                     \
      const u32x2* p_ = reinterpret_cast<const u32x2*>(wb + (((int64_t)tc[t] * nks + 4 * s_) << 9));     \
      const u32x2 w0 = p_[0], w1 = p_[64], w2 = p_[128], w3 = p_[192];                                   \
      rb[d][t] = (u32x8){w0[0], w0[1], w1[0], w1[1], w2[0], w2[1], w3[0], w3[1]};                        \
    }                                                                                                    \
  }
#define MXR_MMA(d)                                                                                       \
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
        _Pragma("unroll") for (int mt = 0; mt < MW; ++mt) acc[mt][t] =                                   \
            mfma_mx(a_[mt], rb[d][t], sa_ >> (8 * mt), acc[mt][t]);                                      \
      }                                                                                                  \
    }                                                                                                    \
  }
// Prologue and loop.  At the top of step s: LDS buffer s & 1 holds stage s of A, stg stage s + 1 (in flight),
// ring slot s & 1 stage s of B.  (At s = nst - 1 the store is a clamped copy nobody reads: no branch around
// the pipeline.)
#define MXR_PIPELINE()                                                                                   \
  MXR_LOAD_A(0)                                                                                          \
  MXR_LOAD_B(0, 0)                                                                                       \
  MXR_STORE_A(0)                                                                                         \
  MXR_LOAD_A(1)                                                                                          \
  lds_barrier();                                                                                         \
  for (int s0 = 0; s0 < nst; s0 += 2) {                                                                  \
    _Pragma("unroll") for (int d = 0; d < 2; ++d) {                                                      \
      const int s = s0 + d;                                                                              \
      if (s >= nst) break;                                                                               \
      MXR_LOAD_B(d ^ 1, s + 1)                                                                           \
      MXR_MMA(d)                                                                                         \
      MXR_STORE_A(d ^ 1)                                                                                 \
      MXR_LOAD_A(s + 2)                                                                                  \
      lds_barrier();                                                                                     \
    }                                                                                                    \
  }
