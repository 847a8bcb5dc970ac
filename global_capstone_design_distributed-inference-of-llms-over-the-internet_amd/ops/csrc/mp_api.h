// The seam between the host bindings (bindings.cpp, compiled as plain C++) and the kernel files:
// the argument structs both sides read and one prototype per extern "C" entry point.  Every .hip
// file that defines an entry point includes this header, so a definition that disagrees with its
// prototype does not compile.  No device code here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace mp {

// The qkv projection left as split-K partial slabs (decode GEMM flag GEMM_PARTIALS, mp_gemm_rwk_split):
// part[s][row][col] fp32, s < S, plus the fused-norm row statistics (gemm_kernels.h EpiArgs::ss_in:
// QP_SS_NSH shards of QP_SS_ROWS rows, fixed-point sums of squares).  The decode attention kernels
// read q / k / v through qkv_part_load8 (common.h), which is the split-K reduce launch's epilogue 0
// inlined: the S slabs summed in split order from zero, times rsqrt(ss / K + eps), rounded to bf16 -
// the same bits the reduce launch would have stored, without its launch.
struct QkvPart {
  const float* part;               // nullptr: read the bf16 qkv rows instead
  int S;                           // split count
  int64_t slab;                    // elements per slab (M x ldn)
  int ldn;                         // row pitch (the qkv width)
  const unsigned long long* ss;    // row statistics, or nullptr (no row scale)
  float inv_k, eps;
};

// What every attention launcher takes (mp_paged_attention, mp_attention_mfma, mp_attention_fa).
struct AttnArgs {
  const void* q;                   // bf16 query rows [T, >= nh * D] (fused RoPE: the unrotated qkv rows)
  int64_t q_stride;
  void* kc;                        // cache pages [pages, nkv, page_size, D]: bf16, or e4m3 codes with
  void* vc;                        //   ks / vs (kv_f8.h); written only at slots[t] by the fused RoPE forms
  void* ks;                        // fp8 cache: e8m0 row scales [pages, nkv, page_size]; nullptr on a bf16 cache
  void* vs;
  const int32_t* bt;               // block tables [sequences, bt_stride]
  int bt_stride;
  const int32_t* q_seq;            // [T] block-table row of each query
  const int32_t* q_ctx;            // [T] context length of each query (0: padding row, output 0)
  void* out;                       // bf16 [T, nh * D], or packed (packed_mt = ceil(T / 16) > 0)
  float* workspace;                // split-K partials when NP > 1: [T, nh, NP, D] outputs, then (max, sum) pairs
  int T, nh, nkv, D, page_size;
  int PS, NP;                      // context tokens per part, parts
  float scale;
  int packed_mt;
  const int64_t* rope_pos;         // fused RoPE + KV write (decode), all nullptr otherwise: [T] positions,
  const float* cos_t;              //   fp32 tables [max_pos, D / 2],
  const float* sin_t;
  const int64_t* slots;            //   [T] cache slot of the new token (< 0: nothing written)
  QkvPart qp;                      // qp.part == nullptr: absent
  int window;                      // sliding window W: a query of context ctx sees cache positions
                                   //   [max(0, ctx - W), ctx); 0: no window (decode kernels, mp_attention_fa's windowed form)
};

// log2 of the page size, or -1 when it is no power of two
inline int attn_page_log2(const AttnArgs& a) {
  int s = 0;
  while ((1 << s) < a.page_size) ++s;
  return (1 << s) == a.page_size ? s : -1;
}

// the (max, sum) half of the split-K workspace; the partial outputs start at a.workspace
inline float* attn_ws_ml(const AttnArgs& a) { return a.workspace + (int64_t)a.T * a.nh * a.NP * a.D; }

// first cache position a query of context ctx sees under the window W (W <= 0: none)
inline
#if defined(__HIPCC__)
    __host__ __device__
#endif
    int
    attn_window_lo(int ctx, int W) {
  return W > 0 && ctx > W ? ctx - W : 0;
}

// the softmax scale in the exp2 domain
inline float attn_scale_log2(const AttnArgs& a) { return a.scale * 1.4426950408889634f; }

struct EpiArgs;  // gemm_kernels.h

// Decode GEMM flag word (GemmArgs::flags); every entry point reads the bits its forms have and
// ignores the rest.  The values are part of the op interface: ops/__init__.py and the tests pass
// them as integers.
constexpr int GEMM_SHARED_A_CFG_SHIFT = 5, GEMM_T2D_SPLIT_SHIFT = 16;
enum GemmFlags : int {
  GEMM_A_PACKED = 1 << 0,    // x is packed (Ap[K/32][ceil(M/16)][64][8])
  GEMM_OUT_PACKED = 1 << 1,  // SwiGLU output packed
  GEMM_STREAM_K = 1 << 2,    // stream-K kernel (needs ws, zero-initialised, used by one stream at a time)
  GEMM_ONE_GROUP = 1 << 3,   // force the one-group-per-workgroup kernel
  GEMM_SHARED_A = 1 << 4,    // shared-A (LDS-staged activation) kernel when the shape allows it
  GEMM_SHARED_A_CFG = 3 << GEMM_SHARED_A_CFG_SHIFT,  // its (NT, CH): 0 = (2, 2), 1 = (2, 4), 2 = (1, 4), 3 = (4, 2)
  GEMM_RING = 1 << 7,            // balanced ring kernel
  GEMM_SPLITK = 1 << 8,          // split-K ring kernel + reduce launch (epilogue 0 / 2 / 3, needs ws)
  GEMM_SPLITK_INLINE = 1 << 9,   // with GEMM_SPLITK: in-launch combine by the last arriver, no reduce launch
  GEMM_ROT_K = 1 << 10,          // rotated k walk per workgroup (EpiArgs::rot)
  GEMM_ROW_SPLIT = 1 << 12,      // row-split ring (epilogue 0 / 2 / 3, even row tiles)
  GEMM_ROW_SPLIT_DEFAULT_CACHE = 1 << 13,  // with GEMM_ROW_SPLIT: weights loaded with the default cache policy
  GEMM_PARTIALS = 1 << 14,       // with GEMM_SPLITK: fp32 partial slabs only, no reduce launch (QkvPart)
  GEMM_T2D = 1 << 15,            // two-dimensionally tiled form, 65..256 rows (gemm_t2d.h)
  GEMM_T2D_SPLIT = 3 << GEMM_T2D_SPLIT_SHIFT,  // its forced k split (lab); 0: picked per shape
  GEMM_T2D_DMA = 1 << 18,        // its LDS-DMA ring
};
inline int gemm_shared_a_cfg(int flags) { return (flags & GEMM_SHARED_A_CFG) >> GEMM_SHARED_A_CFG_SHIFT; }
inline int gemm_t2d_split(int flags) { return (flags & GEMM_T2D_SPLIT) >> GEMM_T2D_SPLIT_SHIFT; }

// What every decode GEMM launcher takes (mp_gemm_bf16 and _wide, mp_gemm_w8, mp_gemm_w4, mp_gemm_mx).
struct GemmArgs {
  const void* x;                   // activation: bf16 rows, or packed (GEMM_A_PACKED; w8 / w4: always);
  int64_t x_stride;                //   mx: the e4m3 bytes of mp_quant_mx.  x_stride: row-major x only (bf16)
  const void* w;                   // packed weight: bf16 (bf16), e4m3 bytes (w8, mx), MXFP4 codes (w4)
  const void* wsc;                 // w8 / mx: fp32 column scales [N]; w4: the e8m0 block scales s4; bf16: nullptr
  const void* as;                  // mx: the e8m0 activation block scales of mp_quant_mx; else nullptr
  void* y;                         // bf16 output rows, or packed (GEMM_OUT_PACKED); nullptr with GEMM_PARTIALS
  int64_t y_stride;
  const void* res;                 // epilogue 2 / 3: residual rows [M, N] (all)
  int64_t res_stride;
  int M, N, K;
  int epilogue;                    // 0 store, 1 SwiGLU, 2 residual add, 3 residual-stream producer
  int flags;                       // GemmFlags
  void* ws;                        // workspace of mp_gemm_workspace_bytes() (bf16, w8; mx: required), or nullptr
  const int* gate;                 // bf16: MoE expert gate, one device int32 (0: GEMM skipped), or nullptr
  void* ap;                        // epilogue 3: packed copy of the output rows (all; EpiArgs, gemm_kernels.h)
  void* ss_out;                    // epilogue 3: row sums of squares are added into it, or nullptr (all)
  void* ss_zero;                   // the other statistics buffer, cleared by the launch, or nullptr (all)
  const void* ss_in;               // epilogue 0 / 1: scale row r by rsqrt(ss_in[r] * inv_k + eps), or nullptr (all)
  float inv_k, eps;
};

// the shape-only arguments of a dry run: every pointer null
inline GemmArgs gemm_shape_args(int M, int N, int K, int epilogue, int flags) {
  GemmArgs a{};
  a.M = M, a.N = N, a.K = K, a.epilogue = epilogue, a.flags = flags;
  return a;
}

// What both batched-LoRA launchers take (lora.hip).  Row m belongs to adapter slot slots[m] in
// [-1, S); a row with slot -1 is a base-model row: nothing of it is read or written.
struct LoraArgs {
  const void* x;                   // shrink: packed bf16 activation (apk_off, common.h), M rows of K
  const void* A;                   // shrink: bf16 [S, R, K], slot s at A + s * a_stride elements
  int64_t a_stride;
  const void* B;                   // expand: bf16 [S, N, R], slot s at B + s * b_stride elements
  int64_t b_stride;
  const float* scale;              // shrink: fp32 [S], lora_alpha / r (or / sqrt(r)) of each slot
  const int32_t* slots;            // int32 [M]
  float* t;                        // fp32 [M, R]: shrink writes scale * (A x), expand reads it
  void* y;                         // expand: bf16 rows [M, N], updated in place
  int64_t y_stride;
  int M, N, K, R, S;               // shrink ignores N, expand ignores K
};

}  // namespace mp

extern "C" {
// norm.hip
int mp_rmsnorm(const void* x, int64_t x_stride, void* res, int64_t res_stride, const void* w, void* y,
               int64_t y_stride, const int32_t* rows, int nrows, int H, float eps, int mode, int packed_mt,
               void* ss_out, void* a8, float* a8_scale, const int64_t* gather, int64_t gather_n,
               hipStream_t stream);
// rope_kv.hip
int mp_rope_kv_write(void* qkv, int64_t qkv_stride, const int64_t* pos, const float* cos_t, const float* sin_t,
                     void* kc, void* vc, const int64_t* slots, int T, int nh, int nkv, int D, int page_size,
                     hipStream_t stream);
int mp_rope_kv_write_f8(void* qkv, int64_t qkv_stride, const int64_t* pos, const float* cos_t, const float* sin_t,
                        void* kc, void* vc, void* ks, void* vs, const int64_t* slots, int T, int nh, int nkv, int D,
                        int page_size, hipStream_t stream);
int mp_kv_write(const void* k, int64_t k_stride, const void* v, int64_t v_stride, void* kc, void* vc,
                const int64_t* slots, int T, int nkv, int D, int page_size, hipStream_t stream);
// attention.hip (a.ks != nullptr: the fp8 cache form), attention_mfma.hip, attention_fa.hip
int mp_paged_attention(const mp::AttnArgs* a, int* counters, int n_counters, hipStream_t stream);
int mp_attention_mfma(const mp::AttnArgs* a, const int32_t* qb_tok0, const int32_t* qb_ntok, int NB,
                      const int32_t* sb_first, const int32_t* sb_n, int NSB, void* mx_ax, void* mx_as,
                      hipStream_t stream);
int mp_attention_fa(const mp::AttnArgs* a, const int32_t* fb_tok0, const int32_t* fb_ntok, int NBF, int nw, int pair,
                    int windowed, hipStream_t stream);  // windowed: the sliding-window form, a->window > 0 (else 0)
// elementwise.hip
int mp_embedding(const int64_t* ids, const void* table, void* out, int T, int H, int64_t vocab, hipStream_t stream);
int mp_swiglu(const void* gu, void* out, int64_t T, int F, hipStream_t stream);
int mp_add(const void* a, const void* b, void* y, int64_t n, hipStream_t stream);
int mp_argmax(const void* logits, int64_t stride, int R, int V, int64_t* out, hipStream_t stream);
// sampling.hip
int mp_sample(const void* logits, int64_t stride, int R, int V, const float* temps, const float* top_ps,
              const int32_t* top_ks, const float* rep_pens, int32_t* recent, int recent_stride, int32_t* recent_len,
              const int64_t* seeds, float* ws, int64_t* out, int update, hipStream_t stream);
// Speculative verify: sample the R rows of S sessions (session s: rows row_start[s] .. row_start[s + 1] - 1,
// each against the history its accepted drafts would leave), keep every session's leading draws that
// equal their draft plus one more, -1 after; count[s] kept ids.  ws holds mp_sample_verify_ws_words words.
int64_t mp_sample_verify_ws_words(int R, int V, int cap);
int mp_sample_verify(const void* logits, int64_t stride, int R, int S, int V, const int32_t* row_start,
                     const int32_t* draft, const float* temps, const float* top_ps, const int32_t* top_ks,
                     const float* rep_pens, int32_t* recent, int cap, int32_t* recent_len, const int64_t* seeds,
                     float* ws, int64_t* tokens, int32_t* count, int update, int all_greedy, hipStream_t stream);
// gemm.hip, gemm_wide.hip.  The GEMM entry points return 0, 1 when no form covers the shape (nothing
// launched), < 0 for a bad call, else the HIP error.
int mp_gemm_ss_elems();
int64_t mp_gemm_slab_offset();
int64_t mp_gemm_slab_bytes();
int mp_gemm_rwk_split(int M, int N, int K, int f8);
int64_t mp_gemm_workspace_bytes();
int mp_gemm_bf16(const mp::GemmArgs* a, hipStream_t stream);
int mp_pack_act(const void* x, int64_t xs, void* ap, int M, int K, hipStream_t stream);
int mp_pack_weight(const void* w, void* wp, int N, int K, hipStream_t stream);
int mp_gemm_bf16_wide(const mp::GemmArgs* a, const mp::EpiArgs& ep, hipStream_t stream);
int mp_gemm_t2d_ok(int M, int N, int K, int epilogue, int out_packed, int with_ws);
int mp_gemm_rw_ok(int M, int N, int K, int epilogue, int out_packed);
// gemm_w8.hip, gemm_w4.hip, gemm_mx.hip
int mp_gemm_w8(const mp::GemmArgs* a, hipStream_t stream);
int mp_gemm_w4(const mp::GemmArgs* a, hipStream_t stream);
int mp_gemm_w4_ok(int M, int N, int K, int epilogue);
int mp_dequant_w4(const void* w4, const void* s4, void* w, int N, int K, hipStream_t stream);
int mp_quant_mx(const void* ap, void* ax, void* as, int M, int K, hipStream_t stream);
int mp_gemm_mx(const mp::GemmArgs* a, hipStream_t stream);
// gemm_moe.hip: the grouped W8A16 GEMMs of a sparse-MoE MLP (all experts of a layer in two launches)
int mp_moe_gate_up_w8(const void* x, const void* w8, const float* wsc, const int32_t* cnt, void* act, int M, int E,
                      int H, int F, hipStream_t stream);
int mp_moe_down_w8(const void* act, const void* w8, const float* wsc, const int32_t* cnt, const float* wd, void* y,
                   int64_t y_stride, int M, int E, int H, int F, hipStream_t stream);
int mp_moe_w8_ok(int M, int E, int H, int F);
// lora.hip: 0, 1 when the shape is not covered (needs M <= 64, K % 32 == 0, N % 8 == 0, R % 16 == 0,
// R <= 192; nothing launched), < 0 for a bad call, else the HIP error.  M == 0 returns 0.
int mp_lora_ok(int M, int N, int K, int R);
int mp_lora_shrink(const mp::LoraArgs* a, hipStream_t stream);
int mp_lora_expand(const mp::LoraArgs* a, hipStream_t stream);
// fp8.hip
void mp_fp8_set_kernel(int kind);
int mp_quant_act_fp8(const void* ap, void* a8, float* scale, float* part, int M, int K, hipStream_t stream);
int mp_quant_rows_fp8(const void* x, int64_t xs, void* a8, float* scale, int M, int K, hipStream_t stream);
int mp_gemm_fp8(const void* a8, const float* as, const void* wq, const float* ws, void* y, int64_t ys, const void* res,
                int64_t rs, int M, int N, int K, int epilogue, int out_packed, int kind, float* part,
                int64_t part_bytes, hipStream_t stream);
}
