// torch custom-op registrations (namespace `mpamd`) for the gfx950 kernels.
//
// Every op writes into caller-provided outputs and launches on the current HIP
// stream, so a whole stage step can be captured into one hipGraph.  Shape and
// dtype checks happen here, on the host, before any kernel sees a pointer.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <torch/library.h>

#include <cmath>
#include <tuple>
#include <utility>

#include "mp_api.h"

namespace {

#define MP_CHECK(cond, msg) TORCH_CHECK(cond, "mpamd: ", msg)

inline void check_launch(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "mpamd: ", what, " launch failed with code ", rc);
}

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

inline void check_bf16_cuda(const at::Tensor& t, const char* name) {
  MP_CHECK(t.is_cuda(), std::string(name) + " must be on the GPU");
  MP_CHECK(t.scalar_type() == at::kBFloat16, std::string(name) + " must be bf16");
}

inline void check_rows(const at::Tensor& t, const char* name) {
  MP_CHECK(t.dim() == 2, std::string(name) + " must be 2-D [rows, cols]");
  MP_CHECK(t.stride(1) == 1, std::string(name) + " must have unit inner stride");
  MP_CHECK(t.stride(0) % 8 == 0, std::string(name) + " row stride must be a multiple of 8");
  MP_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, std::string(name) + " must be 16-B aligned");
}

inline int64_t packed_numel(int64_t M, int64_t K) { return ((M + 15) / 16) * 16 * K; }

// fused-norm row statistics: int64 [32 shards][256 rows] fixed-point sums (gemm.hip EpiArgs)
inline void* opt_ss(const c10::optional<at::Tensor>& t, const char* name) {
  if (!t.has_value()) return nullptr;
  MP_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous() && t->numel() >= mp_gemm_ss_elems(),
           std::string(name) + ": int64 cuda contiguous [32, 256] (ops.norm_stats_buffer)");
  return t->data_ptr();
}

// fp8 weight of the W8A16 / W8A8-MX decode GEMMs and its per-column scales -> (N, K)
inline std::pair<int, int> check_w8_weight(const at::Tensor& wq, const at::Tensor& wsc) {
  MP_CHECK(wq.is_cuda() && wq.scalar_type() == at::kByte && wq.dim() == 4 && wq.size(2) == 64 && wq.size(3) == 8 &&
               wq.is_contiguous(),
           "wq must be an fp8 weight uint8 [N/16, K/32, 64, 8] (ops.pack_weight_w8)");
  const int N = 16 * wq.size(0), K = 32 * wq.size(1);
  MP_CHECK(wsc.is_cuda() && wsc.scalar_type() == at::kFloat && wsc.is_contiguous() && wsc.numel() == N,
           "wsc: fp32 [N] column scales");
  return {N, K};
}

// decode-GEMM output of M rows: packed (SwiGLU only) or row-major; SwiGLU halves the N columns
inline void check_gemm_out(const at::Tensor& y, int64_t M, int64_t N, int64_t epilogue, bool opk) {
  const int64_t ncols = epilogue == 1 ? N / 2 : N;
  if (opk) {
    MP_CHECK(epilogue == 1 && y.is_contiguous() && y.numel() >= packed_numel(M, ncols), "packed y");
    // 32-column groups, as opt_packed: an odd count of gate/up pairs would store past packed_numel(M, ncols)
    MP_CHECK(ncols % 32 == 0, "packed y: the packed output needs N / 2 % 32 == 0");
  } else {
    check_rows(y, "y");
    MP_CHECK(y.size(0) == M && y.size(1) == ncols, "y shape");
  }
}

// optional row-major bf16 [M, N] operand -> (pointer, row stride); (nullptr, 0) when absent
inline std::pair<const void*, int64_t> opt_rows(const c10::optional<at::Tensor>& t, const char* name, int64_t M,
                                                int64_t N) {
  if (!t.has_value()) return {nullptr, 0};
  check_bf16_cuda(*t, name);
  check_rows(*t, name);
  MP_CHECK(t->size(0) == M && t->size(1) == N, std::string(name) + " shape");
  return {t->data_ptr(), t->stride(0)};
}

// optional packed bf16 copy of the [M, N] output (epilogue 3's ``ap``)
inline void* opt_packed(const c10::optional<at::Tensor>& ap, int64_t M, int64_t N) {
  if (!ap.has_value()) return nullptr;
  check_bf16_cuda(*ap, "ap");
  // the packed layout lives in 32-column groups: with an odd column-tile count the last tile's copy
  // would land up to half a group past packed_numel(M, N)
  MP_CHECK(N % 32 == 0, "ap: the packed copy needs N % 32 == 0");
  MP_CHECK(ap->is_contiguous() && ap->numel() >= packed_numel(M, N), "ap: packed [ceil(M/16)*16*N]");
  return ap->data_ptr();
}

// optional GEMM workspace (ops.gemm_workspace)
inline void* opt_workspace(const c10::optional<at::Tensor>& ws) {
  if (!ws.has_value()) return nullptr;
  MP_CHECK(ws->is_cuda() && ws->is_contiguous() && ws->numel() * ws->element_size() >= mp_gemm_workspace_bytes(),
           "gemm workspace too small (ops.gemm_workspace)");
  return ws->data_ptr();
}

void rmsnorm(const at::Tensor& x, at::Tensor& residual, const at::Tensor& w, at::Tensor& y, double eps, int64_t mode,
             const c10::optional<at::Tensor>& rows, int64_t packed, const c10::optional<at::Tensor>& ss,
             const c10::optional<at::Tensor>& a8, const c10::optional<at::Tensor>& a8_scale,
             const c10::optional<at::Tensor>& gather) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(w, "w");
  check_bf16_cuda(y, "y");
  check_rows(x, "x");
  const int H = x.size(1);
  MP_CHECK(w.numel() == H && w.is_contiguous(), "weight shape");
  if (!packed) {
    check_rows(y, "y");
    MP_CHECK(y.size(1) == H, "y cols");
  }
  MP_CHECK(mode >= 0 && mode <= 3, "mode");
  void* ssp = opt_ss(ss, "ss");
  // gather: x is an embedding table and row t of the output / residual is x[gather[t]] (stage entry)
  const int64_t* gp = nullptr;
  int nrows = x.size(0);
  if (gather.has_value()) {
    MP_CHECK(gather->is_cuda() && gather->scalar_type() == at::kLong && gather->is_contiguous() && gather->dim() == 1,
             "gather: int64 cuda [T]");
    MP_CHECK(mode >= 2 && !rows.has_value(), "gather with mode 2 / 3, no rows");
    gp = gather->data_ptr<int64_t>();
    nrows = gather->numel();
  }
  MP_CHECK(mode != 3 || (ssp != nullptr && nrows <= 256), "mode 3 needs ss and <= 256 rows");
  if (mode != 0) {
    check_bf16_cuda(residual, "residual");
    check_rows(residual, "residual");
    MP_CHECK(residual.size(0) == nrows && residual.size(1) == H, "residual shape");
  }
  const int32_t* rp = nullptr;
  if (rows.has_value()) {
    MP_CHECK(rows->scalar_type() == at::kInt && rows->is_contiguous() && rows->is_cuda(), "rows: int32 cuda");
    MP_CHECK(mode == 0, "row gather only with mode 0");
    rp = rows->data_ptr<int32_t>();
    nrows = rows->numel();
  }
  int pmt = 0;
  if (packed) {
    MP_CHECK(H % 32 == 0 && y.is_contiguous() && y.numel() >= packed_numel(nrows, H), "packed y too small");
    pmt = (nrows + 15) / 16;
  } else {
    MP_CHECK(y.size(0) >= nrows, "y rows");
  }
  void* a8p = nullptr;
  float* a8s = nullptr;
  if (a8.has_value()) {  // fp8 output (W8A8 decode path): A8 [K/64][MT][64][16 B] + per-row scales
    MP_CHECK(packed && a8_scale.has_value(), "fp8 output needs packed=1 and a8_scale");
    MP_CHECK(a8->is_cuda() && a8->scalar_type() == at::kByte && a8->is_contiguous() &&
                 a8->numel() >= packed_numel(nrows, H) && H % 64 == 0, "a8: uint8 [packed_numel(rows, H)], H % 64");
    MP_CHECK(a8_scale->is_cuda() && a8_scale->scalar_type() == at::kFloat && a8_scale->numel() >= nrows,
             "a8_scale: fp32 [rows]");
    a8p = a8->data_ptr();
    a8s = a8_scale->data_ptr<float>();
  }
  check_launch(mp_rmsnorm(x.data_ptr(), x.stride(0), mode ? residual.data_ptr() : nullptr,
                          mode ? residual.stride(0) : 0, w.data_ptr(), y.data_ptr(), packed ? 0 : y.stride(0), rp,
                          nrows, H, (float)eps, (int)mode, pmt, ssp, a8p, a8s, gp, gp ? x.size(0) : 0,
                          cur_stream()),
               "rmsnorm");
}

// RoPE operands of the fused qkv rows [T, (nh + 2 nkv) * D]: rotary positions and cache slots int64 [T],
// cos / sin tables fp32 [max_pos, D / 2]
inline void check_rope(const at::Tensor& qkv, const at::Tensor& positions, const at::Tensor& cos,
                       const at::Tensor& sin, const at::Tensor& slots, int64_t nh, int64_t nkv, int D) {
  MP_CHECK(qkv.size(1) == (nh + 2 * nkv) * D, "qkv width");
  const int T = qkv.size(0);
  MP_CHECK(positions.scalar_type() == at::kLong && positions.numel() == T && positions.is_contiguous(), "positions");
  MP_CHECK(slots.scalar_type() == at::kLong && slots.numel() == T && slots.is_contiguous(), "slots");
  MP_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
               sin.is_contiguous() && cos.size(1) == D / 2 && sin.sizes() == cos.sizes(),
           "cos/sin tables fp32 [max_pos, D/2]");
}

// bf16 KV cache of the attention ops: pages [pages, nkv, page, D]; attn_args checks it against nkv
// (an fp8 cache's byte pages handed to a bf16 kernel would be read past their end)
inline void check_kv_bf16(const at::Tensor& k_cache, const at::Tensor& v_cache) {
  check_bf16_cuda(k_cache, "k_cache");
  check_bf16_cuda(v_cache, "v_cache");
  MP_CHECK(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes(), "cache [pages, nkv, page, D]");
}

// fp8 KV cache (kv_f8.h): codes uint8 [pages, nkv, page, D] + e8m0 scales uint8 [pages, nkv, page]
inline void check_kv_f8(const at::Tensor& k_cache, const at::Tensor& v_cache, const at::Tensor& k_scale,
                        const at::Tensor& v_scale, int64_t nkv) {
  for (const at::Tensor* t : {&k_cache, &v_cache, &k_scale, &v_scale})
    MP_CHECK(t->is_cuda() && t->scalar_type() == at::kByte && t->is_contiguous() && t->device() == k_cache.device(),
             "fp8 KV cache: codes and scales are contiguous uint8 tensors on one GPU");
  MP_CHECK(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes() && k_cache.size(1) == nkv,
           "fp8 KV codes [pages, nkv, page, D]");
  MP_CHECK(k_cache.size(3) == 64 || k_cache.size(3) == 128, "fp8 KV cache: head_dim 64 or 128");
  MP_CHECK(k_scale.dim() == 3 && k_scale.sizes() == v_scale.sizes() && k_scale.size(0) == k_cache.size(0) &&
               k_scale.size(1) == nkv && k_scale.size(2) == k_cache.size(2),
           "fp8 KV scales [pages, nkv, page] must match the codes' pages, heads and page_size");
  MP_CHECK(reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % 8 == 0 &&
               reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % 8 == 0, "fp8 KV codes must be 8-B aligned");
}

using OptTensor = c10::optional<at::Tensor>;

// The cache type of an op, told by its trailing k_scale / v_scale: both given - an fp8 cache, neither -
// a bf16 cache.
inline bool kv_is_f8(const OptTensor& k_scale, const OptTensor& v_scale) {
  MP_CHECK(k_scale.has_value() == v_scale.has_value(),
           "fp8 KV cache: k_scale and v_scale are given together (neither: a bf16 cache)");
  return k_scale.has_value();
}

// The cache pair of an attention op, by its type (true: fp8).  Code pages without scales fail the
// bf16 rules and bf16 pages with scales the fp8 rules.
inline bool check_kv(const at::Tensor& k_cache, const at::Tensor& v_cache, const OptTensor& k_scale,
                     const OptTensor& v_scale, int64_t nkv) {
  const bool f8 = kv_is_f8(k_scale, v_scale);
  if (f8) check_kv_f8(k_cache, v_cache, *k_scale, *v_scale, nkv);
  else check_kv_bf16(k_cache, v_cache);
  return f8;
}

// RoPE of q in place + the new tokens' k / v into their cache slots; with scales, quantized into an fp8 cache
void rope_kv_write(at::Tensor& qkv, const at::Tensor& positions, const at::Tensor& cos, const at::Tensor& sin,
                   at::Tensor& k_cache, at::Tensor& v_cache, const at::Tensor& slots, int64_t nh, int64_t nkv,
                   const OptTensor& k_scale, const OptTensor& v_scale) {
  check_bf16_cuda(qkv, "qkv");
  check_rows(qkv, "qkv");
  const bool f8 = kv_is_f8(k_scale, v_scale);
  if (f8) {
    check_kv_f8(k_cache, v_cache, *k_scale, *v_scale, nkv);
  } else {
    check_bf16_cuda(k_cache, "k_cache");
    check_bf16_cuda(v_cache, "v_cache");
    MP_CHECK(k_cache.dim() == 4 && k_cache.is_contiguous() && v_cache.is_contiguous(), "cache [pages, nkv, page, D]");
    MP_CHECK(k_cache.sizes() == v_cache.sizes(), "k/v cache shapes differ");
    MP_CHECK(k_cache.size(1) == nkv, "cache kv heads");
  }
  const int D = k_cache.size(3);
  check_rope(qkv, positions, cos, sin, slots, nh, nkv, D);
  if (f8) {
    check_launch(mp_rope_kv_write_f8(qkv.data_ptr(), qkv.stride(0), positions.data_ptr<int64_t>(),
                                     cos.data_ptr<float>(), sin.data_ptr<float>(), k_cache.data_ptr(),
                                     v_cache.data_ptr(), k_scale->data_ptr(), v_scale->data_ptr(),
                                     slots.data_ptr<int64_t>(), qkv.size(0), nh, nkv, D, k_cache.size(2),
                                     cur_stream()),
                 "rope_kv_write_f8");
    return;
  }
  check_launch(mp_rope_kv_write(qkv.data_ptr(), qkv.stride(0), positions.data_ptr<int64_t>(), cos.data_ptr<float>(),
                                sin.data_ptr<float>(), k_cache.data_ptr(), v_cache.data_ptr(),
                                slots.data_ptr<int64_t>(), qkv.size(0), nh, nkv, D, k_cache.size(2), cur_stream()),
               "rope_kv_write");
}

void kv_write(const at::Tensor& k, const at::Tensor& v, at::Tensor& k_cache, at::Tensor& v_cache,
              const at::Tensor& slots) {
  check_bf16_cuda(k, "k");
  check_bf16_cuda(v, "v");
  check_rows(k, "k");
  check_rows(v, "v");
  MP_CHECK(k_cache.dim() == 4 && k_cache.is_contiguous() && v_cache.is_contiguous(), "cache layout");
  const int nkv = k_cache.size(1), page = k_cache.size(2), D = k_cache.size(3);
  MP_CHECK(k.size(1) == nkv * D && v.size(1) == nkv * D, "k/v width");
  MP_CHECK(slots.scalar_type() == at::kLong && slots.numel() == k.size(0), "slots");
  check_launch(mp_kv_write(k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), k_cache.data_ptr(),
                           v_cache.data_ptr(), slots.data_ptr<int64_t>(), k.size(0), nkv, D, page, cur_stream()),
               "kv_write");
}

// The operands every attention op shares -> the launcher's arguments (mp_api.h), the fused-RoPE group
// and the qkv partials left empty.  The caller has checked the cache pair (check_kv); k_scale / v_scale:
// the fp8 cache's scales.  packed: the output in the packed activation layout.
mp::AttnArgs attn_args(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                       const OptTensor& k_scale, const OptTensor& v_scale, const at::Tensor& block_tables,
                       const at::Tensor& q_seq, const at::Tensor& q_ctx, at::Tensor& out, at::Tensor& workspace,
                       int64_t nh, int64_t nkv, double scale, int64_t part_size, int64_t num_parts, int64_t packed) {
  check_bf16_cuda(q, "q");
  check_rows(q, "q");
  check_bf16_cuda(out, "out");
  MP_CHECK(out.is_contiguous(), "out contiguous");
  const int D = k_cache.size(3);
  const int T = q.size(0);
  MP_CHECK(q.size(1) >= nh * D, "q width");
  if (packed) {
    MP_CHECK(out.numel() >= packed_numel(T, nh * D) && (nh * D) % 32 == 0, "packed out numel");
  } else {
    MP_CHECK(out.numel() == (int64_t)T * nh * D, "out numel");
  }
  MP_CHECK(k_cache.size(1) == nkv && k_cache.is_contiguous() && v_cache.is_contiguous(), "cache");
  MP_CHECK(block_tables.scalar_type() == at::kInt && block_tables.dim() == 2 && block_tables.stride(1) == 1,
           "block_tables int32 [S, max_pages]");
  MP_CHECK(q_seq.scalar_type() == at::kInt && q_seq.numel() == T, "q_seq");
  MP_CHECK(q_ctx.scalar_type() == at::kInt && q_ctx.numel() == T, "q_ctx");
  MP_CHECK(workspace.scalar_type() == at::kFloat, "workspace fp32");
  if (num_parts > 1) MP_CHECK(workspace.numel() >= (int64_t)T * nh * num_parts * (D + 2), "workspace too small");
  mp::AttnArgs a{};
  a.q = q.data_ptr();
  a.q_stride = q.stride(0);
  a.kc = k_cache.data_ptr();
  a.vc = v_cache.data_ptr();
  if (k_scale.has_value()) {
    a.ks = k_scale->data_ptr();
    a.vs = v_scale->data_ptr();
  }
  a.bt = block_tables.data_ptr<int32_t>();
  a.bt_stride = block_tables.stride(0);
  a.q_seq = q_seq.data_ptr<int32_t>();
  a.q_ctx = q_ctx.data_ptr<int32_t>();
  a.out = out.data_ptr();
  a.workspace = workspace.data_ptr<float>();
  a.T = T;
  a.nh = nh;
  a.nkv = nkv;
  a.D = D;
  a.page_size = k_cache.size(2);
  a.PS = part_size;
  a.NP = num_parts;
  a.scale = (float)scale;
  a.packed_mt = packed ? (T + 15) / 16 : 0;
  return a;
}

// The sliding window of a launch (mp::AttnArgs::window).  built: this launch implements it; one that
// does not refuses a window instead of attending to the whole context.
inline void attn_window(mp::AttnArgs& a, int64_t window, bool built, const char* what) {
  MP_CHECK(window >= 0 && window <= INT32_MAX, "window must be >= 0 (0: no sliding window)");
  MP_CHECK(window == 0 || built, std::string(what) + " has no sliding-window form: window must be 0");
  a.window = (int)window;
}

// The qkv projection as split-K partial slabs [S][T][width] fp32 + the fused-norm row statistics
// (mp::QkvPart), read by the decode attention kernels; part == nullptr when absent.
mp::QkvPart qkv_part_args(const c10::optional<at::Tensor>& part, int64_t splits, const c10::optional<at::Tensor>& ss,
                          double inv_k, double eps, int64_t T, int64_t width) {
  if (!part.has_value()) return mp::QkvPart{};
  MP_CHECK(part->is_cuda() && part->scalar_type() == at::kFloat && part->is_contiguous() && part->dim() == 3 &&
               part->size(0) == splits && part->size(1) == T && part->size(2) == width,
           "qkv_part: fp32 [S, T, qkv width] split-K slabs (ops.linear_partials)");
  MP_CHECK(splits >= 1 && splits <= 8, "qkv_part splits");
  const unsigned long long* ssp = nullptr;
  if (ss.has_value()) {
    MP_CHECK(ss->is_cuda() && ss->scalar_type() == at::kLong && ss->is_contiguous() && ss->numel() >= mp_gemm_ss_elems(),
             "part_ss: row statistics [32, 256] int64");
    ssp = reinterpret_cast<const unsigned long long*>(ss->data_ptr<int64_t>());
  }
  return mp::QkvPart{part->data_ptr<float>(), (int)splits, T * width, (int)width, ssp, (float)inv_k, (float)eps};
}

// the fused-RoPE group of a decode launch (operands checked by check_rope) and its qkv partials
inline void fuse_rope(mp::AttnArgs& a, const at::Tensor& positions, const at::Tensor& cos, const at::Tensor& sin,
                      const at::Tensor& slots, const mp::QkvPart& qp) {
  a.rope_pos = positions.data_ptr<int64_t>();
  a.cos_t = cos.data_ptr<float>();
  a.sin_t = sin.data_ptr<float>();
  a.slots = slots.data_ptr<int64_t>();
  a.qp = qp;
}

// int32 [2, N] block table (row 0: first token or block, row 1: count) -> (row 0, N); row 1 = row 0 + N
inline std::pair<const int32_t*, int> check_blocks(const at::Tensor& t, bool on_gpu, int64_t max_n, const char* msg) {
  MP_CHECK((!on_gpu || t.is_cuda()) && t.scalar_type() == at::kInt && t.dim() == 2 && t.size(0) == 2 &&
               t.is_contiguous() && t.size(1) <= max_n, msg);
  return {t.data_ptr<int32_t>(), (int)t.size(1)};
}

// The flash-decoding launch (attention.hip), on a bf16 or an fp8 (a.ks) cache.  counters: optional
// arrival counters of the in-launch split-K combine.
void launch_paged(mp::AttnArgs a, const c10::optional<at::Tensor>& counters, int64_t window) {
  attn_window(a, window, true, "paged_attention");
  int* cp = nullptr;
  int ncnt = 0;
  if (counters.has_value()) {
    MP_CHECK(counters->is_cuda() && counters->scalar_type() == at::kInt && counters->is_contiguous(),
             "counters: zero-initialised cuda int32");
    cp = counters->data_ptr<int32_t>();
    ncnt = (int)counters->numel();
  }
  check_launch(mp_paged_attention(&a, cp, ncnt, cur_stream()),
               a.ks != nullptr ? "paged_attention_f8" : "paged_attention");
}

// Flash-decoding paged attention; with k_scale / v_scale on an fp8 KV cache (attention.hip F8 form).
void paged_attention(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                     const at::Tensor& block_tables, const at::Tensor& q_seq, const at::Tensor& q_ctx,
                     at::Tensor& out, at::Tensor& workspace, int64_t nh, int64_t nkv, double scale, int64_t part_size,
                     int64_t num_parts, int64_t packed, const OptTensor& counters, int64_t window,
                     const OptTensor& k_scale, const OptTensor& v_scale) {
  check_kv(k_cache, v_cache, k_scale, v_scale, nkv);
  launch_paged(attn_args(q, k_cache, v_cache, k_scale, v_scale, block_tables, q_seq, q_ctx, out, workspace, nh, nkv,
                         scale, part_size, num_parts, packed),
               counters, window);
}

// Decode attention with RoPE + KV write fused in (attention.hip ROPE path): q is the unrotated
// fused qkv row; k_cache / v_cache receive the new token at slots[t].  On an fp8 cache: RoPE, the new
// token's quantization + page write and attention in one launch.
void paged_attention_rope(const at::Tensor& qkv, at::Tensor& k_cache, at::Tensor& v_cache,
                          const at::Tensor& block_tables, const at::Tensor& q_seq, const at::Tensor& q_ctx,
                          const at::Tensor& positions, const at::Tensor& cos, const at::Tensor& sin,
                          const at::Tensor& slots, at::Tensor& out, at::Tensor& workspace, int64_t nh, int64_t nkv,
                          double scale, int64_t part_size, int64_t num_parts, int64_t packed,
                          const OptTensor& counters, const OptTensor& qkv_part, int64_t part_splits,
                          const OptTensor& part_ss, double inv_k, double eps, int64_t window,
                          const OptTensor& k_scale, const OptTensor& v_scale) {
  check_kv(k_cache, v_cache, k_scale, v_scale, nkv);
  const int D = k_cache.size(3);
  check_rope(qkv, positions, cos, sin, slots, nh, nkv, D);
  MP_CHECK(D % 16 == 0, "head dim");
  const mp::QkvPart qp = qkv_part_args(qkv_part, part_splits, part_ss, inv_k, eps, qkv.size(0), qkv.size(1));
  mp::AttnArgs a = attn_args(qkv, k_cache, v_cache, k_scale, v_scale, block_tables, q_seq, q_ctx, out, workspace, nh,
                             nkv, scale, part_size, num_parts, packed);
  fuse_rope(a, positions, cos, sin, slots, qp);
  launch_paged(a, counters, window);
}

// The MFMA launch (attention_mfma.hip): query blocks, optional prefill superblocks int32 [2, NSB]
// (first query block, count <= 4), optional MX output.
void launch_mfma(mp::AttnArgs a, const at::Tensor& qblocks, const OptTensor& superblocks, int64_t window,
                 void* mx_ax = nullptr, void* mx_as = nullptr) {
  const auto [qb, NB] = check_blocks(qblocks, false, INT64_MAX, "qblocks int32 [2, NB] (first token, token count)");
  // the window is built for decode blocks (one token per block, NB == T), not for multi-token blocks
  // or the grouped prefill kernel
  attn_window(a, window, NB == a.T && !superblocks.has_value(),
              "attention_mfma with multi-token query blocks or superblocks");
  const int32_t* sb = nullptr;
  int NSB = 0;
  if (superblocks.has_value())
    std::tie(sb, NSB) = check_blocks(*superblocks, true, NB, "superblocks int32 [2, NSB] (ops.query_superblocks)");
  check_launch(mp_attention_mfma(&a, qb, qb + NB, NB, sb, sb != nullptr ? sb + NSB : nullptr, NSB, mx_ax, mx_as,
                                 cur_stream()),
               "attention_mfma");
}

// The MFMA ops on an fp8 cache (attention_mfma.hip F8 form): decode blocks only (one token per query
// block), the whole GQA group in the MFMA rows - no superblocks, no MX output.
inline void check_mfma_f8(const at::Tensor& q, const at::Tensor& qblocks, int64_t nh, int64_t nkv, bool superblocks,
                          bool mx_out) {
  MP_CHECK(!superblocks, "attention_mfma on an fp8 KV cache has no grouped prefill form: superblocks must be None");
  MP_CHECK(!mx_out, "attention_mfma on an fp8 KV cache has no MX output: mx_ax must be None");
  MP_CHECK(nkv > 0 && nh % nkv == 0 && (nh / nkv == 4 || nh / nkv == 8 || (nh / nkv >= 16 && (nh / nkv) % 16 == 0)),
           "attention_mfma on an fp8 KV cache supports GQA group sizes nh / nkv of 4, 8 and multiples of 16");
  MP_CHECK(qblocks.dim() == 2 && qblocks.size(1) == q.size(0),
           "attention_mfma on an fp8 KV cache needs one query token per block (decode)");
}

void attention_mfma(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                    const at::Tensor& block_tables, const at::Tensor& q_seq, const at::Tensor& q_ctx,
                    const at::Tensor& qblocks, at::Tensor& out, at::Tensor& workspace, int64_t nh, int64_t nkv,
                    double scale, int64_t part_size, int64_t num_parts, int64_t packed, const OptTensor& superblocks,
                    int64_t window, const OptTensor& k_scale, const OptTensor& v_scale) {
  if (check_kv(k_cache, v_cache, k_scale, v_scale, nkv))
    check_mfma_f8(q, qblocks, nh, nkv, superblocks.has_value(), false);
  launch_mfma(attn_args(q, k_cache, v_cache, k_scale, v_scale, block_tables, q_seq, q_ctx, out, workspace, nh, nkv,
                        scale, part_size, num_parts, packed),
              qblocks, superblocks, window);
}

// Causal prefill attention, 32x32x16 MFMA FA2 form (attention_fa.hip): row-major output, on a bf16 or an
// fp8 cache.  windowed: the sliding-window form (WIN form), which needs a window W > 0 - a query of
// context ctx sees [max(0, ctx - W), ctx), and part_size x num_parts covers the span a block streams;
// the plain op keeps refusing a window.
void launch_fa(bool windowed, const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
               const at::Tensor& block_tables, const at::Tensor& q_seq, const at::Tensor& q_ctx,
               const at::Tensor& fablocks, at::Tensor& out, at::Tensor& workspace, int64_t nh, int64_t nkv,
               double scale, int64_t part_size, int64_t num_parts, int64_t waves, int64_t pair, int64_t window,
               const OptTensor& k_scale, const OptTensor& v_scale) {
  const bool f8 = check_kv(k_cache, v_cache, k_scale, v_scale, nkv);
  const std::string name = std::string(windowed ? "attention_fa_window" : "attention_fa") + (f8 ? "_f8" : "");
  MP_CHECK(k_cache.size(3) == 128, name + ": head_dim 128");
  mp::AttnArgs a = attn_args(q, k_cache, v_cache, k_scale, v_scale, block_tables, q_seq, q_ctx, out, workspace, nh,
                             nkv, scale, part_size, num_parts, 0);
  attn_window(a, window, windowed, "attention_fa");
  MP_CHECK(!windowed || window > 0, "attention_fa_window: window must be > 0");
  const auto [fb, NB] =
      check_blocks(fablocks, true, INT64_MAX, "fablocks int32 [2, NB] (first token, token count), ops.fa_blocks");
  MP_CHECK(waves == 4 || waves == 8, "waves 4 or 8");
  check_launch(mp_attention_fa(&a, fb, fb + NB, NB, (int)waves, (int)pair, windowed, cur_stream()), name.c_str());
}

void attention_fa(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                  const at::Tensor& block_tables, const at::Tensor& q_seq, const at::Tensor& q_ctx,
                  const at::Tensor& fablocks, at::Tensor& out, at::Tensor& workspace, int64_t nh, int64_t nkv,
                  double scale, int64_t part_size, int64_t num_parts, int64_t waves, int64_t pair, int64_t window,
                  const OptTensor& k_scale, const OptTensor& v_scale) {
  launch_fa(false, q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, out, workspace, nh, nkv, scale,
            part_size, num_parts, waves, pair, window, k_scale, v_scale);
}

void attention_fa_window(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                         const at::Tensor& block_tables, const at::Tensor& q_seq, const at::Tensor& q_ctx,
                         const at::Tensor& fablocks, at::Tensor& out, at::Tensor& workspace, int64_t nh, int64_t nkv,
                         double scale, int64_t part_size, int64_t num_parts, int64_t waves, int64_t pair,
                         int64_t window, const OptTensor& k_scale, const OptTensor& v_scale) {
  launch_fa(true, q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, out, workspace, nh, nkv, scale,
            part_size, num_parts, waves, pair, window, k_scale, v_scale);
}

// GQA decode with RoPE + KV write fused (attention_mfma.hip ROPE path): one token per query block,
// block b = token b (the kernel reads no qblocks on this path; ``decode_qblocks`` builds exactly that).
void attention_mfma_rope(const at::Tensor& qkv, at::Tensor& k_cache, at::Tensor& v_cache,
                         const at::Tensor& block_tables, const at::Tensor& q_seq, const at::Tensor& q_ctx,
                         const at::Tensor& qblocks, const at::Tensor& positions, const at::Tensor& cos,
                         const at::Tensor& sin, const at::Tensor& slots, at::Tensor& out, at::Tensor& workspace,
                         int64_t nh, int64_t nkv, double scale, int64_t part_size, int64_t num_parts, int64_t packed,
                         const OptTensor& qkv_part, int64_t part_splits, const OptTensor& part_ss, double inv_k,
                         double eps, const OptTensor& mx_ax, const OptTensor& mx_as, int64_t window,
                         const OptTensor& k_scale, const OptTensor& v_scale) {
  if (check_kv(k_cache, v_cache, k_scale, v_scale, nkv))
    check_mfma_f8(qkv, qblocks, nh, nkv, false, mx_ax.has_value());
  const int D = k_cache.size(3), T = qkv.size(0);
  check_rope(qkv, positions, cos, sin, slots, nh, nkv, D);
  MP_CHECK(qblocks.size(1) == T, "fused RoPE needs one query token per block (decode)");
  const mp::QkvPart qp = qkv_part_args(qkv_part, part_splits, part_ss, inv_k, eps, T, qkv.size(1));
  void* axp = nullptr;
  void* asp = nullptr;
  if (mx_ax.has_value()) {  // the output as the W8A8-MX GEMM's activation (ops.quant_mx layout)
    MP_CHECK(mx_as.has_value() && packed && num_parts == 1 && D == 128, "mx output: packed, one part, D 128, as_");
    const int64_t K = nh * D, rows = ((T + 15) / 16) * 16;
    MP_CHECK(mx_ax->is_cuda() && mx_ax->scalar_type() == at::kByte && mx_ax->is_contiguous() && mx_ax->numel() >= rows * K,
             "mx_ax: uint8 [ceil(T/16)*16*K]");
    MP_CHECK(mx_as->is_cuda() && mx_as->scalar_type() == at::kByte && mx_as->is_contiguous() && mx_as->numel() >= 2 * K,
             "mx_as: uint8 [2K]");
    axp = mx_ax->data_ptr();
    asp = mx_as->data_ptr();
  }
  mp::AttnArgs a = attn_args(qkv, k_cache, v_cache, k_scale, v_scale, block_tables, q_seq, q_ctx, out, workspace, nh,
                             nkv, scale, part_size, num_parts, packed);
  fuse_rope(a, positions, cos, sin, slots, qp);
  launch_mfma(a, qblocks, c10::nullopt, window, axp, asp);
}

void embedding(const at::Tensor& ids, const at::Tensor& table, at::Tensor& out) {
  check_bf16_cuda(table, "table");
  check_bf16_cuda(out, "out");
  MP_CHECK(ids.scalar_type() == at::kLong && ids.is_contiguous(), "ids int64");
  MP_CHECK(table.is_contiguous() && out.is_contiguous(), "contiguous");
  MP_CHECK(out.numel() == ids.numel() * table.size(1), "out shape");
  check_launch(mp_embedding(ids.data_ptr<int64_t>(), table.data_ptr(), out.data_ptr(), ids.numel(), table.size(1),
                            table.size(0), cur_stream()),
               "embedding");
}

void swiglu(const at::Tensor& gu, at::Tensor& out) {
  check_bf16_cuda(gu, "gu");
  check_bf16_cuda(out, "out");
  MP_CHECK(gu.is_contiguous() && out.is_contiguous(), "contiguous");
  const int64_t T = gu.size(0);
  const int F = gu.size(1) / 2;
  MP_CHECK(out.numel() == T * F, "out shape");
  check_launch(mp_swiglu(gu.data_ptr(), out.data_ptr(), T, F, cur_stream()), "swiglu");
}

void add(const at::Tensor& a, const at::Tensor& b, at::Tensor& y) {
  check_bf16_cuda(a, "a");
  check_bf16_cuda(b, "b");
  check_bf16_cuda(y, "y");
  MP_CHECK(a.is_contiguous() && b.is_contiguous() && y.is_contiguous(), "contiguous");
  MP_CHECK(a.numel() == b.numel() && a.numel() == y.numel(), "numel");
  check_launch(mp_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), cur_stream()), "add");
}

void argmax(const at::Tensor& logits, at::Tensor& out) {
  check_bf16_cuda(logits, "logits");
  check_rows(logits, "logits");
  MP_CHECK(out.scalar_type() == at::kLong && out.numel() == logits.size(0), "out int64 [R]");
  check_launch(mp_argmax(logits.data_ptr(), logits.stride(0), logits.size(0), logits.size(1),
                         out.data_ptr<int64_t>(), cur_stream()),
               "argmax");
}

void sample(const at::Tensor& logits, const at::Tensor& temps, const at::Tensor& top_ps, const at::Tensor& top_ks,
            const at::Tensor& rep_pens, at::Tensor& recent, at::Tensor& recent_len, const at::Tensor& seeds,
            at::Tensor& workspace, at::Tensor& out, int64_t update) {
  check_bf16_cuda(logits, "logits");
  check_rows(logits, "logits");
  const int R = logits.size(0), V = logits.size(1);
  MP_CHECK(temps.scalar_type() == at::kFloat && temps.numel() == R, "temps");
  MP_CHECK(top_ps.scalar_type() == at::kFloat && top_ps.numel() == R, "top_ps");
  MP_CHECK(top_ks.scalar_type() == at::kInt && top_ks.numel() == R, "top_ks");
  MP_CHECK(rep_pens.scalar_type() == at::kFloat && rep_pens.numel() == R, "rep_pens");
  MP_CHECK(recent.scalar_type() == at::kInt && recent.dim() == 2 && recent.size(0) == R && recent.is_contiguous(),
           "recent int32 [R, n]");
  MP_CHECK(recent_len.scalar_type() == at::kInt && recent_len.numel() == R, "recent_len");
  MP_CHECK(seeds.scalar_type() == at::kLong && seeds.numel() == R, "seeds");
  MP_CHECK(workspace.scalar_type() == at::kFloat && workspace.numel() >= (int64_t)R * V, "workspace");
  MP_CHECK(out.scalar_type() == at::kLong && out.numel() == R, "out");
  check_launch(mp_sample(logits.data_ptr(), logits.stride(0), R, V, temps.data_ptr<float>(), top_ps.data_ptr<float>(),
                         top_ks.data_ptr<int32_t>(), rep_pens.data_ptr<float>(), recent.data_ptr<int32_t>(),
                         recent.size(1), recent_len.data_ptr<int32_t>(), seeds.data_ptr<int64_t>(),
                         workspace.data_ptr<float>(), out.data_ptr<int64_t>(), (int)update, cur_stream()),
               "sample");
}

int64_t sample_verify_ws(int64_t R, int64_t V, int64_t cap) { return mp_sample_verify_ws_words(R, V, cap); }

void sample_verify(const at::Tensor& logits, const at::Tensor& row_start, const at::Tensor& draft,
                   const at::Tensor& temps, const at::Tensor& top_ps, const at::Tensor& top_ks,
                   const at::Tensor& rep_pens, at::Tensor& recent, at::Tensor& recent_len, const at::Tensor& seeds,
                   at::Tensor& workspace, at::Tensor& tokens, at::Tensor& count, int64_t update, int64_t all_greedy) {
  check_bf16_cuda(logits, "logits");
  check_rows(logits, "logits");
  const int R = logits.size(0), V = logits.size(1);
  const int S = (int)row_start.numel() - 1;
  MP_CHECK(row_start.scalar_type() == at::kInt && row_start.is_cuda() && row_start.is_contiguous() && S >= 0,
           "row_start int32 [S + 1]");
  MP_CHECK(draft.scalar_type() == at::kInt && draft.is_cuda() && draft.is_contiguous() && draft.numel() == R,
           "draft int32 [R]");
  MP_CHECK(temps.scalar_type() == at::kFloat && temps.is_cuda() && temps.is_contiguous() && temps.numel() == S,
           "temps");
  MP_CHECK(top_ps.scalar_type() == at::kFloat && top_ps.is_cuda() && top_ps.is_contiguous() && top_ps.numel() == S,
           "top_ps");
  MP_CHECK(top_ks.scalar_type() == at::kInt && top_ks.is_cuda() && top_ks.is_contiguous() && top_ks.numel() == S,
           "top_ks");
  MP_CHECK(rep_pens.scalar_type() == at::kFloat && rep_pens.is_cuda() && rep_pens.is_contiguous() &&
               rep_pens.numel() == S,
           "rep_pens");
  MP_CHECK(recent.scalar_type() == at::kInt && recent.is_cuda() && recent.dim() == 2 && recent.size(0) == S &&
               recent.size(1) >= 1 && recent.is_contiguous(),
           "recent int32 [S, n]");
  MP_CHECK(recent_len.scalar_type() == at::kInt && recent_len.is_cuda() && recent_len.is_contiguous() &&
               recent_len.numel() == S,
           "recent_len");
  MP_CHECK(seeds.scalar_type() == at::kLong && seeds.is_cuda() && seeds.is_contiguous() && seeds.numel() == R,
           "seeds int64 [R]");
  MP_CHECK(workspace.scalar_type() == at::kFloat && workspace.is_cuda() && workspace.is_contiguous() &&
               workspace.numel() >= mp_sample_verify_ws_words(R, V, recent.size(1)),
           "workspace (sample_verify_ws floats)");
  MP_CHECK(tokens.scalar_type() == at::kLong && tokens.is_cuda() && tokens.is_contiguous() && tokens.numel() >= R,
           "tokens int64 [R]");
  MP_CHECK(count.scalar_type() == at::kInt && count.is_cuda() && count.is_contiguous() && count.numel() >= S,
           "count int32 [S]");
  check_launch(mp_sample_verify(logits.data_ptr(), logits.stride(0), R, S, V, row_start.data_ptr<int32_t>(),
                                draft.data_ptr<int32_t>(), temps.data_ptr<float>(), top_ps.data_ptr<float>(),
                                top_ks.data_ptr<int32_t>(), rep_pens.data_ptr<float>(), recent.data_ptr<int32_t>(),
                                recent.size(1), recent_len.data_ptr<int32_t>(), seeds.data_ptr<int64_t>(),
                                workspace.data_ptr<float>(), tokens.data_ptr<int64_t>(), count.data_ptr<int32_t>(),
                                (int)update, (int)all_greedy, cur_stream()),
               "sample_verify");
}

// The decode GEMM arguments every gemm* op shares, after its checks (the caller sets x_stride, wsc,
// as, gate where it has them)
static mp::GemmArgs gemm_args(const void* x, const void* w, void* y, int64_t y_stride, const void* res,
                              int64_t res_stride, int M, int N, int K, int64_t epilogue, int64_t flags, void* ws,
                              void* ap, const c10::optional<at::Tensor>& ss_out,
                              const c10::optional<at::Tensor>& ss_zero, const c10::optional<at::Tensor>& ss_in,
                              double inv_k, double eps) {
  mp::GemmArgs a{};
  a.x = x, a.w = w, a.y = y, a.y_stride = y_stride, a.res = res, a.res_stride = res_stride;
  a.M = M, a.N = N, a.K = K, a.epilogue = (int)epilogue, a.flags = (int)flags;
  a.ws = ws, a.ap = ap;
  a.ss_out = opt_ss(ss_out, "ss_out");
  a.ss_zero = opt_ss(ss_zero, "ss_zero");
  a.ss_in = opt_ss(ss_in, "ss_in");
  a.inv_k = (float)inv_k, a.eps = (float)eps;
  return a;
}

// flags (mp::GemmFlags): GEMM_A_PACKED: x holds ceil(M/16)*16*K elements, M given
void gemm(const at::Tensor& x, const at::Tensor& wp, at::Tensor& y, const c10::optional<at::Tensor>& residual,
          int64_t epilogue, int64_t M_, int64_t flags, const c10::optional<at::Tensor>& workspace,
          const c10::optional<at::Tensor>& gate, const c10::optional<at::Tensor>& ap,
          const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& ss_zero,
          const c10::optional<at::Tensor>& ss_in, double inv_k, double eps) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(wp, "wp");
  check_bf16_cuda(y, "y");
  MP_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8 && wp.is_contiguous(),
           "wp must be a packed weight [N/16, K/32, 64, 8] (ops.pack_weight)");
  const int N = 16 * wp.size(0), K = 32 * wp.size(1);
  const bool apk = flags & mp::GEMM_A_PACKED, opk = flags & mp::GEMM_OUT_PACKED;
  int M;
  if (apk) {
    M = (int)M_;
    MP_CHECK(x.is_contiguous() && x.numel() >= packed_numel(M, K), "packed x too small");
  } else {
    check_rows(x, "x");
    M = x.size(0);
    MP_CHECK(x.size(1) == K, "K mismatch between x and packed weight");
  }
  check_gemm_out(y, M, N, epilogue, opk);
  const auto [rp, rs] = opt_rows(residual, "residual", M, N);
  MP_CHECK(epilogue < 2 || rp != nullptr, "residual epilogue needs residual");
  MP_CHECK(epilogue >= 0 && epilogue <= 3, "epilogue");
  void* app = opt_packed(ap, M, N);
  mp::GemmArgs a = gemm_args(x.data_ptr(), wp.data_ptr(), y.data_ptr(), opk ? 0 : y.stride(0), rp, rs, M, N, K, epilogue,
                             flags, nullptr, app, ss_out, ss_zero, ss_in, inv_k, eps);
  a.x_stride = apk ? 0 : x.stride(0);
  MP_CHECK(epilogue != 3 || (app != nullptr && !opk), "epilogue 3 needs ap (and ss_out outside ablations)");
  a.ws = opt_workspace(workspace);
  if (gate.has_value()) {  // MoE expert gate: one int32 on the device (0 -> the GEMM is skipped)
    MP_CHECK(gate->is_cuda() && gate->scalar_type() == at::kInt && gate->numel() == 1, "gate must be one cuda int32");
    a.gate = gate->data_ptr<int>();
  }
  check_launch(mp_gemm_bf16(&a, cur_stream()), "gemm");
}

void pack_act(const at::Tensor& x, at::Tensor& ap) {
  check_bf16_cuda(x, "x");
  check_rows(x, "x");
  MP_CHECK(ap.is_contiguous() && ap.numel() >= packed_numel(x.size(0), x.size(1)), "ap too small");
  check_launch(mp_pack_act(x.data_ptr(), x.stride(0), ap.data_ptr(), x.size(0), x.size(1), cur_stream()), "pack_act");
}

at::Tensor pack_weight(const at::Tensor& w) {
  check_bf16_cuda(w, "w");
  MP_CHECK(w.dim() == 2 && w.is_contiguous(), "w [N, K] contiguous");
  const int N = w.size(0), K = w.size(1);
  MP_CHECK(N % 16 == 0 && K % 32 == 0, "pack_weight needs N % 16 == 0 and K % 32 == 0");
  auto wp = at::empty({N / 16, K / 32, 64, 8}, w.options());
  check_launch(mp_pack_weight(w.data_ptr(), wp.data_ptr(), N, K, cur_stream()), "pack_weight");
  return wp;
}

// W8A16 decode GEMM (gemm.hip mp_gemm_w8): packed bf16 x (M rows), fp8 weight Wq uint8
// [N/16, K/32, 64, 8] + per-column fp32 scales; flags as mp_gemm_w8
void gemm_w8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& wsc, at::Tensor& y,
             const c10::optional<at::Tensor>& residual, int64_t epilogue, int64_t M_, int64_t flags,
             const c10::optional<at::Tensor>& workspace, const c10::optional<at::Tensor>& ap,
             const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& ss_zero,
             const c10::optional<at::Tensor>& ss_in, double inv_k, double eps) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(y, "y");
  const auto [N, K] = check_w8_weight(wq, wsc);
  const int M = (int)M_;
  const bool opk = flags & mp::GEMM_OUT_PACKED;
  MP_CHECK(M >= 0 && M <= 64, "gemm_w8: 0 <= M <= 64");
  MP_CHECK(x.is_contiguous() && x.numel() >= packed_numel(M, K), "packed x too small");
  check_gemm_out(y, M, N, epilogue, opk);
  MP_CHECK(epilogue == 0 || epilogue == 3 || (epilogue == 1 && opk), "gemm_w8: epilogue 0, 3 or packed SwiGLU");
  const auto [rp, rs] = opt_rows(residual, "residual", M, N);
  void* app = opt_packed(ap, M, N);
  MP_CHECK(epilogue != 3 || (app != nullptr && rp != nullptr), "epilogue 3 needs residual and ap");
  void* ws = opt_workspace(workspace);
  mp::GemmArgs a = gemm_args(x.data_ptr(), wq.data_ptr(), y.data_ptr(), opk ? 0 : y.stride(0), rp, rs, M, N, K, epilogue,
                             flags, ws, app, ss_out, ss_zero, ss_in, inv_k, eps);
  a.wsc = wsc.data_ptr<float>();
  const int rc = mp_gemm_w8(&a, cur_stream());
  TORCH_CHECK(rc != 1, "mpamd: gemm_w8: no fp8-weight kernel covers M=", M, " N=", N, " K=", K, " epilogue=",
              epilogue);
  check_launch(rc, "gemm_w8");
}

// Stacked fp8 expert weights of the grouped MoE GEMMs (gemm_moe.hip): uint8 [E, N/16, K/32, 64, 8] +
// per-expert column scales fp32 [E, N] -> (E, N, K)
static std::tuple<int, int, int> check_moe_weight(const at::Tensor& w8, const at::Tensor& wsc) {
  MP_CHECK(w8.is_cuda() && w8.scalar_type() == at::kByte && w8.dim() == 5 && w8.size(3) == 64 && w8.size(4) == 8 &&
               w8.is_contiguous(),
           "w8 must be stacked fp8 expert weights uint8 [E, N/16, K/32, 64, 8] (ops.w8_from_fp8 per expert)");
  const int E = w8.size(0), N = 16 * w8.size(1), K = 32 * w8.size(2);
  MP_CHECK(wsc.is_cuda() && wsc.scalar_type() == at::kFloat && wsc.is_contiguous() && wsc.dim() == 2 &&
               wsc.size(0) == E && wsc.size(1) == N && wsc.device() == w8.device(),
           "wsc: fp32 [E, N] column scales");
  return {E, N, K};
}

// routed-token counts of the grouped MoE GEMMs
static void check_moe_cnt(const at::Tensor& cnt, int E, const at::Tensor& like) {
  MP_CHECK(cnt.is_cuda() && cnt.scalar_type() == at::kInt && cnt.is_contiguous() && cnt.numel() == E &&
               cnt.device() == like.device(),
           "cnt: int32 [E] routed-token counts on the weights' device");
}

// the E packed SwiGLU activations between the two grouped launches
static void check_moe_act(const at::Tensor& act, int M, int E, int F, const at::Tensor& like) {
  check_bf16_cuda(act, "act");
  MP_CHECK(act.is_contiguous() && act.numel() >= E * packed_numel(M, F) && act.device() == like.device() &&
               reinterpret_cast<uintptr_t>(act.data_ptr()) % 16 == 0,
           "act: E packed activations of packed_numel(M, F) bf16 elements each");
}

// Grouped gate/up + SwiGLU of all experts (gemm_moe.hip mp_moe_gate_up_w8): packed bf16 x (M rows)
void moe_gate_up_w8(const at::Tensor& x, const at::Tensor& w8, const at::Tensor& wsc, const at::Tensor& cnt,
                    at::Tensor& act, int64_t M_) {
  check_bf16_cuda(x, "x");
  const auto [E, N, K] = check_moe_weight(w8, wsc);
  const int M = (int)M_;
  MP_CHECK(M >= 0 && M <= 64, "moe_gate_up_w8: 0 <= M <= 64");
  MP_CHECK(N % 32 == 0, "moe_gate_up_w8: SwiGLU needs N % 32 == 0");
  MP_CHECK(x.is_contiguous() && x.numel() >= packed_numel(M, K) && x.device() == w8.device(), "packed x too small");
  check_moe_cnt(cnt, E, w8);
  check_moe_act(act, M, E, N / 2, w8);
  const int rc = mp_moe_gate_up_w8(x.data_ptr(), w8.data_ptr(), wsc.data_ptr<float>(), cnt.data_ptr<int32_t>(),
                                   act.data_ptr(), M, E, K, N / 2, cur_stream());
  TORCH_CHECK(rc != 1, "mpamd: moe_gate_up_w8: no grouped kernel covers M=", M, " E=", E, " H=", K, " F=", N / 2);
  check_launch(rc, "moe_gate_up_w8");
}

// Grouped down + combine (gemm_moe.hip mp_moe_down_w8): y bf16 [M, H] = sum_e wd[:, e] * (act[e] . down[e]^T)
void moe_down_w8(const at::Tensor& act, const at::Tensor& w8, const at::Tensor& wsc, const at::Tensor& cnt,
                 const at::Tensor& wd, at::Tensor& y, int64_t M_) {
  const auto [E, N, K] = check_moe_weight(w8, wsc);
  const int M = (int)M_;
  MP_CHECK(M >= 0 && M <= 64, "moe_down_w8: 0 <= M <= 64");
  check_moe_cnt(cnt, E, w8);
  check_moe_act(act, M, E, K, w8);
  MP_CHECK(wd.is_cuda() && wd.scalar_type() == at::kFloat && wd.is_contiguous() && wd.dim() == 2 && wd.size(0) == M &&
               wd.size(1) == E && wd.device() == w8.device(),
           "wd: fp32 [M, E] dense routing weights");
  check_bf16_cuda(y, "y");
  check_rows(y, "y");
  MP_CHECK(y.size(0) == M && y.size(1) == N && y.device() == w8.device(), "y shape");
  const int rc = mp_moe_down_w8(act.data_ptr(), w8.data_ptr(), wsc.data_ptr<float>(), cnt.data_ptr<int32_t>(),
                                wd.data_ptr<float>(), y.data_ptr(), y.stride(0), M, E, N, K, cur_stream());
  TORCH_CHECK(rc != 1, "mpamd: moe_down_w8: no grouped kernel covers M=", M, " E=", E, " H=", N, " F=", K);
  check_launch(rc, "moe_down_w8");
}

bool moe_w8_ok(int64_t M, int64_t E, int64_t H, int64_t F) {
  return mp_moe_w8_ok((int)M, (int)E, (int)H, (int)F) != 0;
}

// Batched LoRA (lora.hip): the stacked adapter matrices, the row slots and the fp32 intermediate
static mp::LoraArgs lora_args(const at::Tensor& mats, const char* name, const at::Tensor& slots, const at::Tensor& t,
                              int64_t M_) {
  MP_CHECK(M_ >= 0 && M_ <= (1 << 20), "lora: M out of range");
  const int M = (int)M_;
  check_bf16_cuda(mats, name);
  MP_CHECK(mats.dim() == 3 && mats.size(0) >= 1 && mats.stride(2) == 1 && mats.stride(1) == mats.size(2) &&
               mats.stride(0) >= mats.size(1) * mats.size(2) && mats.stride(0) % 8 == 0 &&
               reinterpret_cast<uintptr_t>(mats.data_ptr()) % 16 == 0,
           std::string(name) + ": bf16 [S, rows, cols] stack, rows contiguous, 16-B aligned");
  MP_CHECK(slots.is_cuda() && slots.scalar_type() == at::kInt && slots.is_contiguous() && slots.numel() >= M &&
               slots.device() == mats.device(),
           "slots: int32 [M] on the adapters' device");
  mp::LoraArgs a{};
  a.M = M, a.S = (int)mats.size(0);
  a.slots = slots.data_ptr<int32_t>();
  MP_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.dim() == 2 && t.size(0) >= M &&
               t.device() == mats.device() && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
           "t: fp32 [M, R] contiguous on the adapters' device");
  a.R = (int)t.size(1);
  a.t = t.data_ptr<float>();
  return a;
}

// t[m] = scale[s] * (A[s] x[m]), s = slots[m] >= 0 (lora.hip mp_lora_shrink): packed bf16 x (M rows)
void lora_shrink(const at::Tensor& x, const at::Tensor& A, const at::Tensor& scale, const at::Tensor& slots,
                 at::Tensor& t, int64_t M) {
  mp::LoraArgs a = lora_args(A, "A", slots, t, M);
  MP_CHECK(A.size(1) == a.R, "A: [S, R, K] with R = t.size(1)");
  a.K = (int)A.size(2);
  a.A = A.data_ptr(), a.a_stride = A.stride(0);
  check_bf16_cuda(x, "x");
  MP_CHECK(x.is_contiguous() && x.numel() >= packed_numel(a.M, a.K) && x.device() == A.device() &&
               reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
           "packed x too small");
  MP_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat && scale.is_contiguous() && scale.numel() == a.S &&
               scale.device() == A.device(),
           "scale: fp32 [S]");
  a.x = x.data_ptr(), a.scale = scale.data_ptr<float>();
  const int rc = mp_lora_shrink(&a, cur_stream());
  TORCH_CHECK(rc != 1, "mpamd: lora_shrink: no kernel covers M=", a.M, " K=", a.K, " R=", a.R);
  check_launch(rc, "lora_shrink");
}

// y[m] = bf16(y[m] + B[s] t[m]) in place, s = slots[m] >= 0 (lora.hip mp_lora_expand)
void lora_expand(const at::Tensor& t, const at::Tensor& B, const at::Tensor& slots, at::Tensor& y) {
  check_bf16_cuda(y, "y");
  check_rows(y, "y");
  mp::LoraArgs a = lora_args(B, "B", slots, t, y.size(0));
  MP_CHECK(B.size(2) == a.R, "B: [S, N, R] with R = t.size(1)");
  MP_CHECK(y.size(1) == B.size(1) && y.device() == B.device(), "y: [M, N] with N = B.size(1)");
  a.N = (int)B.size(1);
  a.B = B.data_ptr(), a.b_stride = B.stride(0);
  a.y = y.data_ptr(), a.y_stride = y.stride(0);
  const int rc = mp_lora_expand(&a, cur_stream());
  TORCH_CHECK(rc != 1, "mpamd: lora_expand: no kernel covers M=", a.M, " N=", a.N, " R=", a.R);
  check_launch(rc, "lora_expand");
}

bool lora_ok(int64_t M, int64_t N, int64_t K, int64_t R) { return mp_lora_ok((int)M, (int)N, (int)K, (int)R) != 0; }

// MXFP4 weight operands (gemm_w4.hip): codes uint8 [N/16, K/128, 64, 16] + e8m0 scales uint8 [N/16, K/128, 16, 4]
static void check_w4(const at::Tensor& w4, const at::Tensor& s4) {
  MP_CHECK(w4.is_cuda() && w4.scalar_type() == at::kByte && w4.dim() == 4 && w4.size(2) == 64 && w4.size(3) == 16 &&
               w4.is_contiguous(),
           "w4 must be an MXFP4 weight uint8 [N/16, K/128, 64, 16] (ops.pack_weight_w4)");
  MP_CHECK(s4.is_cuda() && s4.scalar_type() == at::kByte && s4.dim() == 4 && s4.size(0) == w4.size(0) &&
               s4.size(1) == w4.size(1) && s4.size(2) == 16 && s4.size(3) == 4 && s4.is_contiguous() &&
               s4.device() == w4.device(),
           "s4 must be the e8m0 block scales uint8 [N/16, K/128, 16, 4] (ops.pack_weight_w4)");
}

// W4A16 decode GEMM (gemm_w4.hip mp_gemm_w4): packed bf16 x (M rows), MXFP4 weight; flags:
// GEMM_OUT_PACKED = packed SwiGLU output
void gemm_w4(const at::Tensor& x, const at::Tensor& w4, const at::Tensor& s4, at::Tensor& y,
             const c10::optional<at::Tensor>& residual, int64_t epilogue, int64_t M_, int64_t flags,
             const c10::optional<at::Tensor>& ap, const c10::optional<at::Tensor>& ss_out,
             const c10::optional<at::Tensor>& ss_zero, const c10::optional<at::Tensor>& ss_in, double inv_k,
             double eps) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(y, "y");
  check_w4(w4, s4);
  const int N = 16 * w4.size(0), K = 128 * w4.size(1);
  const int M = (int)M_;
  const bool opk = flags & mp::GEMM_OUT_PACKED;
  MP_CHECK(M >= 0 && M <= 64, "gemm_w4: 0 <= M <= 64");
  MP_CHECK(x.is_contiguous() && x.numel() >= packed_numel(M, K), "packed x too small");
  MP_CHECK(epilogue == 0 || epilogue == 3 || (epilogue == 1 && opk), "gemm_w4: epilogue 0, 3 or packed SwiGLU");
  MP_CHECK(epilogue != 1 || N % 32 == 0, "gemm_w4: SwiGLU needs N % 32 == 0");
  check_gemm_out(y, M, N, epilogue, opk);
  const auto [rp, rs] = opt_rows(residual, "residual", M, N);
  void* app = opt_packed(ap, M, N);
  MP_CHECK(epilogue != 3 || (app != nullptr && rp != nullptr), "epilogue 3 needs residual and ap");
  mp::GemmArgs a = gemm_args(x.data_ptr(), w4.data_ptr(), y.data_ptr(), opk ? 0 : y.stride(0), rp, rs, M, N, K, epilogue,
                             flags, nullptr, app, ss_out, ss_zero, ss_in, inv_k, eps);
  a.wsc = s4.data_ptr();
  const int rc = mp_gemm_w4(&a, cur_stream());
  TORCH_CHECK(rc != 1, "mpamd: gemm_w4: no MXFP4-weight kernel covers M=", M, " N=", N, " K=", K, " epilogue=",
              epilogue);
  check_launch(rc, "gemm_w4");
}

bool gemm_w4_ok(int64_t M, int64_t N, int64_t K, int64_t epilogue) {
  return mp_gemm_w4_ok((int)M, (int)N, (int)K, (int)epilogue) != 0;
}

// MXFP4 weight -> row-major bf16 [N, K]
at::Tensor dequant_w4(const at::Tensor& w4, const at::Tensor& s4) {
  check_w4(w4, s4);
  const int N = 16 * w4.size(0), K = 128 * w4.size(1);
  auto w = at::empty({N, K}, w4.options().dtype(at::kBFloat16));
  check_launch(mp_dequant_w4(w4.data_ptr(), s4.data_ptr(), w.data_ptr(), N, K, cur_stream()), "dequant_w4");
  return w;
}

int64_t gemm_workspace_bytes() { return mp_gemm_workspace_bytes(); }
int64_t gemm_slab_offset() { return mp_gemm_slab_offset(); }
int64_t gemm_rwk_split(int64_t M, int64_t N, int64_t K, int64_t f8) {
  return mp_gemm_rwk_split((int)M, (int)N, (int)K, (int)f8);
}
void fp8_gemm_kernel(int64_t kind) { mp_fp8_set_kernel((int)kind); }
bool gemm_t2d_ok(int64_t M, int64_t N, int64_t K, int64_t epilogue, int64_t out_packed) {
  return mp_gemm_t2d_ok((int)M, (int)N, (int)K, (int)epilogue, (int)out_packed, 1) != 0;
}

bool gemm_rw_ok(int64_t M, int64_t N, int64_t K, int64_t epilogue, int64_t out_packed) {
  return mp_gemm_rw_ok((int)M, (int)N, (int)K, (int)epilogue, (int)out_packed) != 0;
}

// packed bf16 decode activation (M rows) -> fp8 A8 [K/64][MT][64][16] (uint8) + row scales (fp32, >= MT*16)
void quant_act_fp8(const at::Tensor& ap, at::Tensor& a8, at::Tensor& scale, int64_t M, int64_t K) {
  check_bf16_cuda(ap, "ap");
  MP_CHECK(ap.is_contiguous() && ap.numel() >= packed_numel(M, K), "packed activation too small");
  MP_CHECK(a8.is_cuda() && a8.scalar_type() == at::kByte && a8.is_contiguous() && a8.numel() >= packed_numel(M, K),
           "a8: uint8 [packed_numel(M, K)]");
  const int64_t rows = ((M + 15) / 16) * 16;
  MP_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat && scale.numel() >= rows * 33,
           "scale: fp32 [ceil(M/16)*16 * 33] (row scales + per-slice absmax scratch)");
  MP_CHECK(K % 64 == 0, "K % 64");
  check_launch(mp_quant_act_fp8(ap.data_ptr(), a8.data_ptr(), scale.data_ptr<float>(), scale.data_ptr<float>() + rows,
                                (int)M, (int)K, cur_stream()),
               "quant_act_fp8");
}

// packed bf16 activation (M rows, K) -> MX e4m3 bytes ax [K/128 * MT * 2 * 64 * 16] + e8m0 block
// scales as [K/128 * 64 * 4] (gemm_mx.hip)
void quant_mx(const at::Tensor& ap, at::Tensor& ax, at::Tensor& as, int64_t M, int64_t K) {
  check_bf16_cuda(ap, "ap");
  MP_CHECK(M >= 1 && M <= 64 && K % 128 == 0, "quant_mx: 1 <= M <= 64, K % 128 == 0");
  MP_CHECK(ap.is_contiguous() && ap.numel() >= packed_numel(M, K), "packed activation too small");
  const int64_t rows = ((M + 15) / 16) * 16;
  MP_CHECK(ax.is_cuda() && ax.scalar_type() == at::kByte && ax.is_contiguous() && ax.numel() >= rows * K,
           "ax: uint8 [ceil(M/16)*16*K]");
  MP_CHECK(as.is_cuda() && as.scalar_type() == at::kByte && as.is_contiguous() && as.numel() >= 2 * K,
           "as: uint8 [K/128 * 64 * 4]");
  check_launch(mp_quant_mx(ap.data_ptr(), ax.data_ptr(), as.data_ptr(), (int)M, (int)K, cur_stream()), "quant_mx");
}

// W8A8-MX decode GEMM (gemm_mx.hip): ax / as from quant_mx, fp8 weight in the W8A16 layout + column
// scales; epilogue 0 (optional ss_in row scale) or 3; flags: GEMM_ROT_K, GEMM_PARTIALS (y unused,
// the slabs stay in the workspace)
void gemm_mx(const at::Tensor& ax, const at::Tensor& as, const at::Tensor& wq, const at::Tensor& wsc, at::Tensor& y,
             const c10::optional<at::Tensor>& residual, int64_t epilogue, int64_t M_, int64_t flags,
             const at::Tensor& workspace, const c10::optional<at::Tensor>& ap,
             const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& ss_zero,
             const c10::optional<at::Tensor>& ss_in, double inv_k, double eps) {
  const auto [N, K] = check_w8_weight(wq, wsc);
  const int M = (int)M_;
  MP_CHECK(M >= 1 && M <= 64 && K % 128 == 0, "gemm_mx: 1 <= M <= 64, K % 128 == 0");
  const int64_t rows = ((M + 15) / 16) * 16;
  MP_CHECK(ax.is_cuda() && ax.scalar_type() == at::kByte && ax.is_contiguous() && ax.numel() >= rows * K, "ax size");
  MP_CHECK(as.is_cuda() && as.scalar_type() == at::kByte && as.is_contiguous() && as.numel() >= 2 * K, "as size");
  MP_CHECK(epilogue == 0 || epilogue == 3, "gemm_mx: epilogue 0 or 3");
  const bool partial = flags & mp::GEMM_PARTIALS;
  if (!partial) {
    check_bf16_cuda(y, "y");
    check_gemm_out(y, M, N, epilogue, false);
  }
  const auto [rp, rs] = opt_rows(residual, "residual", M, N);
  void* app = opt_packed(ap, M, N);
  MP_CHECK(epilogue != 3 || (app != nullptr && rp != nullptr), "epilogue 3 needs residual and ap");
  void* ws = opt_workspace(workspace);
  mp::GemmArgs a = gemm_args(ax.data_ptr(), wq.data_ptr(), partial ? nullptr : y.data_ptr(), partial ? 0 : y.stride(0),
                             rp, rs, M, N, K, epilogue, flags, ws, app, ss_out, ss_zero, ss_in, inv_k, eps);
  a.wsc = wsc.data_ptr<float>();
  a.as = as.data_ptr();
  const int rc = mp_gemm_mx(&a, cur_stream());
  TORCH_CHECK(rc != 1, "mpamd: gemm_mx: no split-K geometry for M=", M, " N=", N, " K=", K);
  check_launch(rc, "gemm_mx");
}

// row-major bf16 x[M, K] -> fp8 A8 (the fp8 GEMM's A layout) + per-row scales
void quant_rows_fp8(const at::Tensor& x, at::Tensor& a8, at::Tensor& scale) {
  check_bf16_cuda(x, "x");
  MP_CHECK(x.dim() == 2 && x.stride(1) == 1, "x: [M, K] with unit column stride");
  const int64_t M = x.size(0), K = x.size(1);
  MP_CHECK(a8.is_cuda() && a8.scalar_type() == at::kByte && a8.is_contiguous() && a8.numel() >= packed_numel(M, K),
           "a8: uint8 [packed_numel(M, K)]");
  MP_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat && scale.numel() >= M, "scale: fp32 [>= M]");
  MP_CHECK(K % 64 == 0 && K <= 65536, "K % 64 == 0 and K <= 65536");
  check_launch(mp_quant_rows_fp8(x.data_ptr(), x.stride(0), a8.data_ptr(), scale.data_ptr<float>(), (int)M, (int)K,
                                 cur_stream()),
               "quant_rows_fp8");
}

// y = epilogue((a8 * as) . (wq * ws)^T); wq: [N/16, K/64, 64, 16] uint8 (ops.pack_weight_fp8)
void gemm_fp8(const at::Tensor& a8, const at::Tensor& as, const at::Tensor& wq, const at::Tensor& ws, at::Tensor& y,
              const c10::optional<at::Tensor>& residual, int64_t epilogue, int64_t M, int64_t out_packed,
              int64_t kind, const c10::optional<at::Tensor>& workspace) {
  MP_CHECK(wq.is_cuda() && wq.scalar_type() == at::kByte && wq.dim() == 4 && wq.size(2) == 64 && wq.size(3) == 16 &&
               wq.is_contiguous(),
           "wq must be a packed fp8 weight [N/16, K/64, 64, 16]");
  const int N = 16 * wq.size(0), K = 64 * wq.size(1);
  MP_CHECK(a8.is_cuda() && a8.scalar_type() == at::kByte && a8.numel() >= packed_numel(M, K), "a8");
  MP_CHECK(as.is_cuda() && as.scalar_type() == at::kFloat && as.numel() >= M, "as");
  MP_CHECK(ws.is_cuda() && ws.scalar_type() == at::kFloat && ws.numel() == N, "ws: fp32 [N]");
  check_bf16_cuda(y, "y");
  check_gemm_out(y, M, N, epilogue, out_packed);
  const void* rp = nullptr;
  int64_t rs = 0;
  if (residual.has_value()) {
    check_bf16_cuda(*residual, "residual");
    check_rows(*residual, "residual");
    rp = residual->data_ptr();
    rs = residual->stride(0);
  }
  MP_CHECK(epilogue != 2 || rp != nullptr, "residual epilogue needs residual");
  float* part = nullptr;
  int64_t part_bytes = 0;
  if (workspace.has_value()) {  // the GEMM workspace (ops.gemm_workspace): its split-K slab region
    MP_CHECK(workspace->is_cuda() && workspace->is_contiguous() &&
                 workspace->numel() * workspace->element_size() >= mp_gemm_workspace_bytes(),
             "workspace: ops.gemm_workspace");
    part = (float*)((char*)workspace->data_ptr() + mp_gemm_slab_offset());
    part_bytes = mp_gemm_slab_bytes();
  }
  check_launch(mp_gemm_fp8(a8.data_ptr(), as.data_ptr<float>(), wq.data_ptr(), ws.data_ptr<float>(), y.data_ptr(),
                           out_packed ? 0 : y.stride(0), rp, rs, (int)M, N, K, (int)epilogue, (int)out_packed,
                           (int)kind, part, part_bytes, cur_stream()),
               "gemm_fp8");
}

}  // namespace

TORCH_LIBRARY(mpamd, m) {
  m.def("gemm_workspace_bytes() -> int", &gemm_workspace_bytes);
  m.def("gemm_slab_offset() -> int", &gemm_slab_offset);
  m.def("gemm_rwk_split(int M, int N, int K, int f8) -> int", &gemm_rwk_split);
  m.def("fp8_gemm_kernel(int kind) -> ()", &fp8_gemm_kernel);
  m.def("gemm_rw_ok(int M, int N, int K, int epilogue, int out_packed) -> bool", &gemm_rw_ok);
  m.def("gemm_t2d_ok(int M, int N, int K, int epilogue, int out_packed) -> bool", &gemm_t2d_ok);
  m.def(
      "rmsnorm(Tensor x, Tensor(a!) residual, Tensor w, Tensor(b!) y, float eps, int mode, Tensor? rows, "
      "int packed, Tensor(c!)? ss=None, Tensor(d!)? a8=None, Tensor(e!)? a8_scale=None, Tensor? gather=None) -> ()");
  // the KV-write and attention ops end in k_scale / v_scale: both given on an fp8 KV cache (k_cache / v_cache
  // then hold its uint8 codes), neither on a bf16 cache
  m.def(
      "rope_kv_write(Tensor(a!) qkv, Tensor positions, Tensor cos, Tensor sin, Tensor(b!) k_cache, "
      "Tensor(c!) v_cache, Tensor slots, int nh, int nkv, Tensor(d!)? k_scale=None, Tensor(e!)? v_scale=None) -> ()");
  m.def("kv_write(Tensor k, Tensor v, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor slots) -> ()");
  m.def(
      "paged_attention(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor q_seq, Tensor q_ctx, "
      "Tensor(a!) out, Tensor(b!) workspace, int nh, int nkv, float scale, int part_size, int num_parts, "
      "int packed, Tensor(c!)? counters=None, int window=0, Tensor? k_scale=None, Tensor? v_scale=None) -> ()");
  m.def(
      "paged_attention_rope(Tensor qkv, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor block_tables, Tensor q_seq, "
      "Tensor q_ctx, Tensor positions, Tensor cos, Tensor sin, Tensor slots, Tensor(c!) out, Tensor(d!) workspace, "
      "int nh, int nkv, float scale, int part_size, int num_parts, int packed, Tensor(e!)? counters=None, "
      "Tensor? qkv_part=None, int part_splits=0, Tensor? part_ss=None, float inv_k=0., float eps=0., int window=0, "
      "Tensor(f!)? k_scale=None, Tensor(g!)? v_scale=None) -> ()");
  m.def(
      "attention_mfma(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor q_seq, Tensor q_ctx, "
      "Tensor qblocks, Tensor(a!) out, Tensor(b!) workspace, int nh, int nkv, float scale, int part_size, "
      "int num_parts, int packed, Tensor? superblocks=None, int window=0, Tensor? k_scale=None, "
      "Tensor? v_scale=None) -> ()");
  m.def(
      "attention_fa(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor q_seq, Tensor q_ctx, "
      "Tensor fablocks, Tensor(a!) out, Tensor(b!) workspace, int nh, int nkv, float scale, int part_size, "
      "int num_parts, int waves, int pair=0, int window=0, Tensor? k_scale=None, Tensor? v_scale=None) -> ()");
  m.def(
      "attention_fa_window(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor q_seq, Tensor q_ctx, "
      "Tensor fablocks, Tensor(a!) out, Tensor(b!) workspace, int nh, int nkv, float scale, int part_size, "
      "int num_parts, int waves, int pair, int window, Tensor? k_scale=None, Tensor? v_scale=None) -> ()");
  m.def(
      "attention_mfma_rope(Tensor qkv, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor block_tables, Tensor q_seq, "
      "Tensor q_ctx, Tensor qblocks, Tensor positions, Tensor cos, Tensor sin, Tensor slots, Tensor(c!) out, "
      "Tensor(d!) workspace, int nh, int nkv, float scale, int part_size, int num_parts, int packed, "
      "Tensor? qkv_part=None, int part_splits=0, Tensor? part_ss=None, float inv_k=0., float eps=0., "
      "Tensor(e!)? mx_ax=None, Tensor(f!)? mx_as=None, int window=0, Tensor(g!)? k_scale=None, "
      "Tensor(h!)? v_scale=None) -> ()");
  m.def("embedding(Tensor ids, Tensor table, Tensor(a!) out) -> ()");
  m.def("swiglu(Tensor gu, Tensor(a!) out) -> ()");
  m.def("add(Tensor a, Tensor b, Tensor(a!) y) -> ()");
  m.def("argmax(Tensor logits, Tensor(a!) out) -> ()");
  m.def(
      "sample(Tensor logits, Tensor temps, Tensor top_ps, Tensor top_ks, Tensor rep_pens, Tensor(c!) recent, "
      "Tensor(d!) recent_len, Tensor seeds, Tensor(a!) workspace, Tensor(b!) out, int update=0) -> ()");
  m.def("sample_verify_ws(int R, int V, int cap) -> int", &sample_verify_ws);
  m.def(
      "sample_verify(Tensor logits, Tensor row_start, Tensor draft, Tensor temps, Tensor top_ps, Tensor top_ks, "
      "Tensor rep_pens, Tensor(c!) recent, Tensor(d!) recent_len, Tensor seeds, Tensor(a!) workspace, "
      "Tensor(b!) tokens, Tensor(e!) count, int update=0, int all_greedy=0) -> ()");
  m.def(
      "gemm(Tensor x, Tensor wp, Tensor(a!) y, Tensor? residual, int epilogue, int M, int flags, "
      "Tensor(b!)? workspace=None, Tensor? gate=None, Tensor(c!)? ap=None, Tensor(d!)? ss_out=None, "
      "Tensor(e!)? ss_zero=None, Tensor? ss_in=None, float inv_k=0., float eps=0.) -> ()");
  m.def(
      "gemm_w8(Tensor x, Tensor wq, Tensor wsc, Tensor(a!) y, Tensor? residual, int epilogue, int M, int flags, "
      "Tensor(b!)? workspace=None, Tensor(c!)? ap=None, Tensor(d!)? ss_out=None, Tensor(e!)? ss_zero=None, "
      "Tensor? ss_in=None, float inv_k=0., float eps=0.) -> ()");
  m.def(
      "gemm_w4(Tensor x, Tensor w4, Tensor s4, Tensor(a!) y, Tensor? residual, int epilogue, int M, int flags, "
      "Tensor(c!)? ap=None, Tensor(d!)? ss_out=None, Tensor(e!)? ss_zero=None, Tensor? ss_in=None, float inv_k=0., "
      "float eps=0.) -> ()");
  m.def("gemm_w4_ok(int M, int N, int K, int epilogue) -> bool", &gemm_w4_ok);
  m.def("dequant_w4(Tensor w4, Tensor s4) -> Tensor");
  m.def("moe_gate_up_w8(Tensor x, Tensor w8, Tensor wsc, Tensor cnt, Tensor(a!) act, int M) -> ()");
  m.def("moe_down_w8(Tensor act, Tensor w8, Tensor wsc, Tensor cnt, Tensor wd, Tensor(a!) y, int M) -> ()");
  m.def("moe_w8_ok(int M, int E, int H, int F) -> bool", &moe_w8_ok);
  m.def("lora_shrink(Tensor x, Tensor A, Tensor scale, Tensor slots, Tensor(a!) t, int M) -> ()");
  m.def("lora_expand(Tensor t, Tensor B, Tensor slots, Tensor(a!) y) -> ()");
  m.def("lora_ok(int M, int N, int K, int R) -> bool", &lora_ok);
  m.def("pack_act(Tensor x, Tensor(a!) ap) -> ()");
  m.def("pack_weight(Tensor w) -> Tensor");
  m.def("quant_act_fp8(Tensor ap, Tensor(a!) a8, Tensor(b!) scale, int M, int K) -> ()");
  m.def("quant_rows_fp8(Tensor x, Tensor(a!) a8, Tensor(b!) scale) -> ()");
  m.def("quant_mx(Tensor ap, Tensor(a!) ax, Tensor(b!) as_, int M, int K) -> ()");
  m.def(
      "gemm_mx(Tensor ax, Tensor as_, Tensor wq, Tensor wsc, Tensor(a!) y, Tensor? residual, int epilogue, int M, "
      "int flags, Tensor(b!) workspace, Tensor(c!)? ap=None, Tensor(d!)? ss_out=None, Tensor(e!)? ss_zero=None, "
      "Tensor? ss_in=None, float inv_k=0., float eps=0.) -> ()");
  m.def(
      "gemm_fp8(Tensor a8, Tensor a_scale, Tensor wq, Tensor w_scale, Tensor(a!) y, Tensor? residual, int epilogue, "
      "int M, int out_packed, int kind=-1, Tensor(b!)? workspace=None) -> ()");
}

TORCH_LIBRARY_IMPL(mpamd, CUDA, m) {
  m.impl("rmsnorm", &rmsnorm);
  m.impl("rope_kv_write", &rope_kv_write);
  m.impl("kv_write", &kv_write);
  m.impl("paged_attention", &paged_attention);
  m.impl("paged_attention_rope", &paged_attention_rope);
  m.impl("attention_mfma", &attention_mfma);
  m.impl("attention_fa", &attention_fa);
  m.impl("attention_fa_window", &attention_fa_window);
  m.impl("attention_mfma_rope", &attention_mfma_rope);
  m.impl("embedding", &embedding);
  m.impl("swiglu", &swiglu);
  m.impl("add", &add);
  m.impl("argmax", &argmax);
  m.impl("sample", &sample);
  m.impl("sample_verify", &sample_verify);
  m.impl("gemm", &gemm);
  m.impl("gemm_w8", &gemm_w8);
  m.impl("gemm_w4", &gemm_w4);
  m.impl("dequant_w4", &dequant_w4);
  m.impl("moe_gate_up_w8", &moe_gate_up_w8);
  m.impl("moe_down_w8", &moe_down_w8);
  m.impl("lora_shrink", &lora_shrink);
  m.impl("lora_expand", &lora_expand);
  m.impl("pack_weight", &pack_weight);
  m.impl("pack_act", &pack_act);
  m.impl("quant_act_fp8", &quant_act_fp8);
  m.impl("quant_rows_fp8", &quant_rows_fp8);
  m.impl("quant_mx", &quant_mx);
  m.impl("gemm_mx", &gemm_mx);
  m.impl("gemm_fp8", &gemm_fp8);
}
