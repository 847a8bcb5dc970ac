"""Plain-PyTorch reference implementations of every HIP op.

Two uses:
* the CPU data path (tests, the GPT-2 plumbing config, any host without a GPU);
* numerics oracles for the GPU kernel tests (computed in fp32 from the same inputs).

Rounding points mirror the kernels (and HF): values are rounded to the activation
dtype where the HF LLaMA modules round them (reference petals/llama/block.py).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

GU_BLOCK = 16  # gate/up weights are interleaved in blocks of 16 rows: [g16 u16 g16 u16 ...]


def pack_act(x, out=None):
    """Row-major [M, K] -> flat packed decode activation Ap[K/32][ceil(M/16)][64][8] (see csrc/common.h)."""
    M, K = x.shape
    MT = (M + 15) // 16
    xp = torch.zeros(MT * 16, K, dtype=x.dtype, device=x.device)
    xp[:M] = x
    # [MT, 16(c), K/32, 4(q), 8(j)] -> [K/32, MT, 4(q), 16(c), 8(j)]
    y = xp.view(MT, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(-1)
    if out is not None:
        out[: y.numel()].copy_(y)
        return out
    return y


def unpack_act(ap, M, K):
    MT = (M + 15) // 16
    x = ap[: MT * 16 * K].view(K // 32, MT, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(MT * 16, K)
    return x[:M]


SS_SHARDS, SS_ROWS, SS_FX = 32, 256, float(1 << 20)


def fx_sumsq(x):
    """Per-row sum of round(x^2 * 2^20) as exact int64 (gemm.hip fused-norm row statistics)."""
    return torch.round(x.float().pow(2).double() * SS_FX).to(torch.int64).sum(-1)


def rmsnorm(x, w, eps, out=None, residual=None, mode=0, rows=None, ss=None):
    dt = x.dtype
    if mode == 3:  # fused-norm stage entry: residual = x, y = raw x, ss = fixed-point sum(x^2) per row
        residual.copy_(x)
        ss.view(SS_SHARDS, SS_ROWS).zero_()
        ss.view(SS_SHARDS, SS_ROWS)[0, : x.shape[0]] = fx_sumsq(x)
        if out is not None:
            out[: x.shape[0]].copy_(x)
            return out
        return x.clone()
    if mode == 1:
        residual.copy_((residual.float() + x.float()).to(dt))
        src = residual
    elif mode == 2:
        residual.copy_(x)
        src = x
    else:
        src = x
    if rows is not None:
        src = src.index_select(0, rows.long())
    xf = src.float()
    n = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(dt)
    y = (n.float() * w.float()).to(dt)
    if out is not None:
        out[: y.shape[0]].copy_(y)
        return out
    return y


def rope_cos_sin(head_dim: int, max_pos: int, theta: float, device=None, scaling: Optional[dict] = None):
    """fp32 cos/sin tables [max_pos, head_dim/2] (HF LlamaRotaryEmbedding, incl. llama3 scaling)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling.get("factor", 8.0)
        lo, hi = scaling.get("low_freq_factor", 1.0), scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        smooth = (old / wl - lo) / (hi - lo)
        mid = (1 - smooth) * scaled / factor + smooth * scaled
        is_mid = (wl <= lo_wl) & (wl >= hi_wl)
        inv = torch.where(is_mid, mid, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def _rotate(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half].float(), x[..., half:].float()
    c, s = cos.unsqueeze(-2), sin.unsqueeze(-2)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def _scatter_cache(cache, slots, rows):
    """rows [T, nkv, D] -> cache[page, :, off, :] for slots >= 0."""
    P, nkv, ps, D = cache.shape
    valid = slots >= 0
    if not bool(valid.any()):
        return
    s = slots[valid]
    page, off = s // ps, s % ps
    cache[page, :, off, :] = rows[valid].to(cache.dtype)


def rope_kv_write(qkv, positions, cos, sin, k_cache, v_cache, slots, nh, nkv):
    T = qkv.shape[0]
    D = k_cache.shape[-1]
    view = qkv[:, : (nh + 2 * nkv) * D].view(T, nh + 2 * nkv, D)
    c, s = cos[positions.long()], sin[positions.long()]
    q = _rotate(view[:, :nh], c, s).to(qkv.dtype)
    k = _rotate(view[:, nh : nh + nkv], c, s).to(qkv.dtype)
    v = view[:, nh + nkv :]
    view[:, :nh] = q
    _scatter_cache(k_cache, slots, k)
    _scatter_cache(v_cache, slots, v)


def kv_write(k, v, k_cache, v_cache, slots):
    nkv, D = k_cache.shape[1], k_cache.shape[3]
    _scatter_cache(k_cache, slots, k.reshape(k.shape[0], nkv, D))
    _scatter_cache(v_cache, slots, v.reshape(v.shape[0], nkv, D))


def paged_attention(q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out=None, window=0):
    """softmax(q k^T * scale) v over the first q_ctx[t] cached tokens of sequence q_seq[t]; with a
    sliding ``window`` W > 0 over the last W of them only, cache positions ``[max(0, ctx - W), ctx)``
    (pages wholly below them are not looked up, so their block-table entries may be released)."""
    window = int(window or 0)
    if window < 0:
        raise ValueError(f"window must be >= 0 (0: no sliding window), got {window}")
    T = q.shape[0]
    D = k_cache.shape[-1]
    ps = k_cache.shape[2]
    rep = nh // nkv
    res = torch.zeros(T, nh, D, dtype=torch.float32, device=q.device)
    qv = q[:, : nh * D].reshape(T, nh, D).float()
    for t in range(T):
        n = int(q_ctx[t])
        if n <= 0:
            continue
        lo = max(0, n - window) if window else 0
        p0 = lo // ps  # first page the window reaches into
        pages = block_tables[int(q_seq[t])][p0: (n + ps - 1) // ps].long()
        k = k_cache[pages].permute(1, 0, 2, 3).reshape(nkv, -1, D)[:, lo - p0 * ps: n - p0 * ps].float()
        v = v_cache[pages].permute(1, 0, 2, 3).reshape(nkv, -1, D)[:, lo - p0 * ps: n - p0 * ps].float()
        k = k.repeat_interleave(rep, 0)
        v = v.repeat_interleave(rep, 0)
        s = torch.einsum("hd,hnd->hn", qv[t], k) * scale
        p = torch.softmax(s, -1)
        res[t] = torch.einsum("hn,hnd->hd", p, v)
    y = res.reshape(T, nh * D).to(q.dtype)
    if out is not None:
        out.view(T, nh * D).copy_(y)
        return out
    return y


# ---------------------------------------------------------------------------------------
# fp8 KV cache (csrc/kv_f8.h): per layer K and V are e4m3 codes uint8 [pages, nkv, page, D] plus one
# e8m0 scale byte per (token, kv head) uint8 [pages, nkv, page] - (D + 1) bytes per token-head.
class KVF8:
    """One fp8 K or V cache of a layer: ``codes`` + ``scales``.  The attention / KV-write ops take
    it where they take a bf16 cache tensor."""

    __slots__ = ("codes", "scales")

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor):
        if codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise TypeError("KVF8: codes and scales are uint8 tensors")
        if codes.dim() != 4 or tuple(scales.shape) != tuple(codes.shape[:3]):
            raise ValueError(f"KVF8: codes [pages, nkv, page, D] and scales [pages, nkv, page], got "
                             f"{tuple(codes.shape)} / {tuple(scales.shape)}")
        self.codes, self.scales = codes, scales

    @property
    def shape(self):
        return self.codes.shape

    @property
    def device(self):
        return self.codes.device

    dtype = torch.uint8

    @classmethod
    def empty(cls, num_pages, nkv, page_size, head_dim, device="cpu"):
        """Zero codes, unit scales (e = 127): every row dequantizes to zeros."""
        return cls(torch.zeros(num_pages, nkv, page_size, head_dim, dtype=torch.uint8, device=device),
                   torch.full((num_pages, nkv, page_size), 127, dtype=torch.uint8, device=device))

    @classmethod
    def from_dense(cls, x: torch.Tensor):
        """Quantize a bf16 cache [pages, nkv, page, D]."""
        return cls(*quant_kv_fp8(x))

    def dequant(self, dtype=torch.bfloat16) -> torch.Tensor:
        return dequant_kv_fp8(self.codes, self.scales, dtype)


_INV448 = torch.tensor(1.0 / 448.0, dtype=torch.float32)


def kv_fp8_exponent(amax: torch.Tensor) -> torch.Tensor:
    """The kernels' ``mx_e8m0`` on fp32 ``amax`` (int32 result): the biased exponent of the smallest
    power-of-two scale s with amax / s <= 448, 127 for a zero row, clamped to [1, 253] - computed
    as the kernels do, from the bits of the fp32 product amax * (1 / 448)."""
    a = amax.float()
    b = (a * _INV448.to(a.device)).view(torch.int32)
    e = ((b >> 23) & 255) + ((b & 0x7FFFFF) != 0).to(torch.int32)
    e = e.clamp(1, 253)
    return torch.where(a > 0, e, torch.full_like(e, 127))


def quant_kv_fp8(x: torch.Tensor):
    """Rows [..., D] (read as bf16) -> (codes uint8 [..., D] e4m3fn, scales uint8 [...] e8m0): the
    fp8 KV cache's row rule, matched by the kernels bit for bit.  amax over the row's bf16 values,
    e = ``kv_fp8_exponent(amax)``, code = e4m3 (RNE, saturating) of x * 2^(127 - e)."""
    v = x.to(torch.bfloat16).float()
    e = kv_fp8_exponent(v.abs().amax(-1))
    inv = ((254 - e) << 23).view(torch.float32)  # 2^(127 - e), as mx_inv_scale
    q = (v * inv.unsqueeze(-1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, e.to(torch.uint8)


def dequant_kv_fp8(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """code * 2^(e - 127): exact in bf16."""
    sc = (scales.to(torch.int32) << 23).view(torch.float32)
    return (codes.view(torch.float8_e4m3fn).float() * sc.unsqueeze(-1)).to(dtype)


def fake_quant_kv_fp8(x: torch.Tensor) -> torch.Tensor:
    """dequant(quant(x)) in x's dtype: what an fp8 KV cache returns for a written row."""
    return dequant_kv_fp8(*quant_kv_fp8(x), dtype=x.dtype)


def _scatter_cache_f8(cache: KVF8, slots, rows):
    """rows [T, nkv, D] bf16 -> quantized into cache[page, :, off] for slots >= 0."""
    ps = cache.codes.shape[2]
    valid = slots >= 0
    if not bool(valid.any()):
        return
    s = slots[valid]
    page, off = s // ps, s % ps
    q, e = quant_kv_fp8(rows[valid])
    cache.codes[page, :, off, :] = q
    cache.scales[page, :, off] = e


def rope_kv_write_f8(qkv, positions, cos, sin, k_cache: KVF8, v_cache: KVF8, slots, nh, nkv):
    """``rope_kv_write`` on an fp8 cache: k is rotated, rounded to bf16, then quantized per head."""
    T = qkv.shape[0]
    D = k_cache.shape[-1]
    view = qkv[:, : (nh + 2 * nkv) * D].view(T, nh + 2 * nkv, D)
    c, s = cos[positions.long()], sin[positions.long()]
    q = _rotate(view[:, :nh], c, s).to(qkv.dtype)
    k = _rotate(view[:, nh : nh + nkv], c, s).to(qkv.dtype)
    v = view[:, nh + nkv :]
    view[:, :nh] = q
    _scatter_cache_f8(k_cache, slots, k)
    _scatter_cache_f8(v_cache, slots, v)


def paged_attention_f8(q, k_cache: KVF8, v_cache: KVF8, block_tables, q_seq, q_ctx, nh, nkv, scale, out=None,
                       window=0):
    """Dequantize, then ``paged_attention``."""
    return paged_attention(q, k_cache.dequant(torch.float32), v_cache.dequant(torch.float32), block_tables, q_seq,
                           q_ctx, nh, nkv, scale, out=out, window=window)


def embedding(ids, table, out=None):
    y = table[ids.long()]
    if out is not None:
        out.copy_(y.view_as(out))
        return out
    return y


def swiglu(gu, out=None):
    """gu [T, 2F] with 16-row interleaved gate/up blocks -> silu(g) * u, HF rounding."""
    T, F2 = gu.shape
    F = F2 // 2
    v = gu.view(T, F // GU_BLOCK, 2, GU_BLOCK)
    g, u = v[:, :, 0].reshape(T, F), v[:, :, 1].reshape(T, F)
    a = torch.nn.functional.silu(g.float()).to(gu.dtype)
    y = (a.float() * u.float()).to(gu.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


def add(a, b, out=None):
    y = (a.float() + b.float()).to(a.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


def argmax(logits, out=None):
    y = torch.argmax(logits.float(), dim=-1)
    if out is not None:
        out.copy_(y)
        return out
    return y


def linear(x, w, out=None, epilogue=0, residual=None, ss_in=None, inv_k=0.0, eps=0.0, ap_out=None, ss_out=None,
           ss_zero=None):
    """``ss_in``: scale row r of x @ w^T by rsqrt(ss_in[r] * inv_k + eps) (fused-norm consumer);
    epilogue 3: r = bf16(bf16(y) + residual) -> residual (in place) and ``ap_out`` (packed),
    ``ss_out[r] += sum(r^2)`` (fused-norm producer)."""
    if ss_zero is not None:
        ss_zero.zero_()
    y = torch.nn.functional.linear(x, w) if x.dtype == w.dtype else torch.nn.functional.linear(x.to(w.dtype), w)
    if ss_in is not None:
        tot = ss_in.view(SS_SHARDS, SS_ROWS).sum(0)[: y.shape[0]].double() / SS_FX
        y = y.float() * torch.rsqrt(tot.float() * inv_k + eps)[:, None]
    y = y.to(x.dtype)
    if epilogue == 3:
        o = add(y, residual)
        residual.copy_(o)
        pack_act(o, out=ap_out)
        ss_out.view(SS_SHARDS, SS_ROWS)[0, : o.shape[0]] += fx_sumsq(o)
        return residual
    if epilogue == 1:
        y = swiglu(y)
    elif epilogue == 2:
        y = add(y, residual)
    if out is not None:
        out.copy_(y)
        return out
    return y


def sample_probs(logits_row: torch.Tensor, temperature: float, top_p: float, top_k: int,
                 repetition_penalty: float = 1.5, generated_tokens=None) -> torch.Tensor:
    """The filtered, renormalised distribution [1, V] a sampled row (temperature > 0) draws from:
    repetition penalty, softmax, top-k, top-p (reference src/rpc_handler.py:345-401)."""
    logits = logits_row.detach().float().clone().view(1, -1)
    temp = max(temperature, 1e-5)
    V = logits.shape[-1]
    if repetition_penalty != 1.0 and generated_tokens:
        recent = list(generated_tokens[-50:])
        counts = {}
        for tok in recent:
            counts[tok] = counts.get(tok, 0) + 1
        for tok, cnt in counts.items():
            if 0 <= tok < V:
                pen = repetition_penalty ** cnt
                if logits[0, tok] > 0:
                    logits[0, tok] /= pen
                else:
                    logits[0, tok] *= pen
        if len(generated_tokens) >= 3:
            last3 = list(generated_tokens[-3:])
            if len(set(last3)) == 1 and 0 <= last3[0] < V:
                pen = repetition_penalty ** 3
                if logits[0, last3[0]] > 0:
                    logits[0, last3[0]] /= pen
                else:
                    logits[0, last3[0]] *= pen
    probs = torch.softmax(logits / temp, dim=-1)
    if 0 < top_k < V:
        tv, ti = torch.topk(probs, top_k, dim=-1)
        probs = torch.zeros_like(probs).scatter(-1, ti, tv)
    if 0.0 < top_p < 1.0:
        sp, si = torch.sort(probs, descending=True, dim=-1)
        cum = torch.cumsum(sp, dim=-1)
        keep = cum <= top_p
        keep[..., 0] = True
        filt = sp * keep
        filt = filt / filt.sum(dim=-1, keepdim=True)
        probs = torch.zeros_like(probs).scatter(-1, si, filt)
    return probs / probs.sum(dim=-1, keepdim=True)


def sample_row(logits_row: torch.Tensor, temperature: float, top_p: float, top_k: int,
               repetition_penalty: float = 1.5, generated_tokens=None, generator=None) -> int:
    """One-row sampler with the reference semantics (reference src/rpc_handler.py:327-403)."""
    if temperature <= 0.0:
        return int(torch.argmax(logits_row.detach().float().view(1, -1), dim=-1).item())
    probs = sample_probs(logits_row, temperature, top_p, top_k, repetition_penalty, generated_tokens)
    return int(torch.multinomial(probs, 1, generator=generator).item())


def push_history(recent, recent_len, toks):
    """Append toks[r] to row r of the left-aligned history (drop the oldest when full)."""
    cap = recent.shape[1]
    for r in range(recent.shape[0]):
        n = int(recent_len[r])
        if n >= cap:
            recent[r, :-1] = recent[r, 1:].clone()
            n = cap - 1
        recent[r, n] = int(toks[r])
        recent_len[r] = n + 1


def sample(logits, temps, top_ps, top_ks, rep_pens, recent, recent_len, seeds, workspace=None, out=None):
    R = logits.shape[0]
    res = torch.empty(R, dtype=torch.long, device=logits.device)
    for r in range(R):
        n = int(recent_len[r])
        hist = [int(t) for t in recent[r, :n].tolist()]
        g = torch.Generator(device="cpu")
        g.manual_seed(int(seeds[r]) & 0x7FFFFFFFFFFFFFFF)
        res[r] = sample_row(logits[r].cpu(), float(temps[r]), float(top_ps[r]), int(top_ks[r]),
                            float(rep_pens[r]), hist, generator=g)
    if out is not None:
        out.copy_(res)
        return out
    return res


def sample_verify(logits, row_start, draft, temps, top_ps, top_ks, rep_pens, recent, recent_len, seeds,
                  update_history: bool = False):
    """Speculative verify, the semantics of ``ops.sample_verify``.  Session s owns the rows
    ``row_start[s] .. row_start[s + 1] - 1``; row j is drawn by ``sample_row`` with the history
    ``(h_s + draft[0..j-1])[-cap:]`` and a generator seeded with ``seeds[row]``.  n_s = the leading
    rows whose draw equals their draft; the session keeps t_0 .. t_{n_s}.  Returns
    (tokens int64 [R]: the kept ids, -1 behind them; count int32 [S] = n_s + 1)."""
    R = logits.shape[0]
    S = row_start.numel() - 1
    cap = recent.shape[1]
    tokens = torch.full((R,), -1, dtype=torch.long, device=logits.device)
    count = torch.zeros(S, dtype=torch.int32, device=logits.device)
    rs = [int(v) for v in row_start.tolist()]
    for s in range(S):
        lo, hi = rs[s], rs[s + 1]
        if hi <= lo:
            continue
        hist = [int(t) for t in recent[s, : int(recent_len[s])].tolist()]
        kept = 0
        for row in range(lo, hi):
            g = torch.Generator(device="cpu")
            g.manual_seed(int(seeds[row]) & 0x7FFFFFFFFFFFFFFF)
            t = sample_row(logits[row].cpu(), float(temps[s]), float(top_ps[s]), int(top_ks[s]), float(rep_pens[s]),
                           hist[-cap:], generator=g)
            tokens[row] = t
            kept += 1
            if row == hi - 1 or t != int(draft[row]):
                break
            hist.append(t)
        count[s] = kept
        if update_history:
            for t in tokens[lo:lo + kept].tolist():
                push_history(recent[s:s + 1], recent_len[s:s + 1], [t])
    return tokens, count


# ------------------------------------------------------------------ fp8 (OCP e4m3fn) W8A8
FP8_MAX = 448.0


def pack_weight_fp8(w):
    """W [N, K] -> (Wq uint8 [N/16, K/64, 64, 16], per-row scale fp32 [N]); see csrc/fp8.hip."""
    N, K = w.shape
    wf = w.float()
    s = wf.abs().amax(1).clamp_min(1e-30) / FP8_MAX
    q = (wf / s[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    qp = q.view(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 64, 64, 16)
    return qp.contiguous(), s.contiguous()


def unpack_weight_fp8(qp, s, dtype=torch.float32):
    n16, k64 = qp.shape[0], qp.shape[1]
    q = qp.view(n16, k64, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(n16 * 16, k64 * 64)
    return (q.view(torch.float8_e4m3fn).float() * s.float()[:, None]).to(dtype)


def quant_rows_fp8(x):
    """x [R, K] float -> (q float8 [R, K], scale [R]) with per-row absmax / 448 (1 for zero rows)."""
    x = x.float()
    amax = x.abs().amax(1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    return (x / s[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn), s


def quant_act_fp8(xp, M, K):
    """Packed bf16 activation (M rows) -> (A8 uint8 flat [K/64][MT][64][16], scale fp32 [MT*16])."""
    MT = (M + 15) // 16
    x = torch.zeros(MT * 16, K, dtype=torch.float32, device=xp.device)
    x[:M] = unpack_act(xp, M, K).float()
    q, s = quant_rows_fp8(x)
    a8 = q.view(torch.uint8).view(MT, 16, K // 64, 2, 4, 8).permute(2, 0, 4, 1, 3, 5).reshape(-1)
    return a8.contiguous(), s


def dequant_act_fp8(a8, s, M, K):
    MT = (M + 15) // 16
    q = a8[: MT * 16 * K].view(K // 64, MT, 4, 16, 2, 8).permute(1, 3, 0, 4, 2, 5).reshape(MT * 16, K)
    return (q.view(torch.float8_e4m3fn).float() * s[: MT * 16, None].float())[:M]


def linear_fp8(a8, a_scale, wq, w_scale, M, epilogue=0, residual=None, dtype=torch.bfloat16):
    """fp32 reference of csrc/fp8.hip gemm_fp8 (same epilogue rounding as the kernel)."""
    N, K = 16 * wq.shape[0], 64 * wq.shape[1]
    y = dequant_act_fp8(a8, a_scale, M, K) @ unpack_weight_fp8(wq, w_scale).t()
    if epilogue == 1:
        F = N // 2
        v = y.view(M, F // GU_BLOCK, 2, GU_BLOCK)
        g = v[:, :, 0].reshape(M, F).to(dtype).float()
        u = v[:, :, 1].reshape(M, F).to(dtype).float()
        a = torch.nn.functional.silu(g).to(dtype).float()
        return (a * u).to(dtype)
    if epilogue == 2:
        return (y.to(dtype).float() + residual.float()).to(dtype)
    return y.to(dtype)


# ------------------------------------------------------------------ OCP MXFP4 weights (W4A16)
# e2m1 codes (sign bit 3, bits 2..0 index E2M1_VALUES) with one e8m0 scale byte per 32 weights
# along K: 4 + 8 / 32 = 4.25 bits per weight.  Packed layout (csrc/gemm_w4.hip):
#   w4 uint8 [N/16, K/128, 64, 16]: lane = 16 q + c, byte 4 s + b holds the codes of
#       W[16 nt + c][128 kb + 32 s + 8 q + 2 b] (low nibble) and of the next k (high nibble) - a
#       lane's 16 bytes are its 8 weights of each of four consecutive 32-deep k-slices s;
#   s4 uint8 [N/16, K/128, 16, 4]: column c, one scale byte per k-slice s.
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MX_BLOCK = 32


def quant_mxfp4(w):
    """W [N, K] -> (codes uint8 [N, K], scale bytes uint8 [N, K/32]) by the OCP MX rule: e =
    clamp(floor(log2(amax)) - 2 + 127, 1, 254) per 32-block (1 for an all-zero block), codes =
    x / 2^(e - 127) rounded to nearest e2m1 with ties to the even code, saturating at +-6; the
    code 0b1000 (negative zero) is never emitted."""
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"MXFP4 needs K % {MX_BLOCK} == 0 (K={K})")
    x = w.detach().float().reshape(N, K // MX_BLOCK, MX_BLOCK)
    amax = x.abs().amax(-1)
    _, ex = torch.frexp(amax)  # amax = m 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, (ex.to(torch.int32) - 1 - 2 + 127).clamp(1, 254), torch.ones_like(ex, dtype=torch.int32))
    scale = (e << 23).view(torch.float32)  # 2^(e - 127), exact
    a = (x / scale[..., None]).abs()
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
            + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = code | (((x < 0) & (code > 0)).to(torch.uint8) << 3)
    return code.reshape(N, K), e.to(torch.uint8)


def dequant_mxfp4(code, e, dtype=torch.float32):
    """codes [N, K], scale bytes [N, K/32] -> W [N, K] = value(code) * 2^(e - 127) (exact in bf16)."""
    N, K = code.shape
    tab = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=code.device)
    scale = (e.to(torch.int32) << 23).view(torch.float32)
    v = tab[code.long()].reshape(N, K // MX_BLOCK, MX_BLOCK) * scale[..., None]
    return v.reshape(N, K).to(dtype)


def pack_mxfp4(code, e):
    """codes [N, K], scale bytes [N, K/32] -> (w4, s4) in the decode GEMM's fragment order (layout above)."""
    N, K = code.shape
    if N % 16 or K % 128:
        raise ValueError(f"MXFP4 weights need N % 16 == 0 and K % 128 == 0 (N={N}, K={K})")
    by = code[:, 0::2] | (code[:, 1::2] << 4)  # [N, K/2]: lower k in the low nibble
    # byte index k/2 = 64 kb + 16 s + 4 q + b  ->  [nt, kb, q, c, s, b]
    w4 = by.view(N // 16, 16, K // 128, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 128, 64, 16)
    s4 = e.view(N // 16, 16, K // 128, 4).permute(0, 2, 1, 3)
    return w4.contiguous(), s4.contiguous()


def unpack_mxfp4(w4, s4):
    """Inverse of ``pack_mxfp4``: (codes uint8 [N, K], scale bytes uint8 [N, K/32])."""
    n16, k128 = w4.shape[0], w4.shape[1]
    N, K = n16 * 16, k128 * 128
    by = w4.view(n16, k128, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(N, K // 2)
    code = torch.stack((by & 15, by >> 4), -1).reshape(N, K)
    e = s4.view(n16, k128, 16, 4).permute(0, 2, 1, 3).reshape(N, K // MX_BLOCK)
    return code, e


def pack_weight_w4(w):
    """W [N, K] (N % 16 == 0, K % 128 == 0) -> (w4 uint8 [N/16, K/128, 64, 16], s4 uint8
    [N/16, K/128, 16, 4]): MXFP4 quantization (``quant_mxfp4``) + the fragment-order layout."""
    N, K = w.shape
    if N % 16 or K % 128:
        raise ValueError(f"MXFP4 weights need N % 16 == 0 and K % 128 == 0 (N={N}, K={K})")
    return pack_mxfp4(*quant_mxfp4(w))


def unpack_weight_w4(w4, s4, dtype=torch.float32):
    """Inverse layout of ``pack_weight_w4`` + dequantization -> W [N, K]."""
    return dequant_mxfp4(*unpack_mxfp4(w4, s4), dtype)
