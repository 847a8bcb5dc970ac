#!/usr/bin/env python3
"""Decode attention alone, with and without a sliding window, under decode conditions: every call
reads another copy of the sessions' pages (the copies a case touches together exceed the 256 MB
last-level cache several times over), so the cache stream comes from HBM as in a real step - the
method of ``kv_fp8_ab.py``.  Per (heads, sessions, context, window, cache format): us per call of the
fused decode attention the executor runs for those heads - ``ops.attention_mfma_rope`` /
``ops.attention_mfma_rope_f8`` for GQA groups of >= 4 heads (Mistral-7B: 32 / 8 / 128), else
``ops.paged_attention_rope`` - with the executor's partition of the streamed span.

Default cases (Mistral-7B heads, W = 4096, 1 and 64 sessions, bf16 and fp8 cache):
  context W, window off          what the capped session costs at its longest
  context 2W and 4W, window W    a session past the window
  context 2W and 4W, window off  what full attention would cost there

The cases alternate inside one process, ``--repeats`` times; a row carries every repeat's time.
``--cases B:ctx:window,...`` and ``--heads`` pick others.  A kernel library without the window
argument (an older build, ``MPAMD_KERNEL_LIB``) runs the window-off cases: ``window=0`` passes no
window argument to the op.

    python lab/tools/window_ab.py --repeats 3
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

HEADS = {"mistral-7b": (32, 8, 128), "llama2-7b": (32, 32, 128), "llama3-8b": (32, 8, 128)}
W = 4096
POOL = 1 << 30  # bytes of fp8 pages the copies of a case cover at least (4 x the last-level cache)
PS = 64


def default_cases():
    out = []
    for B in (1, 64):
        out += [(B, W, 0), (B, 2 * W, W), (B, 4 * W, W), (B, 2 * W, 0), (B, 4 * W, 0)]
    return out


def _fill(P, nkv, D, dev, gen):
    """bf16 caches [P, nkv, PS, D] x2 and their fp8 quantization, built in chunks of pages."""
    kb = torch.empty(P, nkv, PS, D, dtype=torch.bfloat16, device=dev)
    vb = torch.empty_like(kb)
    kf, vf = ops.KVF8.empty(P, nkv, PS, D, dev), ops.KVF8.empty(P, nkv, PS, D, dev)
    for p0 in range(0, P, 512):
        n = min(512, P - p0)
        for dense, f8 in ((kb, kf), (vb, vf)):
            dense[p0:p0 + n] = torch.randn(n, nkv, PS, D, device=dev, generator=gen).to(torch.bfloat16)
            q, e = ops.quant_kv_fp8(dense[p0:p0 + n])
            f8.codes[p0:p0 + n], f8.scales[p0:p0 + n] = q, e
    return kb, vb, kf, vf


def _time(fn, copies, iters):
    for i in range(min(copies, 3)):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % copies)
    e1.record()
    e1.synchronize()
    return 1000 * e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", default="mistral-7b")
    ap.add_argument("--cases", default="", help="B:ctx:window,... (default: the Mistral-7B set above)")
    ap.add_argument("--kv", default="bf16,fp8")
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    ops.require_native()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lib = os.path.basename(os.environ.get("MPAMD_KERNEL_LIB", "")) or "default"
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",") if c] or default_cases()
    kvs = a.kv.split(",")
    for heads in a.heads.split(","):
        nh, nkv, D = HEADS[heads]
        gqa = nh // nkv >= 4  # the executor's rule for the MFMA GQA decode kernel
        scale = 1 / math.sqrt(D)
        max_ctx = max(c for _, c, _ in cases)
        cos, sin = ops.rope_cos_sin(D, max_ctx + 1, 10000.0, dev)
        # one pool for every case: two copies of the largest one
        P = 2 * max(B * math.ceil(c / PS) for B, c, _ in cases)
        kb, vb, kf, vf = _fill(P, nkv, D, dev, gen)
        sides = []
        for B, ctx, win in cases:
            pps = math.ceil(ctx / PS)
            seen = min(ctx, win) if win else ctx  # tokens per session a call reads
            copies = min(max(2, math.ceil(POOL / (2 * B * seen * nkv * (D + 1)))), P // (B * pps))
            perm = torch.randperm(P, device=dev)[: copies * B * pps].to(torch.int32).view(copies, B, pps)
            qkv = (torch.randn(B, (nh + 2 * nkv) * D, device=dev, generator=gen) * 0.5).to(torch.bfloat16)
            q_seq = torch.arange(B, dtype=torch.int32, device=dev)
            q_ctx = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            pos = q_ctx.long() - 1
            slots = [perm[c, :, (ctx - 1) // PS].long() * PS + (ctx - 1) % PS for c in range(copies)]
            out = torch.empty(ops.packed_numel(B, nh * D), dtype=torch.bfloat16, device=dev)
            span = min(ctx, win + 31) if win else ctx  # the executor's _attn_span
            ps, np_ = ops.attention_partition(B, nkv, span, min_part=256 if gqa else 64)
            if gqa:
                ps2 = 128 * math.ceil(ps / 128)
                ps, np_ = ps2, max(1, math.ceil(ps * np_ / ps2))
            ws = ops.attention_workspace(B, nh, D, np_, dev)
            qb = torch.stack([torch.arange(B), torch.ones(B, dtype=torch.long)]).to(torch.int32).to(dev)
            for kv in kvs:
                kc, vc = (kf, vf) if kv == "fp8" else (kb, vb)
                if gqa:
                    op = ops.attention_mfma_rope_f8 if kv == "fp8" else ops.attention_mfma_rope
                    kern = op.__name__

                    def fn(c, op=op, kc=kc, vc=vc, perm=perm, q_seq=q_seq, q_ctx=q_ctx, qb=qb, pos=pos, slots=slots,
                           out=out, ws=ws, ps=ps, np_=np_, win=win, qkv=qkv, ctx=ctx):
                        op(qkv, kc, vc, perm[c], q_seq, q_ctx, qb, pos, cos, sin, slots[c], nh, nkv, scale, out=out,
                           workspace=ws, part_size=ps, num_parts=np_, packed=True, max_ctx=ctx, window=win)
                else:
                    kern = "paged_attention_rope" + ("_f8" if kv == "fp8" else "")

                    def fn(c, kc=kc, vc=vc, perm=perm, q_seq=q_seq, q_ctx=q_ctx, pos=pos, slots=slots, out=out, ws=ws,
                           ps=ps, np_=np_, win=win, qkv=qkv, ctx=ctx):
                        ops.paged_attention_rope(qkv, kc, vc, perm[c], q_seq, q_ctx, pos, cos, sin, slots[c], nh, nkv,
                                                 scale, out=out, workspace=ws, part_size=ps, num_parts=np_, packed=True,
                                                 max_ctx=ctx, window=win)
                nbytes = 2 * B * seen * nkv * ((D + 1) if kv == "fp8" else 2 * D)
                sides.append((dict(lib=lib, heads=heads, nh=nh, nkv=nkv, D=D, sessions=B, ctx=ctx, window=win, kv=kv,
                                   kernel=kern, part_size=ps, num_parts=np_, copies=copies, cache_bytes=nbytes),
                              fn, copies))
        us = [[] for _ in sides]
        for _ in range(a.repeats):
            for i, (_, fn, copies) in enumerate(sides):
                us[i].append(round(_time(fn, copies, a.iters), 2))
        for (row, _, _), u in zip(sides, us):
            print(json.dumps({**row, "us": u, "us_min": min(u), "us_max": max(u),
                              "gb_per_s": round(row["cache_bytes"] / min(u) / 1e3, 1)}), flush=True)
        del kb, vb, kf, vf, sides
        torch.cuda.empty_cache()


if __name__ == "__main__":
    with torch.no_grad():
        main()
