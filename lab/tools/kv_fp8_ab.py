#!/usr/bin/env python3
"""Decode attention on a bf16 vs an fp8 KV cache, isolated, under decode conditions: every call reads
another copy of the sessions' pages (the copies together exceed the 256 MB last-level cache several
times over), so the cache stream comes from HBM as in a real step.  Per (heads, sessions, context):
us per call and achieved cache bytes/s of

  bf16  the fused decode attention the executor runs for that model: ``ops.paged_attention_rope``
        (MHA, flash-decoding kernel) or ``ops.attention_mfma_rope`` (GQA, MFMA kernel), with the
        executor's context partition;
  fp8   ``ops.paged_attention_rope`` on the fp8 cache (the flash-decoding kernel's fp8 form);
  fp8_mfma  (GQA heads only) ``ops.attention_mfma_rope_f8``: the MFMA kernel's fp8 form, with the bf16
        side's partition - what the executor runs for a GQA model on an fp8 cache; ``fp8`` is then
        what it ran before that form existed (MPAMD_KV_FP8_MFMA=0).

The sides alternate inside one process, ``--repeats`` times; a row carries every repeat's time, so the
spread is visible.  One JSON line per (case, format).

    python lab/tools/kv_fp8_ab.py --repeats 3
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

HEADS = {"llama2-7b": (32, 32, 128), "llama3-70b": (64, 8, 128), "llama3-8b": (32, 8, 128)}
CASES = [(64, 170), (64, 2048), (64, 4096), (1, 4096)]  # (sessions, context tokens)
POOL = 1 << 30  # bytes of fp8 pages the copies cover at least (4 x the last-level cache)
PS = 64


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
    ap.add_argument("--models", default=",".join(HEADS))
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    ops.require_native()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    for model in a.models.split(","):
        nh, nkv, D = HEADS[model]
        gqa = nh // nkv >= 4  # the executor's rule for the MFMA GQA decode kernel
        scale = 1 / math.sqrt(D)
        cos, sin = ops.rope_cos_sin(D, 8192, 10000.0, dev)
        for B, ctx in CASES:
            pps = math.ceil(ctx / PS)
            bytes_bf = 2 * B * ctx * nkv * D * 2
            bytes_f8 = 2 * B * ctx * nkv * (D + 1)
            copies = max(2, math.ceil(POOL / bytes_f8))
            P = copies * B * pps
            kb, vb, kf, vf = _fill(P, nkv, D, dev, gen)
            perm = torch.randperm(P, device=dev).to(torch.int32).view(copies, B, pps)
            qkv = (torch.randn(B, (nh + 2 * nkv) * D, device=dev, generator=gen) * 0.5).to(torch.bfloat16)
            q_seq = torch.arange(B, dtype=torch.int32, device=dev)
            q_ctx = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            pos = q_ctx.long() - 1
            slots = [perm[c, :, (ctx - 1) // PS].long() * PS + (ctx - 1) % PS for c in range(copies)]
            out = torch.empty(ops.packed_numel(B, nh * D), dtype=torch.bfloat16, device=dev)
            ps, np_ = ops.attention_partition(B, nkv, ctx, min_part=256 if gqa else 64)
            ps8, np8 = ops.attention_partition(B, nkv, ctx, min_part=64)
            ws = ops.attention_workspace(B, nh, D, max(np_, np8), dev)
            qb = torch.stack([torch.arange(B), torch.ones(B, dtype=torch.long)]).to(torch.int32).to(dev)

            def bf16(c):
                if gqa:
                    ps2 = 128 * math.ceil(ps / 128)
                    ops.attention_mfma_rope(qkv, kb, vb, perm[c], q_seq, q_ctx, qb, pos, cos, sin, slots[c], nh, nkv,
                                            scale, out=out, workspace=ws, part_size=ps2,
                                            num_parts=max(1, math.ceil(ps * np_ / ps2)), packed=True)
                else:
                    ops.paged_attention_rope(qkv, kb, vb, perm[c], q_seq, q_ctx, pos, cos, sin, slots[c], nh, nkv,
                                             scale, out=out, workspace=ws, part_size=ps, num_parts=np_, packed=True)

            def fp8(c):
                ops.paged_attention_rope(qkv, kf, vf, perm[c], q_seq, q_ctx, pos, cos, sin, slots[c], nh, nkv, scale,
                                         out=out, workspace=ws, part_size=ps8, num_parts=np8, packed=True)

            def fp8_mfma(c):
                ps2 = 128 * math.ceil(ps / 128)
                ops.attention_mfma_rope_f8(qkv, kf, vf, perm[c], q_seq, q_ctx, qb, pos, cos, sin, slots[c], nh, nkv,
                                           scale, out=out, workspace=ws, part_size=ps2,
                                           num_parts=max(1, math.ceil(ps * np_ / ps2)), packed=True)

            sides = [("bf16", bf16, bytes_bf, "attention_mfma_rope" if gqa else "paged_attention_rope"),
                     ("fp8", fp8, bytes_f8, "paged_attention_rope_f8")]
            if gqa:
                sides.append(("fp8_mfma", fp8_mfma, bytes_f8, "attention_mfma_rope_f8"))
            us = {label: [] for label, _, _, _ in sides}
            for _ in range(a.repeats):
                for label, fn, _, _ in sides:
                    us[label].append(round(_time(fn, copies, a.iters), 2))
            for label, _, nbytes, kern in sides:
                best = min(us[label])
                print(json.dumps({"heads": model, "nh": nh, "nkv": nkv, "D": D, "sessions": B, "ctx": ctx,
                                  "kv": label, "kernel": kern, "copies": copies, "cache_bytes": nbytes,
                                  "us": us[label], "us_min": best, "us_max": max(us[label]),
                                  "gb_per_s": round(nbytes / best / 1e3, 1)}), flush=True)
            del kb, vb, kf, vf
            torch.cuda.empty_cache()


if __name__ == "__main__":
    with torch.no_grad():
        main()
