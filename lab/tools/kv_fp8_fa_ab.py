#!/usr/bin/env python3
"""Causal prefill attention on an fp8 KV cache, isolated: us per call of

  fa_f8   ``ops.attention_fa_f8`` on the fp8 cache (the FA2 kernel's fp8 form; blocks and waves from
          ``ops.fa_plan``, the op's own parts and pairing) - what the executor runs for a prefill step
          with a row-major output;
  fa_bf16 ``ops.attention_fa`` on the bf16 cache of the dequantized values, same blocks and waves;
  fd_f8   ``ops.paged_attention`` on the fp8 cache with the executor's partition: every prompt token as
          one causal row of the flash-decoding kernel - the path ``fa_f8`` replaces
          (MPAMD_KV_FP8_FA=0).

The three sides alternate inside one process, ``--repeats`` times; a row carries every repeat's time,
its fastest and its slowest.  ``fa_f8`` and ``fa_bf16`` are checked to be equal bit for bit first.
One JSON line per (case, side).

    python lab/tools/kv_fp8_fa_ab.py --repeats 3
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

HEADS = {"llama2-7b": (32, 32, 128), "llama3-8b": (32, 8, 128)}
CASES = [(1, 2048), (64, 128)]  # (prompts, tokens per prompt)
PS = 64


def _time(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1000 * e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(HEADS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    ops.require_native()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    for model in a.models.split(","):
        nh, nkv, D = HEADS[model]
        scale = 1 / math.sqrt(D)
        for B, L in CASES:
            T, pps = B * L, math.ceil(L / PS)
            P = B * pps
            kb = torch.randn(P, nkv, PS, D, device=dev, generator=gen).to(torch.bfloat16)
            vb = torch.randn(P, nkv, PS, D, device=dev, generator=gen).to(torch.bfloat16)
            kf, vf = ops.KVF8.from_dense(kb), ops.KVF8.from_dense(vb)
            kb, vb = kf.dequant(), vf.dequant()
            bt = torch.randperm(P, device=dev).to(torch.int32).view(B, pps)
            qkv = (torch.randn(T, (nh + 2 * nkv) * D, device=dev, generator=gen) * 0.5).to(torch.bfloat16)
            q_seq = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(L)
            q_ctx = torch.arange(1, L + 1, dtype=torch.int32, device=dev).repeat(B)
            fbn, waves = ops.fa_plan([L] * B, nh, nkv, n_cu)
            fb = torch.from_numpy(fbn).to(dev)
            ps, np_ = ops.attention_partition(T, nkv, L, min_part=64)
            ws = ops.attention_workspace(T, nh, D, max(np_, math.ceil(L / 256)), dev)
            out = torch.empty(T, nh * D, dtype=torch.bfloat16, device=dev)

            def fa_f8():
                return ops.attention_fa_f8(qkv, kf, vf, bt, q_seq, q_ctx, fb, nh, nkv, scale, out=out, workspace=ws,
                                           max_ctx=L, waves=waves)

            def fa_bf16():
                return ops.attention_fa(qkv, kb, vb, bt, q_seq, q_ctx, fb, nh, nkv, scale, out=out, workspace=ws,
                                        max_ctx=L, waves=waves)

            def fd_f8():
                return ops.paged_attention(qkv, kf, vf, bt, q_seq, q_ctx, nh, nkv, scale, out=out, workspace=ws,
                                           part_size=ps, num_parts=np_)

            equal = torch.equal(fa_f8().clone(), fa_bf16().clone())
            sides = [("fa_f8", fa_f8, "attention_fa_f8"), ("fa_bf16", fa_bf16, "attention_fa"),
                     ("fd_f8", fd_f8, "paged_attention_f8")]
            us = {label: [] for label, _, _ in sides}
            for _ in range(a.repeats):
                for label, fn, _ in sides:
                    us[label].append(round(_time(fn, a.iters), 2))
            for label, _, kern in sides:
                print(json.dumps({"heads": model, "nh": nh, "nkv": nkv, "D": D, "prompts": B, "prompt_len": L,
                                  "side": label, "op": kern, "waves": waves, "blocks": int(fb.shape[1]),
                                  "fa_f8_equals_fa_bf16": equal, "us": us[label], "us_min": min(us[label]),
                                  "us_max": max(us[label])}), flush=True)


if __name__ == "__main__":
    with torch.no_grad():
        main()
