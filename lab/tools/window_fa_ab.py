#!/usr/bin/env python3
"""Causal prefill attention under a sliding window, isolated: us per call of

  fa_win  ``ops.attention_fa_window`` / ``attention_fa_window_f8`` (the FA2 kernel's windowed form; blocks
          and waves from ``ops.fa_plan``, the op's own parts and pairing) - what the executor runs for a
          row-major prefill step with rows past the window;
  fd_win  ``ops.paged_attention(window=W)`` with the executor's partition: every prompt token as one
          causal row of the flash-decoding kernel - the path ``fa_win`` replaces (MPAMD_WINDOW_FA=0);
  fa_full ``ops.attention_fa`` / ``attention_fa_f8`` without a window on the same prompt.  It reads the
          whole context: more work and another result, a sanity ceiling only.

Each call reads another copy of the cache pages (``copies`` of them, together past the 256 MB last-level
cache), as the layers of a model do: the pages stream from HBM.  The three sides alternate inside one
process, ``--repeats`` times; a row carries every repeat's time, its fastest and its slowest.  ``fa_win``
is first checked against ``fd_win`` (atol = rtol = 2e-2) and, on an fp8 cache, to equal the bf16 form on
the dequantized pages bit for bit.  One JSON line per (case, cache, side).

    python lab/tools/window_fa_ab.py --repeats 3
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

HEADS = {"mistral-7b": (32, 8, 128), "llama2-7b": (32, 32, 128)}
CASES = [(8192, 0), (16384, 0), (512, 8192)]  # (tokens of the step, prefix already in the cache)
PS = 64


def _time(fn, iters):
    for _ in range(2):
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
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(f"{n}@{p}" for n, p in CASES))
    a = ap.parse_args()
    ops.require_native()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    W = a.window
    for model in a.models.split(","):
        nh, nkv, D = HEADS[model]
        scale = 1 / math.sqrt(D)
        for n, pre in [tuple(int(x) for x in c.split("@")) for c in a.cases.split(",")]:
            ctx = pre + n
            pages = math.ceil(ctx / PS)
            copy_bytes = 2 * pages * nkv * PS * D * 2
            copies = max(2, math.ceil((512 << 20) / copy_bytes))
            kb = [(torch.randn(pages, nkv, PS, D, device=dev, generator=gen)).to(torch.bfloat16) for _ in range(copies)]
            vb = [(torch.randn(pages, nkv, PS, D, device=dev, generator=gen)).to(torch.bfloat16) for _ in range(copies)]
            bt = torch.randperm(pages, device=dev).to(torch.int32).view(1, pages)
            qkv = (torch.randn(n, (nh + 2 * nkv) * D, device=dev, generator=gen) * 0.5).to(torch.bfloat16)
            q_seq = torch.zeros(n, dtype=torch.int32, device=dev)
            q_ctx = torch.arange(pre + 1, ctx + 1, dtype=torch.int32, device=dev)
            fbn, waves = ops.fa_plan([n], nh, nkv, n_cu)
            fb = torch.from_numpy(fbn).to(dev)
            ps, np_ = ops.attention_partition(n, nkv, min(ctx, W + 31), min_part=64)  # the executor's, for fd_win
            out = torch.empty(n, nh * D, dtype=torch.bfloat16, device=dev)
            for cache in ("bf16", "fp8"):
                if cache == "fp8":
                    kc = [ops.KVF8.from_dense(x) for x in kb]
                    vc = [ops.KVF8.from_dense(x) for x in vb]
                    win, full = ops.attention_fa_window_f8, ops.attention_fa_f8
                else:
                    kc, vc = kb, vb
                    win, full = ops.attention_fa_window, ops.attention_fa
                ws = ops.attention_workspace(n, nh, D, max(np_, 8), dev)
                turn = [0]

                def pick():
                    turn[0] = (turn[0] + 1) % copies
                    return kc[turn[0]], vc[turn[0]]

                def fa_win():
                    return win(qkv, *pick(), bt, q_seq, q_ctx, fb, nh, nkv, scale, W, out=out, workspace=ws,
                               max_ctx=ctx, waves=waves)

                def fd_win():
                    return ops.paged_attention(qkv, *pick(), bt, q_seq, q_ctx, nh, nkv, scale, out=out, workspace=ws,
                                               part_size=ps, num_parts=np_, window=W, max_ctx=ctx)

                def fa_full():
                    return full(qkv, *pick(), bt, q_seq, q_ctx, fb, nh, nkv, scale, out=out, workspace=ws, max_ctx=ctx,
                                waves=waves)

                turn[0] = 0
                o_fa = fa_win().clone()
                turn[0] = 0
                o_fd = fd_win().clone()
                close = bool(torch.allclose(o_fa.float(), o_fd.float(), atol=2e-2, rtol=2e-2))
                equal = None
                if cache == "fp8":
                    o_bf = ops.attention_fa_window(qkv, kc[1].dequant(), vc[1].dequant(), bt, q_seq, q_ctx, fb, nh, nkv,
                                                   scale, W, max_ctx=ctx, waves=waves)
                    equal = bool(torch.equal(o_fa, o_bf))
                sides = [("fa_win", fa_win, a.iters), ("fd_win", fd_win, max(2, a.iters // 4)),
                         ("fa_full", fa_full, a.iters)]
                us = {label: [] for label, _, _ in sides}
                for _ in range(a.repeats):
                    for label, fn, iters in sides:
                        us[label].append(round(_time(fn, iters), 1))
                for label, _, _ in sides:
                    print(json.dumps({"heads": model, "nh": nh, "nkv": nkv, "D": D, "tokens": n, "prefix": pre,
                                      "window": W, "cache": cache, "side": label, "waves": waves,
                                      "blocks": int(fb.shape[1]), "copies": copies, "fa_win_close_to_fd_win": close,
                                      "fa_win_f8_equals_bf16": equal, "us": us[label], "us_min": min(us[label]),
                                      "us_max": max(us[label])}), flush=True)
                del kc, vc
            del kb, vb
            torch.cuda.empty_cache()


if __name__ == "__main__":
    with torch.no_grad():
        main()
