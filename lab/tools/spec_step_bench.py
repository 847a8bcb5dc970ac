#!/usr/bin/env python3
"""Cost of a speculative verify step on one stage executor: a full Llama-2-7B stage (synthetic
weights, embedding and head included, bf16), one session, contexts 128 and 2048.

    decode   the graph-replayed one-token decode step (what the plain loop pays per token)
    verify   an eager verify step of K + 1 rows, K + 1 in {1, 2, 4, 8, 16}, logits of every row
             (K + 1 = 1 has no draft: it is the decode step again)
    sampler  ops.sample_verify over the K + 1 rows of one session against K + 1 one-row ops.sample calls

Every step rewinds the session to the context (``starts``), so all steps of a row see the same
context.  Times are host wall time per step with a device synchronize around the timed loop (an
eager step is bounded by its launches, not by the GPU).  ``break_even`` is the number of accepted
drafts per verify step at which verify steps emit tokens as fast as decode steps on this one GPU:
(1 + a) / t_verify = 1 / t_decode  ->  a = t_verify / t_decode - 1.  One JSON line per row.

    python lab/tools/spec_step_bench.py --contexts 128,2048 --rows 1,2,4,8,16
"""
import argparse
import json
import os
import sys
import time

import torch


def timed(fn, warm, steps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--contexts", default="128,2048")
    ap.add_argument("--rows", default="1,2,4,8,16")
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--steps", type=int, default=48)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))
    os.environ.setdefault("MPAMD_GEMM_AUTOTUNE", "0")  # the committed kernel table, no timing race
    from src import ops
    from src.models.config import resolve_model
    from src.models.weights import random_stage_weights
    from src.runtime.executor import StageExecutor
    from src.runtime.sampler import RECENT

    dev = torch.device("cuda")
    cfg = resolve_model(a.model)
    V = cfg.vocab_size
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=dev)
    ex = StageExecutor(cfg, w, dev, kv_cache_bytes=4 << 30, max_sessions=4, max_seq_len=4096, warmup=False)
    g = torch.Generator(device=dev).manual_seed(1)
    rows = [int(r) for r in a.rows.split(",")]
    with torch.no_grad():
        for C in (int(c) for c in a.contexts.split(",")):
            ids = torch.randint(0, V, (C,), device=dev, generator=g)
            ex.forward([("s", C)], ids, reset=[True])
            tok = torch.randint(0, V, (1,), device=dev, generator=g)
            t_dec = timed(lambda: ex.forward([("s", 1)], tok, starts=[C]), a.warm, a.steps)
            assert ex.last_graphed, "the decode step did not replay a graph"
            print(json.dumps({"what": "decode", "context": C, "graphed": True, "ms_per_step": round(t_dec, 4)}),
                  flush=True)
            for n in rows:
                blk = torch.randint(0, V, (n,), device=dev, generator=g)
                t_ver = timed(lambda: ex.forward([("s", n)], blk, starts=[C], logit_rows=[n]), a.warm, a.steps)
                # (one row: no draft, the plain decode step and its graph)
                print(json.dumps({"what": "verify", "context": C, "rows": n, "graphed": bool(ex.last_graphed),
                                  "ms_per_step": round(t_ver, 4),
                                  "vs_decode": round(t_ver / t_dec, 3),
                                  "break_even_accepted": round(max(t_ver / t_dec - 1.0, 0.0), 3)}), flush=True)
        # the sampler alone: one session, the CLI's parameters
        f = lambda v, dt=torch.float32: torch.tensor([v], dtype=dt, device=dev)  # noqa: E731
        par = (f(1.0), f(0.92), f(50, torch.int32), f(1.5))
        for n in rows:
            logits = (3.0 * torch.randn(n, V, device=dev, generator=g)).to(torch.bfloat16)
            recent = torch.randint(0, V, (1, RECENT), device=dev, generator=g).int()
            rlen = torch.tensor([RECENT], dtype=torch.int32, device=dev)
            seeds = torch.arange(n, device=dev)
            row_start = torch.tensor([0, n], dtype=torch.int32, device=dev)
            draft = torch.randint(0, V, (n,), device=dev, generator=g).int()
            ws = torch.empty(ops.sample_verify_workspace(n, V, RECENT), dtype=torch.float32, device=dev)
            tokens = torch.empty(n, dtype=torch.long, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            out1 = torch.empty(1, dtype=torch.long, device=dev)
            t_v = timed(lambda: ops.sample_verify(logits, row_start, draft, *par, recent, rlen, seeds, workspace=ws,
                                                  tokens=tokens, count=count), a.warm, 4 * a.steps)

            def one_by_one():
                for j in range(n):
                    ops.sample(logits[j:j + 1], *par, recent, rlen, seeds[j:j + 1], workspace=ws, out=out1)

            t_s = timed(one_by_one, a.warm, 4 * a.steps)
            print(json.dumps({"what": "sampler", "rows": n, "sample_verify_ms": round(t_v, 4),
                              "sample_calls_ms": round(t_s, 4)}), flush=True)


if __name__ == "__main__":
    main()
