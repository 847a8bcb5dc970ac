#!/usr/bin/env python3
"""Decode-step time of one StageExecutor per stored weight format: graph-replayed decode steps on
synthetic Llama-2-7B weights (all 32 blocks, embeddings and head on one GPU), batch 1 and batch 64,
for quant_type none / fp8 / mxfp4.  Per case: prefill, warm-up decode steps (graph capture, the
start-up autotuners), then HIP events around ``--steps`` (>= 20) replayed steps; the median of
``--windows`` such windows is reported with their min / max.  One JSON line per case.
``--kv_cache_dtype bf16,fp8`` runs every case per KV cache format; ``--synthetic_kv`` fills the
prompt's KV pages with random values through ``import_session_kv`` instead of prefilling (long
prompts: the decode step's time does not depend on what the pages hold).  ``--sliding_window attend``
(models with a window, e.g. mistral-7b): sessions run past the window, the imported pages below it
are released before the first step, and the row carries the KV bytes a session holds.

    python lab/tools/quant_step_bench.py --batches 1,64 --steps 32
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402
from src.models.config import resolve_model  # noqa: E402
from src.models.weights import random_stage_weights  # noqa: E402
from src.runtime.executor import StageExecutor  # noqa: E402
from src.runtime.kv_layout import import_session_kv  # noqa: E402


def run_case(cfg, quant, batch, a, dev, kv_dtype="bf16"):
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=dev, seed=0,
                             quant_type=quant)
    total = a.prompt_len + a.warmup + a.windows * a.steps + 8
    attend = a.sliding_window == "attend" and bool(cfg.sliding_window)
    # tokens the page pool must hold: every session whole, or under a rolling window one session whole
    # (the import) next to the others' windows
    pool = batch * total if not attend else total + batch * (min(total, cfg.sliding_window) + 192)
    ex = StageExecutor(cfg, w, dev, max_sessions=batch + 8, max_seq_len=max(256, total),
                       kv_cache_bytes=max(1 << 30, 2 * pool * cfg.kv_bytes_per_token_per_layer(2)
                                          * cfg.num_hidden_layers),
                       use_graphs=True, graph_max_batch=max(batch, 1),
                       **({"kv_cache_dtype": kv_dtype} if kv_dtype != "bf16" else {}),
                       **({"sliding_window": "attend"} if attend else {}))
    gen = torch.Generator(device=dev).manual_seed(1)
    seqs = [(f"s{i}", a.prompt_len) for i in range(batch)]
    if a.synthetic_kv:
        shape = (1, cfg.num_key_value_heads, a.prompt_len, cfg.head_dim)
        kv = [tuple(torch.randn(shape, device=dev, generator=gen).to(torch.bfloat16) for _ in range(2))
              for _ in range(cfg.num_hidden_layers)]
        for s, _ in seqs:
            import_session_kv(ex.sessions, s, kv)
            ex.sessions.release(ex.sessions.get(s))  # (rolling window: the pages no later query sees)
        del kv
        tok = torch.randint(0, cfg.vocab_size, (batch,), device=dev, generator=gen)
    else:
        ids = torch.randint(0, cfg.vocab_size, (batch * a.prompt_len,), device=dev, generator=gen)
        logits = ex.forward(seqs, ids, reset=[True] * batch)
        tok = torch.argmax(logits.float(), -1)
    step = [(s, 1) for s, _ in seqs]

    def one(tok):
        return torch.argmax(ex.forward(step, tok).float(), -1)

    for _ in range(a.warmup):
        tok = one(tok)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            tok = one(tok)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.steps)
    path = "w4a16" if ex._w4 else ("w8a16" if ex._w8 else "bf16")
    held = max(len(ex.sessions.get(s).pages) for s, _ in seqs)
    page_bytes = ex.cache.page_size * cfg.num_hidden_layers * cfg.kv_bytes_per_token_per_layer(2, kv_dtype)
    row = {"model": cfg.name, "quant_type": quant, "kv_cache_dtype": kv_dtype, "synthetic_kv": bool(a.synthetic_kv),
           "sliding_window": ex.sliding_window, "window": ex.window, "context": ex.sessions.get(seqs[0][0]).length,
           "pages_held_per_session": held, "kv_mib_held_per_session": round(held * page_bytes / 2 ** 20, 1),
           "graphs": len(ex._graphs),
           "batch": batch, "prompt_len": a.prompt_len, "steps": a.steps,
           "windows": a.windows, "ms_per_step": round(statistics.median(ms), 4), "min": round(min(ms), 4),
           "max": round(max(ms), 4), "path": path, "fused_norm": bool(ex._fused),
           "weight_gib": round(w.nbytes() / 2 ** 30, 3)}
    del ex, w
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--quants", default="none,fp8,mxfp4")
    ap.add_argument("--prompt_len", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kv_cache_dtype", default="bf16", help="comma-separated: bf16, fp8")
    ap.add_argument("--synthetic_kv", action="store_true")
    ap.add_argument("--sliding_window", default="cap", choices=["cap", "attend"])
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps must be at least 20")
    ops.require_native()
    dev = torch.device("cuda:0")
    cfg = resolve_model(a.model)
    for quant in a.quants.split(","):
        for batch in [int(b) for b in a.batches.split(",")]:
            for kvd in a.kv_cache_dtype.split(","):
                print(json.dumps(run_case(cfg, quant, batch, a, dev, kvd)), flush=True)


if __name__ == "__main__":
    with torch.no_grad():
        main()
