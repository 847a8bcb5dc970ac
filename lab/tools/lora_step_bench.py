#!/usr/bin/env python3
"""Whole-stage cost of LoRA decode steps: a full Llama-2-7B stage (synthetic weights, embedding and
head included), graph-replayed decode steps at 1 and 64 sessions, ms per step for

    none     no adapter loaded (the stage's default step; with MPAMD_FUSED_NORM=0 in the environment,
             the packed path a LoRA step builds on)
    qv       one adapter on q_proj, v_proj (r = 16), every session on it
    all7     one adapter on all seven modules (r = 16), every session on it
    mixed4   four adapters (two on q, v, two on all seven), sessions cycle over them and the base model

Each case builds its own executor over the same weights (the adapters of a case are the only ones
loaded: the fused ranks, and so the launches, are that case's).  ``--repo DIR`` imports the package
from another checkout (a build of the parent commit: only ``none`` exists there); run the two
alternately in one GPU session.  One JSON line per (case, sessions).

    python lab/tools/lora_step_bench.py --cases none,qv,all7,mixed4 --sessions 1,64
    MPAMD_FUSED_NORM=0 python lab/tools/lora_step_bench.py --repo _build_parent --cases none
"""
import argparse
import json
import os
import sys

import torch

ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
CASES = {
    "none": ([], [""]),
    "qv": (["synthetic:qv:16"], ["qv"]),
    "all7": ([f"synthetic:all7:16:{ALL7}"], ["all7"]),
    "mixed4": (["synthetic:m0:16", "synthetic:m1:16", f"synthetic:m2:16:{ALL7}", f"synthetic:m3:16:{ALL7}"],
               ["m0", "m1", "m2", "m3", ""]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--cases", default="none,qv,all7,mixed4")
    ap.add_argument("--sessions", default="1,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))
    os.environ.setdefault("MPAMD_GEMM_AUTOTUNE", "0")  # the committed kernel table, no timing race
    from src.models.config import resolve_model
    from src.models.weights import random_stage_weights
    from src.runtime.executor import StageExecutor

    dev = torch.device("cuda")
    cfg = resolve_model(a.model)
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=dev)
    for case in a.cases.split(","):
        specs, cycle = CASES[case]
        if hasattr(w, "lora"):
            w.lora = None  # (a lab tool: a served stage loads its adapters once)
        if specs:
            w.load_adapters(specs)
        ex = StageExecutor(cfg, w, dev, kv_cache_bytes=16 << 30, max_sessions=64, max_seq_len=1024, warmup=False)
        for n in (int(s) for s in a.sessions.split(",")):
            sids = [f"s{i}" for i in range(n)]
            kw = {"adapters": [cycle[i % len(cycle)] for i in range(n)]} if specs else {}
            g = torch.Generator(device=dev).manual_seed(1)
            with torch.no_grad():
                ids = torch.randint(0, cfg.vocab_size, (n * a.prompt,), device=dev, generator=g)
                lg = ex.forward([(s, a.prompt) for s in sids], ids, reset=[True] * n, **kw)
                tok = torch.argmax(lg.float(), -1)
                for _ in range(a.warm):
                    tok = torch.argmax(ex.forward([(s, 1) for s in sids], tok, **kw).float(), -1)
                graphed = bool(ex.last_graphed)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    tok = torch.argmax(ex.forward([(s, 1) for s in sids], tok, **kw).float(), -1)
                e1.record()
                e1.synchronize()
            for s in sids:
                ex.sessions.close(s)
            print(json.dumps({"tag": a.tag, "case": case, "sessions": n, "graphed": graphed,
                              "fused_norm": os.environ.get("MPAMD_FUSED_NORM", "1"),
                              "ms_per_step": round(e0.elapsed_time(e1) / a.steps, 4)}), flush=True)
        ex.clear_graphs()
        del ex
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
