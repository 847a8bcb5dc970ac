#!/usr/bin/env python3
"""The batched LoRA kernels alone (ops.lora_shrink + ops.lora_expand, csrc/lora.hip) next to the bf16
decode GEMM of the same projection, at the Llama-2-7B shapes, under decode conditions: the adapter
stacks and the packed weights each rotate over ~1 GiB of copies, so neither L2 nor the Infinity
Cache serves them.  Per projection, row count M and number of distinct adapters among the rows
(row m runs adapter m mod D; S = 64 adapters are stacked, r = 16 on all seven modules, i.e. fused
ranks 48 / 16 / 32 / 16): us per shrink + expand pair and us per ``ops.linear`` call with epilogue 0
(the form a LoRA step runs), from the same process.  One JSON line per (projection, M, D).

    python lab/tools/lora_ab.py --ms 1,16,64 --distinct 1,4,64 --repeats 2
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

# name: (N, K, fused rank at r = 16 on every module)
SHAPES = {"7b.qkv": (12288, 4096, 48), "7b.o": (4096, 4096, 16), "7b.gate_up": (22016, 4096, 32),
          "7b.down": (4096, 11008, 16)}
POOL = 1 << 30
S = 64


def _time(fn, iters):
    for i in range(4):
        fn(i)
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        e1.synchronize()
        ts.append(1000 * e0.elapsed_time(e1) / iters)
    return round(min(ts), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="1,16,64")
    ap.add_argument("--distinct", default="1,4,64")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    ops.require_native()
    ops.load_kernel_table()
    dev = torch.device("cuda")
    ops.gemm_workspace(dev)
    for rep in range(a.repeats):
        for name in a.shapes.split(","):
            N, K, R = SHAPES[name]
            nw = max(1, min(8, POOL // (2 * N * K)))
            wps = [ops.pack_weight((0.02 * torch.randn(N, K, device=dev)).to(torch.bfloat16)) for _ in range(nw)]
            ns = max(1, min(8, POOL // (2 * S * R * (N + K))))
            As = [(torch.randn(S, R, K, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(ns)]
            Bs = [(torch.randn(S, N, R, device=dev) * R ** -0.5).to(torch.bfloat16) for _ in range(ns)]
            scale = torch.full((S,), 2.0, device=dev)
            for M in (int(m) for m in a.ms.split(",")):
                xp = ops.pack_act(torch.randn(M, K, device=dev).to(torch.bfloat16))
                y = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
                t = torch.zeros(M, R, device=dev)
                gemm = _time(lambda i: ops.linear(xp, None, out=y, wp=wps[i % nw], a_rows=M), a.iters)
                for D in (int(d) for d in a.distinct.split(",")):
                    sl = (torch.arange(M, device=dev) % min(D, S)).to(torch.int32)

                    def pair(i):
                        ops.lora_shrink(xp, As[i % ns], scale, sl, M, out=t)
                        ops.lora_expand(t, Bs[i % ns], sl, y)

                    print(json.dumps({"shape": name, "N": N, "K": K, "R": R, "M": M, "distinct": min(D, M, S),
                                      "rep": rep, "lora_pair_us": _time(pair, a.iters),
                                      "shrink_us": _time(lambda i: ops.lora_shrink(xp, As[i % ns], scale, sl, M,
                                                                                   out=t), a.iters),
                                      "gemm_bf16_us": gemm}), flush=True)
            del wps, As, Bs


if __name__ == "__main__":
    main()
