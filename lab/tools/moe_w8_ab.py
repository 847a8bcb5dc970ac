"""A/B of one Mixtral MoE layer's expert GEMMs over fp8 weights: the two grouped launches
(ops.moe_gate_up_w8 + ops.moe_down_w8) against 2 E ``ops.linear_w8`` launches + E ``addcmul_`` + the
bf16 copy (what MPAMD_MOE_GROUPED=0 runs).  Mixtral-8x7B shapes by default (H 4096, F 14336, E 8, top-2),
M = 1, 16, 64; the weights rotate over ``--copies`` layer copies (1.41 GB each: far more than the 256 MB
Infinity Cache), the two forms alternate round by round, min..max over the rounds is printed.

    python lab/tools/moe_w8_ab.py [--rounds 5] [--iters 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402
from src.ops import moe  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--topk", type=int, default=2)
    ap.add_argument("--rows", default="1,16,64")
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    H, F, E, k = a.hidden, a.inter, a.experts, a.topk
    g = torch.Generator(device=dev).manual_seed(0)
    ops._W8_MODE = "rw"
    layers = []
    for _ in range(a.copies):  # random e4m3 codes (no NaN code), unit-ish scales: timing only
        layers.append((torch.randint(0, 0x77, (E, 2 * F // 16, H // 32, 64, 8), dtype=torch.uint8, device=dev, generator=g),
                       torch.full((E, 2 * F), 1e-3, device=dev),
                       torch.randint(0, 0x77, (E, H // 16, F // 32, 64, 8), dtype=torch.uint8, device=dev, generator=g),
                       torch.full((E, H), 1e-3, device=dev)))
    layer_bytes = E * 3 * H * F
    rows_out = []
    for M in [int(m) for m in a.rows.split(",")]:
        assert ops.moe_w8_ok(M, E, H, F)
        xp = ops.pack_act(torch.randn(M, H, device=dev, generator=g).to(torch.bfloat16))
        wd = moe.dense_weights(*moe.route(torch.randn(M, E, device=dev, generator=g), k), E)
        cnt = (wd > 0).sum(0, dtype=torch.int32)
        routed = int((cnt > 0).sum())
        slab = ops.packed_numel(M, F)
        act = torch.zeros(E * slab, dtype=torch.bfloat16, device=dev)
        y = torch.empty(M, H, dtype=torch.bfloat16, device=dev)
        y1 = torch.empty(M, H, dtype=torch.bfloat16, device=dev)
        acc = torch.empty(M, H, dtype=torch.float32, device=dev)

        def grouped(i):
            gu8, gus, dn8, dns = layers[i % a.copies]
            ops.moe_gate_up_w8(xp, gu8, gus, cnt, M, out=act)
            ops.moe_down_w8(act, dn8, dns, cnt, wd, M, out=y)

        def looped(i):
            gu8, gus, dn8, dns = layers[i % a.copies]
            acc.zero_()
            for e in range(E):
                ops.linear_w8(xp, gu8[e], gus[e], M, out=act[:slab], epilogue=1, out_packed=True)
                ops.linear_w8(act[:slab], dn8[e], dns[e], M, out=y1)
                acc.addcmul_(y1, wd[:, e:e + 1])
            y.copy_(acc)

        def timed(fn):
            for i in range(3):
                fn(i)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(a.iters):
                fn(i)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e3 / a.iters  # us per layer

        t = {"grouped": [], "looped": []}
        for _ in range(a.rounds):  # alternate the two forms
            t["grouped"].append(timed(grouped))
            t["looped"].append(timed(looped))
        gb = layer_bytes * routed / E  # bytes the grouped launches stream (routed experts only)
        row = {"M": M, "routed": routed, "experts": E,
               "grouped_us": [min(t["grouped"]), max(t["grouped"])], "looped_us": [min(t["looped"]), max(t["looped"])],
               "grouped_bytes": gb, "looped_bytes": layer_bytes,
               "grouped_TBps": [gb / max(t["grouped"]) / 1e6, gb / min(t["grouped"]) / 1e6],
               "looped_TBps": [layer_bytes / max(t["looped"]) / 1e6, layer_bytes / min(t["looped"]) / 1e6]}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
