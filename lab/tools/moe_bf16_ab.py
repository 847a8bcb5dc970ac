"""A/B of one Mixtral MoE layer's expert GEMMs over unquantized (bf16) weights: the two grouped launches
(ops.moe_gate_up + ops.moe_down, MPAMD_MOE_GROUPED_BF16=1) against the loop ``StageExecutor._moe_mlp`` runs
by default - ``zero_``, E x (``ops.linear`` gate/up + SwiGLU, ``ops.linear`` down, ``addcmul_``), ``copy_``,
the GEMMs gated on the device by the routed-token counts while T k <= 2 E, on the kernels the committed
table picks.  Mixtral-8x7B shapes by default (H 4096, F 14336, E 8, top-2), M = 1, 16, 64; the weights rotate
over ``--copies`` layer copies (2.82 GB each: far more than the 256 MB Infinity Cache), the two forms alternate
round by round, min..max over the rounds is printed.

    python lab/tools/moe_bf16_ab.py [--rounds 5] [--iters 20] [--out FILE.json]
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
    ops.load_kernel_table()  # the loop's GEMMs on the kernels an executor would run

    def stack(N, K):  # already in the packed order: timing only
        return (0.02 * torch.randn(E, N // 16, K // 32, 64, 8, device=dev, generator=g)).to(torch.bfloat16)

    layers = [(stack(2 * F, H), stack(H, F)) for _ in range(a.copies)]
    layer_bytes = 2 * E * 3 * H * F
    rows_out = []
    for M in [int(m) for m in a.rows.split(",")]:
        assert ops.moe_ok(M, E, H, F)
        xp = ops.pack_act(torch.randn(M, H, device=dev, generator=g).to(torch.bfloat16))
        wd = moe.dense_weights(*moe.route(torch.randn(M, E, device=dev, generator=g), k), E)
        cnt = (wd > 0).sum(0, dtype=torch.int32)
        routed = int((cnt > 0).sum())
        gated = M * k <= 2 * E
        slab = ops.packed_numel(M, F)
        act = torch.zeros(E * slab, dtype=torch.bfloat16, device=dev)
        y = torch.empty(M, H, dtype=torch.bfloat16, device=dev)
        y1 = torch.zeros(M, H, dtype=torch.bfloat16, device=dev)
        acc = torch.empty(M, H, dtype=torch.float32, device=dev)

        def grouped(i):
            gup, dnp = layers[i % a.copies]
            ops.moe_gate_up(xp, gup, cnt, M, out=act)
            ops.moe_down(act, dnp, cnt, wd, M, out=y)

        def looped(i):
            gup, dnp = layers[i % a.copies]
            acc.zero_()
            for e in range(E):
                gate = cnt[e:e + 1] if gated else None
                ops.linear(xp, None, out=act[:slab], epilogue=1, wp=gup[e], a_rows=M, out_packed=True, gate=gate)
                ops.linear(act[:slab], None, out=y1, wp=dnp[e], a_rows=M, gate=gate)
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
        lb = gb if gated else layer_bytes  # the gated loop skips unrouted experts too
        row = {"M": M, "routed": routed, "experts": E, "loop_gated": gated,
               "grouped_us": [min(t["grouped"]), max(t["grouped"])], "looped_us": [min(t["looped"]), max(t["looped"])],
               "grouped_bytes": gb, "looped_bytes": lb,
               "grouped_TBps": [gb / max(t["grouped"]) / 1e6, gb / min(t["grouped"]) / 1e6],
               "looped_TBps": [lb / max(t["looped"]) / 1e6, lb / min(t["looped"]) / 1e6],
               "grouped_slowest_beats_looped_fastest": max(t["grouped"]) < min(t["looped"])}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
