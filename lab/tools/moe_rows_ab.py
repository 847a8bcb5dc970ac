"""A/B of one Mixtral MoE layer's expert MLP over fp8 weights ABOVE 64 rows: the three row-gathered
launches (ops.moe_group + moe_gate_up_w8_rows + moe_down_w8_rows), the tiled launches for large steps
(ops.moe_group + moe_gate_up_w8_tiled + moe_down_w8_tiled: gemm_moe_tiled.hip), their W8A8-MX form
(moe_gate_up_mx_tiled + moe_down_mx_tiled: gemm_moe_tiled_mx.hip) and the dequantizing schedule they replace (StageExecutor._moe_mlp: argsort + bincount().tolist(), then per routed expert two
``ops.unpack_weight_w8``, ``index_select``, two ``ops.linear`` and an ``index_add_``, the bf16 copy).
Mixtral-8x7B shapes by default (H 4096, F 14336, E 8, top-2), T = 65 .. 2048 (the tiled launches take T >=
65); the weights rotate over ``--copies`` layer copies (1.41 GB each: far more than the 256 MB Infinity
Cache), the forms (``--forms``) alternate round by round, min..max over the rounds is printed.  ``mx_quant_us``: the MX
form's two quantizer launches alone (their share of ``tiled_mx_us``); ``mx_wins``: the MX form's slowest round
beats the W8A16 tiled form's fastest.  ``rows_bytes``: the
fp8 bytes the row-gathered launches stream - an expert with c rows streams its 3 H F bytes ceil(c / 64)
times.  ``tiled_PFLOPs``: 6 T k H F / time.  ``tiled_wins``: its slowest round beats both others' fastest.

    python lab/tools/moe_rows_ab.py [--rows 65,128,...] [--rounds 5] [--iters 10] [--out FILE.json]
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
    ap.add_argument("--rows", default="65,128,256,512,1024,2048")
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--forms", default="rows,tiled,tiled_mx,dequant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    H, F, E, k = a.hidden, a.inter, a.experts, a.topk
    g = torch.Generator(device=dev).manual_seed(0)
    ops.use_tuned_gemms()
    layers = []
    for _ in range(a.copies):  # random e4m3 codes (no NaN code), small scales: timing only
        layers.append((torch.randint(0, 0x77, (E, 2 * F // 16, H // 32, 64, 8), dtype=torch.uint8, device=dev, generator=g),
                       torch.full((E, 2 * F), 1e-3, device=dev),
                       torch.randint(0, 0x77, (E, H // 16, F // 32, 64, 8), dtype=torch.uint8, device=dev, generator=g),
                       torch.full((E, H), 1e-3, device=dev)))
    rows_out = []
    for T in [int(m) for m in a.rows.split(",")]:
        forms = a.forms.split(",")
        assert ("rows" not in forms or ops.moe_rows_ok(T, E, k, H, F)) and ops.moe_tiled_ok(T, E, k, H, F)
        x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
        w, idx = moe.route(torch.randn(T, E, device=dev, generator=g), k)
        counts = torch.bincount(idx.reshape(-1), minlength=E).tolist()
        act = torch.empty(T * k, F, dtype=torch.bfloat16, device=dev)
        y = torch.empty(T, H, dtype=torch.bfloat16, device=dev)
        acc = torch.empty(T, H, dtype=torch.float32, device=dev)

        def rows(i):
            gu8, gus, dn8, dns = layers[i % a.copies]
            off, tok, wsel = ops.moe_group(idx, w, E)
            ops.moe_gate_up_w8_rows(x, gu8, gus, off, tok, out=act)
            ops.moe_down_w8_rows(act, dn8, dns, off, tok, wsel, T, out=y)

        def tiled(i):
            gu8, gus, dn8, dns = layers[i % a.copies]
            off, tok, wsel = ops.moe_group(idx, w, E)
            ops.moe_gate_up_w8_tiled(x, gu8, gus, off, tok, out=act)
            ops.moe_down_w8_tiled(act, dn8, dns, off, tok, wsel, idx, T, out=y)

        def tiled_mx(i):
            gu8, gus, dn8, dns = layers[i % a.copies]
            off, tok, wsel = ops.moe_group(idx, w, E)
            ops.moe_gate_up_mx_tiled(x, gu8, gus, off, tok, out=act)
            ops.moe_down_mx_tiled(act, dn8, dns, off, tok, wsel, idx, T, out=y)

        off0, tok0, _ = ops.moe_group(idx, w, E)

        def mx_quant(i):  # the MX form's two quantizer launches alone
            ops.moe_quant_mx_tiled(x, off0, tok0)
            ops.moe_quant_mx_tiled(act, off0)

        def dequant(i):
            gu8, gus, dn8, dns = layers[i % a.copies]
            acc.zero_()
            flat = idx.reshape(-1)
            order = torch.argsort(flat, stable=True)
            cnt = torch.bincount(flat, minlength=E).tolist()  # the host sync of the schedule
            tok, wsel, off = order // k, w.reshape(-1)[order], 0
            for j, c in enumerate(cnt):
                if c == 0:
                    continue
                r = tok[off:off + c]
                h = ops.linear(x.index_select(0, r), ops.unpack_weight_w8(gu8[j], gus[j], torch.bfloat16), epilogue=1)
                ye = ops.linear(h, ops.unpack_weight_w8(dn8[j], dns[j], torch.bfloat16))
                acc.index_add_(0, r, ye.float() * wsel[off:off + c].unsqueeze(1))
                off += c
            y.copy_(acc)

        def timed(fn):
            for i in range(2):
                fn(i)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(a.iters):
                fn(i)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e3 / a.iters  # us per layer

        fns = {"rows": rows, "tiled": tiled, "tiled_mx": tiled_mx, "dequant": dequant}
        if "tiled_mx" in forms:
            forms.append("mx_quant")
            fns["mx_quant"] = mx_quant
        t = {f: [] for f in forms}
        for _ in range(a.rounds):  # alternate the forms
            for f in forms:
                t[f].append(timed(fns[f]))
        nbytes = sum(-(-c // 64) for c in counts) * 3 * H * F
        pflops = lambda us: [6.0 * T * k * H * F / max(us) / 1e9, 6.0 * T * k * H * F / min(us) / 1e9]  # noqa: E731
        row = {"T": T, "counts": counts, "rows_bytes": nbytes}
        row.update({f + "_us": [min(v), max(v)] for f, v in t.items()})
        row["tiled_PFLOPs"] = pflops(t["tiled"])
        if "tiled_mx" in forms:
            row["tiled_mx_PFLOPs"] = pflops(t["tiled_mx"])
            row["mx_wins"] = max(t["tiled_mx"]) < min(t["tiled"])
        others = [u for f in ("rows", "dequant") if f in forms for u in t[f]]
        if others:
            row["tiled_wins"] = max(t["tiled"]) < min(others)
        if "rows" in forms:
            row["rows_TBps"] = [nbytes / max(t["rows"]) / 1e6, nbytes / min(t["rows"]) / 1e6]
            if "dequant" in forms:
                row["wins"] = max(t["rows"]) < min(t["dequant"])
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
