"""A/B of one fp8 projection ABOVE 64 rows in three forms: ``ops.linear_mx_rows`` (the activation quantizer +
the W8A8-MX GEMM on the block-scaled MFMA, csrc/gemm_mx_rows.hip), ``ops.linear_w8_rows`` (W8A16, the same
weights read in place but multiplied in bf16) and ``ops.unpack_weight_w8`` + ``ops.linear`` (dequantize + the
library GEMM).  Default shapes: the four Llama-3-70B and the four Llama-2-7B projections; T = 65 .. 16384.
Each shape's weights rotate over enough copies to pass ``--rotate-gib`` (far more than the 256 MB Infinity
Cache), the forms alternate round by round and min..max over the rounds is printed, in us per call (device
events around a window that ends in a synchronise).  A timed window holds at least ``--iters`` calls and as
many more as ``--window-ms`` of the fastest form's pilot time needs.  The quantizer launch alone is timed in
the same rounds (``quant_us``), so ``mx_us`` - ``quant_us`` is the GEMM launch.  Before timing, the outputs
on the first copy are compared: W8A16 against dequantize (``rel_w8``, bf16 roundings only: the run stops
above 1e-2) and MX against W8A16 (``rel_mx``: the e4m3 activation blocks, a few percent; the run stops above
0.1).  Per row: the MX form's FLOPs and the rate its slowest / fastest round reached on them.

    python lab/tools/mx_rows_ab.py [--shapes N:K:epi,...] [--rows 65,1024,...] [--rounds 5] [--iters 5] [--window-ms 20] [--out F.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

SHAPES = ("10240:8192:0,8192:8192:0,57344:8192:1,8192:28672:0,"  # Llama-3-70B qkv, o, gate/up, down
          "12288:4096:0,4096:4096:0,22016:4096:1,4096:11008:0")  # Llama-2-7B
FORMS = ("mx", "w8", "dequant", "quant")


def timed(fn, iters):
    for i in range(2):
        fn(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--rows", default="65,1024,4096,8192,16384")
    ap.add_argument("--rotate-gib", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    ops.use_tuned_gemms()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")
    for N, K, epi in [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]:
        copies = max(2, -(-int(a.rotate_gib * (1 << 30)) // (N * K)))
        ws = [(torch.randint(0, 0x77, (N // 16, K // 32, 64, 8), dtype=torch.uint8, device=dev, generator=g),
               torch.full((N,), 1e-3, device=dev)) for _ in range(copies)]  # random codes (no NaN): timing only
        nc = N // 2 if epi else N
        for T in [int(m) for m in a.rows.split(",")]:
            assert ops.mx_rows_ok(T, N, K, epi) and ops.w8_rows_ok(T, N, K, epi)
            x = torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(T, nc, dtype=torch.bfloat16, device=dev)
            ax, as_ = ops.mx_rows_buffers(T, K, dev)
            fns = {"mx": lambda i: ops.linear_mx_rows(x, *ws[i % copies], out=y, epilogue=epi),
                   "w8": lambda i: ops.linear_w8_rows(x, *ws[i % copies], out=y, epilogue=epi),
                   "dequant": lambda i: ops.linear(x, ops.unpack_weight_w8(*ws[i % copies]), out=y, epilogue=epi),
                   "quant": lambda i: ops.quant_mx_rows(x, ax, as_)}
            got = {}
            for k in ("mx", "w8", "dequant"):
                fns[k](0)
                got[k] = y.float()
            rel_w8 = float((got["w8"] - got["dequant"]).norm() / got["dequant"].norm())
            rel_mx = float((got["mx"] - got["w8"]).norm() / got["w8"].norm())
            assert rel_w8 < 1e-2 and rel_mx < 0.1, f"the forms disagree at N={N} K={K} T={T}: {rel_w8} {rel_mx}"
            del got
            pilot = min(timed(fns[k], 3) for k in ("mx", "w8", "dequant"))  # us: the fastest form sets the count
            iters = max(a.iters, min(400, int(a.window_ms * 1e3 / pilot) + 1))
            t = {k: [] for k in FORMS}
            for _ in range(a.rounds):  # alternate the forms
                for k in FORMS:
                    t[k].append(timed(fns[k], iters))
            flops = 2 * T * N * K
            row = {"N": N, "K": K, "epilogue": epi, "T": T, "copies": copies, "iters": iters, "rel_w8": rel_w8,
                   "rel_mx": rel_mx, "flops": flops}
            row.update({k + "_us": [min(v), max(v)] for k, v in t.items()})
            row["mx_TFLOPs"] = [flops / max(t["mx"]) / 1e6, flops / min(t["mx"]) / 1e6]
            row["w8_TFLOPs"] = [flops / max(t["w8"]) / 1e6, flops / min(t["w8"]) / 1e6]
            row["beats_w8"] = max(t["mx"]) < min(t["w8"])
            row["beats_dequant"] = max(t["mx"]) < min(t["dequant"])
            print(json.dumps(row), flush=True)
            if out:
                out.write(json.dumps(row) + "\n")
                out.flush()
        del ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
