"""A/B of one W4A16 projection ABOVE 64 rows: ``ops.linear_w4_rows`` (the MXFP4 codes and block scales read in
place) against the schedule it replaces in ``StageExecutor._layers_dense`` - ``ops.unpack_weight_w4`` (the HIP
dequantizer's bf16 copy of the whole projection) plus ``ops.linear`` on the result, timed together.  Default
shapes: the four projections of Llama-2-7B and of Llama-3-70B; T = 65 .. 8192.  Each shape's weights rotate
over enough copies to pass ``--rotate-gib`` (far more than the 256 MB Infinity Cache), the two forms alternate
round by round and min..max over the rounds is printed.  A timed window holds at least ``--iters`` calls and
as many more as ``--window-ms`` of the faster form's pilot time needs, so that short kernels are not timed by
their enqueue.  Before timing, the two forms' outputs on the first copy are compared (``rel_fro``: relative
Frobenius distance; both multiply the same exact bf16 weight values, so they differ by the summation order
and the last rounding only) and the run stops if they are further apart than 1e-2.  Per row: the bytes the
new kernel must stream at least (codes + scales once, x, y), its FLOPs, and the rate its slowest / fastest
round reached on each.

    python lab/tools/w4_rows_ab.py [--shapes N:K:epi,...] [--rows 65,128,...] [--rounds 5] [--iters 5] [--window-ms 20] [--out F.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

SHAPES = ("12288:4096:0,4096:4096:0,22016:4096:1,4096:11008:0,"      # Llama-2-7B qkv, o, gate/up, down
          "10240:8192:0,8192:8192:0,57344:8192:1,8192:28672:0")      # Llama-3-70B


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--rows", default="65,128,256,1024,4096,8192")
    ap.add_argument("--rotate-gib", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    ops.use_tuned_gemms()
    rows_out = []
    for N, K, epi in [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]:
        wbytes = N * K // 2 + N * K // 32
        copies = max(2, -(-int(a.rotate_gib * (1 << 30)) // wbytes))
        # random codes (every e2m1 code is finite) x 2^-15 .. 2^-8: timing only
        ws = [(torch.randint(0, 256, (N // 16, K // 128, 64, 16), dtype=torch.uint8, device=dev, generator=g),
               torch.randint(112, 120, (N // 16, K // 128, 16, 4), dtype=torch.uint8, device=dev, generator=g))
              for _ in range(copies)]
        nc = N // 2 if epi else N
        for T in [int(m) for m in a.rows.split(",")]:
            assert ops.w4_rows_ok(T, N, K, epi)
            x = torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(T, nc, dtype=torch.bfloat16, device=dev)

            def inplace(i):
                ops.linear_w4_rows(x, *ws[i % copies], out=y, epilogue=epi)

            def dequant(i):
                ops.linear(x, ops.unpack_weight_w4(*ws[i % copies]), out=y, epilogue=epi)

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

            inplace(0)
            got = y.float()
            dequant(0)
            rel = float((got - y.float()).norm() / y.float().norm())
            assert rel < 1e-2, f"the two forms disagree at N={N} K={K} T={T}: rel fro {rel}"
            pilot = min(timed(inplace, 3), timed(dequant, 3))  # us: the faster form sets the call count
            iters = max(a.iters, min(400, int(a.window_ms * 1e3 / pilot) + 1))

            t = {"inplace": [], "dequant": []}
            for _ in range(a.rounds):  # alternate the two forms
                t["inplace"].append(timed(inplace, iters))
                t["dequant"].append(timed(dequant, iters))
            nbytes, flops = wbytes + 2 * T * K + 2 * T * nc, 2 * T * N * K
            lo, hi = min(t["inplace"]), max(t["inplace"])
            row = {"N": N, "K": K, "epilogue": epi, "T": T, "copies": copies, "iters": iters, "rel_fro": rel,
                   "inplace_us": [lo, hi],
                   "dequant_us": [min(t["dequant"]), max(t["dequant"])], "bytes": nbytes, "flops": flops,
                   "inplace_TBps": [nbytes / hi / 1e6, nbytes / lo / 1e6],
                   "inplace_TFLOPs": [flops / hi / 1e6, flops / lo / 1e6], "wins": hi < min(t["dequant"])}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        del ws
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows_out)


if __name__ == "__main__":
    main()
