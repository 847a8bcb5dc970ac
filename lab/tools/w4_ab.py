#!/usr/bin/env python3
"""W4A16 (MXFP4) vs W8A16 (fp8) vs bf16 decode projections, isolated, under decode conditions (the
weights rotated over ~1 GiB of copies, so neither L2 nor the Infinity Cache serves them): per shape
and row count, us per call of ``ops.linear`` (bf16 packed weights), ``ops.linear_w8`` and
``ops.linear_w4`` with the epilogue the layer uses.  One JSON line per (shape, M); ``--repeats``
runs the whole table that many times (the run-to-run spread of the w8a16 column is the margin a
w4a16 win has to clear).

    python lab/tools/w4_ab.py --ms 1,16,64 --repeats 3
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from src import ops  # noqa: E402
from mx_ab import SHAPES as MX_SHAPES  # noqa: E402

SHAPES = dict(MX_SHAPES)  # name: (N, K, epilogue)
SHAPES.update({"7b.gate_up": (22016, 4096, 1), "70b.gate_up": (57344, 8192, 1)})
POOL = 1 << 30  # bytes of weight copies a label rotates over


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
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    ops.require_native()
    ops.load_kernel_table()
    dev = torch.device("cuda")
    ops.gemm_workspace(dev)
    ms = [int(m) for m in a.ms.split(",")]
    for rep in range(a.repeats):
        for name in a.shapes.split(","):
            N, K, epi = SHAPES[name]
            ncols = N // 2 if epi == 1 else N
            # one weight format resident at a time: each rotates over its own ~1 GiB
            for label in ("bf16", "w8a16", "w4a16"):
                per = N * K * {"bf16": 2, "w8a16": 1, "w4a16": 0.53125}[label]
                copies = max(2, int(POOL // per))
                ws = []
                for _ in range(copies):
                    w = torch.randn(N, K, device=dev) * 0.02
                    if label == "bf16":
                        ws.append((ops.pack_weight(w.to(torch.bfloat16)),))
                    elif label == "w8a16":
                        wq, wsc = ops.pack_weight_fp8(w)
                        ws.append((ops.w8_from_fp8(wq), wsc))
                    else:
                        ws.append(ops.pack_weight_w4(w))
                    del w
                for M in ms:
                    xp = ops.pack_act(torch.randn(M, K, device=dev).to(torch.bfloat16))
                    if epi == 3:
                        out = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
                        ss = ops.norm_stats_buffer(dev, 2)
                        kw = dict(out=out, epilogue=3, residual=out, ss_out=ss[0], ss_zero=ss[1],
                                  ap_out=torch.zeros(ops.packed_numel(M, N), dtype=torch.bfloat16, device=dev))
                    elif epi == 1:
                        kw = dict(out=torch.zeros(ops.packed_numel(M, ncols), dtype=torch.bfloat16, device=dev),
                                  epilogue=1, out_packed=True, ss_in=ops.norm_stats_buffer(dev)[0], eps=1e-5)
                    else:
                        kw = dict(out=torch.zeros(M, N, dtype=torch.bfloat16, device=dev),
                                  ss_in=ops.norm_stats_buffer(dev)[0], eps=1e-5)

                    if label == "bf16":
                        def fn(i):
                            ops.linear(xp, None, wp=ws[i % copies][0], a_rows=M, **kw)
                    elif label == "w8a16":
                        def fn(i):
                            ops.linear_w8(xp, ws[i % copies][0], ws[i % copies][1], M, **kw)
                    else:
                        def fn(i):
                            ops.linear_w4(xp, ws[i % copies][0], ws[i % copies][1], M, **kw)
                    row = {"repeat": rep, "shape": name, "M": M, "N": N, "K": K, "epilogue": epi, "kernel": label,
                           "copies": copies}
                    try:
                        row["us"] = _time(fn, a.iters)
                    except Exception as e:  # noqa: BLE001 - a shape a form does not cover
                        row["us"] = None
                        row["error"] = str(e)[:80]
                    print(json.dumps(row), flush=True)
                del ws
                torch.cuda.empty_cache()


if __name__ == "__main__":
    with torch.no_grad():
        main()
