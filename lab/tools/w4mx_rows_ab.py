"""A/B of one MXFP4 projection ABOVE 64 rows in three forms: ``ops.linear_w4mx_rows`` (the natural-block activation
quantizer + the W4A8-MX GEMM on the block-scaled MFMA, csrc/gemm_w4mx_rows.hip), ``ops.linear_w4_rows`` (W4A16:
the same codes read in place but converted to bf16) and ``ops.unpack_weight_w4`` + ``ops.linear`` (the HIP
dequantizer + the library GEMM, the default schedule).  Default shapes: the four Llama-2-7B and the four
Llama-3-70B projections; T = 65 .. 8192.  w4_rows_ab.py's protocol: each shape's weights rotate over enough
copies to pass ``--rotate-gib`` (far more than the 256 MB Infinity Cache), the forms alternate round by round
and min..max over the rounds is printed, in us per call (device events around a window that ends in a
synchronise).  A timed window holds at least ``--iters`` calls and as many more as ``--window-ms`` of the
fastest form's pilot time needs.  The quantizer launch alone is timed in the same rounds (``quant_us``), so
``w4mx_us`` - ``quant_us`` is the GEMM launch.  Before timing, the outputs on the first copy are compared:
W4A16 against dequantize (``rel_w4``, summation order and the last rounding only: the run stops above 1e-2)
and W4A8-MX against W4A16 (``rel_w4mx``: the e4m3 activation blocks, a few percent; the run stops above 0.1).

    python lab/tools/w4mx_rows_ab.py [--shapes N:K:epi,...] [--rows 65,256,...] [--rounds 5] [--iters 5] [--window-ms 20] [--out F.jsonl]
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
FORMS = ("w4mx", "w4", "dequant", "quant")


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
    ap.add_argument("--rows", default="65,256,1024,4096,8192")
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
        wbytes = N * K // 2 + N * K // 32
        copies = max(2, -(-int(a.rotate_gib * (1 << 30)) // wbytes))
        # random codes (every e2m1 code is finite) x 2^-15 .. 2^-8: timing only
        ws = [(torch.randint(0, 256, (N // 16, K // 128, 64, 16), dtype=torch.uint8, device=dev, generator=g),
               torch.randint(112, 120, (N // 16, K // 128, 16, 4), dtype=torch.uint8, device=dev, generator=g))
              for _ in range(copies)]
        nc = N // 2 if epi else N
        for T in [int(m) for m in a.rows.split(",")]:
            assert ops.w4mx_rows_ok(T, N, K, epi) and ops.w4_rows_ok(T, N, K, epi)
            x = torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(T, nc, dtype=torch.bfloat16, device=dev)
            axn, asn = ops.mx_rows_buffers(T, K, dev)
            fns = {"w4mx": lambda i: ops.linear_w4mx_rows(x, *ws[i % copies], out=y, epilogue=epi),
                   "w4": lambda i: ops.linear_w4_rows(x, *ws[i % copies], out=y, epilogue=epi),
                   "dequant": lambda i: ops.linear(x, ops.unpack_weight_w4(*ws[i % copies]), out=y, epilogue=epi),
                   "quant": lambda i: ops.quant_mxn_rows(x, axn, asn)}
            got = {}
            for k in ("w4mx", "w4", "dequant"):
                fns[k](0)
                got[k] = y.float()
            rel_w4 = float((got["w4"] - got["dequant"]).norm() / got["dequant"].norm())
            rel_w4mx = float((got["w4mx"] - got["w4"]).norm() / got["w4"].norm())
            assert rel_w4 < 1e-2 and rel_w4mx < 0.1, f"the forms disagree at N={N} K={K} T={T}: {rel_w4} {rel_w4mx}"
            del got
            pilot = min(timed(fns[k], 3) for k in ("w4mx", "w4", "dequant"))  # us: the fastest form sets the count
            iters = max(a.iters, min(400, int(a.window_ms * 1e3 / pilot) + 1))
            t = {k: [] for k in FORMS}
            for _ in range(a.rounds):  # alternate the forms
                for k in FORMS:
                    t[k].append(timed(fns[k], iters))
            flops = 2 * T * N * K
            row = {"N": N, "K": K, "epilogue": epi, "T": T, "copies": copies, "iters": iters, "rel_w4": rel_w4,
                   "rel_w4mx": rel_w4mx, "flops": flops}
            row.update({k + "_us": [min(v), max(v)] for k, v in t.items()})
            row["w4mx_TFLOPs"] = [flops / max(t["w4mx"]) / 1e6, flops / min(t["w4mx"]) / 1e6]
            row["w4_TFLOPs"] = [flops / max(t["w4"]) / 1e6, flops / min(t["w4"]) / 1e6]
            row["beats_w4"] = max(t["w4mx"]) < min(t["w4"])
            row["beats_dequant"] = max(t["w4mx"]) < min(t["dequant"])
            print(json.dumps(row), flush=True)
            if out:
                out.write(json.dumps(row) + "\n")
                out.flush()
        del ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
