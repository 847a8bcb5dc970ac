"""A/B of one projection's LoRA update ABOVE 64 rows: ``ops.lora_update_rows`` (the two segmented MFMA kernels,
slots read on the device) against the form it replaces in ``StageExecutor._layers_dense`` - ``ops.lora_update``,
the torch loop over runs of equal slot.  Default shapes: the four Llama-2-7B projections with r = 16 on all
seven modules (stacked ranks: qkv 48, o 16, gate_up 32, down 16); T = 65 .. 8192; two slot layouts per row count:
``one`` - one adapter for the whole step - and ``s64`` - 64 sessions' worth of runs (T rows cut into 64 runs as
evenly as rows allow) over four adapters plus base rows.  The stacks, x and y of a shape rotate over enough copies
to pass ``--rotate-gib`` (far more than the 256 MB Infinity Cache), the two forms alternate round by round and
min..max over the rounds is printed.  A timed window holds at least ``--iters`` calls and as many more as
``--window-ms`` of the faster form's pilot time needs.  Before timing, the two forms' results on the first copy are
compared on a zeroed y (``rel_fro`` of the update itself: the forms differ in summation order only, t stays
fp32 in both, so what is left is the one rounding to bf16) and the run stops if they are further apart than 1e-2.
Per row: the bytes the kernels must move at least (x once, y twice, t twice, the named stacks once) and the rate
their slowest / fastest round reached.  The last line is the default that follows: the largest T at which the
kernels' slowest round beats the torch form's fastest on every row of that T and of every smaller one, or 0.

    python lab/tools/lora_rows_ab.py [--shapes N:K:R,...] [--rows 65,128,...] [--rounds 5] [--iters 5] [--window-ms 20] [--out F.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from src import ops  # noqa: E402

SHAPES = "12288:4096:48,4096:4096:16,22016:4096:32,4096:11008:16"
S = 4


def layout(T, kind):
    """Host slots of a T-row step."""
    if kind == "one":
        return [0] * T
    sl = []
    for i in range(64):  # session i owns rows [i T / 64, (i + 1) T / 64)
        sl += [(0, 1, 2, 3, -1)[i % 5]] * ((i + 1) * T // 64 - i * T // 64)
    return sl


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--rows", default="65,128,512,2048,8192")
    ap.add_argument("--rotate-gib", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    scale = torch.tensor([2.0, 0.5, 1.0, 1.5], device=dev)
    rows_out = []
    for N, K, R in [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]:
        for T in [int(m) for m in a.rows.split(",")]:
            assert ops.lora_rows_ok(T, N, K, R)
            per = 2 * (S * R * (K + N) + T * (K + N))
            copies = max(2, min(64, -(-int(a.rotate_gib * (1 << 30)) // per)))
            sets = [((torch.randn(S, R, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16),
                     (torch.randn(S, N, R, device=dev, generator=g) * 1e-2).to(torch.bfloat16),
                     torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16),
                     torch.randn(T, N, device=dev, generator=g).to(torch.bfloat16)) for _ in range(copies)]
            t = torch.empty(T, R, device=dev)
            for kind in ("one", "s64"):
                host = layout(T, kind)
                runs = ops.lora_runs(host)
                slots = torch.tensor(host, dtype=torch.int32, device=dev)

                def kernels(i):
                    A, B, x, y = sets[i % copies]
                    ops.lora_update_rows(x, y, A, B, scale, slots, t=t)

                def torch_runs(i):
                    A, B, x, y = sets[i % copies]
                    ops.lora_update(x, y, A, B, scale, runs)

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

                A, B, x, y = sets[0]
                y0 = y.clone()
                y.zero_()
                kernels(0)
                got = y.float()
                y.zero_()
                torch_runs(0)
                want = y.float()
                y.copy_(y0)
                rel = float((got - want).norm() / want.norm())
                assert rel < 1e-2, f"the two forms disagree at N={N} K={K} R={R} T={T} {kind}: rel fro {rel}"
                pilot = min(timed(kernels, 3), timed(torch_runs, 3))  # us: the faster form sets the call count
                iters = max(a.iters, min(400, int(a.window_ms * 1e3 / pilot) + 1))
                tm = {"kernels": [], "torch": []}
                for _ in range(a.rounds):  # alternate the two forms
                    tm["kernels"].append(timed(kernels, iters))
                    tm["torch"].append(timed(torch_runs, iters))
                live = sum(1 for s in host if s >= 0)
                named = len(set(s for s in host if s >= 0))
                nbytes = 2 * live * K + 4 * live * N + 8 * live * R + 2 * named * R * (K + N)
                lo, hi = min(tm["kernels"]), max(tm["kernels"])
                row = {"N": N, "K": K, "R": R, "T": T, "layout": kind, "runs": len(runs), "copies": copies,
                       "iters": iters, "rel_fro": rel, "kernels_us": [lo, hi],
                       "torch_us": [min(tm["torch"]), max(tm["torch"])], "bytes": nbytes,
                       "kernels_TBps": [nbytes / hi / 1e6, nbytes / lo / 1e6], "wins": hi < min(tm["torch"])}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
            del sets
            torch.cuda.empty_cache()
    default = 0
    for T in sorted(set(r["T"] for r in rows_out)):
        if not all(r["wins"] for r in rows_out if r["T"] == T):
            break
        default = T
    print(json.dumps({"MPAMD_LORA_ROWS": default}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows_out)
            f.write(json.dumps({"MPAMD_LORA_ROWS": default}) + "\n")


if __name__ == "__main__":
    main()
