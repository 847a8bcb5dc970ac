"""Device-dispatching op layer.

GPU tensors go to the hand-written gfx950 HIP kernels (``torch.ops.mpamd.*`` from
``ops/_mpamd_kernels.so``); CPU tensors go to the plain-PyTorch implementations in
``ops.reference``.  There is no silent fallback on the GPU: if the kernel library is
missing on a GPU host the first GPU op raises (``require_native``).

Projection GEMMs (``linear``) are dispatched by shape: decode-sized inputs (M <= 64,
K % 256 == 0) use the native weight-streaming MFMA kernel with fused epilogues;
larger (prefill) GEMMs go to hipBLASLt through ``torch.nn.functional.linear`` plus the
native epilogue kernels.  ``MPAMD_GEMM=native|hipblaslt|auto`` overrides the policy.
"""
from __future__ import annotations

import math
import os
import threading
from functools import partial
from typing import Optional, Tuple

import torch

from . import reference as ref
from .reference import GU_BLOCK, rope_cos_sin  # noqa: F401  (re-export)
from .reference import KVF8, dequant_kv_fp8, fake_quant_kv_fp8, quant_kv_fp8  # noqa: F401  (fp8 KV cache)

_LOCK = threading.Lock()
_LOADED: Optional[bool] = None
_LOAD_ERROR: Optional[str] = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_mpamd_kernels.so")
# an ablation build (``MPAMD_HIPCC_EXTRA=... python -m src.ops.build --out PATH``) is loaded as is
_LIB_OVERRIDE = os.environ.get("MPAMD_KERNEL_LIB")
if _LIB_OVERRIDE:
    LIB_PATH = os.path.abspath(_LIB_OVERRIDE)


def load_library(build_if_missing: bool = True) -> bool:
    """Load (building first if needed and possible) the HIP kernel library."""
    global _LOADED, _LOAD_ERROR
    with _LOCK:
        if _LOADED is not None:
            return _LOADED
        try:
            if build_if_missing and not _LIB_OVERRIDE:
                try:
                    from .build import build

                    build()
                except Exception as e:  # no hipcc / read-only tree: use a prebuilt library if present
                    if not os.path.exists(LIB_PATH):
                        raise
                    _LOAD_ERROR = f"rebuild skipped: {e}"
            torch.ops.load_library(LIB_PATH)
            _LOADED = True
        except Exception as e:  # pragma: no cover - depends on host toolchain
            _LOADED = False
            _LOAD_ERROR = str(e)
        return _LOADED


def native_available() -> bool:
    return load_library()


def require_native() -> None:
    if not load_library():
        raise RuntimeError(
            "mpamd HIP kernels are not available on this GPU host "
            f"({_LOAD_ERROR}); build them with `python -m src.ops.build`")


def _native(t: torch.Tensor) -> bool:
    if t.is_cuda:
        require_native()
        return True
    return False


_GEMM_POLICY = os.environ.get("MPAMD_GEMM", "auto")


def set_gemm_policy(policy: str) -> None:
    global _GEMM_POLICY
    assert policy in ("auto", "native", "hipblaslt")
    _GEMM_POLICY = policy


def gemm_policy() -> str:
    return _GEMM_POLICY


# Library (hipBLASLt / rocBLAS) solutions for the row-major GEMMs - prefill and decode steps above
# 128 rows - picked per shape by PyTorch TunableOp on MI355X (lab/tools/tune_gemms.py; the file's
# validator lines pin the ROCm / hipBLASLt build it was measured on, other builds ignore it).
# Loaded read-only: tuning stays off, shapes not in the file keep the library heuristic.
TUNED_GEMMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gemm_gfx950.csv")
_TUNED_STATE = {"loaded": None}


def use_tuned_gemms(path: Optional[str] = None) -> bool:
    """Turn on TunableOp with the shipped solution table (once per process); False if off
    (``MPAMD_TUNED_GEMMS=0``), no GPU, or the table does not load."""
    if _TUNED_STATE["loaded"] is not None:
        return _TUNED_STATE["loaded"]
    ok = False
    path = path or TUNED_GEMMS
    if os.environ.get("MPAMD_TUNED_GEMMS", "1") != "0" and torch.cuda.is_available() and os.path.exists(path):
        import tempfile

        from torch.cuda import tunable

        try:
            tunable.tuning_enable(False)
            # results are never written back into the package: any output goes to a scratch file
            tunable.set_filename(os.path.join(tempfile.gettempdir(), f"mpamd_tunableop_{os.getpid()}.csv"))
            tunable.enable(True)
            ok = bool(tunable.read_file(path))
            if not ok:
                tunable.enable(False)
        except Exception:  # noqa: BLE001 - a TunableOp-less build: keep the heuristic
            ok = False
    _TUNED_STATE["loaded"] = ok
    return ok


# Decode GEMM kernel choice (gemm.hip): the one-group-per-workgroup kernel or the stream-K
# kernel.  "auto" = per (M bucket, N, K, epilogue) choice measured by ``autotune_gemm`` (the
# executor tunes its own shapes at start-up; untuned shapes use the first kernel); "on" /
# "off" force the stream-K kernel on / off wherever it applies.
_GEMM_SK = "auto"
_GEMM_WS = {}
_SK_CHOICE = {}  # (m_bucket, N, K, epilogue) -> kernel name (see _KERNEL_FLAGS)
# decode-GEMM kernels (csrc/gemm.hip): one-group-per-workgroup, stream-K, and the shared-A (LDS)
# form with (NT column tiles per wave, CH column waves sharing each k-split's A) = (2,2)/(2,4)/(4,2),
# the balanced ring form "rw" (every CU one workgroup with ceil/floor of tiles / CUs) and its
# split-K variant "rwk" (+ a reduce / epilogue launch) for the narrow projections, with the
# in-launch combine "rwki" (the last arriving split sums the slabs), and the row-split ring "rwr"
# (a pair of workgroups per column group, half the rows each: no K split, no combine)
_KERNEL_FLAGS = {"pk": 0, "sk": 4, "lds22": 16, "lds24": 16 | 32, "lds42": 16 | 96, "rw": 128, "rwk": 256,
                 "rwki": 256 | 512, "rwr": 4096, "t2d": 32768}
_LDS_CFG = {"lds22": (2, 2), "lds24": (2, 4), "lds42": (4, 2)}
# "<kernel>+r": the same kernel with every workgroup's k walk rotated (csrc/gemm_kernels.h
# rw_krot, flags bit 10) - kept by the autotuners per shape only where it measures faster
ROT_FLAG = 1024


def _base(name: str) -> str:
    return name[:-2] if name.endswith("+r") else name


def _kflags(name: str) -> int:
    return _KERNEL_FLAGS[_base(name)] | (ROT_FLAG if name.endswith("+r") else 0)


def set_gemm_sk(mode: str) -> None:
    """"auto" (autotuned table), "on" / "off" (stream-K wherever it applies / never), or a kernel
    name from ``_KERNEL_FLAGS`` to force it wherever it applies."""
    global _GEMM_SK
    assert mode in ("auto", "on", "off") or _base(mode) in _KERNEL_FLAGS
    _GEMM_SK = mode


def _dev_key(device):
    """Key of the per-device caches: an index-less CUDA device means the current one."""
    device = torch.device(device)
    return device.type, device.index if device.index is not None else torch.cuda.current_device()


def gemm_workspace(device) -> torch.Tensor:
    """Per-device scratch of the stream-K GEMM: split-group arrival counters, a zero A
    fragment for masked units, and fp32 partial slabs.

    Zero-initialised once; the kernel leaves the counters at zero after every launch, so the
    buffer is reusable by every later launch and graph replay.  One compute stream per device
    uses it at a time (the executors' decode step is single-stream).  Call this before a
    hipGraph capture so the allocation does not happen inside it.
    """
    key = _dev_key(device)
    ws = _GEMM_WS.get(key)
    if ws is None:
        require_native()
        nbytes = int(torch.ops.mpamd.gemm_workspace_bytes())
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _GEMM_WS[key] = ws
    return ws


def _m_bucket(M: int) -> int:
    """Autotune row buckets: 4 (batch-1..4 decode: latency-bound, its own winner), then 16-row
    steps (the packed layout's row tiles)."""
    return 4 if M <= 4 else 16 * ((M + 15) // 16)


def _sk_covered(N: int, K: int) -> bool:
    nks = K // 32
    return (N // 16) % 2 == 0 and nks % 8 == 0 and nks >= 32


def _lds_covered(name: str, M: int, N: int, K: int, epilogue: int) -> bool:
    nt, ch = _LDS_CFG[name]
    mt = (M + 15) // 16
    return (N // 16) % (nt * ch) == 0 and K % 64 == 0 and (2 * mt) % ch == 0 and not (epilogue == 1 and nt % 2)


def _covered(name: str, M: int, N: int, K: int, epilogue: int) -> bool:
    name = _base(name)
    if name == "pk":
        return True
    if name == "sk":
        return _sk_covered(N, K)
    if name == "rw":  # widths the launcher does not build fall back to the other kernels by itself
        return True
    if name == "rwk":  # split-K ring + reduce launch: plain / residual / fused-norm producer epilogues
        return epilogue != 1 and N % 2048 == 0
    if name == "rwki":  # the same with an in-launch combine (M <= 64)
        return epilogue != 1 and N % 2048 == 0 and M <= 64
    if name == "rwr":  # row-split ring: 2 or 4 row tiles split over a workgroup pair
        return epilogue != 1 and N % 2048 == 0 and (M + 15) // 16 in (2, 4)
    if name == "t2d":  # row blocks x column groups: more than 64 rows only (picked by linear itself)
        return 64 < M <= 256 and t2d_ok(M, N, K, epilogue, epilogue == 1)
    return _lds_covered(name, M, N, K, epilogue)


def _kernel_for(M: int, N: int, K: int, epilogue: int) -> str:
    mode = _GEMM_SK
    if mode == "off":
        return "pk"
    if mode == "on":
        mode = "sk"
    if mode == "auto":
        mode = _SK_CHOICE.get((_m_bucket(M), N, K, int(epilogue)), "pk")
    return mode if _covered(mode, M, N, K, epilogue) else "pk"


def _use_sk(M: int, N: int, K: int, epilogue: int) -> bool:
    return _kernel_for(M, N, K, epilogue) == "sk"


_TUNE_POOL_BYTES = 1 << 30

# ---------------------------------------------------------------------------------------
# Committed decode-kernel table (ops/tuned/decode_kernels_gfx950.json, written by
# ``python -m src.ops.tune`` on an MI355X): the autotuners' per-shape choices and the
# executors' end-to-end qkv-fold decisions.  Loaded by default, so two boxes running the same
# tree run the same kernel mix (a start-up timing race used to pick a different kernel for 4 of
# 35 Llama-2-7B shapes from box to box).  ``MPAMD_GEMM_AUTOTUNE``: "1" (default) times only
# shapes the table lacks, "0" never times (untabled shapes take the first kernel), "force"
# re-times every shape an executor uses.  ``MPAMD_KERNEL_TABLE``: another table, or "0" for none.
KERNEL_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "decode_kernels_gfx950.json")
_QKV_FOLD_PIN = {}  # (graph batch bucket, N, K, fp8) -> bool: the decode-graph A/B's decision
_TABLE = {"path": None, "file_sha": None, "runtime": set()}


def autotune_mode() -> str:
    m = os.environ.get("MPAMD_GEMM_AUTOTUNE", "1")
    return {"0": "off", "1": "missing", "force": "force"}.get(m, "missing")


def _k4(k) -> str:
    return f"M{k[0]}:N{k[1]}xK{k[2]}e{k[3]}"


def _kfold(k, tag) -> str:
    return f"{tag}{k[0]}:N{k[1]}xK{k[2]}:{'fp8' if k[3] else 'bf16'}"


def _parse_key(s: str):
    head, nk, last = (s.split(":") + [""])[:3]
    n, k = nk[1:].split("xK")
    if "e" in k:
        k, e = k.split("e")
        return int(head[1:]), int(n), int(k), int(e)
    return int(head[1:]), int(n), int(k), last == "fp8"


def kernel_table() -> dict:
    """The decode-kernel choices this process currently runs, in the table's JSON form."""
    return {"arch": "gfx950",
            "gemm": {_k4(k): v for k, v in sorted(_SK_CHOICE.items())},
            "w8": {_k4(k): v for k, v in sorted(_W8_CHOICE.items())},
            "fp8": {_k4(k): v for k, v in sorted(_FP8_CHOICE.items())},
            "qkv_fold_cand": {_kfold(k, "M"): bool(v) for k, v in sorted(_QKV_FOLD_CAND.items())},
            "qkv_fold": {_kfold(k, "B"): bool(v) for k, v in sorted(_QKV_FOLD_PIN.items())}}


def kernel_table_sha(table: Optional[dict] = None) -> str:
    import hashlib
    import json

    body = json.dumps(table if table is not None else kernel_table(), sort_keys=True).encode()
    return hashlib.sha256(body).hexdigest()[:16]


def load_kernel_table(path: Optional[str] = None) -> Optional[str]:
    """Load the committed choice table into the autotuners' dicts (entries already present -
    tuned or loaded earlier in this process - are kept).  Returns the file's table sha, or None
    when there is no table (``MPAMD_KERNEL_TABLE=0``, missing file).  Once per process."""
    import json

    if _TABLE["path"] is not None:
        return _TABLE["file_sha"]
    path = path or os.environ.get("MPAMD_KERNEL_TABLE") or KERNEL_TABLE
    _TABLE["path"] = path
    if path == "0" or not os.path.exists(path):
        return None
    with open(path) as f:
        t = json.load(f)
    for name, dst in (("gemm", _SK_CHOICE), ("w8", _W8_CHOICE), ("fp8", _FP8_CHOICE)):
        for s, v in t.get(name, {}).items():
            dst.setdefault(_parse_key(s), str(v))
    for s, v in t.get("qkv_fold_cand", {}).items():
        _QKV_FOLD_CAND.setdefault(_parse_key(s), bool(v))
    for s, v in t.get("qkv_fold", {}).items():
        _QKV_FOLD_PIN.setdefault(_parse_key(s), bool(v))
    _TABLE["file_sha"] = kernel_table_sha(
        {k: t.get(k, {}) for k in ("gemm", "w8", "fp8", "qkv_fold_cand", "qkv_fold")} | {"arch": "gfx950"})
    return _TABLE["file_sha"]


def save_kernel_table(path: str) -> str:
    import json

    t = kernel_table()
    with open(path, "w") as f:
        json.dump(t, f, indent=1, sort_keys=True)
        f.write("\n")
    return kernel_table_sha(t)


def kernel_table_report() -> dict:
    """For the bench JSON: the committed table's sha, the sha of the mix this process runs, and
    the shapes timed at run time (not in the table; empty = the process ran the table as is)."""
    return {"table": os.path.relpath(_TABLE["path"], os.path.dirname(os.path.abspath(__file__)))
            if _TABLE["path"] not in (None, "0") else None,
            "gemm_table_sha": _TABLE["file_sha"], "effective_sha": kernel_table_sha(),
            "tuned_at_runtime": sorted(_TABLE["runtime"])}


def _todo(table: dict, keys) -> list:
    """Keys the autotuner must time under ``MPAMD_GEMM_AUTOTUNE`` (dropping them first on force)."""
    mode = autotune_mode()
    if mode == "off":
        return []
    if mode == "force":
        for k in keys:
            table.pop(k, None)
    out = [k for k in keys if k not in table]
    _TABLE["runtime"].update(_k4(k) if len(k) == 4 and not isinstance(k[3], bool) else _kfold(k, "M") for k in out)
    return out


def _todo_rows(table: dict, N: int, K: int, epi: int, ms) -> list:
    """The row counts an autotuner times for one (N, K, epilogue): the last of ``ms`` in each M bucket
    whose (bucket, N, K, epilogue) key ``_todo`` says to time."""
    rows = {_m_bucket(M): M for M in ms}
    keys = _todo(table, [(b, N, K, int(epi)) for b in rows])
    return [M for b, M in rows.items() if (b, N, K, int(epi)) in keys]


def _time_candidates(cands: dict, iters: int, rounds: int) -> dict:
    """{name: best ms per call} of the callables ``cands[name](i)``, i = the call's number (which the
    tuners use to rotate over weight copies).  The candidates are timed in alternating rounds, in
    mapping order: two warm-up calls, then ``iters`` calls between two events; best round each."""
    t = {name: float("inf") for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            for i in range(2):
                fn(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(i)
            e1.record()
            e1.synchronize()
            t[name] = min(t[name], e0.elapsed_time(e1) / iters)
    return t


def qkv_fold_pinned(bucket: int, N: int, K: int, fp8: bool) -> Optional[bool]:
    if autotune_mode() == "force":
        return None
    return _QKV_FOLD_PIN.get((int(bucket), int(N), int(K), bool(fp8)))


def pin_qkv_fold(bucket: int, N: int, K: int, fp8: bool, fold: bool) -> None:
    _QKV_FOLD_PIN[(int(bucket), int(N), int(K), bool(fp8))] = bool(fold)


def autotune_gemm(shapes, device, ms=(4, 16, 32, 48, 64), iters: int = 24, rounds: int = 3) -> dict:
    """Time every applicable decode-GEMM kernel (one-group, stream-K, shared-A variants) on each
    (N, K, epilogue) for each M bucket and record the fastest for ``linear``.  Returns the table.

    Conditions match the decode step: the packed weight is rotated over copies in a 1 GiB pool
    (a decode step streams gigabytes between two uses of a layer's weights, so the 256 MB
    Infinity Cache never serves them; timing one resident copy favoured the wrong kernel by up
    to 30 %), and the two kernels are timed in alternating rounds, best round each."""
    global _GEMM_SK
    device = torch.device(device)
    if device.type != "cuda":
        return {}
    require_native()
    gemm_workspace(device)
    saved = _GEMM_SK
    pool = None
    try:
        for (N, K, epi) in shapes:
            todo = _todo_rows(_SK_CHOICE, N, K, epi, ms)
            if not todo:
                continue
            if pool is None:
                pool = (torch.randn(_TUNE_POOL_BYTES // 2, device=device) * 0.02).to(torch.bfloat16)
            n = N * K
            if n > pool.numel():  # one weight larger than the pool (e.g. a 128K-vocab lm_head): it is
                # MALL-cold by itself, so a single dedicated copy gives the same conditions
                wps = [torch.empty(n, dtype=torch.bfloat16, device=device).normal_(0, 0.02)
                       .view(N // 16, K // 32, 64, 8)]
            else:
                wps = [pool[i * n:(i + 1) * n].view(N // 16, K // 32, 64, 8)
                       for i in range(min(16, pool.numel() // n))]
            copies = len(wps)
            for M in todo:
                key = (_m_bucket(M), N, K, int(epi))
                cands = [k for k in _KERNEL_FLAGS if _covered(k, M, N, K, epi)]
                if len(cands) == 1:
                    _SK_CHOICE[key] = "pk"
                    continue
                xp = pack_act(torch.randn(M, K, device=device).to(torch.bfloat16))
                res = torch.zeros(M, N, dtype=torch.bfloat16, device=device) if epi in (2, 3) else None
                # fused-norm producer: packed copy + per-row sum of squares
                extra = _epi3_scratch(M, N, device) if epi == 3 else {}
                out = res if epi == 3 else _gemm_out(M, N // 2 if epi == 1 else N, epi == 1, torch.bfloat16, device)

                def call(mode, i):
                    global _GEMM_SK
                    _GEMM_SK = mode
                    linear(xp, None, out=out, epilogue=epi, residual=res, wp=wps[i % copies], a_rows=M,
                           out_packed=epi == 1, **extra)

                t = _time_candidates({k: partial(call, k) for k in cands}, iters, rounds)
                best = min(t, key=t.get)
                # keep the one-group kernel unless another wins by > 3 % (timing noise guard)
                best = best if t[best] < 0.97 * t["pk"] else "pk"
                # then the same kernel with the rotated k walk, kept if it wins by > 1 %
                tr = _time_candidates({k: partial(call, k) for k in (best, best + "+r")}, iters, rounds)
                if tr[best + "+r"] < 0.99 * tr[best]:
                    best = best + "+r"
                _SK_CHOICE[key] = best
    finally:
        _GEMM_SK = saved
        del pool
    return dict(_SK_CHOICE)


# ---------------------------------------------------------------------------------------
def packed_numel(M: int, K: int) -> int:
    """Elements of a packed decode activation (rows padded to a multiple of 16)."""
    return ((M + 15) // 16) * 16 * K


def pack_act(x, out=None):
    """Row-major [M, K] -> packed decode-GEMM activation layout (flat, ``packed_numel`` elements)."""
    M, K = x.shape
    if not _native(x):
        return ref.pack_act(x, out=out)
    if out is None:
        out = torch.zeros(packed_numel(M, K), dtype=x.dtype, device=x.device)
    torch.ops.mpamd.pack_act(x, out)
    return out


def unpack_act(ap, M, K):
    return ref.unpack_act(ap, M, K)


def norm_stats_buffer(device, n: int = 1) -> torch.Tensor:
    """Zeroed fixed-point row statistics for the fused-norm decode path: int64 [n, 32, 128]
    (32 atomic shards x 128 rows of exact sums of round(x^2 * 2^20), csrc/gemm.hip EpiArgs):
    decode steps of up to 128 rows."""
    return torch.zeros(n, ref.SS_SHARDS, ref.SS_ROWS, dtype=torch.int64, device=device)


def _gemm_out(M: int, ncols: int, out_packed: bool, dtype, device) -> torch.Tensor:
    """Output buffer of a decode GEMM or attention step of M rows: flat in the packed activation
    layout (the next GEMM's input), or row-major [M, ncols]."""
    return torch.empty(packed_numel(M, ncols) if out_packed else (M, ncols), dtype=dtype, device=device)


def _epi3_scratch(M: int, N: int, device) -> dict:
    """``linear*`` arguments of an autotuner's epilogue-3 call: the packed copy and the row statistics."""
    return dict(ap_out=torch.zeros(packed_numel(M, N), dtype=torch.bfloat16, device=device),
                ss_out=norm_stats_buffer(device)[0], ss_zero=norm_stats_buffer(device)[0])


def rmsnorm(x, w, eps, out=None, residual=None, mode=0, rows=None, packed=False, ss=None, a8=None, a8_scale=None):
    """mode 0: y = norm(x)*w; 1: residual += x, y = norm(residual)*w; 2: residual = x, y = norm(x)*w;
    3: residual = x, y = x, ``ss`` = fixed-point row sums of squares (``norm_stats_buffer``; entry of
    the fused-norm decode path).

    ``packed``: write y in the packed decode-GEMM activation layout (``out`` flat).
    ``a8`` / ``a8_scale`` (with ``packed``): emit y quantized for the fp8 GEMM instead (the
    ``quant_act_fp8`` layout and per-row scales; ``out`` is then not written)."""
    if not _native(x):
        y = ref.rmsnorm(x, w, eps, out=None if packed else out, residual=residual, mode=mode, rows=rows, ss=ss)
        if a8 is not None:
            q, s = ref.quant_act_fp8(ref.pack_act(y), y.shape[0], y.shape[1])
            a8[: q.numel()].copy_(q)
            a8_scale[: y.shape[0]].copy_(s[: y.shape[0]])
            return a8
        return ref.pack_act(y, out=out) if packed else y
    n = rows.numel() if rows is not None else x.shape[0]
    if out is None:
        out = _gemm_out(n, x.shape[1], packed, x.dtype, x.device)
    torch.ops.mpamd.rmsnorm(x, residual if residual is not None else x, w, out, float(eps), int(mode), rows,
                            int(bool(packed)), ss, a8, a8_scale)
    return a8 if a8 is not None else out


def embed_stage_entry(ids, table, out, residual, ss):
    """Embedding lookup + the fused-norm path's stage entry (``rmsnorm`` mode 3) in one launch:
    residual[t] = table[ids[t]], ``out`` = the same rows packed, ``ss`` = their fixed-point row sums of
    squares.  (reference: the embedding + input_layernorm of petals/llama/block.py, here the entry of a
    first stage whose norm is folded into the qkv GEMM.)"""
    if not _native(table):
        h = embedding(ids, table)
        return rmsnorm(h, table[0], 0.0, out=out, residual=residual, mode=3, packed=True, ss=ss)
    torch.ops.mpamd.rmsnorm(table, residual, table[0], out, 0.0, 3, None, 1, ss, None, None, ids)
    return out


def _kv_f8(k_cache, v_cache) -> bool:
    """True when the caches are fp8 (``KVF8`` codes + scales); both or neither."""
    f8 = isinstance(k_cache, KVF8)
    if f8 != isinstance(v_cache, KVF8):
        raise TypeError("k_cache and v_cache must both be bf16 tensors or both be fp8 (ops.KVF8) caches")
    return f8


def _no_kv_f8(k_cache, v_cache, what: str) -> None:
    if isinstance(k_cache, KVF8) or isinstance(v_cache, KVF8):
        raise NotImplementedError(f"ops.{what} does not read an fp8 KV cache: an fp8 cache runs on the flash-decoding "
                                  "kernel (ops.paged_attention / ops.paged_attention_rope), for GQA decode on "
                                  "ops.attention_mfma_f8 / ops.attention_mfma_rope_f8, for prefill on "
                                  "ops.attention_fa_f8")


def _need_kv_f8(k_cache, v_cache, what: str) -> None:
    if not (isinstance(k_cache, KVF8) and isinstance(v_cache, KVF8)):
        raise TypeError(f"ops.{what} takes fp8 KV caches (ops.KVF8); bf16 caches run on ops.{what[:-3]}")


def _kv_pages(k_cache, v_cache):
    """(k pages, v pages, scale keyword arguments) of a ``torch.ops.mpamd`` call: an fp8 cache's
    (``KVF8``) codes with ``k_scale`` / ``v_scale``, bf16 pages as they come."""
    if isinstance(k_cache, KVF8):
        return k_cache.codes, v_cache.codes, {"k_scale": k_cache.scales, "v_scale": v_cache.scales}
    return k_cache, v_cache, {}


def rope_kv_write(qkv, positions, cos, sin, k_cache, v_cache, slots, nh, nkv):
    """RoPE of q (in place) and the new tokens' k / v into their page slots; an fp8 cache (``KVF8``)
    gets k (rotated, rounded to bf16) and v quantized per head (``quant_kv_fp8``)."""
    f8 = _kv_f8(k_cache, v_cache)
    if not _native(qkv):
        return (ref.rope_kv_write_f8 if f8 else ref.rope_kv_write)(qkv, positions, cos, sin, k_cache, v_cache, slots,
                                                                  nh, nkv)
    kc, vc, scales = _kv_pages(k_cache, v_cache)
    torch.ops.mpamd.rope_kv_write(qkv, positions, cos, sin, kc, vc, slots, int(nh), int(nkv), **scales)


def kv_write(k, v, k_cache, v_cache, slots):
    _no_kv_f8(k_cache, v_cache, "kv_write")
    if not _native(k):
        return ref.kv_write(k, v, k_cache, v_cache, slots)
    torch.ops.mpamd.kv_write(k, v, k_cache, v_cache, slots)


def attention_partition(num_queries: int, nkv: int, max_ctx: int, target_wgs: int = 1024,
                        min_part: int = 64) -> Tuple[int, int]:
    """(part_size, num_parts) for split-K flash decoding: enough workgroups to fill 256 CUs,
    but no slice shorter than ``min_part`` tokens.  The executor asks for 256-token slices on
    the MFMA GQA decode kernel (Llama-3-8B, 64 sessions: 13147 -> 13675 tok/s; batch 1:
    278 -> 281) and keeps 64 on the flash-decoding kernel, where short slices + the reduce
    launch measured slightly faster at batch 1 (334 vs 327 tok/s, Llama-2-7B)."""
    max_ctx = max(int(max_ctx), 1)
    if min_part < 256 and num_queries * nkv <= 64:
        # few (query, head) pairs: 256-token slices, so short contexts need no split-K combine
        # (its cost exceeds what 64 / 128-token slices save at batch 1 / 2: profiles/r4t)
        min_part, target_wgs = 256, 256
    min_part = int(min_part)
    want = max(1, math.ceil(target_wgs / max(1, num_queries * nkv)))
    np_ = max(1, min(want, math.ceil(max_ctx / 64)))
    ps = 64 * math.ceil(math.ceil(max_ctx / np_) / 64)
    ps = min(max(ps, 64 * math.ceil(min_part / 64)), 2048)
    np_ = math.ceil(max_ctx / ps)
    return ps, np_


def _window_kw(window: int) -> dict:
    """The ops' trailing ``window`` argument, passed only when a window is set."""
    return {"window": int(window)} if window else {}


def _window_span(window, max_ctx, pad: int = 0):
    """Tokens per query a windowed launch streams: ``min(max_ctx, W + pad)`` (``pad`` = 31 on the
    MFMA kernel, whose slices start at the 32-token step that holds the window's first key);
    ``max_ctx`` itself without a window.  ``max_ctx`` None (unknown): ``W + pad``."""
    window = int(window or 0)
    if window < 0:
        raise ValueError(f"window must be >= 0 (0: no sliding window), got {window}")
    if window == 0:
        return max_ctx
    return window + pad if max_ctx is None else min(int(max_ctx), window + pad)


def _check_window_parts(what: str, window, max_ctx, part_size, num_parts, pad: int = 0) -> None:
    """Explicit slices of a windowed launch must cover the streamed span (the kernels place them
    from the window's first key; keys past the last slice would be dropped without a word)."""
    if not window:
        return
    span = _window_span(window, max_ctx, pad)
    if int(part_size) * int(num_parts) < span:
        raise ValueError(f"ops.{what}: part_size {part_size} x num_parts {num_parts} does not cover the "
                         f"{span} tokens a window of {window} streams")


def _token_blocks(ntoks, tb: int):
    """int32 [2, NB] = (first flat token, count): runs of <= ``tb`` consecutive tokens of ONE
    sequence.  ``ntoks``: tokens per sequence in flat order."""
    import numpy as np

    n = np.asarray(ntoks, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]) if n.size else n
    nb = (n + tb - 1) // tb
    seq_of_block = np.repeat(np.arange(n.size), nb)
    k = np.arange(int(nb.sum())) - np.repeat(np.concatenate([[0], np.cumsum(nb)[:-1]]) if nb.size else nb, nb)
    tok0 = off[seq_of_block] + k * tb
    cnt = np.minimum(tb, n[seq_of_block] - k * tb)
    return np.stack([tok0, cnt]).astype(np.int32)


def query_blocks(ntoks, nrep: int):
    """MFMA attention query blocks for a ragged step: int32 [2, NB] = (first flat token, count).

    A block holds 16 / min(nrep, 16) consecutive tokens of ONE sequence (x the GQA group's
    heads = 16 MFMA rows).  ``ntoks``: tokens per sequence in flat order."""
    return _token_blocks(ntoks, 16 // min(max(int(nrep), 1), 16))


def query_superblocks(ntoks, nrep: int, group: int = 8):
    """Runs of <= ``group`` consecutive query blocks (``query_blocks`` order) of one sequence:
    int32 [2, NSB] = (first block, count).  The grouped MFMA prefill kernel runs one workgroup
    per run and streams each K/V step once for all of its blocks."""
    import numpy as np

    tb = 16 // min(max(int(nrep), 1), 16)
    nb = (np.asarray(ntoks, dtype=np.int64) + tb - 1) // tb
    first, cnt, b = [], [], 0
    for n in nb.tolist():
        for k in range(0, n, group):
            first.append(b + k)
            cnt.append(min(group, n - k))
        b += n
    return np.array([first, cnt], dtype=np.int32).reshape(2, -1)


def _attn_launch(what: str, q, k_cache, q_ctx, nh, window, pad: int, partition, part_size, num_parts, max_ctx, out,
                 workspace, packed=False, grow_workspace=True):
    """What every attention wrapper settles before its launch -> (part_size, num_parts, out, workspace).
    Without a ``part_size`` the slices are ``partition(span)`` of the tokens a query streams
    (``_window_span`` with the kernel's ``pad``; ``max_ctx`` is read from ``q_ctx`` when unknown);
    explicit slices must cover a window's span (``_check_window_parts``, as ``ops.<what>``).
    ``grow_workspace``: a caller's workspace too small for the parts is replaced; the flash-decoding
    ops allocate only when given none."""
    T, D = q.shape[0], k_cache.shape[-1]
    if part_size is None:
        if max_ctx is None:
            max_ctx = int(q_ctx.max().item()) if T else 1
        part_size, num_parts = partition(_window_span(window, max_ctx, pad))
    else:
        _check_window_parts(what, window, max_ctx, part_size, num_parts, pad)
    if out is None:
        out = _gemm_out(T, nh * D, packed, q.dtype, q.device)
    if grow_workspace:
        workspace = _attn_workspace(workspace, T, nh, D, num_parts, q.device)
    elif workspace is None:
        workspace = attention_workspace(T, nh, D, num_parts, q.device)
    return part_size, num_parts, out, workspace


def attention_mfma(q, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, nh, nkv, scale, out=None,
                   workspace=None, part_size=None, num_parts=None, max_ctx=None, packed=False, superblocks=None,
                   window=0):
    """MFMA flash attention (csrc/attention_mfma.hip): prefill blocks of 16 query rows and GQA
    decode.  Same semantics and output as ``paged_attention``; ``qblocks`` from
    ``query_blocks`` (device int32 [2, NB]); ``superblocks`` (``query_superblocks``, device)
    selects the grouped prefill kernel (up to 4 blocks of a sequence per workgroup).  ``window``
    (sliding window, ``paged_attention``): decode blocks only - one token per block, no superblocks."""
    _no_kv_f8(k_cache, v_cache, "attention_mfma")
    return _attention_mfma("attention_mfma", q, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, nh, nkv, scale,
                           out, workspace, part_size, num_parts, max_ctx, packed, window, superblocks=superblocks)


def _mfma_partition(nblocks: int, nh: int, nkv: int, max_ctx: int) -> Tuple[int, int]:
    """Default (part_size, num_parts) of ``attention_mfma`` / ``attention_mfma_f8``: about 1024
    workgroups, slices of a multiple of 128 tokens."""
    nblk = nblocks * (nh // min(nh // nkv, 16))
    want = max(1, math.ceil(1024 / max(1, nblk)))
    num_parts = max(1, min(want, math.ceil(max_ctx / 128)))
    part_size = 128 * math.ceil(math.ceil(max_ctx / num_parts) / 128)
    return part_size, math.ceil(max(max_ctx, 1) / part_size)


def attention_mfma_f8(q, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, nh, nkv, scale, out=None,
                      workspace=None, part_size=None, num_parts=None, max_ctx=None, packed=False, window=0):
    """``attention_mfma`` for GQA decode on an fp8 KV cache (``KVF8``; csrc/attention_mfma.hip F8
    form): one query token per block (``decode_qblocks``), GQA groups of 4, 8 or a multiple of 16
    heads.  The kernel converts the codes exactly and then does the bf16 kernel's arithmetic, so the
    output equals ``attention_mfma`` on the dequantized cache bit for bit."""
    _need_kv_f8(k_cache, v_cache, "attention_mfma_f8")
    return _attention_mfma("attention_mfma_f8", q, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, nh, nkv,
                           scale, out, workspace, part_size, num_parts, max_ctx, packed, window)


def _attention_mfma(what, q, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, nh, nkv, scale, out, workspace,
                    part_size, num_parts, max_ctx, packed, window, superblocks=None, rope=(), qkv_part=None,
                    mx_out=None):
    """The four ``attention_mfma*`` ops, on the cache as it comes.  ``rope`` = (positions, cos, sin,
    slots): the fused RoPE decode form, where ``q`` is the unrotated qkv projection."""
    if qkv_part is not None and not _native(q):
        q = reduce_qkv_part(qkv_part, q.dtype)
        qkv_part = None
    if not _native(q):
        if rope:
            positions, cos, sin, slots = rope
            q = q.clone()
            (ref.rope_kv_write_f8 if isinstance(k_cache, KVF8) else ref.rope_kv_write)(
                q, positions, cos, sin, k_cache, v_cache, slots, nh, nkv)
        return paged_attention(q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out=out,
                               packed=packed, window=window)
    if rope:  # one part unless the caller sets the slices
        partition = lambda span: (128 * math.ceil(max(span, 1) / 128), 1)  # noqa: E731
    else:
        nblk = superblocks.shape[1] if superblocks is not None else qblocks.shape[1]
        partition = lambda span: _mfma_partition(nblk, nh, nkv, span)  # noqa: E731
    part_size, num_parts, out, workspace = _attn_launch(what, q, k_cache, q_ctx, nh, window, 31, partition, part_size,
                                                        num_parts, max_ctx, out, workspace, packed)
    kc, vc, scales = _kv_pages(k_cache, v_cache)
    tail = (out, workspace, int(nh), int(nkv), float(scale), int(part_size), int(num_parts), int(bool(packed)))
    if rope:
        torch.ops.mpamd.attention_mfma_rope(q, kc, vc, block_tables, q_seq, q_ctx, qblocks, *rope, *tail,
                                            *_qkv_part_args(qkv_part),
                                            *(mx_out if mx_out is not None else (None, None)),
                                            **_window_kw(window), **scales)
    else:
        torch.ops.mpamd.attention_mfma(q, kc, vc, block_tables, q_seq, q_ctx, qblocks, *tail, superblocks,
                                       **_window_kw(window), **scales)
    return out


FA_WAVES = 4  # default waves per prefill workgroup (32 query rows each); fa_plan picks 4 or 8 per step
FA_WAVES_FORCE = None  # 4 / 8: every prefill step on that workgroup size (A/B runs)


def fa_blocks(ntoks, nrep: int, waves: int = None):
    """Workgroup blocks of the FA2 prefill kernel (csrc/attention_fa.hip): int32 [2, NB] =
    (first flat token, count), each <= 32 x waves / nrep consecutive tokens of ONE sequence."""
    return _token_blocks(ntoks, max(1, (32 * int(waves or FA_WAVES)) // max(int(nrep), 1)))


def fa_plan(ntoks, nh: int, nkv: int, n_cu: int = 256):
    """(blocks, waves) for a prefill step on the FA2 kernel: 8-wave workgroups (256 query rows,
    half the K/V traffic per row) unless their grid would not give every CU a second workgroup
    (a single 2K GQA prompt: 4 waves measured 74.7 vs 91.7 us, profiles/r3_fa2/attn.jsonl)."""
    nrep = max(1, nh // nkv)
    fb8 = fa_blocks(ntoks, nrep, 8)
    if FA_WAVES_FORCE in (4, 8):
        return (fb8 if FA_WAVES_FORCE == 8 else fa_blocks(ntoks, nrep, 4)), FA_WAVES_FORCE
    if fb8.shape[1] * nkv > n_cu:
        return fb8, 8
    return fa_blocks(ntoks, nrep, 4), 4


FA_PAIR = "auto"  # "0" / "1" force the pairing off / on (A/B runs)


def fa_pair(nblocks: int, nh: int, nkv: int, num_parts: int, n_cu: int = 256) -> bool:
    """Pair each long causal query block with its short mirror in one workgroup (csrc/attention_fa.hip
    ``pair``): every workgroup then streams the same context, so the longest blocks no longer set
    the kernel time, and there are half as many workgroups to launch.  Measured faster or equal
    in every case of profiles/r4d/attn_pair.jsonl (1 x 2048 MHA 116.6 -> 80.9 us, 1 x 4096 MHA
    231.7 -> 159.8, 64 x 128 GQA 59.3 -> 54.5), so it is on whenever the context is not split."""
    if FA_PAIR in ("0", "1"):
        return FA_PAIR == "1" and num_parts == 1
    return num_parts == 1 and nblocks >= 2


def fa_ok(nh: int, nkv: int, D: int, page_size: int) -> bool:
    """Shapes the FA2 prefill kernel covers (else the 16x16 grouped kernel runs)."""
    return D == 128 and nh % nkv == 0 and (nh // nkv) in (1, 2, 4, 8) and page_size % 64 == 0


def attention_fa(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, out=None,
                 workspace=None, max_ctx=None, waves=None, num_parts=None, pair=None, window=0):
    """Causal prefill attention, FA2 form on 32x32x16 MFMA with the transposed LDS reads of V
    (csrc/attention_fa.hip).  Same semantics as ``paged_attention``; row-major output only.
    ``fablocks`` from ``fa_blocks`` (device int32 [2, NB]).  The context is split over parts
    only when the grid would leave CUs idle.  This op keeps ``window`` at 0 (``window`` > 0 raises):
    the kernel's sliding-window form is ``attention_fa_window``."""
    _no_kv_f8(k_cache, v_cache, "attention_fa")
    return _attention_fa(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, out, workspace,
                         max_ctx, waves, num_parts, pair, window)


def attention_fa_f8(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, out=None,
                    workspace=None, max_ctx=None, waves=None, num_parts=None, pair=None, window=0):
    """``attention_fa`` on an fp8 KV cache (``KVF8``; csrc/attention_fa.hip F8 form), with the same
    blocks, parts and pairing.  The kernel converts the codes exactly while staging them into the LDS
    tiles and then does the bf16 kernel's arithmetic, so the output equals ``attention_fa`` on the
    dequantized cache bit for bit."""
    _need_kv_f8(k_cache, v_cache, "attention_fa_f8")
    return _attention_fa(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, out, workspace,
                         max_ctx, waves, num_parts, pair, window)


def attention_fa_window(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, window, out=None,
                        workspace=None, max_ctx=None, waves=None, num_parts=None, pair=None, part_size=None):
    """``attention_fa`` under a sliding window W = ``window`` > 0 (csrc/attention_fa.hip WIN form): a
    query of context ctx sees cache positions [max(0, ctx - W), ctx), the decode kernels' rule.  A block
    streams from the 64-token step that holds its first row's first key, and the parts split that
    span (at most W + tokens per block + 62), not the context; ``part_size`` (a multiple of 64) with
    ``num_parts`` sets the slices explicitly and must cover the span.  No block-table entry below the
    page of a block's first visible key is read (rolling pages)."""
    _no_kv_f8(k_cache, v_cache, "attention_fa_window")
    return _attention_fa(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, out, workspace,
                         max_ctx, waves, num_parts, pair, window, windowed=True, part_size=part_size)


def attention_fa_window_f8(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, window,
                           out=None, workspace=None, max_ctx=None, waves=None, num_parts=None, pair=None,
                           part_size=None):
    """``attention_fa_window`` on an fp8 KV cache (``KVF8``): only the staging differs, so the output
    equals ``attention_fa_window`` on the dequantized cache bit for bit."""
    _need_kv_f8(k_cache, v_cache, "attention_fa_window_f8")
    return _attention_fa(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, out, workspace,
                         max_ctx, waves, num_parts, pair, window, windowed=True, part_size=part_size)


def fa_window_pad(nh: int, nkv: int, waves: int) -> int:
    """``pad`` of ``_window_span`` for the windowed FA2 kernel: BT + 62, BT = the most tokens a block
    holds.  A block of n consecutive tokens with first context c streams from ``base = max(0, c - W) &
    ~63`` to ``c + n - 1``: at most W + n + 62 tokens."""
    return max(1, (32 * int(waves)) // max(1, nh // nkv)) + 62


def _fa_partition(nblocks: int, nh: int, nkv: int, span: int, num_parts=None) -> Tuple[int, int]:
    """(part_size, num_parts) of the FA2 ops over ``span`` streamed tokens: parts (the caller's count,
    else enough for about 512 workgroups, none under 256 tokens) of a multiple of 64 tokens."""
    span = max(span, 1)
    if num_parts is None:
        nblk = nblocks * (nh // (nh // nkv))
        want = max(1, math.ceil(512 / max(1, nblk)))
        num_parts = max(1, min(want, math.ceil(span / 256)))
    part_size = 64 * math.ceil(math.ceil(span / max(1, int(num_parts))) / 64)
    return part_size, math.ceil(span / part_size)


def _attention_fa(q, k_cache, v_cache, block_tables, q_seq, q_ctx, fablocks, nh, nkv, scale, out, workspace, max_ctx,
                  waves, num_parts, pair, window=0, windowed=False, part_size=None):
    """The four ``attention_fa*`` ops, on the cache as it comes: the partition rule (``windowed``: on
    the streamed span, or the caller's ``part_size``; the plain ops always derive theirs), the pairing
    rule and the launch."""
    waves = int(waves or FA_WAVES)
    pad = 0
    if windowed:
        window = int(window)
        if window <= 0:
            raise ValueError(f"ops.attention_fa_window: window must be > 0, got {window}")
        pad = fa_window_pad(nh, nkv, waves)
        if part_size is not None:  # (refused before the fallback too)
            if num_parts is None or int(part_size) <= 0 or int(part_size) % 64:
                raise ValueError("ops.attention_fa_window: part_size is a positive multiple of 64 given with num_parts")
            _check_window_parts("attention_fa_window", window, max_ctx, part_size, num_parts, pad)
    if not _native(q):
        return paged_attention(q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out=out, window=window)
    nblocks = int(fablocks.shape[1])
    # (a window on the plain ops is the binding's to refuse: their slices split the context)
    part_size, num_parts, out, workspace = _attn_launch(
        "attention_fa_window", q, k_cache, q_ctx, nh, window if windowed else 0, pad,
        lambda span: _fa_partition(nblocks, nh, nkv, span, num_parts), part_size, num_parts, max_ctx, out, workspace)
    if pair is None:
        pair = fa_pair(nblocks, nh, nkv, num_parts)
    kc, vc, scales = _kv_pages(k_cache, v_cache)
    args = (q, kc, vc, block_tables, q_seq, q_ctx, fablocks, out, workspace, int(nh), int(nkv), float(scale),
            int(part_size), int(num_parts), waves, int(bool(pair) and num_parts == 1))
    if windowed:
        torch.ops.mpamd.attention_fa_window(*args, window, **scales)
    else:
        torch.ops.mpamd.attention_fa(*args, **_window_kw(window), **scales)
    return out


def attention_mfma_rope(qkv, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, positions, cos, sin, slots, nh,
                        nkv, scale, out=None, workspace=None, part_size=None, num_parts=None, max_ctx=None,
                        packed=False, qkv_part=None, mx_out=None, window=0):
    """GQA decode step on the MFMA kernel with RoPE of q / new k and the new token's page-slot
    write folded in (csrc/attention_mfma.hip ROPE path).  ``qblocks`` must hold one token per block,
    block i = token i (``decode_qblocks``: the kernel takes that as given and reads no qblocks); ``qkv`` is the unrotated fused projection and is not modified; with
    ``qkv_part`` the kernel reads q / k / v from the qkv GEMM's partial slabs instead.  ``mx_out =
    (ax, as_)`` (packed, one part, head_dim 128): the kernel writes its output as the W8A8-MX GEMM's
    activation (``quant_mx`` layout) there instead of ``out`` - the o projection's input, quantized
    in the attention epilogue."""
    _no_kv_f8(k_cache, v_cache, "attention_mfma_rope")
    return _attention_mfma("attention_mfma_rope", qkv, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, nh, nkv,
                           scale, out, workspace, part_size, num_parts, max_ctx, packed, window,
                           rope=(positions, cos, sin, slots), qkv_part=qkv_part, mx_out=mx_out)


def attention_mfma_rope_f8(qkv, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, positions, cos, sin, slots,
                           nh, nkv, scale, out=None, workspace=None, part_size=None, num_parts=None, max_ctx=None,
                           packed=False, qkv_part=None, window=0):
    """``attention_mfma_rope`` on an fp8 KV cache (``KVF8``): the new token's rotated k and its v are
    quantized per head (``quant_kv_fp8``), written as codes + scale, and attended to through their
    dequantized values - what every later step reads.  GQA groups of 4, 8 or a multiple of 16 heads;
    no MX output."""
    _need_kv_f8(k_cache, v_cache, "attention_mfma_rope_f8")
    return _attention_mfma("attention_mfma_rope_f8", qkv, k_cache, v_cache, block_tables, q_seq, q_ctx, qblocks, nh,
                           nkv, scale, out, workspace, part_size, num_parts, max_ctx, packed, window,
                           rope=(positions, cos, sin, slots), qkv_part=qkv_part)


_ATTN_CNT = {}


def attention_counters(device) -> torch.Tensor:
    """Per-device zeroed int32 arrival counters of the flash-decoding kernel's in-launch split-K
    combine (csrc/attention.hip split_combine): one per (query, head group) of a step; the
    last-arriving slice re-zeroes its counter.  Steps with more (query, group) pairs than this
    holds fall back to the separate reduce launch.  Call before a hipGraph capture."""
    key = _dev_key(device)
    c = _ATTN_CNT.get(key)
    if c is None:
        c = _ATTN_CNT[key] = torch.zeros(1 << 16, dtype=torch.int32, device=device)
    return c


# the flash-decoding split-K combine inside the attention launch (last-arriving slice) instead of
# the reduce launch: off - measured at batch 1 (Llama-2-7B, 1 MI355X) 2.984 ms/step with it vs
# 2.921 with the separate reduce launch (profiles/r2_attn_combine); kept bit-identical and tested
ATTN_INLAUNCH_REDUCE = False


def _attn_cnt(device):
    if not ATTN_INLAUNCH_REDUCE:
        return None
    return attention_counters(device)


def attention_workspace(num_queries: int, nh: int, head_dim: int, num_parts: int, device) -> torch.Tensor:
    return torch.empty(max(1, num_queries * nh * num_parts * (head_dim + 2)), dtype=torch.float32, device=device)


def _attn_workspace(workspace, num_queries: int, nh: int, head_dim: int, num_parts: int, device) -> torch.Tensor:
    """The caller's split-K workspace, or a new one if it has none or one too small for ``num_parts``."""
    if workspace is None or (num_parts > 1 and workspace.numel() < num_queries * nh * num_parts * (head_dim + 2)):
        return attention_workspace(num_queries, nh, head_dim, num_parts, device)
    return workspace


def paged_attention(q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out=None, workspace=None,
                    part_size=None, num_parts=None, max_ctx=None, packed=False, window=0):
    """Flash-decoding paged attention (csrc/attention.hip).  ``k_cache`` / ``v_cache``: bf16 pages, or
    an fp8 cache (``KVF8``), read by the kernel's fp8 form.  ``window`` W > 0 (sliding window): a
    query of context ``ctx`` sees cache positions ``[max(0, ctx - W), ctx)`` only, and neither the
    pages below them nor their block-table entries are read; 0: the whole context."""
    f8 = _kv_f8(k_cache, v_cache)
    if not _native(q):
        y = (ref.paged_attention_f8 if f8 else ref.paged_attention)(
            q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out=None if packed else out,
            window=window)
        return ref.pack_act(y, out=out) if packed else y
    return _flash_decoding("paged_attention", q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out,
                           workspace, part_size, num_parts, max_ctx, packed, window)


def _flash_decoding(what, q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out, workspace, part_size,
                    num_parts, max_ctx, packed, window, rope=(), qkv_part=None):
    """The launch of ``paged_attention`` and, with ``rope`` = (positions, cos, sin, slots) and ``q`` the
    unrotated qkv projection, of ``paged_attention_rope``, on the cache as it comes."""
    T = q.shape[0]
    part_size, num_parts, out, workspace = _attn_launch(
        what, q, k_cache, q_ctx, nh, window, 0, lambda span: attention_partition(T, nkv, span), part_size, num_parts,
        max_ctx, out, workspace, packed, grow_workspace=False)
    kc, vc, scales = _kv_pages(k_cache, v_cache)
    tail = (out, workspace, int(nh), int(nkv), float(scale), int(part_size), int(num_parts), int(bool(packed)),
            _attn_cnt(q.device))
    if rope:
        torch.ops.mpamd.paged_attention_rope(q, kc, vc, block_tables, q_seq, q_ctx, *rope, *tail,
                                             *_qkv_part_args(qkv_part), **_window_kw(window), **scales)
    else:
        torch.ops.mpamd.paged_attention(q, kc, vc, block_tables, q_seq, q_ctx, *tail, **_window_kw(window), **scales)
    return out


def _qkv_part_args(qkv_part):
    """(part, splits, ss, inv_k, eps) op arguments of a ``qkv_part`` = (slabs [S, T, width],
    row statistics or None, inv_k, eps) from ``linear_partials``; all-None when absent."""
    if qkv_part is None:
        return None, 0, None, 0.0, 0.0
    part, ss, inv_k, eps = qkv_part
    return part, int(part.shape[0]), ss, float(inv_k), float(eps)


def reduce_qkv_part(qkv_part, dtype=torch.bfloat16):
    """The bf16 qkv rows a ``qkv_part`` stands for (reference of the in-kernel fold)."""
    part, ss, inv_k, eps = qkv_part
    acc = torch.zeros_like(part[0])
    for s in range(part.shape[0]):
        acc = acc + part[s]
    if ss is not None:
        tot = ss.view(-1, ref.SS_ROWS).sum(0)[: part.shape[1]].double()
        rs = torch.rsqrt((tot.float() * (1.0 / 1048576.0)) * inv_k + eps)
        acc = acc * rs[:, None]
    return acc.to(dtype)


def paged_attention_rope(qkv, k_cache, v_cache, block_tables, q_seq, q_ctx, positions, cos, sin, slots, nh, nkv,
                         scale, out=None, workspace=None, part_size=None, num_parts=None, max_ctx=None,
                         packed=False, qkv_part=None, window=0):
    """Decode step (one query per sequence, q_ctx = position + 1): RoPE of q / new k, the new
    token's page-slot write and paged attention in ONE kernel (csrc/attention.hip ROPE path).
    ``qkv`` is the unrotated fused projection and is not modified; with ``qkv_part``
    (``linear_partials`` slabs + row statistics) the kernel reads q / k / v from the slabs and
    ``qkv`` is not read at all.  On an fp8 cache (``KVF8``) the new token is quantized per head,
    written as codes + scale, and attended to through its dequantized values."""
    f8 = _kv_f8(k_cache, v_cache)
    if qkv_part is not None and not _native(qkv):
        qkv = reduce_qkv_part(qkv_part, qkv.dtype)
        qkv_part = None
    if not _native(qkv):
        q = qkv.clone()
        (ref.rope_kv_write_f8 if f8 else ref.rope_kv_write)(q, positions, cos, sin, k_cache, v_cache, slots, nh, nkv)
        return paged_attention(q, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale, out=out,
                               workspace=workspace, part_size=part_size, num_parts=num_parts, max_ctx=max_ctx,
                               packed=packed, window=window)
    return _flash_decoding("paged_attention_rope", qkv, k_cache, v_cache, block_tables, q_seq, q_ctx, nh, nkv, scale,
                           out, workspace, part_size, num_parts, max_ctx, packed, window,
                           rope=(positions, cos, sin, slots), qkv_part=qkv_part)


def embedding(ids, table, out=None):
    if not _native(table):
        return ref.embedding(ids, table, out=out)
    if out is None:
        out = torch.empty(ids.numel(), table.shape[1], dtype=table.dtype, device=table.device)
    torch.ops.mpamd.embedding(ids, table, out)
    return out


def swiglu(gu, out=None):
    if not _native(gu):
        return ref.swiglu(gu, out=out)
    if out is None:
        out = torch.empty(gu.shape[0], gu.shape[1] // 2, dtype=gu.dtype, device=gu.device)
    torch.ops.mpamd.swiglu(gu, out)
    return out


def add(a, b, out=None):
    if not _native(a):
        return ref.add(a, b, out=out)
    if out is None:
        out = torch.empty_like(a)
    torch.ops.mpamd.add(a, b, out)
    return out


def argmax(logits, out=None):
    if not _native(logits):
        return ref.argmax(logits, out=out)
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
    torch.ops.mpamd.argmax(logits, out)
    return out


def sample(logits, temps, top_ps, top_ks, rep_pens, recent, recent_len, seeds, workspace=None, out=None,
           update_history: bool = False):
    """Batched reference-semantics sampler.  ``update_history`` appends each drawn id to its
    row of ``recent`` / ``recent_len`` (left-aligned, last ``recent.shape[1]`` ids) in place."""
    if not _native(logits):
        out = ref.sample(logits, temps, top_ps, top_ks, rep_pens, recent, recent_len, seeds, out=out)
        if update_history:
            ref.push_history(recent, recent_len, out)
        return out
    R, V = logits.shape
    if out is None:
        out = torch.empty(R, dtype=torch.long, device=logits.device)
    if workspace is None:
        workspace = torch.empty(max(1, R * V), dtype=torch.float32, device=logits.device)
    torch.ops.mpamd.sample(logits, temps, top_ps, top_ks, rep_pens, recent, recent_len, seeds, workspace, out,
                           int(bool(update_history)))
    return out


def sample_verify_workspace(R: int, V: int, cap: int) -> int:
    """fp32 elements of workspace ``sample_verify`` needs for R rows of a V-wide vocabulary and
    histories of ``cap`` ids: the samplers' R * V, then the per-row arguments it expands."""
    return int(torch.ops.mpamd.sample_verify_ws(int(R), int(V), int(cap))) if native_available() else 1


def sample_verify(logits, row_start, draft, temps, top_ps, top_ks, rep_pens, recent, recent_len, seeds,
                  workspace=None, tokens=None, count=None, update_history: bool = False, all_greedy: bool = False):
    """Speculative verify.  Session s owns the logits rows ``row_start[s] .. row_start[s + 1] - 1``
    (K_s + 1 of them); row j is drawn as ``sample`` would draw it with the history
    ``(h_s + draft[0..j-1])[-cap:]``, seed ``seeds[row]`` and s as the random number's row term,
    and checked against ``draft[row]`` (-1 on the session's last row).  ``tokens`` gets the
    session's leading draws that equal their draft and the one after them, -1 behind;
    ``count[s]`` how many that is.  ``update_history`` pushes exactly those into ``recent[s]``.
    ``all_greedy``: the caller knows every temperature is <= 0 (argmax rows, no sampler).
    Returns (tokens int64 [R], count int32 [S])."""
    R, V = logits.shape
    S = row_start.numel() - 1
    if not _native(logits):
        t, c = ref.sample_verify(logits, row_start, draft, temps, top_ps, top_ks, rep_pens, recent, recent_len, seeds,
                                 update_history=update_history)
        if tokens is not None:
            tokens[:R].copy_(t)
            t = tokens
        if count is not None:
            count[:S].copy_(c)
            c = count
        return t, c
    if tokens is None:
        tokens = torch.empty(R, dtype=torch.long, device=logits.device)
    if count is None:
        count = torch.empty(S, dtype=torch.int32, device=logits.device)
    if workspace is None:
        workspace = torch.empty(sample_verify_workspace(R, V, recent.shape[1]), dtype=torch.float32,
                                device=logits.device)
    torch.ops.mpamd.sample_verify(logits, row_start, draft, temps, top_ps, top_ks, rep_pens, recent, recent_len,
                                  seeds, workspace, tokens, count, int(bool(update_history)), int(bool(all_greedy)))
    return tokens, count


_RW_OK = {}


def wide_gemm_ok(M: int, N: int, K: int, epilogue: int = 0, out_packed: bool = False) -> bool:
    """65..256 decode rows: the balanced ring kernel covers (packed A; epilogue 0 or packed SwiGLU,
    the widths it is built for; 129..256 rows at 12 / 16 row tiles) - or, from ``T2D_MIN`` rows
    up, the two-dimensionally tiled kernel (every decode epilogue)."""
    if t2d_rows(M):
        return t2d_ok(M, N, K, epilogue, out_packed)
    key = (M, N, K, int(epilogue), bool(out_packed))
    if key not in _RW_OK:
        _RW_OK[key] = bool(native_available() and
                           torch.ops.mpamd.gemm_rw_ok(int(M), int(N), int(K), int(epilogue), int(bool(out_packed))))
    return _RW_OK[key]


# decode rows the ring kernels take.  They are built and tested up to 256 rows (12 / 16 row tiles),
# but at 256 sessions they measured slower than hipBLASLt + the unfused path (11.18 vs ~9.5
# ms/step, profiles/r4d: one column group per workgroup takes in the whole 256-row activation
# block, 5x its weight bytes); MPAMD_WIDE_ROWS=256 turns them on above 128.
WIDE_ROWS = int(os.environ.get("MPAMD_WIDE_ROWS", "128"))
# Decode rows from which the two-dimensionally tiled kernel (csrc/gemm_t2d.h: row blocks x column
# groups, both operands shared through LDS) runs every projection of the packed / fused-norm path,
# up to 256 (MPAMD_T2D_MIN; 257 = never: hipBLASLt + the unfused path above WIDE_ROWS).  Measured
# on the whole decode step against hipBLASLt (profiles/r5x): 136 / 160 / 192 / 224 / 256 sessions
# 7.49 / 7.85 / 8.35 / 8.95 / 9.53 ms vs 7.61 / 8.91 / 10.01 / 9.37 / 9.78.
T2D_MIN = int(os.environ.get("MPAMD_T2D_MIN", "129"))
# its operand stages arrive by LDS-DMA (global_load_lds) instead of a register ring + ds_write
T2D_GL = os.environ.get("MPAMD_T2D_GL", "1") == "1"
_T2D_OK = {}


def t2d_rows(M: int) -> bool:
    return max(T2D_MIN, 65) <= M <= 256


def wide_rows() -> int:
    """Largest decode row count the packed (hand-written GEMM) path takes."""
    return 256 if T2D_MIN <= 256 else WIDE_ROWS


def t2d_ok(M: int, N: int, K: int, epilogue: int = 0, out_packed: bool = False) -> bool:
    key = (M, N, K, int(epilogue), bool(out_packed))
    if key not in _T2D_OK:
        _T2D_OK[key] = bool(native_available() and
                            torch.ops.mpamd.gemm_t2d_ok(int(M), int(N), int(K), int(epilogue), int(bool(out_packed))))
    return _T2D_OK[key]


def native_gemm_ok(M: int, N: int, K: int, epilogue: int = 0, out_packed: bool = False) -> bool:
    if not (K % 128 == 0 and N % (32 if epilogue == 1 else 16) == 0):
        return False
    if 64 < M <= wide_rows():
        return wide_gemm_ok(M, N, K, epilogue, out_packed)
    return 0 < M <= 64


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """W [N, K] -> fragment-native layout [N/16, K/32, 64, 8] consumed by the decode GEMM."""
    if not _native(w):
        N, K = w.shape
        return w.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(N // 16, K // 32, 64, 8).contiguous()
    return torch.ops.mpamd.pack_weight(w.contiguous())


def unpack_weight(wp: torch.Tensor) -> torch.Tensor:
    nt, ks = wp.shape[0], wp.shape[1]
    return wp.view(nt, ks, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(nt * 16, ks * 32)


def linear(x, w, out=None, epilogue=0, residual=None, policy=None, wp=None, a_rows=None, out_packed=False,
           gate=None, ss_in=None, eps=0.0, ap_out=None, ss_out=None, ss_zero=None):
    """y = epilogue(x @ w^T). epilogue 0: none; 1: SwiGLU (16-row interleaved gate/up w); 2: + residual;
    3: fused-norm producer (``residual`` updated in place to bf16(y + residual), also written packed to
    ``ap_out``, per-row sum of squares added to ``ss_out``; ``ss_zero`` is cleared).

    ``wp`` is the packed copy of ``w`` (``pack_weight``); the native decode GEMM needs it.
    ``a_rows`` (int) says ``x`` is a PACKED activation holding that many rows (decode path);
    ``out_packed`` (SwiGLU only) writes the output packed for the next GEMM.
    ``ss_in`` (fused-norm consumer): ``x`` is the raw residual stream, ``w`` has the RMSNorm weight
    folded into its columns, and row r of the product is scaled by rsqrt(ss_in[r] / K + eps).
    """
    if not _native(x):
        K = 32 * wp.shape[1] if wp is not None else w.shape[1]
        if a_rows is not None:
            x = ref.unpack_act(x, a_rows, K)
        y = ref.linear(x, w if w is not None else unpack_weight(wp), out=None if out_packed or epilogue == 3 else out,
                       epilogue=epilogue, residual=residual, ss_in=ss_in, inv_k=1.0 / K, eps=eps, ap_out=ap_out,
                       ss_out=ss_out, ss_zero=ss_zero)
        return ref.pack_act(y, out=out) if out_packed else y
    if a_rows is not None:
        M = int(a_rows)
        K = 32 * wp.shape[1]
    else:
        M, K = x.shape
    N = w.shape[0] if w is not None else 16 * wp.shape[0]
    policy = policy or _GEMM_POLICY
    ok = wp is not None and native_gemm_ok(M, N, K, epilogue, out_packed) and (
        a_rows is not None or (x.stride(0) % 8 == 0 and x.stride(1) == 1))
    if ok and (policy in ("auto", "native") or a_rows is not None or out_packed):
        ncols = N // 2 if epilogue == 1 else N
        if a_rows is None:  # row-major caller: pack x into the fragment layout first
            x = pack_act(x)
        if out is None:
            out = _gemm_out(M, ncols, out_packed, x.dtype, x.device)
        if gate is not None:
            kern = "pk"
        elif M > 64 and t2d_rows(M) and t2d_ok(M, N, K, epilogue, out_packed):
            kern = "t2d"  # row blocks x column groups (129..256 rows)
        elif M > 64:  # 65..256 rows: split-K ring where it applies (o, down), else the ring kernel
            kern = "rwk" if (not out_packed and _covered("rwk", M, N, K, epilogue)) else "rw"
        else:
            kern = _kernel_for(M, N, K, epilogue)
        flags = 1 | (2 if out_packed else 0) | _kflags(kern) | (262144 if kern == "t2d" and T2D_GL else 0)
        ws = gemm_workspace(x.device) if _base(kern) in ("sk", "rwk", "rwki", "t2d") else None
        torch.ops.mpamd.gemm(x, wp, out, residual, int(epilogue), M, flags, ws, gate, ap_out, ss_out, ss_zero, ss_in,
                             1.0 / K, float(eps))
        return out
    if epilogue == 3 or ss_in is not None:
        raise RuntimeError(f"the fused-norm epilogues need the native decode GEMM (M={M}, N={N}, K={K})")
    if a_rows is not None or out_packed:
        raise RuntimeError(f"packed activations need the native decode GEMM (M={M}, N={N}, K={K})")
    if w is None:
        raise RuntimeError(f"no row-major weight for the hipBLASLt path (M={M}, N={N}, K={K})")
    if epilogue == 0 and out is not None and out.is_contiguous() and out.dtype == x.dtype and \
            out.shape == (M, N) and x.dim() == 2:
        return torch.mm(x, w.t(), out=out)  # hipBLASLt straight into the caller's buffer (no copy)
    y = torch.nn.functional.linear(x, w)  # hipBLASLt
    if epilogue == 1:
        return swiglu(y, out=out)
    if epilogue == 2:
        return add(y, residual, out=out)
    if out is not None:
        out.copy_(y)
        return out
    return y


# ---------------------------------------------------------------------------------------
# qkv projection as split-K partial slabs, summed by the decode attention kernel (the "fold"):
# the split-K ring streams the weights without the reduce launch, and the attention kernel's q /
# k / v loads add the S slabs, apply the fused-norm row scale and round to bf16 - the bits the
# reduce launch would have stored (csrc/common.h qkv_part_load8).
PART_FLAG = 16384
_RWK_SPLIT = {}
# (m_bucket, N, K, fp8) -> bool: the qkv GEMM alone measured faster as partial slabs
# (autotune_qkv_fold).  A candidate only: the decision the decode path uses is each executor's
# end-to-end decode-graph A/B per batch bucket (StageExecutor.qkv_fold_by_bucket), because the fold
# also moves work into the attention kernel
_QKV_FOLD_CAND = {}


def rwk_split(M: int, N: int, K: int, fp8=False) -> int:
    """Split count of the split-K ring form for this shape (0: not covered).  ``fp8``: False (bf16
    weights), True (W8A16) or 2 (the W8A8-MX form, ``linear_mx``)."""
    f8 = 2 if fp8 == 2 and not isinstance(fp8, bool) else int(bool(fp8))
    key = (int(M), int(N), int(K), f8)
    if key not in _RWK_SPLIT:
        _RWK_SPLIT[key] = int(torch.ops.mpamd.gemm_rwk_split(int(M), int(N), int(K), f8))
    return _RWK_SPLIT[key]


def _slab_view(device, S: int, M: int, N: int) -> torch.Tensor:
    ws = gemm_workspace(device)
    off = int(torch.ops.mpamd.gemm_slab_offset())
    return ws[off:off + S * M * N * 4].view(torch.float32).view(S, M, N)


def linear_partials(x, M: int, wp=None, w8=None, w_scale=None, out=None, rot: bool = False):
    """The decode GEMM of a PACKED activation as fp32 split-K partial slabs [S, M, N] (a view into
    the GEMM workspace, valid until the next split-K GEMM on this device's stream): no epilogue,
    no row scale.  ``wp`` (bf16 packed) or ``w8`` / ``w_scale`` (fp8 W8A16).  ``out`` is the
    caller's would-be output (not written; the op needs a tensor of the output's shape)."""
    f8 = w8 is not None
    N = 16 * (w8.shape[0] if f8 else wp.shape[0])
    K = 32 * (w8.shape[1] if f8 else wp.shape[1])
    S = rwk_split(M, N, K, f8)
    if S <= 0:
        raise RuntimeError(f"no split-K ring form for M={M}, N={N}, K={K}")
    if out is None:
        out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    flags = 1 | 256 | PART_FLAG | (ROT_FLAG if rot else 0)
    ws = gemm_workspace(x.device)
    if f8:
        torch.ops.mpamd.gemm_w8(x, w8, w_scale, out, None, 0, M, flags, ws, None, None, None, None, 1.0 / K, 0.0)
    else:
        torch.ops.mpamd.gemm(x, wp, out, None, 0, M, flags, ws, None, None, None, None, None, 1.0 / K, 0.0)
    return _slab_view(x.device, S, M, N)


def autotune_qkv_fold(N: int, K: int, device, fp8: bool = False, ms=(16, 32, 48, 64), iters: int = 24,
                      rounds: int = 3) -> dict:
    """Per M bucket: the qkv GEMM as partial slabs (no reduce launch) vs the kernel the GEMM
    autotuner chose for the full projection; the fold is kept where it wins by > 3 %.  Weights
    rotated over ~1 GiB of copies, as in ``autotune_gemm``."""
    device = torch.device(device)
    if device.type != "cuda" or os.environ.get("MPAMD_QKV_FOLD", "1") == "0":
        return {}
    todo = _todo(_QKV_FOLD_CAND, [k for k in dict.fromkeys((_m_bucket(M), N, K, bool(fp8)) for M in ms)
                                  if rwk_split(k[0], N, K, fp8) > 0])
    if not todo:
        return dict(_QKV_FOLD_CAND)
    copies = max(1, min(8, (1 << 30) // (N * K * (1 if fp8 else 2))))
    if fp8:
        ws = [torch.randint(0, 0x77, (N // 16, K // 32, 64, 8), dtype=torch.uint8, device=device)
              for _ in range(copies)]
        wsc = torch.full((N,), 1e-3, dtype=torch.float32, device=device)
    else:
        ws = [(torch.randn(N // 16, K // 32, 64, 8, device=device) * 0.02).to(torch.bfloat16) for _ in range(copies)]
    for M in ms:
        key = (_m_bucket(M), N, K, bool(fp8))
        if key not in todo or key in _QKV_FOLD_CAND or rwk_split(M, N, K, fp8) <= 0:
            continue
        xp = pack_act(torch.randn(M, K, device=device).to(torch.bfloat16))
        y = torch.empty(M, N, dtype=torch.bfloat16, device=device)

        def full(i):
            if fp8:
                linear_w8(xp, ws[i % copies], wsc, M, out=y)
            else:
                linear(xp, None, out=y, wp=ws[i % copies], a_rows=M)

        def part(i):
            if fp8:
                linear_partials(xp, M, w8=ws[i % copies], w_scale=wsc, out=y)
            else:
                linear_partials(xp, M, wp=ws[i % copies], out=y)

        t = _time_candidates({"full": full, "part": part}, iters, rounds)
        _QKV_FOLD_CAND[key] = t["part"] < 0.97 * t["full"]
    del ws
    return dict(_QKV_FOLD_CAND)


# ---------------------------------------------------------------------------------------
# FP8 (OCP e4m3fn) W8A8 decode GEMM (csrc/fp8.hip) - the Llama-3-70B fp8 MFMA path.
def pack_weight_fp8(w: torch.Tensor):
    """W [N, K] -> (Wq uint8 [N/16, K/64, 64, 16], per-output-channel scale fp32 [N])."""
    return ref.pack_weight_fp8(w)


def unpack_weight_fp8(wq: torch.Tensor, w_scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    return ref.unpack_weight_fp8(wq, w_scale, dtype)


def fp8_gemm_ok(M: int, N: int, K: int) -> bool:
    return 0 < M <= 64 and K % 256 == 0 and N % 32 == 0


def quant_act_fp8(xp: torch.Tensor, M: int, K: int, out=None, scale=None):
    """Packed bf16 decode activation -> (fp8 A8 uint8, per-row scale fp32; the first
    ceil(M/16)*16 entries are the row scales, the rest (GPU) is kernel scratch)."""
    if not _native(xp):
        a8, s = ref.quant_act_fp8(xp, M, K)
        if out is not None:
            out[: a8.numel()].copy_(a8)
            a8 = out
        if scale is not None:
            scale[: s.numel()].copy_(s)
            s = scale
        return a8, s
    if out is None:
        out = torch.empty(packed_numel(M, K), dtype=torch.uint8, device=xp.device)
    if scale is None:  # row scales, then the kernel's per-slice absmax scratch
        scale = torch.empty(((M + 15) // 16) * 16 * 33, dtype=torch.float32, device=xp.device)
    torch.ops.mpamd.quant_act_fp8(xp, out, scale, int(M), int(K))
    return out, scale


def quant_rows_fp8(x: torch.Tensor, out=None, scale=None):
    """Row-major bf16 x[M, K] -> (fp8 A8 in the fp8 GEMM's A layout, per-row scales)."""
    M, K = x.shape
    if not _native(x):
        a8, s = ref.quant_act_fp8(ref.pack_act(x), M, K)
        if out is not None:
            out[: a8.numel()].copy_(a8)
            a8 = out
        if scale is not None:
            scale[: s.numel()].copy_(s)
            s = scale
        return a8, s
    if out is None:
        out = torch.empty(packed_numel(M, K), dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty(((M + 15) // 16) * 16, dtype=torch.float32, device=x.device)
    torch.ops.mpamd.quant_rows_fp8(x, out, scale)
    return out, scale


_FP8_KERNELS = {"pk": 0, "rw": 1, "rwk": 2}
_FP8_CHOICE = {}  # (m_bucket, N, K, epilogue) -> fp8 kernel name, from autotune_fp8
_FP8_MODE = "auto"


def set_fp8_kernel(name: str) -> None:
    """fp8 decode GEMM form (csrc/fp8.hip): "auto" (autotuned table, else the balanced ring),
    "rw" (balanced ring, M > 16) or "pk" (one-group-per-workgroup) everywhere."""
    global _FP8_MODE
    assert name == "auto" or name in _FP8_KERNELS
    _FP8_MODE = name


def _fp8_kind(M: int, N: int, K: int, epilogue: int) -> int:
    if _FP8_MODE != "auto":
        return _FP8_KERNELS[_FP8_MODE]
    name = _FP8_CHOICE.get((_m_bucket(M), N, K, int(epilogue)))
    return -1 if name is None else _FP8_KERNELS[name]


def autotune_fp8(shapes, device, ms=(32, 48, 64), iters: int = 12, rounds: int = 3) -> dict:
    """``autotune_gemm`` for the fp8 GEMM: time both forms on each (N, K, epilogue) per M bucket
    (M <= 16 always runs the one-group form) on weights rotated over ~1 GiB, keep the faster."""
    global _FP8_MODE
    device = torch.device(device)
    if device.type != "cuda":
        return {}
    require_native()
    saved = _FP8_MODE
    try:
        for (N, K, epi) in shapes:
            todo = _todo_rows(_FP8_CHOICE, N, K, epi, ms)
            if not todo:
                continue
            copies = max(1, min(8, (1 << 30) // (N * K)))
            wqs = [torch.randint(0, 0x77, (N // 16, K // 64, 64, 16), dtype=torch.uint8, device=device)
                   for _ in range(copies)]
            wsc = torch.full((N,), 1e-3, dtype=torch.float32, device=device)
            ncols = N // 2 if epi == 1 else N
            for M in todo:
                a8 = torch.randint(0, 0x77, (packed_numel(M, K),), dtype=torch.uint8, device=device)
                asc = torch.ones(((M + 15) // 16) * 16, dtype=torch.float32, device=device)
                out = torch.empty(M, ncols, dtype=torch.bfloat16, device=device)

                def call(name, i):
                    global _FP8_MODE
                    _FP8_MODE = name
                    linear_fp8(a8, asc, wqs[i % copies], wsc, M, out=out, epilogue=epi)

                t = _time_candidates({k: partial(call, k) for k in _FP8_KERNELS}, iters, rounds)
                _FP8_CHOICE[(_m_bucket(M), N, K, int(epi))] = min(t, key=t.get)
            del wqs
    finally:
        _FP8_MODE = saved
    return dict(_FP8_CHOICE)


def linear_fp8(a8, a_scale, wq, w_scale, M: int, out=None, epilogue: int = 0, residual=None,
               out_packed: bool = False):
    """y = epilogue((a8 * a_scale) . (wq * w_scale)^T) for M <= 64 decode rows."""
    N = 16 * wq.shape[0]
    ncols = N // 2 if epilogue == 1 else N
    if not _native(a8):
        y = ref.linear_fp8(a8, a_scale, wq, w_scale, M, epilogue, residual)
        if out_packed:
            return ref.pack_act(y, out=out)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if out is None:
        out = _gemm_out(M, ncols, out_packed, torch.bfloat16, a8.device)
    kind = _fp8_kind(M, N, 64 * wq.shape[1], epilogue)
    torch.ops.mpamd.gemm_fp8(a8, a_scale, wq, w_scale, out, residual, int(epilogue), int(M), int(bool(out_packed)),
                             kind, gemm_workspace(a8.device) if kind == 2 else None)
    return out


# ---------------------------------------------------------------------------------------
# W8A16 decode GEMM (csrc/gemm.hip mp_gemm_w8): fp8 weights dequantized in registers into the
# bf16 MFMA, bf16 activations - the fused-norm decode path of an fp8 stage (no activation
# quantization launches).  Weight layout: the bf16 fragment order at 1 byte per element.
def w8_from_fp8(wq: torch.Tensor) -> torch.Tensor:
    """W8A8 layout uint8 [N/16, K/64, 64, 16] -> W8A16 layout [N/16, K/32, 64, 8] (same bytes:
    the two 32-deep k-slices of a 16-byte lane chunk become consecutive k-slices)."""
    n16, k64 = wq.shape[0], wq.shape[1]
    return wq.view(n16, k64, 64, 2, 8).permute(0, 1, 3, 2, 4).reshape(n16, 2 * k64, 64, 8).contiguous()


def fp8_from_w8(w8: torch.Tensor) -> torch.Tensor:
    n16, k32 = w8.shape[0], w8.shape[1]
    return w8.view(n16, k32 // 2, 2, 64, 8).permute(0, 1, 3, 2, 4).reshape(n16, k32 // 2, 64, 16)


def unpack_weight_w8(w8: torch.Tensor, w_scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    return ref.unpack_weight_fp8(fp8_from_w8(w8), w_scale, dtype)


_W8_KERNELS = {"rw": 128, "rwk": 256, "rwki": 256 | 512}
_W8_CHOICE = {}  # (m_bucket, N, K, epilogue) -> "rw" / "rwk", from autotune_w8
_W8_MODE = "auto"  # or a _W8_KERNELS name forced everywhere it applies (tests, A/B runs)


def _w8_kernel(M: int, N: int, K: int, epilogue: int) -> str:
    rwk_ok = epilogue != 1 and N % 2048 == 0
    mode = _W8_MODE if _W8_MODE != "auto" else _W8_CHOICE.get((_m_bucket(M), N, K, int(epilogue)), "rw")
    if _base(mode) in ("rwk", "rwki") and rwk_ok:
        return mode
    return "rw+r" if mode.endswith("+r") else "rw"


def linear_w8(x, w8, w_scale, a_rows: int, out=None, epilogue: int = 0, residual=None, out_packed: bool = False,
              ss_in=None, eps: float = 0.0, ap_out=None, ss_out=None, ss_zero=None):
    """``linear`` with an fp8 weight (``w8_from_fp8`` layout + per-column scales) and a PACKED
    bf16 activation of ``a_rows`` rows (M <= 64): same epilogues as the bf16 decode GEMM
    (0 with optional ``ss_in`` row scale, packed SwiGLU, 3 = residual-stream producer)."""
    M = int(a_rows)
    N, K = 16 * w8.shape[0], 32 * w8.shape[1]
    if not _native(x):
        return linear(x, None, out=out, epilogue=epilogue, residual=residual, wp=pack_weight(
            unpack_weight_w8(w8, w_scale, x.dtype)), a_rows=M, out_packed=out_packed, ss_in=ss_in, eps=eps,
            ap_out=ap_out, ss_out=ss_out, ss_zero=ss_zero)
    ncols = N // 2 if epilogue == 1 else N
    if out is None:
        out = _gemm_out(M, ncols, out_packed, x.dtype, x.device)
    kern = _w8_kernel(M, N, K, epilogue)
    flags = 1 | (2 if out_packed else 0) | _W8_KERNELS[_base(kern)] | (ROT_FLAG if kern.endswith("+r") else 0)
    torch.ops.mpamd.gemm_w8(x, w8, w_scale, out, residual, int(epilogue), M, flags,
                            gemm_workspace(x.device) if _base(kern) in ("rwk", "rwki") else None, ap_out, ss_out,
                            ss_zero, ss_in,
                            1.0 / K, float(eps))
    return out


# ---------------------------------------------------------------------------------------
# Grouped W8A16 GEMMs of a sparse-MoE MLP (csrc/gemm_moe.hip): every expert of a layer in two
# launches.  Weights: the W8A16 layout stacked per expert, uint8 [E, N/16, K/32, 64, 8] + fp32 [E, N];
# ``cnt`` int32 [E]: tokens routed to each expert (0: the expert is skipped on the device - neither
# its weights nor its activation slab are read); ``wd`` fp32 [M, E]: the dense routing matrix
# (ops.moe.dense_weights).  Between the two launches the SwiGLU outputs travel as E consecutive
# packed activations of ``packed_numel(M, F)`` elements.
_MOE_OK = {}


def moe_w8_ok(M: int, E: int, H: int, F: int) -> bool:
    """Whether both grouped kernels cover the shape (M <= 64 rows; a dry dispatch, as ``w4_gemm_ok``)."""
    key = (int(M), int(E), int(H), int(F))
    if key not in _MOE_OK:
        _MOE_OK[key] = bool(native_available() and torch.ops.mpamd.moe_w8_ok(*key))
    return _MOE_OK[key]


def _moe_dims(w8: torch.Tensor, w_scale: torch.Tensor, cnt: torch.Tensor, M: int):
    """(E, N, K) of stacked expert weights, with the checks both grouped ops share."""
    if w8.dim() != 5 or tuple(w8.shape[3:]) != (64, 8) or w8.dtype != torch.uint8:
        raise ValueError("w8 must be stacked fp8 expert weights uint8 [E, N/16, K/32, 64, 8]")
    E, N, K = w8.shape[0], 16 * w8.shape[1], 32 * w8.shape[2]
    if tuple(w_scale.shape) != (E, N) or w_scale.dtype != torch.float32:
        raise ValueError(f"w_scale must be fp32 [E, N] = [{E}, {N}]")
    if cnt.numel() != E or cnt.dtype != torch.int32:
        raise ValueError(f"cnt must be int32 [{E}] routed-token counts")
    if not 0 <= M <= 64:
        raise ValueError(f"the grouped MoE GEMMs take 0..64 rows, got {M}")
    return E, N, K


def moe_gate_up_w8(x, w8, w_scale, cnt, a_rows: int, out=None):
    """act[e] = SwiGLU(x @ gate_up[e]^T) for every routed expert, one launch: ``x`` packed bf16
    (``a_rows`` rows), output E packed slabs (an unrouted expert's slab is left untouched).  A routed
    slab holds the bits of ``linear_w8(x, w8[e], w_scale[e], a_rows, epilogue=1, out_packed=True)`` on
    the ring form."""
    M = int(a_rows)
    E, N, K = _moe_dims(w8, w_scale, cnt, M)
    F_ = N // 2
    slab = packed_numel(M, F_)
    if out is None:
        out = torch.zeros(E * slab, dtype=x.dtype, device=x.device)
    if not _native(x):
        xr = ref.unpack_act(x, M, K)
        for e, c in enumerate(cnt.tolist()):
            if c <= 0:
                continue
            y = (xr.float() @ unpack_weight_w8(w8[e], w_scale[e], torch.float32).t()).to(x.dtype)
            ref.pack_act(ref.swiglu(y), out=out[e * slab:(e + 1) * slab])  # SwiGLU output rounded to bf16
        return out
    torch.ops.mpamd.moe_gate_up_w8(x, w8, w_scale, cnt, out, M)
    return out


def moe_down_w8(act, w8, w_scale, cnt, wd, a_rows: int, out=None):
    """y [M, H] = bf16(sum over routed experts e of wd[:, e] * (act[e] @ down[e]^T)), one launch:
    channel scales and routing weights applied in fp32, ONE bf16 rounding of the combined sum."""
    M = int(a_rows)
    E, N, K = _moe_dims(w8, w_scale, cnt, M)
    if tuple(wd.shape) != (M, E) or wd.dtype != torch.float32:
        raise ValueError(f"wd must be the fp32 [{M}, {E}] dense routing matrix")
    if out is None:
        out = torch.empty(M, N, dtype=act.dtype, device=act.device)
    if not _native(act):
        slab = packed_numel(M, K)
        tot = torch.zeros(M, N, dtype=torch.float32)
        for e, c in enumerate(cnt.tolist()):
            if c <= 0:
                continue
            a = ref.unpack_act(act[e * slab:(e + 1) * slab], M, K)
            tot += wd[:, e:e + 1] * (a.float() @ unpack_weight_w8(w8[e], w_scale[e], torch.float32).t())
        out.copy_(tot.to(out.dtype))
        return out
    torch.ops.mpamd.moe_down_w8(act, w8, w_scale, cnt, wd, out, M)
    return out


# ---------------------------------------------------------------------------------------
# W4A16 decode GEMM (csrc/gemm_w4.hip mp_gemm_w4): OCP MXFP4 weights - e2m1 codes, one e8m0 scale
# per 32 weights along K, 4.25 bits per weight - dequantized in registers into the bf16 MFMA
# (v_cvt_scalef32_pk_bf16_fp4), bf16 activations.  Weight layout, in the bf16 fragment order:
#   w4 uint8 [N/16, K/128, 64, 16]: lane = 16 q + c; byte 4 s + b = the codes of
#       W[16 nt + c][128 kb + 32 s + 8 q + 2 b] (low nibble) and the next k (high nibble): one
#       16-byte lane load is the lane's 8 weights of each of four consecutive 32-deep k-slices s;
#   s4 uint8 [N/16, K/128, 16, 4]: column c, one scale byte per k-slice (its four q groups share it).
def pack_weight_w4(w: torch.Tensor):
    """W [N, K] (N % 16 == 0, K % 128 == 0) -> (w4, s4), quantized by the OCP MX rule
    (``reference.quant_mxfp4``); runs on CPU and GPU tensors."""
    return ref.pack_weight_w4(w)


def unpack_weight_w4(w4: torch.Tensor, s4: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """MXFP4 -> row-major W [N, K] (exact: code x 2^(e - 127) is a bf16 value).  GPU tensors go
    through the HIP dequantizer (one launch) when the kernel library is loaded."""
    if w4.is_cuda and native_available():
        w = torch.ops.mpamd.dequant_w4(w4, s4)
        return w if dtype == torch.bfloat16 else w.to(dtype)
    return ref.unpack_weight_w4(w4, s4, dtype)


_W4_OK = {}


def w4_gemm_ok(M: int, N: int, K: int, epilogue: int = 0) -> bool:
    """Whether the W4A16 ring kernel covers the shape (M <= 64; epilogue 0, 1 = packed SwiGLU, 3)."""
    key = (int(M), int(N), int(K), int(epilogue))
    if key not in _W4_OK:
        _W4_OK[key] = bool(native_available() and torch.ops.mpamd.gemm_w4_ok(*key))
    return _W4_OK[key]


def linear_w4(x, w4, s4, a_rows: int, out=None, epilogue: int = 0, residual=None, out_packed: bool = False,
              ss_in=None, eps: float = 0.0, ap_out=None, ss_out=None, ss_zero=None):
    """``linear`` with an MXFP4 weight (``pack_weight_w4``) and a PACKED bf16 activation of
    ``a_rows`` rows (M <= 64): the one-launch ring kernel with the fused-norm path's epilogues (0
    with optional ``ss_in`` row scale, packed SwiGLU, 3 = residual-stream producer).  A shape the
    kernel does not cover raises.  Out of scope for 4-bit weights: the split-K ring,
    ``linear_partials`` / the qkv fold, a start-up autotuner, W4A8 / W4A4 on the block-scaled
    MFMA, and MoE / tensor-parallel / offloaded stages."""
    M = int(a_rows)
    N, K = 16 * w4.shape[0], 128 * w4.shape[1]
    if not _native(x):
        return linear(x, None, out=out, epilogue=epilogue, residual=residual, wp=pack_weight(
            unpack_weight_w4(w4, s4, x.dtype)), a_rows=M, out_packed=out_packed, ss_in=ss_in, eps=eps,
            ap_out=ap_out, ss_out=ss_out, ss_zero=ss_zero)
    ncols = N // 2 if epilogue == 1 else N
    if out is None:
        out = _gemm_out(M, ncols, out_packed, x.dtype, x.device)
    torch.ops.mpamd.gemm_w4(x, w4, s4, out, residual, int(epilogue), M, 1 | (2 if out_packed else 0), ap_out, ss_out,
                            ss_zero, ss_in, 1.0 / K, float(eps))
    return out


# ---------------------------------------------------------------------------------------
# W8A8-MX decode GEMM (csrc/gemm_mx.hip): the W8A16 fp8 weights x MX e4m3 activations (e8m0 scale
# per 32-element block) on gfx950's block-scaled MFMA, split-K ring form + reduce launch.
def mx_buffers(M: int, K: int, device):
    """(ax, as) buffers of ``quant_mx`` for M rows x K."""
    rows = 16 * ((int(M) + 15) // 16)
    return (torch.empty(rows * K, dtype=torch.uint8, device=device),
            torch.full((2 * K,), 127, dtype=torch.uint8, device=device))  # [K/128][64][4]


def quant_mx(xp: torch.Tensor, M: int, K: int, ax=None, as_=None):
    """Packed bf16 activation (M rows, K) -> MX e4m3 bytes + e8m0 block scales (gemm_mx.hip layout)."""
    if ax is None or as_ is None:
        ax, as_ = mx_buffers(M, K, xp.device)
    torch.ops.mpamd.quant_mx(xp, ax, as_, int(M), int(K))
    return ax, as_


def mx_block_quant(x: torch.Tensor) -> torch.Tensor:
    """fp32 reference of ``quant_mx`` + dequantization on row-major x[M, K]: the values the MX GEMM
    multiplies.  Block map (gemm_mx.hip): k = 128 kb + 32 s + 8 q + j, block (s >> 1, q >> 1)."""
    M, K = x.shape
    v = x.to(torch.bfloat16).float().view(M, K // 128, 2, 2, 2, 2, 8)  # [M, kb, sh, sl, qh, ql, j]
    amax = v.abs().amax(dim=(3, 5, 6), keepdim=True)
    t = amax / 448.0
    m, ex = torch.frexp(t)
    e = torch.where(m > 0.5, ex, ex - 1).clamp(-126, 126)  # ceil(log2(amax / 448))
    e = torch.where(amax > 0, e, torch.zeros_like(e)).float()
    q = (v * torch.exp2(-e)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
    return (q * torch.exp2(e)).view(M, K)


def linear_mx(ax, as_, w8, w_scale, a_rows: int, out=None, epilogue: int = 0, residual=None, ss_in=None,
              eps: float = 0.0, ap_out=None, ss_out=None, ss_zero=None, partials: bool = False, rot: bool = False):
    """The W8A8-MX decode GEMM (M <= 64): epilogue 0 (optional ``ss_in`` row scale) or 3 (residual-
    stream producer), or with ``partials`` the fp32 split-K slabs [S, M, N] (a workspace view, as
    ``linear_partials``)."""
    M = int(a_rows)
    N, K = 16 * w8.shape[0], 32 * w8.shape[1]
    ws = gemm_workspace(ax.device)
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=ax.device)
    flags = 1 | 256 | (PART_FLAG if partials else 0) | (ROT_FLAG if rot else 0)
    torch.ops.mpamd.gemm_mx(ax, as_, w8, w_scale, out, residual, int(epilogue), M, flags, ws, ap_out, ss_out, ss_zero,
                            ss_in, 1.0 / K, float(eps))
    if partials:
        return _slab_view(ax.device, rwk_split(M, N, K, 2), M, N)
    return out


def autotune_w8(shapes, device, ms=(4, 16, 32, 48, 64), iters: int = 12, rounds: int = 3) -> dict:
    """``autotune_gemm`` for the W8A16 GEMM: ring vs split-K ring per (N, K, epilogue) and M
    bucket, on fp8 weights rotated over ~1 GiB (decode never finds them in the Infinity Cache)."""
    global _W8_MODE
    device = torch.device(device)
    if device.type != "cuda":
        return {}
    require_native()
    gemm_workspace(device)
    saved = _W8_MODE
    try:
        for (N, K, epi) in shapes:
            todo = _todo_rows(_W8_CHOICE, N, K, epi, ms)
            if not todo:
                continue
            # the ring form only (SwiGLU / narrow N) or all three, each also with the rotated k walk
            names = ["rw"] if (epi == 1 or N % 2048) else list(_W8_KERNELS)
            names = names + [n + "+r" for n in names]
            copies = max(1, min(8, (1 << 30) // (N * K)))
            wqs = [torch.randint(0, 0x77, (N // 16, K // 32, 64, 8), dtype=torch.uint8, device=device)
                   for _ in range(copies)]
            wsc = torch.full((N,), 1e-3, dtype=torch.float32, device=device)
            for M in todo:
                xp = pack_act(torch.randn(M, K, device=device).to(torch.bfloat16))
                res = torch.zeros(M, N, dtype=torch.bfloat16, device=device) if epi == 3 else None
                extra = _epi3_scratch(M, N, device) if epi == 3 else {}
                out = res if epi == 3 else _gemm_out(M, N // 2 if epi == 1 else N, epi == 1, torch.bfloat16, device)

                def call(name, i):
                    global _W8_MODE
                    _W8_MODE = name
                    linear_w8(xp, wqs[i % copies], wsc, M, out=out, epilogue=epi, residual=res,
                              out_packed=epi == 1, **extra)

                t = _time_candidates({k: partial(call, k) for k in names}, iters, rounds)
                # the best plain form, rotated unless the rotation measures > 1 % slower: isolated
                # timings under-rank it (Llama-3-70B fp8 64 sessions, all forms rotated: 17.47 ->
                # 17.23 ms; the isolated choice had kept three of four shapes plain, profiles/r3_70)
                plain = min((n for n in t if not n.endswith("+r")), key=t.get)
                _W8_CHOICE[(_m_bucket(M), N, K, int(epi))] = \
                    plain + "+r" if t[plain + "+r"] <= 1.01 * t[plain] else plain
            del wqs
    finally:
        _W8_MODE = saved
    return dict(_W8_CHOICE)


# ---------------------------------------------------------------------------------------
# Batched LoRA (csrc/lora.hip): rows of one ragged step carry the slot of their adapter, int32 in
# [-1, S); slot -1 is a base-model row, which neither op reads or writes.  Stacked adapter matrices
# ``A`` [S, R, K], ``B`` [S, N, R] and ``scale`` fp32 [S] (models/adapters.py); for every row m with
# s = slots[m] >= 0
#     t[m]  = scale[s] * (A[s] x[m])                       fp32 [R], never rounded to bf16
#     y[m]  = dtype( fp32(y[m]) + fp32(B[s]) t[m] )        one more rounding of the stored y
# A row's result depends on its own x, slot and the shape alone - never on the other rows' slots.
_LORA_OK = {}


def lora_ok(M: int, N: int, K: int, R: int) -> bool:
    """Whether the two kernels cover the shape: 1 <= M <= 64, K % 32 == 0, N % 8 == 0, R % 16 == 0,
    R <= 192 (a dry dispatch where the library is loaded, as ``moe_w8_ok``)."""
    key = (int(M), int(N), int(K), int(R))
    if key not in _LORA_OK:
        if native_available():
            _LORA_OK[key] = bool(key[0] >= 1 and torch.ops.mpamd.lora_ok(*key))
        else:
            _LORA_OK[key] = bool(1 <= key[0] <= 64 and key[1] > 0 and key[1] % 8 == 0 and key[2] > 0 and
                                 key[2] % 32 == 0 and 0 < key[3] <= 192 and key[3] % 16 == 0)
    return _LORA_OK[key]


def _lora_dims(mats: torch.Tensor, name: str, slots: torch.Tensor, t: Optional[torch.Tensor], M: int):
    """(S, rows, cols) of an adapter stack, with the checks both LoRA ops share."""
    if mats.dim() != 3 or not mats.is_contiguous():
        raise ValueError(f"{name} must be a contiguous adapter stack [S, rows, cols], got {tuple(mats.shape)}")
    if slots.dtype != torch.int32 or slots.dim() != 1 or slots.numel() < M or slots.device != mats.device:
        raise ValueError(f"slots must be int32 [{M}] on the adapters' device")
    if M < 0:
        raise ValueError(f"the LoRA ops take M >= 0 rows, got {M}")
    R = mats.shape[1] if name == "A" else mats.shape[2]
    if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < M or t.shape[1] != R or
                          not t.is_contiguous() or t.device != mats.device):
        raise ValueError(f"t must be contiguous fp32 [{M}, {R}] on the adapters' device")
    return mats.shape[0], mats.shape[1], mats.shape[2]


def _lora_rows(slots: torch.Tensor, M: int, S: int):
    """(row indices, their slots) of the rows with a slot in [0, S) - the torch forms' gather."""
    sl = slots[:M].long()
    idx = torch.nonzero((sl >= 0) & (sl < S)).flatten()
    return idx, sl[idx]


def lora_shrink(x, A, scale, slots, a_rows: int, out=None):
    """t fp32 [M, R]: ``x`` packed (``a_rows`` = M rows of K, M <= 64 on the GPU).  Rows with slot -1
    are not written (``out`` keeps what it held; a fresh one holds zeros)."""
    M = int(a_rows)
    if out is None:
        out = torch.zeros(M, A.shape[1] if A.dim() == 3 else 0, dtype=torch.float32, device=A.device)
    S, R, K = _lora_dims(A, "A", slots, out, M)
    if scale.dtype != torch.float32 or scale.numel() != S:
        raise ValueError(f"scale must be fp32 [{S}]")
    if x.numel() < packed_numel(M, K):
        raise ValueError(f"packed x holds fewer than {M} rows of {K}")
    if M == 0:
        return out
    if not _native(x):
        xr = ref.unpack_act(x, M, K)
        for m, s in zip(*map(torch.Tensor.tolist, _lora_rows(slots, M, S))):  # row by row: a row's bits
            out[m] = scale[s] * torch.mv(A[s].float(), xr[m].float())       # never depend on the others
        return out
    torch.ops.mpamd.lora_shrink(x, A, scale, slots, out, M)
    return out


def lora_expand(t, B, slots, y):
    """``y`` [M, N] (row-major, any row stride that is a multiple of 8) updated in place."""
    M = int(y.shape[0])
    S, N, R = _lora_dims(B, "B", slots, t, M)
    if y.dim() != 2 or y.shape[1] != N or y.stride(1) != 1 or y.dtype != B.dtype:
        raise ValueError(f"y must be [M, {N}] rows of the adapters' dtype with unit inner stride")
    if M == 0:
        return y
    if not _native(y):
        for m, s in zip(*map(torch.Tensor.tolist, _lora_rows(slots, M, S))):
            y[m] = (y[m].float() + torch.mv(B[s].float(), t[m])).to(y.dtype)
        return y
    torch.ops.mpamd.lora_expand(t, B, slots, y)
    return y


def lora_runs(slots) -> list:
    """Maximal runs (row0, row1, slot) of consecutive rows with the same slot >= 0, from the
    host-side slots of a plan (no device read)."""
    runs, r0 = [], 0
    sl = [int(s) for s in slots]
    for i in range(1, len(sl) + 1):
        if i == len(sl) or sl[i] != sl[r0]:
            if sl[r0] >= 0:
                runs.append((r0, i, sl[r0]))
            r0 = i
    return runs


def lora_update(x, y, A, B, scale, runs):
    """The whole update in torch, by runs, on row-major ``x`` [T, K] and ``y`` [T, N] (in place):
    the form of steps the kernels do not take (more than 64 rows, prefill, CPU stages), with the
    semantics above - fp32 ``t``, one rounding into ``y``'s dtype."""
    for r0, r1, s in runs:
        t = scale[s] * (x[r0:r1].float() @ A[s].float().t())
        y[r0:r1] = (y[r0:r1].float() + t @ B[s].float().t()).to(y.dtype)
    return y
