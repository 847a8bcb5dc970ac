"""StageExecutor: one pipeline stage (a contiguous block range) on one device.

Replaces the reference's Stage0 / StageSegment / StageLast modules
(reference src/llama_partition.py:76-474) and the optimized HF layer they wrap
(petals/llama/block.py:39-248) with an MI355X-first step function:

* weights resident in HBM (no per-forward CPU<->GPU layer streaming),
* a paged KV cache written in place by the fused RoPE kernel,
* ragged batches: any mix of sessions, each contributing ``n_tokens`` (prefill chunks,
  decode steps, replays) executed as ONE forward over the concatenated tokens,
* one layer loop per step, chosen by ``StageExecutor._step_path`` from the step's row count T (prefill chunks
  and decode steps alike), its deep prompt and its adapters; the first that applies:
  - "w8a8": fp8 weights under MPAMD_FP8_MODE=w8a8, T <= 64: fp8 MFMA GEMMs, activations quantized per row;
  - "fused" (the default decode path): dense bf16 / W8A16 / MXFP4 stages, T <= 64 (bf16: up to 256 where the
    wide kernels cover it): 5 launches per layer - qkv, RoPE + attention, o, gate/up, down; no norm kernels,
    the GEMM epilogues carry the residual stream and its row statistics;
  - "moe_w8": fp8 Mixtral, T <= 64: packed activations, norm kernels, W8A16 qkv / o, grouped experts;
  - "packed": other steps of T <= 256 with every projection packed for the native GEMMs (no fused path,
    Mixtral, 65..256 rows, LoRA steps of <= 64 rows): 7 launches per layer - add+RMSNorm, qkv, RoPE +
    attention, o, add+RMSNorm, gate/up with SwiGLU, down - on activations in the MFMA-fragment layout;
  - "dense": everything else (CPU, prefill, deep prompts, --gemm hipblaslt): those 7 on row-major activations;
* decode steps replayed from hipGraphs captured per (batch bucket, context bucket);
* the last stage applies the final norm and ``lm_head`` to the LAST token of each
  sequence only (the reference projects every prefill position, src/llama_partition.py:470).

Attention is causal for prefill (the reference's optimized layer gets no mask and is
NOT causal: src/llama_partition.py:118 -> petals/llama/block.py:136-137).
"""
from __future__ import annotations

import dataclasses
import gc
import logging
import math
import os
import threading
import types
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import native, ops
from ..ops import moe
from ..models.config import ModelConfig
from ..models.weights import StageWeights
from .kv_cache import KV_DTYPES, PagedKVCache
from .session import SessionManager, SessionState

logger = logging.getLogger(__name__)

# per-path weight tensors a layer loop reads (what CPU offload streams)
_PACKED_FIELDS = ("input_norm", "post_norm", "qkv_p", "o_p", "gate_up_p", "down_p", "router_p")
_DENSE_FIELDS = ("input_norm", "post_norm", "qkv", "o", "gate_up", "down", "router")
_GPT2_FIELDS = ("ln1_w", "ln1_b", "attn_w", "attn_b", "proj_w", "proj_b", "ln2_w", "ln2_b", "fc_w", "fc_b",
                "fc2_w", "fc2_b")


@dataclasses.dataclass
class Plan:
    """Host-side description of one ragged step.

    ``h64`` / ``h32`` are the step's metadata in pinned host memory; the device copies
    (``meta()``) are made on first use.  A graph-replayed decode step never
    touches them: it stages the padded metadata of its batch bucket in ONE host-to-device
    copy of its own (``_DecodeGraph.replay``)."""
    sessions: List[SessionState]
    ntoks: np.ndarray
    starts: np.ndarray
    T: int
    max_ctx: int
    is_decode: bool
    h64: np.ndarray                     # [2, T] positions, slots (pinned host view)
    h32: np.ndarray                     # [2*T + S] q_seq, q_ctx, last_rows (pinned host view)
    qblocks: Optional[torch.Tensor] = None  # [2, NB] MFMA-attention query blocks (prefill steps)
    superblocks: Optional[torch.Tensor] = None  # [2, NSB] runs of <= 4 blocks (grouped prefill kernel)
    fablocks: Optional[torch.Tensor] = None  # [2, NBF] FA2 prefill workgroup blocks (csrc/attention_fa.hip)
    fa_waves: int = 4                   # waves per FA2 workgroup (ops.fa_plan)
    lora_slots: Optional[np.ndarray] = None  # int32 [T] adapter slot of every row; None: a base-model step
    # ``logit_rows`` steps: (rows whose logits the step returns, in output order; where the sequences' last
    # rows sit in that order; where the other rows sit)
    extra: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]] = None
    _extra_dev: Optional[tuple] = None
    _lora_dev: Optional[torch.Tensor] = None
    _dev: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
    _upload: Optional[object] = None    # callable making the device copies

    def meta(self):
        """(positions, slots, q_seq, q_ctx, last_rows) on the device: the metadata tensors of a ``_Step``."""
        if self._dev is None:
            self._dev = self._upload()
        (i64, i32), T = self._dev, self.T
        return i64[0], i64[1], i32[:T], i32[T:2 * T], i32[2 * T:]

    def extra_rows(self, device):
        """``_Step.extra`` of a ``logit_rows`` step: (the rows besides the last rows, int32; output positions of
        the last rows; of the other rows; every returned row in output order), on the device."""
        if self.extra is None:
            return None
        if self._extra_dev is None:
            rows, lp, ep = self.extra
            parts = (rows[ep], lp, ep, rows)
            blob = torch.from_numpy(np.concatenate(parts)).to(device)  # one host-to-device copy
            more, lp_d, ep_d, rows_d = torch.split(blob, [len(a) for a in parts])
            self._extra_dev = (more.to(torch.int32), lp_d, ep_d, rows_d)
        return self._extra_dev

    def lora(self, device):
        """(device slots int32 [T], host runs) of a LoRA step: ``_Step.lora``."""
        if self._lora_dev is None:
            self._lora_dev = torch.from_numpy(self.lora_slots).to(device, non_blocking=True)
        return self._lora_dev, ops.lora_runs(self.lora_slots)


@dataclasses.dataclass
class _Step:
    """What one forward pass of a Llama-family stage reads: built by ``run`` from a ``Plan`` and by a
    ``_DecodeGraph`` from its static tensors.  ``_begin`` fills in ``part`` (where None) and ``ws``."""
    x: torch.Tensor                     # token ids [T] (first stage) or hidden [T, H]
    positions: torch.Tensor
    slots: torch.Tensor
    q_seq: torch.Tensor
    q_ctx: torch.Tensor
    last_rows: torch.Tensor
    T: int
    max_ctx: int
    decode: bool
    device: torch.device                # where, and in which dtype, ``buf`` allocates
    dtype: torch.dtype
    part: Optional[Tuple[int, int]] = None  # (part_size, num_parts) of the split-K attention kernels
    ws: Optional[torch.Tensor] = None
    qblocks: Optional[torch.Tensor] = None      # prefill steps: Plan.qblocks / superblocks / fablocks / fa_waves
    superblocks: Optional[torch.Tensor] = None
    fablocks: Optional[torch.Tensor] = None
    fa_waves: int = 4
    prompt: Optional[tuple] = None      # deep prompt (rows [R], values [n_layers, R, H])
    lora: Optional[tuple] = None        # (device slots int32 [T], host runs or None); None: a base-model step
    extra: Optional[tuple] = None       # ``Plan.extra_rows``: more logit rows than the last ones (verify steps)
    bufs: dict = dataclasses.field(default_factory=dict)  # named buffers the caller keeps (else allocated)

    def buf(self, name: str, shape, dtype=None) -> torch.Tensor:
        if name in self.bufs:
            return self.bufs[name]
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.device)


_NO_LORA = types.SimpleNamespace(qkv=None, o=None, gate_up=None, down=None)  # a base step's adapter layer: no target


class _Pinned:
    """Double-buffered pinned host staging for per-step metadata (async H2D without races)."""

    def __init__(self, n_i64: int, n_i32: int, device):
        self.device = torch.device(device)
        pin = self.device.type == "cuda"
        self.i64 = [torch.empty(n_i64, dtype=torch.int64, pin_memory=pin) for _ in range(2)]
        self.i32 = [torch.empty(n_i32, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self.events = [None, None]
        self.k = 0

    def next(self):
        self.k ^= 1
        ev = self.events[self.k]
        if ev is not None:
            ev.synchronize()
        return self.i64[self.k], self.i32[self.k]

    def mark(self):
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            self.events[self.k] = ev


# what a stage does with a config's ``sliding_window``: cap sessions at it, or attend through it
SLIDING_WINDOW_MODES = ("cap", "attend")


class StageExecutor:
    def __init__(self, cfg: ModelConfig, weights: StageWeights, device, *, dtype=torch.bfloat16,
                 page_size: int = 64, max_sessions: int = 256, max_seq_len: Optional[int] = None,
                 kv_cache_bytes: Optional[int] = None, kv_fraction: float = 0.9, use_graphs: Optional[bool] = None,
                 graph_max_batch: int = 256, max_tokens_per_step: int = 8192, offload: bool = False,
                 keep_layers_on_gpu: int = 0, tp=None, warmup: Optional[bool] = None,
                 kv_cache_dtype: str = "bf16", sliding_window: str = "cap"):
        """``tp``: a ``parallel.tensor_parallel.TPGroup`` when ``weights`` is a tensor-parallel
        shard (``cfg`` is then the shard config); partial sums are all-reduced after the
        o and down projections.  ``kv_cache_dtype="fp8"``: e4m3 pages + e8m0 row scales
        (runtime/kv_cache.py); attention then runs the fp8 forms of the flash-decoding, MFMA GQA decode
        and FA2 prefill kernels (``_attend``).  ``sliding_window`` (configs with ``sliding_window``
        W, e.g. Mistral): "cap" limits sessions to W tokens, inside which full causal attention is
        the windowed one; "attend" lets them grow to ``max_seq_len``: every query attends to its last
        W keys only (``window`` of the decode and FA2 prefill kernels) and the session's KV pages roll
        (runtime/session.py).  GPT-2 and configs without a window ignore it."""
        cfg.validate()
        if sliding_window not in SLIDING_WINDOW_MODES:
            raise ValueError(f"sliding_window must be one of {SLIDING_WINDOW_MODES}, got {sliding_window!r}")
        if kv_cache_dtype not in KV_DTYPES:
            raise ValueError(f"kv_cache_dtype must be one of {KV_DTYPES}, got {kv_cache_dtype!r}")
        if kv_cache_dtype == "fp8" and cfg.model_type == "gpt2":
            raise ValueError("the fp8 KV cache needs the RoPE attention path: GPT-2 keeps a bf16 cache")
        if kv_cache_dtype == "fp8" and cfg.head_dim not in (64, 128):
            raise ValueError(f"the fp8 KV cache supports head_dim 64 and 128, got {cfg.head_dim}")
        self.kv_cache_dtype = kv_cache_dtype
        self._kv_fp8 = kv_cache_dtype == "fp8"
        if offload and cfg.is_moe:
            # the streamed slot layers carry only the per-path projection fields; the MoE MLP
            # also reads the router and per-expert row-major weights.  Mixtral-8x7B (93 GB bf16)
            # fits one MI355X resident, so offload is rejected rather than half-supported.
            raise ValueError("CPU offload is not supported for MoE (Mixtral) models: serve them resident")
        self._tp = tp if (tp is not None and getattr(tp, "active", tp.size > 1)) else None
        # LoRA adapters (StageWeights.load_adapters): dense 16-bit Llama stages, resident, one device
        self._lora = getattr(weights, "lora", None)
        if self._lora is not None:
            for bad, what in ((cfg.model_type == "gpt2", "GPT-2"), (cfg.is_moe, "MoE (Mixtral) models"),
                              (weights.fp8 or weights.w4, "fp8 or MXFP4 weights"),
                              (self._tp is not None, "tensor parallelism"), (bool(offload), "CPU offload"),
                              (ops.gemm_policy() == "hipblaslt", "--gemm hipblaslt (MPAMD_GEMM=hipblaslt)")):
                if bad:
                    raise ValueError(f"adapters with {what} are not built")
        self._lora_graphs: Dict[tuple, "_DecodeGraph"] = {}
        self.cfg = cfg
        self.w = weights
        self.device = torch.device(device)
        self.dtype = dtype
        self.n_layers = len(weights.layers)
        self.start, self.end = weights.start, weights.end
        self.is_first = weights.has_embed
        self.is_last = weights.has_head
        self.nh, self.nkv, self.D = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        self.scale = 1.0 / math.sqrt(self.D)
        self.max_seq_len = int(max_seq_len or cfg.max_position_embeddings)
        # the window every attention call gets (0: none): sessions run past it and their pages roll
        self.window = int(cfg.sliding_window) if (sliding_window == "attend" and cfg.sliding_window and
                                                   cfg.model_type != "gpt2") else 0
        self.sliding_window = "attend" if self.window else ("cap" if cfg.sliding_window else None)
        if cfg.sliding_window and not self.window and self.max_seq_len > cfg.sliding_window:
            # Mistral / Mixtral sliding-window attention: sessions are capped at the window, inside
            # which sliding-window and full causal attention are the same computation
            logger.info(f"max_seq_len capped at sliding_window={cfg.sliding_window}")
            self.max_seq_len = int(cfg.sliding_window)
        self.max_tokens = max_tokens_per_step
        if cfg.model_type != "gpt2":
            self.cos, self.sin = ops.rope_cos_sin(self.D, self.max_seq_len, cfg.rope_theta, self.device,
                                                  cfg.rope_scaling)
        if kv_cache_bytes is None:
            kv_cache_bytes = PagedKVCache.auto_budget_bytes(self.device, fraction=kv_fraction)
        num_pages = PagedKVCache.pages_for_bytes(kv_cache_bytes, self.n_layers, self.nkv, self.D, page_size,
                                                 kv_dtype=kv_cache_dtype)
        max_useful = max_sessions * math.ceil(self.max_seq_len / page_size)
        num_pages = max(1, min(num_pages, max_useful))
        self.cache = PagedKVCache(self.n_layers, num_pages, self.nkv, self.D, page_size, dtype, self.device,
                                  kv_dtype=kv_cache_dtype)
        self.sessions = SessionManager(self.cache, max_sessions, self.max_seq_len, window=self.window)
        self.use_graphs = (self.device.type == "cuda") if use_graphs is None else bool(use_graphs)
        self.use_graphs = self.use_graphs and self.device.type == "cuda" and cfg.model_type != "gpt2" and \
            os.environ.get("MPAMD_GRAPHS", "1") != "0"
        if self._tp is not None and not getattr(self._tp, "capturable", False):
            # torch's all-reduce (gloo, or ProcessGroupNCCL's private stream) is not replayable:
            # graphs under TP need the direct RCCL communicator (parallel/rccl.py)
            self.use_graphs = False
        self.graph_max_batch = graph_max_batch
        self._graphs: Dict[tuple, "_DecodeGraph"] = {}
        self._graph_pool = None
        # graph_input: receive graphs are per OWNER (a channel engine): two engines sharing this
        # executor never hand each other's hidden states to a replay.  Owner -> small tag (part of
        # the graph key); (tag, base key) -> last receive slot handed out; tag -> (key, graph) its
        # next step replays
        self._owner_tags = weakref.WeakKeyDictionary()
        self._owner_strong: Dict[int, tuple] = {}
        self._next_tag = 1
        self._recv_slot: Dict[tuple, int] = {}
        self._recv_pin: Dict[int, tuple] = {}
        # qkv fold per decode-graph batch bucket (_confirm_qkv_fold's end-to-end A/B on THIS executor)
        self.qkv_fold_by_bucket: Dict[int, bool] = {}
        self._pinned = _Pinned(2 * max_tokens_per_step, 2 * max_tokens_per_step + max_sessions, self.device)
        self.last_step_ms: Optional[float] = None
        # graph_hook(out): recorded at the END of every decode graph capture (the static output
        # buffer), e.g. the stage hop's RCCL send (parallel/engine.py graph hop); last_graphed
        # says whether the last step ran as a graph replay
        self.graph_hook = None
        self._hook_owner = None
        self.last_graphed = self.last_hooked = False
        # MFMA flash attention for prefill steps (csrc/attention_mfma.hip)
        self._attn_mfma_prefill = cfg.model_type != "gpt2" and cfg.head_dim in (64, 128)
        # GQA decode: the whole group of a kv head in the MFMA rows (2x the VALU kernel at nrep 8)
        # MHA decode stays on the flash-decoding kernel: forcing it onto the MFMA kernel (15 of 16
        # MFMA rows idle) measured 11005 vs 13617 tok/s at 64 sessions and 13847 vs 16248 at 128
        # (Llama-2-7B, profiles/r1_attn_mha_mfma_vs_simt/)
        self._attn_mfma_gqa = self._attn_mfma_prefill and self.nh // self.nkv >= 4
        # decode steps of GQA models on the MFMA kernel (a lab script may flip this before the
        # first decode step to A/B the flash-decoding kernel)
        # (an fp8 KV cache runs none of the bf16 MFMA kernels and has no MX epilogue)
        self.gqa_decode_mfma = self._attn_mfma_gqa and not self._kv_fp8
        # ... and on an fp8 KV cache the kernel's fp8 form (decode steps only; prefill: prefill_fa_f8
        # below); MPAMD_KV_FP8_MFMA=0 keeps the flash-decoding kernel there too
        self.gqa_decode_mfma_f8 = self._attn_mfma_gqa and self._kv_fp8 and \
            os.environ.get("MPAMD_KV_FP8_MFMA", "1") != "0"
        # prefill: up to 4 query blocks of a sequence per workgroup share each K/V step
        # (csrc/attention_mfma.hip attn_mfma_grp_kernel)
        self._attn_grouped = True
        # prefill steps with a row-major attention output: the FA2 kernel on 32x32x16 MFMA with
        # transposed LDS reads of V (csrc/attention_fa.hip); other shapes keep the 16x16 one
        self._attn_fa = self._attn_mfma_prefill and \
            ops.fa_ok(cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, page_size)
        # ... and on an fp8 KV cache the kernel's fp8 form; MPAMD_KV_FP8_FA=0 keeps those steps on the
        # flash-decoding kernel (per-query causal rows)
        self.prefill_fa_f8 = self._attn_fa and self._kv_fp8 and os.environ.get("MPAMD_KV_FP8_FA", "1") != "0"
        # sliding window ("attend"): row-major prefill steps past the window on the FA2 kernel's windowed
        # form (bf16 and fp8 caches); MPAMD_WINDOW_FA=0 puts them back on the flash-decoding rows
        self.window_fa = bool(self.window) and self._attn_fa and os.environ.get("MPAMD_WINDOW_FA", "1") != "0"
        self._n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count \
            if self.device.type == "cuda" else 256
        # decode steps on the flash-decoding kernel fold RoPE + the KV page write into it
        self._fuse_rope = True
        # shortest split-K context slice (ops.attention_partition): longer on the MFMA GQA kernel
        self._attn_min_part = 256 if (self.gqa_decode_mfma or self.gqa_decode_mfma_f8) else 64
        self._decode_qb: Dict[int, torch.Tensor] = {}
        self._moe_y: Dict[int, torch.Tensor] = {}
        self.timing = False
        # one executor may be driven by the TCP handler's GPU worker AND a device-channel
        # engine thread: every device step (incl. hipGraph capture) runs under this lock
        self.exec_lock = threading.RLock()
        # fp8 weights: W8A16 (ops.linear_w8: fp8 weights dequantized into the bf16 MFMA, bf16
        # activations, the fused-norm path below; default) or W8A8 (MPAMD_FP8_MODE=w8a8: fp8 MFMA,
        # activations quantized per row before every GEMM, RMSNorm kernels; also under TP).
        # MPAMD_FP8_MODE=mx: the W8A16 path with the o projection of <= 64-row GQA decode steps on the
        # W8A8-MX GEMM (ops.linear_mx: MX e4m3 activations, block-scaled MFMA), its input written as
        # MX by the attention kernel's epilogue (no quantizer launch); profiles/r6mx
        fp8_mode = os.environ.get("MPAMD_FP8_MODE", "w8a16")
        self._w8 = (self.device.type == "cuda" and weights.fp8 and cfg.model_type != "gpt2" and not cfg.is_moe and
                    self._tp is None and fp8_mode in ("w8a16", "mx") and
                    os.environ.get("MPAMD_FUSED_NORM", "1") != "0" and
                    all(d % 256 == 0 for d in (cfg.hidden_size, cfg.q_dim, cfg.intermediate_size)) and
                    (cfg.q_dim + 2 * cfg.kv_dim) % 32 == 0)
        self._mx = bool(self._w8 and fp8_mode == "mx")
        if self._w8:
            weights.prepare_w8a16(fold_norms=True)
        # fp8 MoE (Mixtral) weights: W8A16 WITHOUT the fused-norm path (norm kernels with the real
        # weights, the router in bf16).  Steps of <= 64 rows run qkv / o on ops.linear_w8 and all
        # experts in two grouped launches (ops.moe_gate_up_w8 / moe_down_w8: unrouted experts skipped
        # on the device); MPAMD_MOE_GROUPED=0 - or a shape the grouped kernels do not cover - runs them
        # expert by expert through ops.linear_w8 + addcmul_ instead.  Larger steps and prefill take the
        # expert-grouped schedule and dequantize one expert's projection at a time, so this stage's
        # graphs stop at 64 rows.  CPU executors dequantize everywhere.
        self._moe_w8 = False
        if cfg.is_moe and weights.fp8:
            if self._tp is not None:
                raise ValueError("fp8 MoE (Mixtral) weights are not supported under tensor parallelism")
            if self.device.type == "cuda":
                if fp8_mode != "w8a16":
                    raise ValueError(f"MPAMD_FP8_MODE={fp8_mode} is not built for MoE (Mixtral) models: fp8 experts "
                                     f"run W8A16 only")
                self._moe_w8 = (all(d % 256 == 0 for d in (cfg.hidden_size, cfg.q_dim, cfg.intermediate_size)) and
                                (cfg.q_dim + 2 * cfg.kv_dim) % 32 == 0 and ops.gemm_policy() != "hipblaslt")
                if self._moe_w8:
                    weights.prepare_w8a16(fold_norms=False)
                    self._w8 = True  # the W8A16 layout and kernels (never the fused-norm path: _fused stays off)
                    self.graph_max_batch = min(self.graph_max_batch, 64)
        self._moe_grouped = os.environ.get("MPAMD_MOE_GROUPED", "1") != "0"
        # MXFP4 weights (StageWeights.quantize_mxfp4: norm weights folded in before the one
        # quantization): <= 64-row decode steps run the fused-norm path on ops.linear_w4, everything
        # else dequantizes one projection at a time (LlamaLayer.dense) and normalises with unit weights
        self._w4 = bool(self.device.type == "cuda" and weights.w4 and cfg.model_type != "gpt2" and
                        not cfg.is_moe and self._tp is None)
        if weights.w4 and self._tp is not None:
            raise ValueError("MXFP4 weights are not supported under tensor parallelism")
        # fused-norm decode path (ops/csrc/gemm.hip EpiArgs): no RMSNorm kernels between the
        # layers' GEMMs - dense bf16 or W8A16 Llama stages without TP (MoE / W8A8 / TP keep the
        # norm kernels)
        self._fused = (self.device.type == "cuda" and cfg.model_type != "gpt2" and not cfg.is_moe and
                       self._tp is None and (not weights.fp8 or self._w8) and ops.gemm_policy() != "hipblaslt" and
                       os.environ.get("MPAMD_FUSED_NORM", "1") != "0" and
                       all(d % 128 == 0 for d in (cfg.hidden_size, cfg.q_dim, cfg.intermediate_size)))
        self._ss = ops.norm_stats_buffer(self.device, 2) if self._fused else None
        # first stage on that path: the stage-entry kernel gathers the embedding rows itself
        # (ops.embed_stage_entry; MPAMD_FUSED_ENTRY=0 keeps the separate embedding launch)
        self._fused_entry = os.environ.get("MPAMD_FUSED_ENTRY", "1") != "0"
        # unit RMSNorm weight for > 64-row decode steps over norm-folded packed weights (made
        # here, not inside a hipGraph capture)
        self._ones = torch.ones(cfg.hidden_size, dtype=self.dtype, device=self.device) if self._fused else None
        if self.device.type == "cuda":
            ops.require_native()
            if cfg.model_type != "gpt2" and ops.gemm_policy() != "hipblaslt":
                weights.pack_for_decode(fold_norms=self._fused)
                if self._fused and not all(getattr(L, "folded", False) for L in weights.layers):
                    self._fused = False  # packed before (e.g. a shared weights object): norm kernels
                ops.use_tuned_gemms()  # library GEMM solutions for the row-major shapes
                ops.gemm_workspace(self.device)  # allocated before any hipGraph capture
                ops.attention_counters(self.device)
                ops.load_kernel_table()  # the committed per-shape kernel choices (ops.KERNEL_TABLE)
                if ops.autotune_mode() != "off":
                    H, F = cfg.hidden_size, cfg.intermediate_size
                    shapes = [] if (weights.fp8 or weights.w4 or not weights.layers) else \
                        [(cfg.q_dim + 2 * cfg.kv_dim, H, 0), (H, cfg.q_dim, 0), (2 * F, H, 1), (H, F, 0)]
                    if self._fused and shapes:
                        shapes += [(H, cfg.q_dim, 3), (H, F, 3)]
                    if cfg.is_moe and shapes:
                        shapes.append((16 * ((cfg.num_local_experts + 15) // 16), H, 0))  # router
                    if weights.lm_head_p is not None:
                        shapes.append((16 * weights.lm_head_p.shape[0], H, 0))
                    ops.autotune_gemm(shapes, self.device)
                    if self._moe_w8 and weights.layers:  # qkv / o only: the experts run the grouped kernels
                        ops.autotune_w8([(cfg.q_dim + 2 * cfg.kv_dim, H, 0), (H, cfg.q_dim, 0)], self.device)
                    elif self._w8 and weights.layers:
                        ops.autotune_w8([(cfg.q_dim + 2 * cfg.kv_dim, H, 0), (H, cfg.q_dim, 3), (2 * F, H, 1),
                                         (H, F, 3)], self.device)
                    if self._w4:
                        pass  # no 4-bit autotuner, no qkv fold: one ring form per shape
                    elif self._fused and weights.layers and self._fuse_rope:
                        # qkv as split-K partials summed in the attention kernel, per row bucket
                        ops.autotune_qkv_fold(cfg.q_dim + 2 * cfg.kv_dim, H, self.device, fp8=bool(self._w8))
                    elif weights.fp8 and weights.layers and not cfg.is_moe:
                        ops.autotune_fp8([(cfg.q_dim + 2 * cfg.kv_dim, H, 0), (H, cfg.q_dim, 0), (2 * F, H, 1),
                                          (H, F, 0)], self.device)
        if self._lora is not None:
            self._lora.fold_norms(weights.layers)  # A diag(g) for the layers packed with folded norms
        self._streamer, self._n_stream = None, self.n_layers
        if offload and self.device.type == "cuda":
            self._setup_offload(keep_layers_on_gpu)
        if warmup is None:
            warmup = self.device.type == "cuda" and os.environ.get("MPAMD_WARMUP", "1") != "0"
        # (not under TP: a shape that fails on one rank would desynchronise the all-reduces)
        if warmup and self.device.type == "cuda" and self.n_layers and self._tp is None and self._streamer is None:
            self.warmup()
        logger.info(f"StageExecutor blocks [{self.start},{self.end}) embed={self.is_first} head={self.is_last} "
                    f"kv_pages={num_pages} x {page_size} tokens ({self.cache.nbytes / 2**30:.2f} GiB) "
                    f"graphs={self.use_graphs}")

    @property
    def quant_type(self) -> str:
        """Stored weight format of this span's blocks: "none", "fp8" or "mxfp4" (announced by the server)."""
        return "mxfp4" if self.w.w4 else ("fp8" if self.w.fp8 else "none")

    # ================================================================== planning
    def plan(self, seqs: Sequence[Tuple[str, int]], *, reset: Sequence[bool] = (), max_length: Optional[int] = None,
             starts: Optional[Sequence[int]] = None, adapters: Optional[Sequence[Optional[str]]] = None,
             logit_rows: Optional[Sequence[int]] = None) -> Plan:
        """Open/extend sessions and build device metadata for a ragged step.

        ``seqs``: (session_id, n_tokens) pairs.  ``reset[i]`` clears the session first
        (prefill / replay).  ``starts[i]`` (optional) rewinds a session to that position
        (Petals' ``start_from_position``).  ``adapters[i]``: the LoRA adapter session i runs ("" or
        None: the base model), set when the session is opened or reset; a later step has to name the
        same one.  Without ``adapters`` every session keeps its own.  ``logit_rows[i]`` (last stage): the
        number of trailing rows of sequence i whose logits the step returns (default 1, its last row;
        a speculative verify step asks for all of them).
        """
        S = len(seqs)
        if logit_rows is not None:
            if len(logit_rows) != S:
                raise ValueError(f"logit_rows names {len(logit_rows)} sequences, the step has {S}")
            for (sid, n), lr in zip(seqs, logit_rows):
                if not 1 <= int(lr) <= max(int(n), 1):
                    raise ValueError(f"logit_rows {int(lr)} of session {sid[:8]}: a {int(n)}-token sequence has "
                                     f"1..{max(int(n), 1)} trailing rows")
            if all(int(lr) == 1 for lr in logit_rows):
                logit_rows = None  # every sequence's last row: the plain step
        if adapters is not None and len(adapters) != S:
            raise ValueError(f"adapters names {len(adapters)} sessions, the step has {S}")
        want = None if adapters is None else [self.adapter_slot(a) for a in adapters]  # (before any session opens)
        sess: List[SessionState] = []
        ntoks = np.empty(S, dtype=np.int32)
        st = np.empty(S, dtype=np.int32)
        for i, (sid, n) in enumerate(seqs):
            fresh = self.sessions.get(sid) is None
            s = self.sessions.open(sid, max_length)
            if reset and reset[i]:
                self.sessions.reset(sid)
                fresh = True
            if fresh:
                s.adapter = want[i] if want is not None else -1
            elif want is not None and want[i] != s.adapter:
                raise ValueError(f"session {sid[:8]} runs adapter {self.adapter_name(s.adapter)!r}: a step cannot "
                                 f"switch it to {self.adapter_name(want[i])!r}")
            if starts is not None and starts[i] is not None and starts[i] < s.length:
                self.sessions.rewind(s, int(starts[i]))
            self.sessions.reserve(s, s.length + int(n))
            sess.append(s)
            ntoks[i] = n
            st[i] = s.length
        T = int(ntoks.sum())
        if T > self.max_tokens:
            raise ValueError(f"step has {T} tokens > max_tokens_per_step {self.max_tokens}")
        rows = np.fromiter((s.row for s in sess), dtype=np.int32, count=S)
        h64, h32 = self._pinned.next()
        n64 = h64[: 2 * T].numpy().reshape(2, T) if T else np.empty((2, 0), np.int64)
        n32 = h32[: 2 * T + S].numpy()
        native.build_meta(rows, st, ntoks, self.sessions.table, self.cache.page_size, n64[0], n64[1], n32[:T],
                          n32[T:2 * T], n32[2 * T:])
        extra = None
        if logit_rows is not None:
            # sequence i's trailing logit_rows[i] rows, in sequence order; the last rows stay what they are
            ends = np.cumsum(ntoks)
            lrows = np.concatenate([np.arange(e - int(lr), e) for e, lr in zip(ends, logit_rows)]).astype(np.int64)
            is_last = np.concatenate([np.arange(int(lr)) == int(lr) - 1 for lr in logit_rows])
            extra = (lrows, np.flatnonzero(is_last), np.flatnonzero(~is_last))
        self.sessions.sync_table()
        max_ctx = int((st + ntoks).max()) if S else 0
        is_decode = bool(S and (ntoks == 1).all())
        pinned = self._pinned

        def upload():
            if self.device.type == "cuda":
                d64 = h64[: 2 * T].view(2, T).to(self.device, non_blocking=True)
                d32 = h32[: 2 * T + S].to(self.device, non_blocking=True)
                pinned.mark()  # the pinned buffers are reused two plans later: after this copy
            else:
                d64 = h64[: 2 * T].view(2, T).clone()
                d32 = h32[: 2 * T + S].clone()
            return d64, d32

        qb = sb = fb = None
        fa_waves = 4
        if self.device.type == "cuda" and not is_decode and self._attn_fa:
            fbn, fa_waves = ops.fa_plan(ntoks, self.nh, self.nkv, self._n_cu)
            fb = torch.from_numpy(fbn).to(self.device, non_blocking=True)
        if self.device.type == "cuda" and not is_decode and self._attn_mfma_prefill:
            qb = torch.from_numpy(ops.query_blocks(ntoks, self.nh // self.nkv)).to(self.device, non_blocking=True)
            if self._attn_grouped:
                sb = torch.from_numpy(ops.query_superblocks(ntoks, self.nh // self.nkv)).to(self.device,
                                                                                              non_blocking=True)
        row_slots = None
        if self._lora is not None and any(s.adapter >= 0 for s in sess):
            row_slots = np.repeat(np.fromiter((s.adapter for s in sess), dtype=np.int32, count=S), ntoks)
        return Plan(sess, ntoks, st, T, max_ctx, is_decode, n64, n32, qb, sb, fb, fa_waves, lora_slots=row_slots,
                    extra=extra, _upload=upload)

    def adapter_slot(self, name: Optional[str]) -> int:
        """Slot of a hosted adapter; -1 for "" / None (the base model).  Unknown: ``KeyError("adapter X not found")``."""
        if not name:
            return -1
        if self._lora is None:
            raise KeyError(f"adapter {name} not found")
        return self._lora.slot(name)

    def adapter_name(self, slot: int) -> str:
        return self._lora.names[slot] if (self._lora is not None and slot >= 0) else ""

    @property
    def adapters(self) -> List[str]:
        """Names of the hosted adapters, in slot order (announced by the server)."""
        return list(self._lora.names) if self._lora is not None else []

    def commit(self, plan: Plan) -> None:
        for s, n in zip(plan.sessions, plan.ntoks):
            s.length += int(n)
            s.step += 1
            self.sessions.release(s)  # (sliding window: the pages no later query can see)

    # ================================================================== execution
    def forward(self, seqs: Sequence[Tuple[str, int]], x: torch.Tensor, **plan_kw) -> torch.Tensor:
        """One ragged step.  ``x``: token ids [T] (first stage) or hidden [T, H].

        Returns hidden [T, H] (non-last stage) or last-token logits [S, V] (last stage; with
        ``logit_rows`` the logits of every sequence's trailing ``logit_rows[i]`` rows, in sequence
        order: [sum(logit_rows), V]).
        Steps larger than ``max_tokens_per_step`` run as consecutive chunks (chunked prefill,
        upstream Petals TransformerBackend.inference_step): a long prompt is split at token
        boundaries, later pieces attend to the KV the earlier pieces wrote.
        """
        T = sum(int(n) for _, n in seqs)
        prompts = plan_kw.pop("prompts", None)
        hook_owner = plan_kw.pop("hook_owner", None)
        if prompts is not None and not any(p is not None for p in prompts):
            prompts = None
        if T > self.max_tokens:
            if prompts is not None:
                raise ValueError("deep prompts need the step to fit max_tokens_per_step")
            return self._forward_chunked(seqs, x, **plan_kw)
        plan = self.plan(seqs, **plan_kw)
        out = self.run(plan, x, prompt=self._prompt_rows(seqs, prompts) if prompts is not None else None,
                       hook_owner=hook_owner)
        self.commit(plan)
        return out

    def _prompt_rows(self, seqs, prompts):
        """Deep prompts (upstream iterate_rpc_inference / TransformerBackend: before every block,
        ``hidden[:, :P] += prompt``, applied to the first P tokens of this step). ``prompts[i]`` is
        None or ``[n_layers, P, H]`` for sequence i. Returns (rows [R], values [n_layers, R, H])."""
        rows, vals, off = [], [], 0
        for (sid, n), p in zip(seqs, prompts):
            if p is not None:
                if p.dim() != 3 or p.shape[0] != self.n_layers or p.shape[2] != self.cfg.hidden_size:
                    raise ValueError(f"prompts must be [{self.n_layers}, P, {self.cfg.hidden_size}], "
                                     f"got {tuple(p.shape)}")
                k = min(int(p.shape[1]), int(n))
                rows.extend(range(off, off + k))
                vals.append(p[:, :k])
            off += int(n)
        if not rows:
            return None
        return (torch.tensor(rows, dtype=torch.long, device=self.device),
                torch.cat(vals, 1).to(self.device, self.dtype))

    def _forward_chunked(self, seqs, x, reset: Sequence[bool] = (), starts=None, max_length=None, adapters=None,
                         logit_rows=None):
        C = self.max_tokens
        if logit_rows is not None and len(logit_rows) != len(seqs):
            raise ValueError(f"logit_rows names {len(logit_rows)} sequences, the step has {len(seqs)}")
        pieces = []  # (seq index, token offset within the seq, count, offset into x)
        xoff = 0
        for i, (sid, n) in enumerate(seqs):
            off = 0
            while off < n:
                pieces.append((i, off, min(int(n) - off, C), xoff + off))
                off += pieces[-1][2]
            xoff += int(n)
        chunks, cur, used = [], [], 0
        for pc in pieces:
            if used + pc[2] > C and cur:
                chunks.append(cur)
                cur, used = [], 0
            take = pc
            while used + take[2] > C:  # a piece longer than the room left: split it
                room = C - used
                cur.append((take[0], take[1], room, take[3]))
                chunks.append(cur)
                cur, used = [], 0
                take = (take[0], take[1] + room, take[2] - room, take[3] + room)
            cur.append(take)
            used += take[2]
        if cur:
            chunks.append(cur)
        if logit_rows is not None:
            # a sequence's trailing rows come from its last piece alone (checked before any chunk runs)
            for ch in chunks:
                for (i, off, c, _) in ch:
                    if off + c == int(seqs[i][1]) and int(logit_rows[i]) > c:
                        raise ValueError(f"logit_rows {int(logit_rows[i])} of session {seqs[i][0][:8]} reach past "
                                         f"the last chunk ({c} rows) of a chunked step")
        hidden, logits = [], [None] * len(seqs)
        for ch in chunks:
            sub = [(seqs[i][0], c) for (i, off, c, _) in ch]
            sub_reset = [bool(reset[i]) if (reset and off == 0) else False for (i, off, c, _) in ch]
            sub_starts = [(starts[i] if (starts is not None and off == 0) else None) for (i, off, c, _) in ch]
            xs = torch.cat([x[xo:xo + c] for (_, _, c, xo) in ch])
            sub_ad = None if adapters is None else [adapters[i] for (i, _, _, _) in ch]
            sub_lr = None
            if logit_rows is not None:
                sub_lr = [int(logit_rows[i]) if off + c == int(seqs[i][1]) else 1 for (i, off, c, _) in ch]
            out = self.forward(sub, xs, reset=sub_reset, starts=sub_starts, max_length=max_length, adapters=sub_ad,
                               logit_rows=sub_lr)
            if self.is_last:
                o = 0
                for r, (i, off, c, _) in enumerate(ch):
                    n = 1 if sub_lr is None else sub_lr[r]
                    if off + c == int(seqs[i][1]):
                        logits[i] = out[o] if logit_rows is None else out[o:o + n]
                    o += n
            else:
                hidden.append(out)
        if self.is_last:
            if logit_rows is not None:
                return torch.cat(logits)
            return torch.stack(logits)
        return torch.cat(hidden)

    def run(self, plan: Plan, x: torch.Tensor, prompt=None, hook_owner=None) -> torch.Tensor:
        if plan.T == 0:
            H = self.cfg.hidden_size
            return torch.empty(0, self.cfg.vocab_size if self.is_last else H, dtype=self.dtype, device=self.device)
        x = x.to(self.device)
        if not self.is_first and x.dtype != self.dtype:
            x = x.to(self.dtype)
        ev = None
        if self.timing and self.device.type == "cuda":
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        self.last_graphed = self.last_hooked = False
        lora = None
        if plan.lora_slots is not None:
            if prompt is not None:
                raise ValueError("adapters with deep prompts are not built: a session runs one or the other")
            lora = plan.lora  # (the device copy is made by the eager branch only: a graph stages its own)
        if lora is not None and self.use_graphs and plan.is_decode and \
                plan.T <= min(self.graph_max_batch, 64) and self._lora_packed_ok(self._bucket(plan.T)):
            out = self._run_lora_graph(plan, x)
            self.last_graphed = True
        elif lora is None and prompt is None and self.use_graphs and plan.is_decode and \
                plan.T <= self.graph_max_batch:
            hooked = self.graph_hook is not None and hook_owner is not None and hook_owner is self._hook_owner
            out = self._run_graph(plan, x, hooked, owner=hook_owner)
            self.last_graphed, self.last_hooked = True, hooked
        elif self.cfg.model_type == "gpt2":
            out = self._forward_gpt2(plan, x, prompt=prompt)
        else:
            out = self._forward_llama(_Step(
                x, *plan.meta(), plan.T, plan.max_ctx, plan.is_decode, self.device, self.dtype, qblocks=plan.qblocks,
                superblocks=plan.superblocks, fablocks=plan.fablocks, fa_waves=plan.fa_waves, prompt=prompt,
                lora=lora(self.device) if lora else None, extra=plan.extra_rows(self.device)))
        if ev is not None:
            ev[1].record()
            ev[1].synchronize()
            self.last_step_ms = ev[0].elapsed_time(ev[1])
        return out

    # ------------------------------------------------------------------ llama
    def decode_qblocks(self, T: int) -> torch.Tensor:
        """Query blocks of a decode step (one token per block); cached per batch size so
        hipGraph captures reuse the same buffer."""
        qb = self._decode_qb.get(T)
        if qb is None:
            qb = torch.from_numpy(np.stack([np.arange(T), np.ones(T)]).astype(np.int32)).to(self.device)
            self._decode_qb[T] = qb
        return qb

    def _attend(self, st: _Step, qkv, kc, vc, out, packed):
        """Paged attention of step ``st``: ``qkv`` against one layer's cache pair ``kc`` / ``vc`` into ``out``
        (``packed``: in the packed layout).  MFMA flash attention for prefill blocks (``st.qblocks``) and GQA
        decode, else the flash-decoding kernel.  An fp8 KV cache has the fp8 forms of the MFMA GQA decode
        kernel, of the FA2 prefill kernel (row-major output) and of the flash-decoding kernel; its
        other prefill blocks (packed output, shapes outside ``fa_ok``) run on the latter as
        per-query causal rows (``qblocks`` is ignored).  Under a sliding window a prefill step with a
        row past the window runs the FA2 kernel's windowed form where FA2 covers it, else those rows."""
        (ps, np_), max_ctx = st.part, st.max_ctx
        f8, win, prefill = self._kv_fp8, self.window, st.qblocks is not None
        # FA2 covers a prefill step with blocks (plan.fablocks) and a row-major output
        fa = prefill and st.fablocks is not None and not packed
        # what every attention op takes: its leading arguments, the head geometry, its trailing keywords
        a, hs = (qkv, kc, vc, self.sessions.table_dev, st.q_seq, st.q_ctx), (self.nh, self.nkv, self.scale)
        kw = dict(out=out, workspace=st.ws, max_ctx=max_ctx)

        def flash():
            return ops.paged_attention(*a, *hs, part_size=ps, num_parts=np_, packed=packed, window=win, **kw)

        # sliding window: the decode kernels take it, and so does the FA2 prefill kernel's windowed form
        # (row-major steps it covers: window_fa).  The grouped MFMA kernel has none: a prefill step keeps
        # the unwindowed kernels only while no row is past the window (the same computation) and
        # otherwise runs the windowed FA2 form, or the flash-decoding kernel as per-query causal rows
        if win and prefill and max_ctx > win:
            if self.window_fa and fa and (self.prefill_fa_f8 if f8 else self._attn_fa):
                op = ops.attention_fa_window_f8 if f8 else ops.attention_fa_window
                return op(*a, st.fablocks, *hs, win, waves=st.fa_waves, **kw)
            return flash()
        if not prefill and (self.gqa_decode_mfma_f8 if f8 else self.gqa_decode_mfma) and self.device.type == "cuda":
            ps2, np2 = self._parts128(ps, np_)
            op = ops.attention_mfma_f8 if f8 else ops.attention_mfma
            return op(*a, self.decode_qblocks(qkv.shape[0]), *hs, part_size=ps2, num_parts=np2, packed=packed,
                      window=win, **kw)
        if fa and (self.prefill_fa_f8 or not f8):
            op = ops.attention_fa_f8 if f8 else ops.attention_fa
            return op(*a, st.fablocks, *hs, waves=st.fa_waves, **kw)
        if prefill and not f8:
            return ops.attention_mfma(*a, st.qblocks, *hs, packed=packed, superblocks=st.superblocks, **kw)
        return flash()

    @staticmethod
    def _parts128(ps: int, np_: int):
        """The step's context slices re-cut for the MFMA kernel: a multiple of 128 tokens each."""
        ps2 = 128 * math.ceil(ps / 128)
        return ps2, max(1, math.ceil(ps * np_ / ps2))

    def _qkv_fold(self, T: int) -> bool:
        """Decode steps of T rows: qkv as split-K partial slabs folded into the attention kernel's
        loads - where ``_confirm_qkv_fold``'s decode-step A/B on this executor found it faster for
        the batch bucket the step replays (an unconfirmed bucket keeps the reduce launch)."""
        if not (self._fuse_rope and self._fused and self.device.type == "cuda") or self._w4 or \
                os.environ.get("MPAMD_QKV_FOLD", "1") == "0":
            return False  # (a 4-bit stage has no split-K ring: never folded)
        cfg = self.cfg
        return bool(self.qkv_fold_by_bucket.get(self._bucket(T), False)) and \
            ops.rwk_split(T, cfg.q_dim + 2 * cfg.kv_dim, cfg.hidden_size, bool(self._w8)) > 0

    def _rope_attend(self, st: _Step, qkv, kc, vc, out, packed, qkv_part=None, mx_out=None):
        """RoPE + KV write + attention of step ``st`` (``qkv``, ``kc`` / ``vc``, ``out``, ``packed``: as ``_attend``).
        Decode steps do all three in one launch (ops.paged_attention_rope on the flash-decoding kernel,
        ops.attention_mfma_rope on the MFMA GQA one); everything else keeps rope_kv_write.  ``qkv_part``: q / k / v
        as the qkv GEMM's split-K slabs (decode RoPE paths only).  ``mx_out``: (ax, as_) MX buffers the MFMA GQA
        kernel writes INSTEAD of ``out``: passed only where it runs and can (one part, head_dim 128)."""
        one_launch = st.decode and st.qblocks is None and self._fuse_rope
        f8, (ps, np_) = self._kv_fp8, st.part
        a = (qkv, kc, vc, self.sessions.table_dev, st.q_seq, st.q_ctx)
        rope = (st.positions, self.cos, self.sin, st.slots, self.nh, self.nkv, self.scale)
        kw = dict(out=out, workspace=st.ws, packed=packed, qkv_part=qkv_part, window=self.window, max_ctx=st.max_ctx)
        if one_launch and (self.gqa_decode_mfma_f8 if f8 else self.gqa_decode_mfma) and self.device.type == "cuda":
            ps2, np2 = self._parts128(ps, np_)
            if not f8:  # (an fp8 cache has no MX epilogue)
                kw["mx_out"] = mx_out
            op = ops.attention_mfma_rope_f8 if f8 else ops.attention_mfma_rope
            return op(*a, self.decode_qblocks(qkv.shape[0]), *rope, part_size=ps2, num_parts=np2, **kw)
        if mx_out is not None or (qkv_part is not None and not one_launch):
            raise RuntimeError("qkv partial slabs and an MX output need a fused RoPE decode attention kernel")
        if one_launch:
            return ops.paged_attention_rope(*a, *rope, part_size=ps, num_parts=np_, **kw)
        ops.rope_kv_write(qkv, st.positions, self.cos, self.sin, kc, vc, st.slots, self.nh, self.nkv)
        return self._attend(st, qkv, kc, vc, out, packed)

    def _step_path(self, T: int, prompt, lora) -> str:
        """The layer loop a step of ``T`` rows with deep prompt ``prompt`` and adapter rows ``lora`` (or None) takes:
        "w8a8", "fused", "moe_w8", "packed" or "dense" (module docstring).  The ONLY place that decides it."""
        base = lora is None and prompt is None
        # (a LoRA step goes packed only where the batched kernels cover every targeted projection)
        lora_pk = lora is not None and prompt is None and T <= 64 and self._packed_ok(T) and self._lora_packed_ok(T)
        if base and self._fp8_ok(T):
            return "w8a8"
        if base and self._fused and self.n_layers > 0 and (
                T <= 64 and (self._w8 or self._w4_ok(T) or self._packed_ok(T)) or
                (not self._w8 and not self._w4 and self._fused_wide_ok(T))):
            return "fused"
        if base and self._moe_w8 and 0 < T <= 64:
            return "moe_w8"
        if prompt is None and self._packed_ok(T) and (lora is None or lora_pk):
            return "packed"
        return "dense"

    def _forward_llama(self, st: _Step) -> torch.Tensor:
        """One forward pass over step ``st``: the layer loop of its path (``_layers_<path>``), then the head.
        A layer loop returns (res, mlp, stream): the residual stream, the last down projection still to be
        added to it (None: already added) and, from the fused path, what lm_head can read instead."""
        layers = getattr(self, "_layers_" + self._step_path(st.T, st.prompt, st.lora))
        return self._head(st, *layers(st))

    def _begin(self, st: _Step, embed: bool = True):
        """What every path starts with: the embedding (first stage; ``embed=False``: the path gathers the
        rows itself and gets None), the attention partition and workspace, and the buffers (h, res, qkv, o, mlp)."""
        T, H, h = st.T, self.cfg.hidden_size, st.x
        if self.is_first:
            h = ops.embedding(st.x, self.w.embed, out=st.buf("h", (T, H))) if embed else None
        if st.part is None:
            st.part = ops.attention_partition(T, self.nkv, self._attn_span(st.max_ctx), min_part=self._attn_min_part)
        st.ws = st.buf("attn_ws", (max(1, T * self.nh * st.part[1] * (self.D + 2)),), torch.float32)
        return (h, st.buf("res", (T, H)), st.buf("qkv", (T, self.cfg.q_dim + 2 * self.cfg.kv_dim)),
                st.buf("o", (T, H)), st.buf("mlp", (T, H)))

    def _layers_w8a8(self, st: _Step):
        """fp8 W8A8 decode path: packed bf16 activations are quantized per row right before each GEMM
        (csrc/fp8.hip); weights stream at 1 byte per parameter."""
        cfg, T, eps = self.cfg, st.T, self.cfg.rms_norm_eps
        H, F = cfg.hidden_size, cfg.intermediate_size
        h, res, qkv, o, mlp = self._begin(st)
        pk = ops.packed_numel
        xn = st.buf("xn_p", (pk(T, H),))
        # row-major: their only reader is the row quantization kernel (coalesced rows)
        attn = st.buf("attn", (T, cfg.q_dim))
        act = st.buf("act", (T, F))
        a8 = st.buf("a8", (pk(T, max(H, cfg.q_dim, cfg.intermediate_size)),), torch.uint8)
        asc = st.buf("a8_scale", (((T + 15) // 16) * 16 * 33,), torch.float32)
        # the two norm sites emit fp8 + row scales themselves (norm.hip a8 output): only the
        # attention output and the SwiGLU output still take a separate quantization pass
        for li, L in enumerate(self.w.layers):
            ops.rmsnorm(h if li == 0 else mlp, L.input_norm, eps, out=xn, residual=res, mode=2 if li == 0 else 1,
                        packed=True, a8=a8, a8_scale=asc)
            ops.linear_fp8(a8, asc, L.qkv_q, L.qkv_s, T, out=qkv)
            kc, vc = self.cache.layer(li)
            self._rope_attend(st, qkv, kc, vc, attn, False)
            ops.quant_rows_fp8(attn, out=a8, scale=asc)
            ops.linear_fp8(a8, asc, L.o_q, L.o_s, T, out=o)
            self._ar(o)
            ops.rmsnorm(o, L.post_norm, eps, out=xn, residual=res, mode=1, packed=True, a8=a8, a8_scale=asc)
            ops.linear_fp8(a8, asc, L.gate_up_q, L.gate_up_s, T, out=act, epilogue=1)
            ops.quant_rows_fp8(act, out=a8, scale=asc)
            ops.linear_fp8(a8, asc, L.down_q, L.down_s, T, out=mlp)
            self._ar(mlp)
        return res, mlp, None

    def _layers_fused(self, st: _Step):
        """Fused-norm decode path: 5 launches per layer (qkv, attention, o, gate/up, down).  The residual stream
        r lives row-major in ``res`` and packed in ``xr``; o / down add their product into it in their epilogue
        and accumulate sum(r^2) per row, and qkv / gate_up (norm weights folded into their packed weights) scale
        their rows by rsqrt(mean r^2 + eps).  ss[0] / ss[1]: input- / post-attention-norm statistics; each
        producer clears the other buffer, whose consumer has already run."""
        cfg, T, eps = self.cfg, st.T, self.cfg.rms_norm_eps
        H, Q = cfg.hidden_size, cfg.q_dim
        # first stage: the stage-entry kernel gathers the embedding rows itself (h is None)
        h, res, qkv, _, _ = self._begin(st, embed=not (self._fused_entry and st.x.dim() == 1 and st.x.is_contiguous()))
        pk = ops.packed_numel
        xr = st.buf("xr_p", (pk(T, H),))
        attn = st.buf("attn_p", (pk(T, Q),))
        act = st.buf("act_p", (pk(T, cfg.intermediate_size),))
        ss_in, ss_post = self._ss[0], self._ss[1]
        if self._w8 or self._w4:  # W8A16 / W4A16: same launches, 1 byte / 4.25 bits per weight streamed
            lin, wn, sn = (ops.linear_w8, "_w8", "_ws") if self._w8 else (ops.linear_w4, "_w4", "_s4")

            def gemm(a, L, name, **kw):
                return lin(a, getattr(L, name + wn), getattr(L, name + sn), T, **kw)
        else:
            def gemm(a, L, name, **kw):
                return ops.linear(a, None, wp=getattr(L, name + "_p"), a_rows=T, **kw)
        one_launch = st.decode and st.qblocks is None  # (RoPE + attention in one decode kernel: _rope_attend)
        # decode steps whose qkv GEMM measured faster as split-K partial slabs: the attention
        # kernel sums the slabs + applies the row scale on its q / k / v loads (no reduce launch)
        fold = one_launch and self._qkv_fold(T)
        # W8A8-MX o projection: the MFMA GQA decode kernel's epilogue writes the MX activation; it can with
        # one context part and head_dim 128 (the partition is the step's: the same for every layer)
        mx_o = None
        if (self._mx and one_launch and T <= 64 and self.gqa_decode_mfma and not self._kv_fp8 and self._fuse_rope and
                ops.rwk_split(T, H, Q, 2) > 0 and self._parts128(*st.part)[1] == 1 and self.D == 128):
            mx_o = (st.buf(f"mx_ax{Q}", (16 * ((T + 15) // 16) * Q,), torch.uint8),
                    st.buf(f"mx_as{Q}", (2 * Q,), torch.uint8))
        for li, L in self._iter_layers(_PACKED_FIELDS):
            if li == 0 and h is None:  # first stage: embedding lookup + stage entry in one launch
                ops.embed_stage_entry(st.x, self.w.embed, xr, res, ss_in)
            elif li == 0:
                ops.rmsnorm(h, L.input_norm, eps, out=xr, residual=res, mode=3, packed=True, ss=ss_in)
            qp = None
            if fold:
                wkw = dict(w8=L.qkv_w8, w_scale=L.qkv_ws) if self._w8 else dict(wp=L.qkv_p)
                qp = (ops.linear_partials(xr, T, out=qkv, **wkw), ss_in, 1.0 / H, eps)
            else:
                gemm(xr, L, "qkv", out=qkv, ss_in=ss_in, eps=eps)
            kc, vc = self.cache.layer(li)
            self._rope_attend(st, qkv, kc, vc, attn, True, qkv_part=qp, mx_out=mx_o)
            if mx_o is not None:
                ops.linear_mx(mx_o[0], mx_o[1], L.o_w8, L.o_ws, T, out=res, epilogue=3, residual=res, ap_out=xr,
                              ss_out=ss_post, ss_zero=ss_in)
            else:
                gemm(attn, L, "o", out=res, epilogue=3, residual=res, ap_out=xr, ss_out=ss_post, ss_zero=ss_in)
            gemm(xr, L, "gate_up", out=act, epilogue=1, out_packed=True, ss_in=ss_post, eps=eps)
            gemm(act, L, "down", out=res, epilogue=3, residual=res, ap_out=xr, ss_out=ss_in, ss_zero=ss_post)
        return res, None, (xr, ss_in)

    def _layers_moe_w8(self, st: _Step):
        """fp8 MoE decode path: packed activations, norm kernels with the real weights, qkv / o on
        the W8A16 GEMM, the experts in two grouped launches (_moe_mlp_w8)."""
        cfg, T, eps = self.cfg, st.T, self.cfg.rms_norm_eps
        h, res, qkv, o, mlp = self._begin(st)
        pk = ops.packed_numel
        xn = st.buf("xn_p", (pk(T, cfg.hidden_size),))
        attn = st.buf("attn_p", (pk(T, cfg.q_dim),))
        act = st.buf("moe_act_p", (cfg.num_local_experts * pk(T, cfg.intermediate_size),))
        for li, L in enumerate(self.w.layers):
            ops.rmsnorm(h if li == 0 else mlp, L.input_norm, eps, out=xn, residual=res, mode=2 if li == 0 else 1,
                        packed=True)
            ops.linear_w8(xn, L.qkv_w8, L.qkv_ws, T, out=qkv)
            kc, vc = self.cache.layer(li)
            self._rope_attend(st, qkv, kc, vc, attn, True)
            ops.linear_w8(attn, L.o_w8, L.o_ws, T, out=o)
            ops.rmsnorm(o, L.post_norm, eps, out=xn, residual=res, mode=1, packed=True)
            self._moe_mlp_w8(st, L, xn, mlp, act)
        return res, mlp, None

    def _layers_packed(self, st: _Step):
        """Packed decode path: activations feeding a GEMM stay in the packed MFMA-fragment layout.  A LoRA step adds
        shrink + expand on the row-major output of every targeted projection (gate/up then leaves its epilogue)."""
        cfg, T, eps = self.cfg, st.T, self.cfg.rms_norm_eps
        H, F = cfg.hidden_size, cfg.intermediate_size
        lo = self._lora if st.lora is not None else None
        h, res, qkv, o, mlp = self._begin(st)
        pk = ops.packed_numel
        xn = st.buf("xn_p", (pk(T, H),))
        attn = st.buf("attn_p", (pk(T, cfg.q_dim),))
        act = st.buf("act_p", (pk(T, F),))

        def lora_add(lp, xp, y, unit=False):
            # y += B (scale A x) for the rows with an adapter: two launches, slots read on the device
            if lp is not None:
                t = ops.lora_shrink(xp, lp.a_for(unit), lo.scale, st.lora[0], T,
                                    out=st.buf(f"lora_t{lp.A.shape[1]}", (T, lp.A.shape[1]), torch.float32))
                ops.lora_expand(t, lp.B, st.lora[0], y)

        for li, L in self._iter_layers(_PACKED_FIELDS):
            LL = lo.layers[li] if lo is not None else _NO_LORA
            # weights packed for the fused path (a base step of > 64 rows, a LoRA step) carry the norm
            # weights in their columns: normalise with a unit weight
            unit = bool(getattr(L, "folded", False))
            g_in, g_post = (self._unit_norm(), self._unit_norm()) if unit else (L.input_norm, L.post_norm)
            ops.rmsnorm(h if li == 0 else mlp, g_in, eps, out=xn, residual=res, mode=2 if li == 0 else 1, packed=True)
            ops.linear(xn, L.qkv, out=qkv, wp=L.qkv_p, a_rows=T)
            lora_add(LL.qkv, xn, qkv, unit)
            kc, vc = self.cache.layer(li)
            self._rope_attend(st, qkv, kc, vc, attn, True)
            ops.linear(attn, L.o, out=o, wp=L.o_p, a_rows=T)
            lora_add(LL.o, attn, o)
            self._ar(o)
            ops.rmsnorm(o, g_post, eps, out=xn, residual=res, mode=1, packed=True)
            if L.moe:
                self._moe_mlp(st, L, xn, mlp, act, packed=True)
                continue
            if LL.gate_up is not None:
                gu = ops.linear(xn, L.gate_up, out=st.buf("gu", (T, 2 * F)), wp=L.gate_up_p, a_rows=T)
                lora_add(LL.gate_up, xn, gu, unit)
                ops.pack_act(ops.swiglu(gu, out=st.buf("act", (T, F))), out=act)
            else:
                ops.linear(xn, L.gate_up, out=act, epilogue=1, wp=L.gate_up_p, a_rows=T, out_packed=True)
            ops.linear(act, L.down, out=mlp, wp=L.down_p, a_rows=T)
            lora_add(LL.down, act, mlp)
            self._ar(mlp)
        return res, mlp, None

    def _layers_dense(self, st: _Step):
        """Row-major path: any row count, any device; deep prompts, and LoRA steps with the torch form of
        the update by runs of rows (``ops.lora_update``)."""
        cfg, T, eps, prompt = self.cfg, st.T, self.cfg.rms_norm_eps, st.prompt
        H, F = cfg.hidden_size, cfg.intermediate_size
        lo, runs = (self._lora, st.lora[1]) if st.lora is not None else (None, None)
        h, res, qkv, o, mlp = self._begin(st)
        xn = st.buf("xn", (T, H))
        attn = st.buf("attn", (T, cfg.q_dim))
        act = st.buf("act", (T, F))
        # (a LoRA step keeps the real norm weights and the unfolded row-major weights: its gate/up
        # may run with epilogue 0, which the per-step fold decision does not cover)
        fold_native = lo is None and self._folded_native(T)
        for li, L in self._iter_layers(_DENSE_FIELDS):
            LL = lo.layers[li] if lo is not None else _NO_LORA
            # W8A16 / MXFP4 layers' only weights carry the norm weights folded in (prepare_w8a16,
            # quantize_mxfp4).
            # bf16 layers packed for the fused path carry them in qkv_p / gate_up_p only: when
            # the native GEMM would pick those up, normalise with a unit weight; otherwise
            # keep the real norm weights and hand the GEMM the unfolded row-major weight only
            quant = L.w8 or L.w4
            folded_bf16 = L.folded and not quant
            unit = (L.folded and quant) or (folded_bf16 and fold_native)
            g_in, g_post = (self._unit_norm(), self._unit_norm()) if unit else (L.input_norm, L.post_norm)
            qkv_p = None if (folded_bf16 and not fold_native) else L.qkv_p
            gu_p = None if (folded_bf16 and not fold_native) else L.gate_up_p
            if prompt is not None:  # deep prompt: the block input (residual stream) += prompt[li]
                cur = h.clone() if li == 0 else ops.add(res, mlp)
                cur.index_add_(0, prompt[0], prompt[1][li])
                ops.rmsnorm(cur, g_in, eps, out=xn, residual=res, mode=2)
            else:
                ops.rmsnorm(h if li == 0 else mlp, g_in, eps, out=xn, residual=res, mode=2 if li == 0 else 1)
            # (fp8 MoE layers dequantize into the executor's dtype: an fp32 CPU stage stays fp32)
            wdt = self.dtype if L.moe else torch.bfloat16
            ops.linear(xn, L.dense("qkv", wdt), out=qkv, wp=qkv_p)
            if LL.qkv is not None:
                ops.lora_update(xn, qkv, LL.qkv.A, LL.qkv.B, lo.scale, runs)
            kc, vc = self.cache.layer(li)
            self._rope_attend(st, qkv, kc, vc, attn, False)
            ops.linear(attn, L.dense("o", wdt), out=o, wp=L.o_p)
            if LL.o is not None:
                ops.lora_update(attn, o, LL.o.A, LL.o.B, lo.scale, runs)
            self._ar(o)
            ops.rmsnorm(o, g_post, eps, out=xn, residual=res, mode=1)
            if L.moe:
                self._moe_mlp(st, L, xn, mlp, act, packed=False)
                continue
            if LL.gate_up is not None:  # epilogue 0, the update, then SwiGLU
                gu = ops.linear(xn, L.dense("gate_up"), out=st.buf("gu", (T, 2 * F)), wp=gu_p)
                ops.lora_update(xn, gu, LL.gate_up.A, LL.gate_up.B, lo.scale, runs)
                ops.swiglu(gu, out=act)
            else:
                ops.linear(xn, L.dense("gate_up"), out=act, epilogue=1, wp=gu_p)
            ops.linear(act, L.dense("down"), out=mlp, wp=L.down_p)
            if LL.down is not None:
                ops.lora_update(act, mlp, LL.down.A, LL.down.B, lo.scale, runs)
            self._ar(mlp)
        return res, mlp, None

    def _head(self, st: _Step, res, mlp, stream) -> torch.Tensor:
        """What every path ends with: the last residual add (``mlp`` None: done already), then (last stage) the
        final norm and ``lm_head`` on every sequence's last row.  ``stream``: the fused path's (xr, ss_in)."""
        T, H, V = st.T, self.cfg.hidden_size, self.cfg.vocab_size
        hout = res if mlp is None else ops.add(res, mlp, out=st.buf("hout", (T, H)))
        if not self.is_last:
            return hout
        logits = self._lm_head(st, hout, stream, st.last_rows)
        if st.extra is None:
            return logits
        # a ``logit_rows`` step: the other rows go through the head in a launch of their own, so the last
        # rows' logits are the plain step's bit for bit (a decode GEMM's row bits can depend on its row count)
        rows, last_pos, extra_pos, _ = st.extra
        more = self._lm_head(st, hout, None, rows)
        out = torch.empty(last_pos.numel() + extra_pos.numel(), V, dtype=logits.dtype, device=logits.device)
        out[last_pos] = logits
        out[extra_pos] = more
        return out

    def _lm_head(self, st: _Step, hout, stream, rows) -> torch.Tensor:
        """Final norm and ``lm_head`` on ``rows`` of the residual stream ``hout``."""
        cfg, w, T, eps = self.cfg, self.w, st.T, self.cfg.rms_norm_eps
        H, V = cfg.hidden_size, cfg.vocab_size
        S = rows.numel()
        if w.lm_head_p is not None and self._head_packed_ok(S):
            Vp = 16 * w.lm_head_p.shape[0]
            if w.lm_head_folded and stream is not None and S == T:
                # fused-norm path, every row a last row (decode): lm_head (final norm folded in)
                # reads the packed residual stream the last down GEMM left in ``xr`` and scales
                # each row by its rsqrt(mean r^2 + eps) from ``ss_in`` - no final norm launch
                logits = ops.linear(stream[0], None, out=st.buf("logits", (S, Vp)), wp=w.lm_head_p, a_rows=S,
                                    ss_in=stream[1], eps=eps)
                return logits[:, :V]
            fn = ops.rmsnorm(hout, self._unit_norm() if w.lm_head_folded else w.final_norm, eps,
                             out=st.buf("fn_p", (ops.packed_numel(S, H),)), rows=rows, packed=True)
            logits = ops.linear(fn, None, out=st.buf("logits", (S, Vp)), wp=w.lm_head_p, a_rows=S)
            return logits[:, :V]
        fn = ops.rmsnorm(hout, w.final_norm, eps, out=st.buf("fn", (S, H)), rows=rows)
        return ops.linear(fn, w.lm_head, out=st.buf("logits", (S, V)))

    def warmup(self, sizes: Optional[Sequence[int]] = None) -> None:
        """Run throwaway prefill steps at start-up so the first real request does not pay the
        first-call costs of its shapes (hipBLASLt algorithm selection for the row-major GEMMs,
        first launches of the prefill kernels): a cold 64 x 128-token prefill round took 4x
        the warm one.  One single-sequence prefill per size (default: the step
        capacity, 2048 and 512 tokens); the probe session is closed afterwards."""
        cap = min(self.max_tokens, self.max_seq_len - 1)
        sizes = sorted({int(n) for n in (sizes or (cap, 2048, 512)) if 128 < int(n) <= cap}, reverse=True)
        if not sizes:
            return
        sid = "__warmup__"
        with self.exec_lock, torch.inference_mode():
            for n in sizes:
                if self.is_first:
                    x = torch.randint(0, self.cfg.vocab_size, (n,), device=self.device)
                else:
                    x = (0.1 * torch.randn(n, self.cfg.hidden_size, device=self.device)).to(self.dtype)
                try:
                    self.forward([(sid, n)], x, reset=[True])
                except Exception as e:  # noqa: BLE001 - e.g. no KV room for n tokens: warm what fits
                    logger.info(f"warmup of a {n}-token step skipped: {e}")
                finally:
                    self.sessions.close(sid)
            torch.cuda.synchronize(self.device)

    def warmup_serving(self, batch: int, prompt_len: int, decode_steps: int = 2) -> bool:
        """Warm the shapes a serving engine's FIRST steps run, so the first request pays no
        first-call costs: one ragged prefill of ``batch`` sequences x ``prompt_len`` tokens (the
        library GEMM heuristics at batch x prompt rows, the FA2 prefill plan, the last-row lm_head
        and sampler shapes), then ``decode_steps`` decode steps of the batch - the first one
        captures the decode hipGraph of that batch bucket, which the real steps then replay (same
        bucket, same attention partition).  The probe sessions are closed afterwards.  Once per
        (batch, prompt_len) per executor; returns False when skipped (already warm, no room)."""
        if self.device.type != "cuda" or not self.n_layers or batch < 1 or prompt_len < 1:
            return False
        key = (int(batch), int(prompt_len))
        done = self.__dict__.setdefault("_served_warm", set())
        if key in done:
            return False
        ab_steps = 88  # the fold A/B below: 8 windows x (1 capture / warm + 10 timed) steps
        prompt_len = int(min(prompt_len, self.max_seq_len - decode_steps - 2 - ab_steps))
        if prompt_len < 1 or batch > self.sessions.max_sessions:
            return False
        sids = [f"__warm{i}__" for i in range(batch)]
        H = self.cfg.hidden_size
        gen = torch.Generator(device=self.device).manual_seed(1)
        # no_grad, not inference_mode: the decode graph captured here keeps its static buffers,
        # which later steps (inside or outside inference mode) update in place
        with self.exec_lock, torch.no_grad():
            try:
                T = batch * prompt_len
                if self.is_first:
                    x = torch.randint(0, self.cfg.vocab_size, (T,), device=self.device, generator=gen)
                else:
                    x = (0.1 * torch.randn(T, H, device=self.device, generator=gen)).to(self.dtype)
                out = self.forward([(s, prompt_len) for s in sids], x, reset=[True] * batch)
                if self.is_last:
                    self._warm_sampler(out)
                cfg = self.cfg
                pin = ops.qkv_fold_pinned(self._bucket(batch), cfg.q_dim + 2 * cfg.kv_dim, cfg.hidden_size,
                                          bool(self._w8))
                if pin is not None and cfg.model_type != "gpt2":
                    self.qkv_fold_by_bucket[self._bucket(batch)] = pin  # capture the pinned variant below
                for _ in range(decode_steps):
                    if self.is_first:
                        x = torch.randint(0, self.cfg.vocab_size, (batch,), device=self.device, generator=gen)
                    else:
                        x = (0.1 * torch.randn(batch, H, device=self.device, generator=gen)).to(self.dtype)
                    out = self.forward([(s, 1) for s in sids], x)
                    if self.is_last:
                        self._warm_sampler(out)
                self._confirm_qkv_fold(sids, gen)
                done.add(key)
            except Exception as e:  # noqa: BLE001 - e.g. no KV room: the first request warms itself
                logger.info(f"serving warm-up ({batch} x {prompt_len}) skipped: {e}")
                return False
            finally:
                for s in sids:
                    self.sessions.close(s)
            torch.cuda.synchronize(self.device)
        return True

    def _confirm_qkv_fold(self, sids, gen, reps: int = 10) -> Optional[dict]:
        """End-to-end check of the qkv fold for this decode batch: ``ops.autotune_qkv_fold`` times
        the qkv GEMM alone (partials vs the full projection), but the fold also moves work into the
        attention kernel (its q / k / v loads sum the slabs), so the whole decode step - graph
        replays of this batch bucket - is timed both ways and the faster variant kept.  The losing variant's graph is dropped.  Returns {fold: ms} or None.

        Every timed step grows the contexts by a token, so the two variants run in ABBAABBA order
        and each keeps the MEAN of its four windows: both see the same average context (a fixed
        order with the minimum kept handed the first variant ~0.6 % of shorter attention on
        Llama-3-70B, where the fold's real gain is ~1.1 %: profiles/r5z), and short interleaved
        windows see the same clock / thermal state."""
        B = len(sids)
        cfg = self.cfg
        N = cfg.q_dim + 2 * cfg.kv_dim
        key = (ops._m_bucket(B), N, cfg.hidden_size, bool(self._w8))
        if not self.use_graphs or B > self.graph_max_batch or not (self._fuse_rope and self._fused) or self._w4 or \
                os.environ.get("MPAMD_QKV_FOLD", "1") == "0":
            return None
        Bb = self._bucket(B)
        pinned = ops.qkv_fold_pinned(Bb, N, cfg.hidden_size, bool(self._w8))
        if pinned is not None:  # the committed table's decision for this bucket: no timing race
            self.qkv_fold_by_bucket[Bb] = pinned
            return None
        if not ops._QKV_FOLD_CAND.get(key) or ops.autotune_mode() == "off":
            return None
        H = cfg.hidden_size

        def step():
            if self.is_first:
                x = torch.randint(0, cfg.vocab_size, (B,), device=self.device, generator=gen)
            else:
                x = (0.1 * torch.randn(B, H, device=self.device, generator=gen)).to(self.dtype)
            self.forward([(s, 1) for s in sids], x)

        t = {True: 0.0, False: 0.0}
        order = (True, False, False, True, True, False, False, True)
        for fold in order:
            self.qkv_fold_by_bucket[Bb] = fold
            step()  # capture (first time) / warm
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                step()
            e1.record()
            e1.synchronize()
            t[fold] += e0.elapsed_time(e1) / reps / (len(order) // 2)
        # (interleaved windows measured the 70B fold 0.2-0.8 % faster on five boxes and the 7B one
        # 0.3-1.9 % slower, profiles/r5z: the faster variant wins - with unbiased windows a near
        # tie costs nothing either way)
        keep = t[True] < t[False]
        self.qkv_fold_by_bucket[Bb] = keep
        ops.pin_qkv_fold(Bb, N, cfg.hidden_size, bool(self._w8), keep)  # (ops.save_kernel_table keeps it)
        self.__dict__.setdefault("qkv_fold_ab_ms", {})[Bb] = (round(t[True], 4), round(t[False], 4))
        for k in [k for k in self._graphs if k[0] == Bb and k[3] != keep]:
            del self._graphs[k]
        logger.info(f"qkv fold at batch {B}: {t[True]:.3f} ms/step folded vs {t[False]:.3f} unfolded -> "
                    f"{'fold' if keep else 'reduce launch'}")
        return t

    def _warm_sampler(self, logits: torch.Tensor) -> None:
        """The sampling kernel at this row count, on scratch parameters (no session state)."""
        n, dev = logits.shape[0], self.device
        from .sampler import RECENT

        ops.sample(logits, torch.ones(n, device=dev), torch.full((n,), 0.92, device=dev),
                   torch.full((n,), 50, dtype=torch.int32, device=dev), torch.full((n,), 1.5, device=dev),
                   torch.zeros(n, RECENT, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                   torch.arange(n, dtype=torch.int64, device=dev),
                   workspace=torch.empty(max(n, 64) * logits.shape[1], dtype=torch.float32, device=dev),
                   update_history=True)

    def _folded_native(self, T: int) -> bool:
        """Would ``ops.linear`` run BOTH norm-consuming projections (qkv, gate/up) of a T-row
        row-major step on the native GEMM (i.e. over the norm-folded packed weights)?  The
        row-major branch must then normalise with a unit weight, else with the real one and
        the unfolded weights (one decision per step, so the two never mix)."""
        if self.device.type != "cuda" or ops.gemm_policy() == "hipblaslt":
            return False
        cfg = self.cfg
        H, F = cfg.hidden_size, cfg.intermediate_size
        return ops.native_gemm_ok(T, cfg.q_dim + 2 * cfg.kv_dim, H, 0) and \
            ops.native_gemm_ok(T, 2 * F, H, 1)

    def _unit_norm(self) -> torch.Tensor:
        u = getattr(self, "_ones", None)
        if u is None:
            u = self._ones = torch.ones(self.cfg.hidden_size, dtype=self.dtype, device=self.device)
        return u

    def _moe_mlp_w8(self, st: _Step, L, xn, mlp, act) -> None:
        """Sparse-MoE MLP of a <= 64-row step over fp8 experts into ``mlp``: the bf16 router, the
        routing math (ops/moe.py), then two grouped launches for all experts - gate/up + SwiGLU into
        E packed slabs of ``act``, down + combine (channel scales and routing weights in fp32, one
        bf16 rounding).  Experts no row is routed to are skipped on the device by ``cnt``: no host
        sync, the step stays graph-capturable.  MPAMD_MOE_GROUPED=0 (and shapes the grouped kernels
        do not cover): every expert through ops.linear_w8 + addcmul_, nothing skipped."""
        cfg, T, e = self.cfg, st.T, st.buf
        E, k, H, F = cfg.num_local_experts, cfg.num_experts_per_tok, cfg.hidden_size, cfg.intermediate_size
        logits = ops.linear(xn, None, out=e("moe_logits", (T, 16 * L.router_p.shape[0])), wp=L.router_p,
                            a_rows=T)[:, :E]
        w, idx = moe.route(logits, k)
        wd = moe.dense_weights(w, idx, E, out=e("moe_w", (T, E), torch.float32))
        if self._moe_grouped and ops.moe_w8_ok(T, E, H, F):
            cnt = (wd > 0).sum(0, dtype=torch.int32)
            ops.moe_gate_up_w8(xn, L.gate_up_w8, L.gate_up_ws, cnt, T, out=act)
            ops.moe_down_w8(act, L.down_w8, L.down_ws, cnt, wd, T, out=mlp)
            return
        acc = e("moe_acc", (T, H), torch.float32)
        acc.zero_()
        y = e("moe_y", (T, H))
        a1 = act[: ops.packed_numel(T, F)]
        for j in range(E):
            ops.linear_w8(xn, L.gate_up_w8[j], L.gate_up_ws[j], T, out=a1, epilogue=1, out_packed=True)
            ops.linear_w8(a1, L.down_w8[j], L.down_ws[j], T, out=y)
            acc.addcmul_(y, wd[:, j:j + 1])
        mlp.copy_(acc)

    def _moe_mlp(self, st: _Step, L, xn, mlp, act, packed: bool) -> None:
        """Mixtral sparse-MoE MLP into ``mlp`` (ops/moe.py has the routing math and the
        decode-vs-prefill strategy).  Decode steps run every expert on the whole batch with a
        dense combine matrix: no host sync, so the step stays graph-capturable."""
        cfg, T, e = self.cfg, st.T, st.buf
        E, k, H = cfg.num_local_experts, cfg.num_experts_per_tok, cfg.hidden_size
        if packed:
            logits = ops.linear(xn, None, out=e("moe_logits", (T, 16 * L.router_p.shape[0])), wp=L.router_p,
                                a_rows=T)[:, :E]
        else:
            logits = ops.linear(xn, L.router)
        w, idx = moe.route(logits, k)
        acc = e("moe_acc", (T, H), torch.float32)
        acc.zero_()
        gp = (lambda j: L.gate_up_p[j]) if L.gate_up_p is not None else (lambda j: None)  # noqa: E731
        dp = (lambda j: L.down_p[j]) if L.down_p is not None else (lambda j: None)  # noqa: E731
        # fp8 experts (no 16-bit copy kept): dequantize ONE expert's projection at a time
        gw = (lambda j: L.gate_up[j]) if L.gate_up is not None else \
            (lambda j: L.dense("gate_up", self.dtype, expert=j))  # noqa: E731
        dw = (lambda j: L.down[j]) if L.down is not None else \
            (lambda j: L.dense("down", self.dtype, expert=j))  # noqa: E731
        capturing = self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if packed or T <= 64 or capturing:
            wd = moe.dense_weights(w, idx, E, out=e("moe_w", (T, E), torch.float32))
            # small decode batches leave experts unrouted: their GEMMs are skipped on the device
            # (gate = routed-token count) so a 1-session step streams ~k/E of the expert bytes.
            # y persists per T and starts zeroed: a skipped GEMM leaves finite values * weight 0.
            gated = packed and T * k <= 2 * E
            cnt = (wd > 0).sum(0, dtype=torch.int32) if gated else None
            y = self._moe_y.get(T)
            if y is None:
                y = self._moe_y[T] = torch.zeros(T, H, dtype=self.dtype, device=self.device)
            for j in range(E):
                if packed:
                    g = cnt[j:j + 1] if gated else None
                    ops.linear(xn, gw(j), out=act, epilogue=1, wp=gp(j), a_rows=T, out_packed=True, gate=g)
                    ops.linear(act, dw(j), out=y, wp=dp(j), a_rows=T, gate=g)
                else:
                    ops.linear(xn, gw(j), out=act, epilogue=1, wp=gp(j))
                    ops.linear(act, dw(j), out=y, wp=dp(j))
                acc.addcmul_(y, wd[:, j:j + 1])
        else:
            # prefill: group the T*k (token, expert) pairs by expert (one host sync per layer)
            flat = idx.reshape(-1)
            order = torch.argsort(flat, stable=True)
            counts = torch.bincount(flat, minlength=E).tolist()
            tok = order // k
            wsel = w.reshape(-1)[order]
            off = 0
            for j, c in enumerate(counts):
                if c == 0:
                    continue
                rows = tok[off:off + c]
                xe = xn.index_select(0, rows)
                a = ops.linear(xe, gw(j), epilogue=1, wp=gp(j))  # (experts without rows: skipped above,
                ye = ops.linear(a, dw(j), wp=dp(j))              # before anything is dequantized)
                acc.index_add_(0, rows, ye.float() * wsel[off:off + c].unsqueeze(1))
                off += c
        mlp.copy_(acc)
        self._ar(mlp)

    def _ar(self, t: torch.Tensor) -> None:
        """Tensor parallelism: sum the row-parallel partial results over the TP group."""
        if self._tp is not None:
            self._tp.all_reduce(t)

    def _iter_layers(self, fields):
        """``(index, layer)`` over this stage's blocks; with CPU offload the streamed layers come
        from the pinned-host ring (runtime/offload.py) and the resident tail follows."""
        if self._streamer is None:
            yield from enumerate(self.w.layers)
            return
        yield from self._streamer.layers(fields)
        for j in range(self._n_stream, self.n_layers):
            yield j, self.w.layers[j]

    def _setup_offload(self, keep_layers_on_gpu: int) -> None:
        from .offload import LayerStreamer, pin_layer

        w = self.w
        if w.fp8:
            raise ValueError("CPU offload is not supported with fp8 weights")
        if w.w4:
            raise ValueError("CPU offload is not supported with MXFP4 weights")

        keep = max(0, min(int(keep_layers_on_gpu), self.n_layers))
        n_stream = self.n_layers - keep
        host = [pin_layer(L) for L in w.layers[:n_stream]]
        tail = [dataclasses.replace(L, **{f.name: getattr(L, f.name).to(self.device) for f in dataclasses.fields(L)
                                          if isinstance(getattr(L, f.name), torch.Tensor)})
                for L in w.layers[n_stream:]]
        w.layers = host + tail
        for name in ("embed", "pos_embed", "final_norm", "final_norm_b", "lm_head", "lm_head_p"):
            t = getattr(w, name)
            if t is not None:
                setattr(w, name, t.to(self.device))
        self._n_stream = n_stream
        self._streamer = LayerStreamer(host, self.device) if host else None
        self.use_graphs = False  # the slot ring is re-filled every step; graphs would pin one layer set
        logger.info(f"CPU offload: {n_stream} layers streamed from pinned host memory, {keep} resident")

    def _fused_wide_ok(self, M: int) -> bool:
        """Fused-norm decode path at 65..256 rows (bf16): the wide kernels cover every
        projection with its fused epilogue - qkv and gate/up consume the row statistics
        (balanced ring or split-K ring + reduce), o and down produce them (split-K ring, the
        reduce launch applies the residual / packed copy / statistics epilogue)."""
        if not 64 < M <= ops.wide_rows() or self.device.type != "cuda" or not self._packed_ok(M):
            return False
        cfg = self.cfg
        H, F = cfg.hidden_size, cfg.intermediate_size
        return ops.wide_gemm_ok(M, H, cfg.q_dim, 3) and ops.wide_gemm_ok(M, H, F, 3)

    def _head_packed_ok(self, M: int) -> bool:
        return self.device.type == "cuda" and ops.gemm_policy() != "hipblaslt" and 0 < M <= 64 and \
            self.cfg.hidden_size % 128 == 0

    def _fp8_ok(self, M: int) -> bool:
        """fp8 W8A8 decode path: GPU, fp8 weights, fp8 GEMM shape constraints."""
        if self.device.type != "cuda" or not 0 < M <= 64 or not self.w.fp8 or self._w8 or self.cfg.is_moe:
            return False
        cfg = self.cfg
        return all(d % 256 == 0 for d in (cfg.hidden_size, cfg.q_dim, cfg.intermediate_size)) and \
            (cfg.q_dim + 2 * cfg.kv_dim) % 32 == 0

    def _w4_ok(self, M: int) -> bool:
        """Fused-norm decode path of an MXFP4 stage: <= 64 rows, every projection's shape covered by
        the W4A16 ring kernel (otherwise the step takes the dequantizing dense path)."""
        if not self._w4 or not 0 < M <= 64:
            return False
        cfg = self.cfg
        H, F = cfg.hidden_size, cfg.intermediate_size
        return all(ops.w4_gemm_ok(M, N, K, epi) for N, K, epi in
                   ((cfg.q_dim + 2 * cfg.kv_dim, H, 0), (H, cfg.q_dim, 3), (2 * F, H, 1), (H, F, 3)))

    def _lora_packed_ok(self, M: int) -> bool:
        """A LoRA step of M rows on the packed branch: the batched kernels cover every targeted projection."""
        if self._lora is None or self.device.type != "cuda" or not 0 < M <= 64:
            return False
        from ..models.adapters import fused_shape

        return all(ops.lora_ok(M, *fused_shape(self.cfg, p), R) for p, R in self._lora.ranks.items() if R)

    def _packed_ok(self, M: int) -> bool:
        """Packed-activation decode path: GPU, native GEMM allowed, all projections packed; 65..256
        rows when the balanced ring kernel covers every projection of the layer (dense Llama)."""
        if self.device.type != "cuda" or ops.gemm_policy() == "hipblaslt" or not 0 < M <= ops.wide_rows():
            return False
        if getattr(self, "_packed_ready", None) is None:
            cfg = self.cfg
            dims_ok = all(d % 128 == 0 for d in (cfg.hidden_size, cfg.q_dim, cfg.intermediate_size))
            self._packed_ready = dims_ok and all(getattr(L, "qkv_p", None) is not None for L in self.w.layers)
        if not self._packed_ready:
            return False
        if M > 64:
            cfg = self.cfg
            H, F = cfg.hidden_size, cfg.intermediate_size
            return not cfg.is_moe and self._tp is None and all(
                ops.wide_gemm_ok(M, N, K, epi, epi == 1) for N, K, epi in
                ((cfg.q_dim + 2 * cfg.kv_dim, H, 0), (H, cfg.q_dim, 0), (2 * F, H, 1), (H, F, 0)))
        return True

    # ------------------------------------------------------------------ gpt2 (plumbing family)
    def _forward_gpt2(self, plan: Plan, x, prompt=None):
        cfg, w = self.cfg, self.w
        F = torch.nn.functional
        H = cfg.hidden_size
        positions, slots, q_seq, q_ctx, last_rows = plan.meta()
        table = self.sessions.table_dev
        if self.is_first:
            h = w.embed[x.long()] + w.pos_embed[positions]
        else:
            h = x
        for li, L in self._iter_layers(_GPT2_FIELDS):
            if prompt is not None:
                h = h.index_add(0, prompt[0], prompt[1][li])
            a = F.layer_norm(h, (H,), L.ln1_w, L.ln1_b, cfg.layer_norm_eps)
            qkv = F.linear(a, L.attn_w, L.attn_b)
            q, k, v = qkv.split(H, dim=1)
            kc, vc = self.cache.layer(li)
            ops.kv_write(k.contiguous(), v.contiguous(), kc, vc, slots)
            att = ops.paged_attention(q.contiguous(), kc, vc, table, q_seq, q_ctx, self.nh, self.nkv,
                                      self.scale, max_ctx=plan.max_ctx)
            h = h + F.linear(att, L.proj_w, L.proj_b)
            m = F.layer_norm(h, (H,), L.ln2_w, L.ln2_b, cfg.layer_norm_eps)
            m = F.gelu(F.linear(m, L.fc_w, L.fc_b), approximate="tanh")
            h = h + F.linear(m, L.fc2_w, L.fc2_b)
        if not self.is_last:
            return h
        extra = plan.extra_rows(self.device)
        hl = h.index_select(0, last_rows.long() if extra is None else extra[3])
        hl = F.layer_norm(hl, (H,), w.final_norm, w.final_norm_b, cfg.layer_norm_eps)
        return F.linear(hl, w.lm_head)

    # ------------------------------------------------------------------ hipGraph decode
    def _bucket(self, b: int) -> int:
        for cand in (1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 192, 256):
            if b <= cand:
                return min(cand, self.graph_max_batch)
        return b

    def _ctx_bucket(self, c: int) -> int:
        c = max(c, 256)
        return 1 << (c - 1).bit_length()

    def _attn_span(self, ctx: int) -> int:
        """Tokens per query the attention kernels stream at context ``ctx``: under a sliding window W
        at most W + 31 (the MFMA kernel starts at the 32-token step that holds the first key)."""
        return min(int(ctx), self.window + 31) if self.window else int(ctx)

    def _graph_key(self, T: int, max_ctx: int, hooked: bool, slot: int = 0, tag: int = 0) -> tuple:
        """(batch bucket, attention part size, parts, qkv fold, hooked, owner tag, input slot).  Slot 0
        (tag 0) is the graph every caller replays; slots 1 / 2 are an owner's two receive graphs
        (``graph_input``)."""
        B = self._bucket(T)
        # (sliding window: the streamed span is bucketed, not the context - a session far past the
        # window replays one graph; the kernels compute each row's first key from q_ctx themselves)
        ctxb = self._attn_span(min(self._ctx_bucket(max_ctx), self._ctx_bucket(self.max_seq_len)))
        part = ops.attention_partition(B, self.nkv, ctxb, min_part=self._attn_min_part)
        return (B, part[0], part[1], self._qkv_fold(B), bool(hooked), int(tag), int(slot))

    def _graph(self, key: tuple, lora: bool = False) -> "_DecodeGraph":
        """The decode graph of ``key``, captured on first use.  LoRA graphs live in ``_lora_graphs`` under the same key
        tuple: one serves every mix of adapters, since the row slots are data of the replay (the metadata blob)."""
        graphs = self._lora_graphs if lora else self._graphs
        g = graphs.get(key)
        if g is None:
            if self._graph_pool is None:
                self._graph_pool = torch.cuda.graph_pool_handle()
            g = graphs[key] = _DecodeGraph(self, key[0], (key[1], key[2]), self._graph_pool,
                                           hook=self.graph_hook if key[4] else None, lora=lora)
        return g

    def _run_graph(self, plan: Plan, x: torch.Tensor, hooked: bool = False, owner=None) -> torch.Tensor:
        key = self._graph_key(plan.T, plan.max_ctx, hooked)
        read = None  # a receive graph whose static input this replay reads without being that graph
        tag = self._tag_of(owner)
        pin = self._recv_pin.pop(tag, None) if tag is not None else None
        if pin is not None:
            pkey, pg = pin
            if pkey[:5] == key[:5] and self._graphs.get(pkey) is pg:
                key = pkey  # the receive graph whose static input the hop landed in
            else:  # (step shape changed, or the graph was dropped meanwhile): copied from its input
                read = pg
        g = self._graph(key)
        out = g.replay(plan, x)
        g.mark_replayed()
        if read is not None:  # the next receive into that buffer must wait for this replay's copy
            read.done_ev = g.done_ev
        return out

    def _run_lora_graph(self, plan: Plan, x: torch.Tensor) -> torch.Tensor:
        g = self._graph(self._graph_key(plan.T, plan.max_ctx, False), lora=True)
        out = g.replay(plan, x)
        g.mark_replayed()
        return out

    def graph_input(self, T: int, max_ctx: int, owner=None):
        """Receive target of a stage hop (``PipelineServingEngine``): the static input of the decode
        graph the owner's NEXT step of ``T`` rows will replay, and the event after which that buffer
        is free (the end of its last replay), or None when that step runs eagerly.  The hidden
        states then land where the graph reads them: no receive slab, no copy.  Two receive graphs
        per (owner, bucket) alternate, so the hop of step k lands in one while step k - 1 still
        replays the other (a single buffer would serialise every receive behind the previous step's
        compute); other callers of the executor - other owners included - never replay them."""
        if self.is_first or not (self.use_graphs and T <= self.graph_max_batch) or owner is None:
            return None
        with self.exec_lock:
            tag = self._tag_of(owner)
            if tag is None:
                tag = self._next_tag
                self._next_tag += 1
                try:
                    self._owner_tags[owner] = tag
                except TypeError:  # an owner without weak references: kept alive until release_owner
                    self._owner_strong[id(owner)] = (owner, tag)
            hooked = self.graph_hook is not None and owner is self._hook_owner
            base = self._graph_key(T, max_ctx, hooked)
            sk = (tag,) + base[:5]
            slot = 3 - self._recv_slot.get(sk, 2)  # 1, 2, 1, ...
            self._recv_slot[sk] = slot
            key = base[:5] + (tag, slot)
            g = self._graph(key)
            self._recv_pin[tag] = (key, g)
            return g.x, g.done_ev

    def _tag_of(self, owner) -> Optional[int]:
        if owner is None:
            return None
        try:
            return self._owner_tags.get(owner)
        except TypeError:
            got = self._owner_strong.get(id(owner))
            return got[1] if got is not None and got[0] is owner else None

    def release_owner(self, owner) -> None:
        """Drop ``owner``'s receive graphs and pins (its engine stopped or failed)."""
        with self.exec_lock:
            tag = self._tag_of(owner)
            if tag is None:
                return
            try:
                self._owner_tags.pop(owner, None)
            except TypeError:
                self._owner_strong.pop(id(owner), None)
            self._recv_pin.pop(tag, None)
            for k in [k for k in self._recv_slot if k[0] == tag]:
                del self._recv_slot[k]
            for k in [k for k in self._graphs if k[5] == tag]:
                del self._graphs[k]

    def graph_rows(self, T: int, is_decode: bool) -> Optional[int]:
        """Rows of the static output a step of ``T`` tokens would replay into (its batch bucket),
        or None when the step runs eagerly (same rule as ``run``, no deep prompts)."""
        if self.use_graphs and is_decode and T <= self.graph_max_batch:
            return self._bucket(T)
        return None

    def graph_hook_free(self, owner=None) -> bool:
        """True when no other owner's graph hook is installed (``owner`` may hold it already)."""
        return self.graph_hook is None or self._hook_owner is owner

    def set_graph_hook(self, fn, owner=None) -> None:
        """Record ``fn(out)`` at the end of the decode graphs captured for ``owner`` (the engine
        whose stage hop it is).  Steps run with ``forward(..., hook_owner=owner)`` replay those
        graphs; every other caller (a second engine on a shared executor, TCP requests, the
        throughput probe) gets hook-free graphs of its own, so a recorded send can never be
        replayed on someone else's behalf.  One owner at a time: a different owner raises."""
        with self.exec_lock:
            if fn is not None and not self.graph_hook_free(owner):
                raise RuntimeError("this executor already records another engine's graph hop")
            self._drop_hooked()
            self.graph_hook = fn
            self._hook_owner = owner if fn is not None else None

    def clear_graph_hook(self, owner=None) -> None:
        """Remove ``owner``'s hook and the graphs that recorded it (no-op for a non-owner)."""
        with self.exec_lock:
            if self.graph_hook is not None and self._hook_owner is owner:
                self._drop_hooked()
                self.graph_hook = None
                self._hook_owner = None

    def _drop_hooked(self) -> None:
        for k in [k for k in self._graphs if k[4]]:
            del self._graphs[k]

    def clear_graphs(self):
        self._graphs.clear()
        self._lora_graphs.clear()


class _DecodeGraph:
    """A captured decode step for a fixed (batch bucket, attention partition).

    Its metadata lives in ONE device blob (positions, slots | q_seq, q_ctx, last_rows) that a
    replay refills with a single host-to-device copy from a double-buffered pinned staging
    blob, padded for the bucket (padding rows: slot -1, context 0): round 1 issued six small
    copies / fills per step (profiles/r2_decode_step_*.txt).  A LoRA graph (``lora``) appends the
    rows' adapter slots, int32 [B] (padding rows: -1), to the same blob."""

    def __init__(self, ex: StageExecutor, B: int, part: Tuple[int, int], pool, hook=None, lora: bool = False):
        self.ex, self.B, self.part = ex, B, part
        dev, H, dt = ex.device, ex.cfg.hidden_size, ex.dtype
        if ex.is_first:
            self.x = torch.zeros(B, dtype=torch.long, device=dev)
        else:
            self.x = torch.zeros(B, H, dtype=dt, device=dev)
        nbytes = 16 * B + 12 * B + (4 * B if lora else 0)  # int64 [2, B] + int32 [3 B] (+ int32 [B] slots)
        self.blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.meta64 = self.blob[: 16 * B].view(torch.int64).view(2, B)
        self.meta32 = self.blob[16 * B: 28 * B].view(torch.int32)
        self.lora_slots = self.blob[28 * B:].view(torch.int32) if lora else None
        self._stage = [torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._stage_ev = [None, None]
        self._k = 0
        host = self._stage[0].numpy()
        h64 = host[: 16 * B].view(np.int64).reshape(2, B)
        h32 = host[16 * B:].view(np.int32)
        h64[0] = 0
        h64[1] = -1
        h32[:] = 0
        h32[2 * B:3 * B] = np.arange(B, dtype=np.int32)
        h32[3 * B:] = -1  # (a LoRA graph's row slots)
        self.blob.copy_(self._stage[0])
        self._stage[1].copy_(self._stage[0])
        if ex.gqa_decode_mfma or ex.gqa_decode_mfma_f8:
            ex.decode_qblocks(B)  # allocated outside the capture
        self.bufs: dict = {}
        self.done_ev = None  # end of the last replay on the compute stream (graph_input)
        def step():  # (a fresh one per pass: each allocates its own workspace)
            return _Step(self.x, self.meta64[0], self.meta64[1], self.meta32[:B], self.meta32[B:2 * B],
                         self.meta32[2 * B:], B, 0, True, dev, dt, part=part, bufs=self.bufs,
                         lora=(self.lora_slots, None) if lora else None)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warm up (allocator, hipBLASLt heuristics) outside capture
                ex._forward_llama(step())
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        # Python's cyclic collector must not run inside the capture: a dead executor and its graphs
        # (executor <-> _DecodeGraph reference cycles, freed by the collector only) would be destroyed
        # on the capturing thread in mid-capture, which the runtime answers with an abort.  Collect
        # them now (torch.cuda.graph no longer does) and hold the collector off until capture_end.
        gc.collect()
        gc_on = gc.isenabled()
        gc.disable()
        try:
            # thread-local capture: another thread's stream work (a channel receive posted outside the
            # executor lock) neither breaks this capture nor fails because of it
            with torch.cuda.graph(self.graph, pool=pool, capture_error_mode="thread_local"):
                self.out = ex._forward_llama(step())
                if hook is not None:  # recorded only: the warm-up runs above never call it
                    hook(self.out)
        finally:
            if gc_on:
                gc.enable()
        self.mark_replayed()  # the warm-up runs read ``x``: a receive into it waits for them

    def replay(self, plan: Plan, x: torch.Tensor) -> torch.Tensor:
        b, B = plan.T, self.B
        self._k ^= 1
        k = self._k
        if self._stage_ev[k] is not None:
            self._stage_ev[k].synchronize()  # the copy issued two replays ago
        host = self._stage[k].numpy()
        h64 = host[: 16 * B].view(np.int64).reshape(2, B)
        h32 = host[16 * B:].view(np.int32)
        h64[:, :b] = plan.h64
        h64[0, b:] = 0
        h64[1, b:] = -1
        h32[:b] = plan.h32[:b]
        h32[b:B] = 0
        h32[B:B + b] = plan.h32[b:2 * b]
        h32[B + b:2 * B] = 0
        if self.lora_slots is not None:
            h32[3 * B:3 * B + b] = plan.lora_slots
            h32[3 * B + b:] = -1
        self.blob.copy_(self._stage[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._stage_ev[k] = ev
        if self.ex.is_first:
            self.x[:b].copy_(x.view(-1))
        elif x.data_ptr() != self.x.data_ptr():  # (a hop received into the static input: no copy)
            self.x[:b].copy_(x)
        self.graph.replay()
        return self.out[:b]

    def mark_replayed(self) -> None:
        ev = torch.cuda.Event()
        ev.record()
        self.done_ev = ev
