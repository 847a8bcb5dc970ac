"""LoRA adapters of a stage: PEFT directories or synthetic ones, stacked per fused projection.

Upstream Petals servers host PEFT LoRA adapters (``--adapters``; a request names one in its
``active_adapter`` metadata, reference petals/server/handler.py ``_get_active_adapter``,
backend.py ``using_adapter``).  There every adapter wraps every Linear and the active one is a
process-wide switch.  Here the adapters of a stage are stacked into a few tensors per layer, indexed
by an adapter *slot*, so one ragged step can carry rows of different adapters (and base-model rows,
slot -1) and the batched kernels (ops/csrc/lora.hip) pick each row's matrices on the device.

For a projection ``y = W x`` and an adapter with ``A [r, K]``, ``B [N, r]``:

    y' = bf16( fp32(y) + sum_j fp32(B[n, j]) * t[j] ),    t = scale * (A x) in fp32,

``scale = lora_alpha / r`` (``/ sqrt(r)`` with ``use_rslora``), an fp32 value per slot that is never
folded into ``B``.

Storage per layer and per *fused* projection P of the project's own (qkv, o, gate_up, down), over
the S loaded adapters: ``A`` [S, R, K], ``B`` [S, N, R] in the stage's dtype (bf16 on the GPU) and
one ``scale`` fp32 [S]; R is the largest fused rank of P over the adapters, zero-padded to a
multiple of 16 (at most 192).

* qkv: ``A = cat(A_q, A_k, A_v)`` along the rank; ``B`` is block structured - ``B_q`` fills rows
  [0, q_dim) of its own rank columns, ``B_k`` / ``B_v`` theirs, zero elsewhere.
* gate_up: ``A = cat(A_gate, A_up)``; the rows of ``B`` follow the 16-row gate/up interleave of
  the base weight (``weights.interleave_gate_up``, the same routine).
* a module an adapter does not target contributes no rank columns; a projection no loaded adapter
  targets gets no storage (and no launch).
* a layer whose packed qkv / gate_up carry the RMSNorm weight g (``LlamaLayer.folded``) is fed
  unit-normalised rows: for those the loader also keeps ``A diag(g)``, computed in fp32 and rounded
  once (``LoraProj.A_folded``); the executor hands the kernel whichever matches its ``xn``.

A PEFT directory holds ``adapter_config.json`` + ``adapter_model.safetensors`` with HF key names
``base_model.model.model.layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight`` and
``...mlp.{gate,up,down}_proj...``; only this stage's blocks are read, by key.  ``peft`` itself is
not needed.  ``synthetic:NAME:R[:mod,mod...]`` makes a deterministic adapter from (seed, NAME, layer
index, module) - the same on every stage - for presets and measurements.
"""
from __future__ import annotations

import dataclasses
import hashlib
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .config import ModelConfig
from .weights import LlamaLayer, StageWeights, interleave_gate_up

MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
# fused projection -> the HF modules whose rank columns it concatenates, in order
FUSED = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",), "gate_up": ("gate_proj", "up_proj"),
         "down": ("down_proj",)}
MAX_RANK = 64         # per module (adapter_config.json ``r``)
MAX_FUSED_RANK = 192  # per fused projection, after padding (the kernels' limit: 3 x 64)
RANK_PAD = 16
SYNTHETIC_MODULES = ("q_proj", "v_proj")
CONFIG_FILE, WEIGHT_FILE = "adapter_config.json", "adapter_model.safetensors"


def module_shape(cfg: ModelConfig, mod: str) -> Tuple[int, int]:
    """(N, K) of the base Linear an HF module name stands for."""
    H, F = cfg.hidden_size, cfg.intermediate_size
    return {"q_proj": (cfg.q_dim, H), "k_proj": (cfg.kv_dim, H), "v_proj": (cfg.kv_dim, H), "o_proj": (H, cfg.q_dim),
            "gate_proj": (F, H), "up_proj": (F, H), "down_proj": (H, F)}[mod]


def fused_shape(cfg: ModelConfig, proj: str) -> Tuple[int, int]:
    H, F = cfg.hidden_size, cfg.intermediate_size
    return {"qkv": (cfg.q_dim + 2 * cfg.kv_dim, H), "o": (H, cfg.q_dim), "gate_up": (2 * F, H), "down": (H, F)}[proj]


@dataclasses.dataclass
class Adapter:
    """One adapter's matrices for a block range: ``layers[i][module] = (A [r, K], B [N, r])`` (CPU)."""
    name: str
    r: int
    lora_alpha: float
    use_rslora: bool
    modules: Tuple[str, ...]
    layers: Dict[int, Dict[str, Tuple[torch.Tensor, torch.Tensor]]]

    @property
    def scale(self) -> float:
        return self.lora_alpha / (math.sqrt(self.r) if self.use_rslora else self.r)


def parse_spec(spec: str) -> dict:
    """``synthetic:NAME:R[:mod,mod...]`` | ``NAME=path`` | ``path`` (name: the directory's base name)."""
    spec = str(spec)
    if spec.startswith("synthetic:"):
        parts = spec.split(":")
        if len(parts) not in (3, 4) or not parts[1] or not parts[2].isdigit():
            raise ValueError(f"adapter spec {spec!r}: expected synthetic:NAME:R[:mod,mod...]")
        mods = tuple(m for m in parts[3].split(",") if m) if len(parts) == 4 else SYNTHETIC_MODULES
        return {"kind": "synthetic", "name": parts[1], "r": int(parts[2]), "modules": _check_modules(mods, spec)}
    if "=" in spec and not os.path.isdir(spec):
        name, path = spec.split("=", 1)
    else:
        name, path = os.path.basename(os.path.normpath(spec)), spec
    if not name:
        raise ValueError(f"adapter spec {spec!r} has no name")
    return {"kind": "peft", "name": name, "path": path}


def _check_modules(mods, where) -> Tuple[str, ...]:
    if isinstance(mods, str) or not isinstance(mods, (list, tuple)):
        raise ValueError(f"{where}: target_modules must be a list of module names, got {mods!r} "
                         f"(a string is a regular expression in PEFT: not supported)")
    bad = [m for m in mods if m not in MODULES]
    if bad or not mods:
        raise ValueError(f"{where}: target_modules must be drawn from {MODULES}, got {list(mods)}")
    return tuple(m for m in MODULES if m in mods)


def _check_rank(r, where) -> int:
    if not isinstance(r, int) or isinstance(r, bool) or not 1 <= r <= MAX_RANK:
        raise ValueError(f"{where}: r must be an integer in [1, {MAX_RANK}], got {r!r}")
    return r


def read_peft_config(path: str) -> dict:
    """Validated ``adapter_config.json``: {r, lora_alpha, use_rslora, modules}.  Every field this
    project does not implement raises a ValueError that names it."""
    fn = os.path.join(path, CONFIG_FILE)
    if not os.path.exists(fn):
        raise FileNotFoundError(f"adapter directory {path!r} has no {CONFIG_FILE}")
    with open(fn) as f:
        c = json.load(f)
    where = fn
    if str(c.get("peft_type", "")).upper() != "LORA":
        raise ValueError(f"{where}: peft_type must be LORA, got {c.get('peft_type')!r}")
    if c.get("use_dora"):
        raise ValueError(f"{where}: use_dora is not supported")
    if c.get("modules_to_save"):
        raise ValueError(f"{where}: modules_to_save is not supported")
    for k in ("rank_pattern", "alpha_pattern"):
        if c.get(k):
            raise ValueError(f"{where}: a non-empty {k} is not supported")
    if c.get("fan_in_fan_out"):
        raise ValueError(f"{where}: fan_in_fan_out is not supported")
    if c.get("bias", "none") != "none":
        raise ValueError(f"{where}: bias must be \"none\", got {c.get('bias')!r}")
    mods = _check_modules(c.get("target_modules"), where)
    r = _check_rank(c.get("r"), where)
    alpha = c.get("lora_alpha", r)
    if not isinstance(alpha, (int, float)) or isinstance(alpha, bool):
        raise ValueError(f"{where}: lora_alpha must be a number, got {alpha!r}")
    return {"r": r, "lora_alpha": float(alpha), "use_rslora": bool(c.get("use_rslora", False)), "modules": mods}


def hf_key(layer: int, mod: str, which: str) -> str:
    blk = "self_attn" if mod in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
    return f"base_model.model.model.layers.{layer}.{blk}.{mod}.lora_{which}.weight"


def load_peft_adapter(cfg: ModelConfig, name: str, path: str, start: int, end: int) -> Adapter:
    """Read blocks [start, end) of a local PEFT LoRA directory (only their keys are touched)."""
    c = read_peft_config(path)
    fn = os.path.join(path, WEIGHT_FILE)
    if not os.path.exists(fn):
        raise FileNotFoundError(f"adapter directory {path!r} has no {WEIGHT_FILE}")
    from safetensors import safe_open

    r = c["r"]
    layers: Dict[int, dict] = {}
    with safe_open(fn, framework="pt") as h:
        keys = set(h.keys())
        for i in range(start, end):
            mods = {}
            for mod in c["modules"]:
                N, K = module_shape(cfg, mod)
                ka, kb = hf_key(i, mod, "A"), hf_key(i, mod, "B")
                if ka not in keys or kb not in keys:
                    raise ValueError(f"adapter {name!r}: {fn} lacks {ka if ka not in keys else kb}")
                A, B = h.get_tensor(ka), h.get_tensor(kb)
                if tuple(A.shape) != (r, K) or tuple(B.shape) != (N, r):
                    raise ValueError(f"adapter {name!r}: shapes of layer {i} {mod} do not fit the model: lora_A "
                                     f"{tuple(A.shape)} (expected {(r, K)}), lora_B {tuple(B.shape)} (expected "
                                     f"{(N, r)})")
                mods[mod] = (A, B)
            layers[i] = mods
    return Adapter(name, r, c["lora_alpha"], c["use_rslora"], c["modules"], layers)


def synthetic_adapter(cfg: ModelConfig, name: str, r: int, modules: Sequence[str], start: int, end: int,
                      seed: int = 0, dtype=torch.bfloat16) -> Adapter:
    """Deterministic from (seed, name, layer index, module): the same matrices on every stage.
    ``lora_alpha = 2 r`` and entries of std 0.07 r^-1/4, so ``scale * B A`` has entries of std ~0.01 -
    half the synthetic base weights' own (weights.INIT_STD): the adapter changes the logits
    by far more than any rounding (tests/test_lora.py checks it on the CPU)."""
    r = _check_rank(int(r), f"synthetic adapter {name!r}")
    modules = _check_modules(tuple(modules), f"synthetic adapter {name!r}")
    std = 0.07 * r ** -0.25
    layers: Dict[int, dict] = {}
    for i in range(start, end):
        mods = {}
        for mod in modules:
            N, K = module_shape(cfg, mod)
            digest = hashlib.sha256(f"{seed}/{name}/{i}/{mod}".encode()).digest()
            g = torch.Generator().manual_seed(int.from_bytes(digest[:7], "little"))
            A = torch.empty(r, K).normal_(0.0, std, generator=g).to(dtype)
            B = torch.empty(N, r).normal_(0.0, std, generator=g).to(dtype)
            mods[mod] = (A, B)
        layers[i] = mods
    return Adapter(name, r, 2.0 * r, False, modules, layers)


def load_adapter(cfg: ModelConfig, spec: str, start: int, end: int, seed: int = 0, dtype=torch.bfloat16) -> Adapter:
    if cfg.model_type == "gpt2" or cfg.is_moe:
        raise ValueError(f"adapters with {'GPT-2' if cfg.model_type == 'gpt2' else 'MoE (Mixtral)'} models are not "
                         f"built: LoRA adapters serve dense Llama-family stages")
    p = parse_spec(spec)
    if p["kind"] == "synthetic":
        return synthetic_adapter(cfg, p["name"], p["r"], p["modules"], start, end, seed=seed, dtype=dtype)
    if not os.path.isdir(p["path"]):
        raise FileNotFoundError(f"adapter {p['name']!r}: {p['path']!r} is not a directory")
    return load_peft_adapter(cfg, p["name"], p["path"], start, end)


def spec_ranks(spec: str) -> Tuple[int, Tuple[str, ...]]:
    """(r, target modules) of a spec without reading any weights (block sizing)."""
    p = parse_spec(spec)
    if p["kind"] == "synthetic":
        return _check_rank(p["r"], spec), p["modules"]
    c = read_peft_config(p["path"])
    return c["r"], c["modules"]


def fused_rank(ranks: Sequence[Tuple[int, Sequence[str]]], proj: str) -> int:
    """Padded rank R of fused projection ``proj`` over adapters given as (r, modules); 0: untargeted."""
    R = max((r * sum(1 for m in FUSED[proj] if m in mods) for r, mods in ranks), default=0)
    R = -(-R // RANK_PAD) * RANK_PAD
    if R > MAX_FUSED_RANK:
        raise ValueError(f"fused LoRA rank {R} of projection {proj} exceeds {MAX_FUSED_RANK}")
    return R


@dataclasses.dataclass
class LoraProj:
    A: torch.Tensor                           # [S, R, K]
    B: torch.Tensor                           # [S, N, R]
    A_folded: Optional[torch.Tensor] = None   # A diag(g) for unit-normalised rows (norm-folded base weights)

    def a_for(self, unit_norm: bool) -> torch.Tensor:
        return self.A_folded if (unit_norm and self.A_folded is not None) else self.A


@dataclasses.dataclass
class LoraLayer:
    qkv: Optional[LoraProj] = None
    o: Optional[LoraProj] = None
    gate_up: Optional[LoraProj] = None
    down: Optional[LoraProj] = None


@dataclasses.dataclass
class LoraStacks:
    """The adapters of a stage, attached as ``StageWeights.lora``."""
    names: List[str]               # slot order
    scale: torch.Tensor            # fp32 [S]
    layers: List[LoraLayer]        # one per block of the stage
    ranks: Dict[str, int]          # fused projection -> R (0: no storage)

    def slot(self, name: str) -> int:
        """Slot of adapter ``name`` (-1 for "" / None: the base model); unknown names raise upstream's text."""
        if not name:
            return -1
        try:
            return self.names.index(name)
        except ValueError:
            raise KeyError(f"adapter {name} not found") from None

    def tensors(self):
        yield self.scale
        for L in self.layers:
            for p in FUSED:
                lp = getattr(L, p)
                if lp is not None:
                    yield lp.A
                    yield lp.B
                    if lp.A_folded is not None:
                        yield lp.A_folded

    def nbytes(self, folded: bool = True) -> int:
        """Bytes of the stacks (``folded=False``: without the A diag(g) copies and the scales -
        what ``block_utils.adapter_bytes_per_block`` predicts per block)."""
        n = 0
        for L in self.layers:
            for p in FUSED:
                lp = getattr(L, p)
                if lp is not None:
                    n += lp.A.numel() * lp.A.element_size() + lp.B.numel() * lp.B.element_size()
                    if folded and lp.A_folded is not None:
                        n += lp.A_folded.numel() * lp.A_folded.element_size()
        return n + (self.scale.numel() * 4 if folded else 0)

    def fold_norms(self, layers: Sequence[LlamaLayer]) -> None:
        """Make ``A diag(g)`` for the qkv / gate_up of layers whose packed base weights carry g."""
        for lay, L in zip(layers, self.layers):
            if not getattr(lay, "folded", False):
                continue
            for p, g in (("qkv", lay.input_norm), ("gate_up", lay.post_norm)):
                lp = getattr(L, p)
                if lp is not None and lp.A_folded is None:
                    lp.A_folded = (lp.A.float() * g.float().to(lp.A.device)[None, None, :]).to(lp.A.dtype).contiguous()


def _fuse(cfg: ModelConfig, proj: str, mods: Dict[str, Tuple[torch.Tensor, torch.Tensor]], R: int):
    """One adapter's (A [R, K], B [N, R]) of a fused projection in fp32, zero-padded to rank R."""
    N, K = fused_shape(cfg, proj)
    A = torch.zeros(R, K)
    parts, row, col = [], 0, 0
    for m in FUSED[proj]:
        n, _ = module_shape(cfg, m)
        Bm = torch.zeros(n, R)
        if m in mods:
            a, b = mods[m]
            r = a.shape[0]
            A[col:col + r] = a.float()
            Bm[:, col:col + r] = b.float()
            col += r
        parts.append(Bm)
        row += n
    if proj == "gate_up":  # the base weight's own 16-row gate/up interleave
        B = interleave_gate_up(parts[0], parts[1])
    else:
        B = torch.cat(parts, 0)
    return A, B.contiguous()


def build_stacks(cfg: ModelConfig, adapters: Sequence[Adapter], start: int, end: int, device, dtype) -> LoraStacks:
    names = [a.name for a in adapters]
    if len(set(names)) != len(names) or "" in names:
        raise ValueError(f"adapter names must be unique and non-empty, got {names}")
    if not adapters:
        raise ValueError("no adapters to load")
    ranks = {p: fused_rank([(a.r, a.modules) for a in adapters], p) for p in FUSED}
    layers = []
    for i in range(start, end):
        L = LoraLayer()
        for p, R in ranks.items():
            if R == 0:
                continue
            fused = [_fuse(cfg, p, a.layers[i], R) for a in adapters]
            setattr(L, p, LoraProj(torch.stack([f[0] for f in fused]).to(device=device, dtype=dtype).contiguous(),
                                   torch.stack([f[1] for f in fused]).to(device=device, dtype=dtype).contiguous()))
        layers.append(L)
    scale = torch.tensor([a.scale for a in adapters], dtype=torch.float32, device=device)
    return LoraStacks(names, scale, layers, ranks)


def check_adapters_supported(weights: StageWeights) -> None:
    """The combinations that are not built, named (see README "LoRA adapters")."""
    cfg = weights.cfg
    if cfg.model_type == "gpt2":
        raise ValueError("adapters with GPT-2 are not built: LoRA adapters serve dense Llama-family stages")
    if cfg.is_moe:
        raise ValueError("adapters with MoE (Mixtral) models are not built")
    if weights.layers and any(L.fp8 or L.w4 for L in weights.layers):
        raise ValueError("adapters with fp8 or MXFP4 weights are not built: serve adapters on 16-bit weights")


def merged_weights(weights: StageWeights, slot: int) -> StageWeights:
    """A copy of ``weights`` whose projections are ``W + scale * B A`` of adapter ``slot`` in fp32
    (slot -1: the base weights in fp32): what a dense oracle runs (tests, measurement tools)."""
    lora: Optional[LoraStacks] = getattr(weights, "lora", None)
    layers = []
    for li, lay in enumerate(weights.layers):
        kw = {}
        for p in FUSED:
            W = getattr(lay, p).float()
            lp = getattr(lora.layers[li], p) if (lora is not None and slot >= 0) else None
            if lp is not None:
                W = W + float(lora.scale[slot]) * (lp.B[slot].float() @ lp.A[slot].float())
            kw[p] = W
        layers.append(LlamaLayer(lay.input_norm.float(), kw["qkv"], kw["o"], lay.post_norm.float(), kw["gate_up"],
                                 kw["down"]))
    f = lambda t: None if t is None else t.float()  # noqa: E731
    return StageWeights(weights.cfg, weights.start, weights.end, layers, embed=f(weights.embed),
                        final_norm=f(weights.final_norm), lm_head=f(weights.lm_head))
