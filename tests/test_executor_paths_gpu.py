"""The stage executor's step function on the GPU: every decode path issues the recorded ``ops.*`` /
``moe.*`` calls - the same ops, in the same order, on the same buffers - and ``_step_path`` names the path
the case was written for (tests/step_trace.py; traces under tests/golden/executor_paths/, recorded before
``_step_path`` existed: they carry no path name).

Row counts: 1, 17 (no multiple of 16) and 64 are below and at the limit of the <= 64-row kernels, 65 is
the first past it, 256 is ``ops.wide_rows()`` and 257 one past it.  Every case: two blocks of small-llama
(hidden 512, head_dim 128; GQA with one kv head) or tiny-mixtral, an eager executor unless the case is
about graphs, ``warmup=False``, ``max_seq_len=128`` (512 under the sliding window), a 64 MiB KV budget
(128 MiB where 256 / 257 MHA sessions need more than its 256 pages), fixed seeds.  A "200-token prefill"
is two sessions of 100 tokens, which ``max_seq_len=128`` holds.
"""
import dataclasses

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor
from tests import step_trace as st

pytestmark = pytest.mark.gpu
DEV = "cuda"
RAGGED = [5, 70, 1]
ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
TARGETED = ["synthetic:a:16", f"synthetic:b:8:{ALL7}"]
UNTARGETED = ["synthetic:a:16", "synthetic:b:8:q_proj,k_proj,v_proj,o_proj,down_proj"]
LORA = (None, None)  # what ``_step_path`` takes for "a LoRA step"
CASES = {}


def case(fn):
    CASES["gpu_" + fn.__name__] = fn
    return fn


def executor(model="small-llama", *, gqa=False, window=0, quant=None, adapters=None, first=True, last=True,
             offload=False, sessions=18, **kw):
    cfg = resolve_model(model)
    if gqa:
        cfg = dataclasses.replace(cfg, num_key_value_heads=1)
    if window:
        cfg = dataclasses.replace(cfg, model_type="mistral", sliding_window=window, name=f"{model}-w{window}")
    w = random_stage_weights(cfg, 0, 2, has_embed=first, has_head=last, device="cpu" if offload else DEV,
                             dtype=torch.bfloat16, seed=3, quant_type=quant)
    if adapters:
        w.load_adapters(adapters)
    if offload:
        kw.update(offload=True, keep_layers_on_gpu=1)
    kw.setdefault("use_graphs", False)
    kw.setdefault("max_seq_len", 128)
    return StageExecutor(cfg, w, DEV, kv_cache_bytes=(128 if sessions > 256 else 64) << 20, max_sessions=sessions,
                         warmup=False, **kw)


def decode(mp, rows, path, **kw):
    """A recorded decode step of ``rows`` sessions -> (lines, path checks)."""
    ex = executor(sessions=rows + 1, **kw)
    return st.record_decode(mp, ex, rows).lines, [(ex, rows, None, None, path)]


def graphed(mp, path, adapters=None, **kw):
    """Two decode steps of 17 rows on a ``use_graphs=True`` executor: the first one's trace (two warm-up
    passes and the capture); the replay launches nothing from the executor."""
    ex = executor(use_graphs=True, adapters=adapters, **kw)
    plan_kw = dict(adapters=[("", "a", "b")[i % 3] for i in range(17)]) if adapters else {}
    first = st.record_decode(mp, ex, 17, **plan_kw)
    assert ex.last_graphed
    replay = st.record_steps(mp, ex, [[1] * 17], **plan_kw)
    assert ex.last_graphed and not replay.launches(), replay.launches()
    assert len(ex._lora_graphs if adapters else ex._graphs) == 1
    return first.lines, [(ex, 17, None, LORA if adapters else None, path)]


# ------------------------------------------------------------------------------------ bf16 MHA
@case
def mha_ragged_prefill(mp):
    ex = executor()
    return st.record_steps(mp, ex, [RAGGED]).lines, [(ex, sum(RAGGED), None, None, "packed")]


@case
def mha_prefill_200(mp):
    ex = executor()
    return st.record_steps(mp, ex, [[100, 100]]).lines, [(ex, 200, None, None, "dense")]


@case
def mha_decode_1(mp):
    return decode(mp, 1, "fused")


@case
def mha_decode_17(mp):
    return decode(mp, 17, "fused")


@case
def mha_decode_64(mp):
    return decode(mp, 64, "fused")


@case
def mha_decode_65(mp):
    return decode(mp, 65, "packed")


@case
def mha_decode_256(mp):
    return decode(mp, 256, "dense")


@case
def mha_decode_257(mp):
    return decode(mp, 257, "dense")


@case
def mha_unfused_decode_17(mp):
    mp.setenv("MPAMD_FUSED_NORM", "0")
    return decode(mp, 17, "packed")


@case
def mha_unfused_decode_65(mp):
    mp.setenv("MPAMD_FUSED_NORM", "0")
    return decode(mp, 65, "packed")


@case
def mha_hipblaslt_decode_17(mp):
    policy = ops.gemm_policy()
    ops.set_gemm_policy("hipblaslt")
    try:
        return decode(mp, 17, "dense")
    finally:
        ops.set_gemm_policy(policy)


@case
def mha_middle_stage_decode_17(mp):
    return decode(mp, 17, "fused", first=False, last=False)


@case
def mha_separate_embedding_decode_17(mp):
    mp.setenv("MPAMD_FUSED_ENTRY", "0")
    return decode(mp, 17, "fused")


# ------------------------------------------------------------------------------------ bf16 GQA
@case
def gqa_decode_17(mp):
    return decode(mp, 17, "fused", gqa=True)


@case
def gqa_qkv_fold_decode_17(mp):
    ex = executor(gqa=True)
    ex.qkv_fold_by_bucket[ex._bucket(17)] = True
    return st.record_decode(mp, ex, 17).lines, [(ex, 17, None, None, "fused")]


# ------------------------------------------------------------------------------------ quantized weights
def _fp8(mp, mode, rows, path):
    if mode:
        mp.setenv("MPAMD_FP8_MODE", mode)
    else:
        mp.delenv("MPAMD_FP8_MODE", raising=False)
    return decode(mp, rows, path, gqa=True, quant="fp8")


@case
def fp8_decode_17(mp):
    return _fp8(mp, None, 17, "fused")


@case
def fp8_decode_65(mp):
    return _fp8(mp, None, 65, "dense")


@case
def fp8_w8a8_decode_17(mp):
    return _fp8(mp, "w8a8", 17, "w8a8")


@case
def fp8_w8a8_decode_65(mp):
    return _fp8(mp, "w8a8", 65, "dense")


@case
def fp8_mx_decode_17(mp):
    return _fp8(mp, "mx", 17, "fused")


@case
def fp8_mx_decode_65(mp):
    return _fp8(mp, "mx", 65, "dense")


@case
def mxfp4_decode_17(mp):
    return decode(mp, 17, "fused", quant="mxfp4")


@case
def mxfp4_decode_65(mp):
    return decode(mp, 65, "dense", quant="mxfp4")


# ------------------------------------------------------------------------------------ Mixtral
@case
def moe_decode_4(mp):  # T k <= 2 E: the gated expert GEMMs
    return decode(mp, 4, "packed", model="tiny-mixtral")


@case
def moe_decode_17(mp):
    return decode(mp, 17, "packed", model="tiny-mixtral")


@case
def moe_prefill_70(mp):
    ex = executor("tiny-mixtral")
    return st.record_steps(mp, ex, [[70]]).lines, [(ex, 70, None, None, "dense")]


@case
def moe_fp8_decode_17(mp):
    return decode(mp, 17, "moe_w8", model="tiny-mixtral", quant="fp8")


@case
def moe_fp8_decode_65(mp):
    return decode(mp, 65, "dense", model="tiny-mixtral", quant="fp8")


@case
def moe_fp8_ungrouped_decode_17(mp):
    mp.setenv("MPAMD_MOE_GROUPED", "0")
    return decode(mp, 17, "moe_w8", model="tiny-mixtral", quant="fp8")


# ------------------------------------------------------------------------------------ LoRA
def _lora_decode(mp, specs, rows, path):
    ex = executor(adapters=specs, sessions=rows + 1)
    names = [("", "a", "b")[i % 3] for i in range(rows)]  # rows on slots -1, 0 and 1
    return st.record_decode(mp, ex, rows, adapters=names).lines, [(ex, rows, None, LORA, path)]


@case
def lora_decode_3_gate_up_targeted(mp):
    return _lora_decode(mp, TARGETED, 3, "packed")


@case
def lora_decode_3_gate_up_untargeted(mp):
    return _lora_decode(mp, UNTARGETED, 3, "packed")


@case
def lora_decode_65(mp):
    return _lora_decode(mp, TARGETED, 65, "dense")


@case
def lora_prefill_20(mp):
    ex = executor(adapters=TARGETED)
    rec = st.record_steps(mp, ex, [[9, 4, 7]], adapters=["", "a", "b"])
    return rec.lines, [(ex, 20, None, LORA, "packed")]


# ------------------------------------------------------------------------------------ fp8 KV cache
@case
def kv_fp8_decode_17(mp):
    return decode(mp, 17, "fused", gqa=True, kv_cache_dtype="fp8")


@case
def kv_fp8_prefill_200(mp):
    ex = executor(gqa=True, kv_cache_dtype="fp8")
    return st.record_steps(mp, ex, [[100, 100]]).lines, [(ex, 200, None, None, "dense")]


# ------------------------------------------------------------------------------------ sliding window
def _window(mp, **kw):
    ex = executor(window=96, sliding_window="attend", max_seq_len=512, **kw)
    assert ex.window == 96
    return ex, st.record_steps(mp, ex, [[250]]).lines


@case
def window_prefill_250(mp):
    ex, lines = _window(mp)
    return lines, [(ex, 250, None, None, "dense")]


@case
def window_prefill_250_in_chunks_of_100(mp):
    ex, lines = _window(mp, max_tokens_per_step=100)
    return lines, [(ex, 100, None, None, "packed"), (ex, 50, None, None, "fused")]


@case
def window_decode_after_the_prefill(mp):
    ex = executor(window=96, sliding_window="attend", max_seq_len=512)
    ex.forward([("s0", 250)], st.step_input(ex, 250, seed=9))
    return st.record_steps(mp, ex, [[1]]).lines, [(ex, 1, None, None, "fused")]


# ------------------------------------------------------------------------------------ CPU offload
@case
def offload_prefill_20_and_decode(mp):
    ex = executor(offload=True)
    assert ex._streamer is not None and ex._n_stream == 1
    return st.record_steps(mp, ex, [[20], [1]]).lines, [(ex, 20, None, None, "fused"), (ex, 1, None, None, "fused")]


# ------------------------------------------------------------------------------------ graph captures
@case
def graph_mha_decode_17(mp):
    return graphed(mp, "fused")


@case
def graph_fp8_decode_17(mp):
    mp.delenv("MPAMD_FP8_MODE", raising=False)
    return graphed(mp, "fused", gqa=True, quant="fp8")


@case
def graph_mxfp4_decode_17(mp):
    return graphed(mp, "fused", quant="mxfp4")


@case
def graph_moe_fp8_decode_17(mp):
    return graphed(mp, "moe_w8", model="tiny-mixtral", quant="fp8")


@case
def graph_lora_decode_17(mp):
    return graphed(mp, "packed", adapters=TARGETED)


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_issues_the_recorded_calls(name, monkeypatch):
    lines, paths = CASES[name](monkeypatch)
    for ex, T, prompt, lora, want in paths:
        assert ex._step_path(T, prompt, lora) == want, (T, want)
    st.assert_matches(name, lines)
