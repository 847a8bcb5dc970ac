"""The stage executor's step function on the CPU issues the recorded ``ops.*`` / ``moe.*`` calls: the same
ops, in the same order, on the same buffers (tests/step_trace.py; traces under
tests/golden/executor_paths/).  A CPU executor takes the row-major ("dense") path for every step; the
GPU paths are in tests/test_executor_paths_gpu.py.

Every case: two blocks, fp32, ``warmup=False``, a 64 MiB KV budget, ``max_seq_len=128``, fixed seeds.
"""
import pytest
import torch

from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor
from tests import step_trace as st

RAGGED = [5, 70, 1]
ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
CASES = {}


def case(fn):
    CASES["cpu_" + fn.__name__] = fn
    return fn


def executor(model, *, first=True, last=True, adapters=None, max_sessions=4):
    cfg = resolve_model(model)
    w = random_stage_weights(cfg, 0, 2, has_embed=first, has_head=last, device="cpu", dtype=torch.float32, seed=7)
    if adapters:
        w.load_adapters(adapters)
    return StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=64 << 20, max_sessions=max_sessions,
                         max_seq_len=128, warmup=False)


# Every case returns (trace lines, [(executor, T, prompt, lora, expected path), ...]).
@case
def llama_ragged_prefill(mp):
    ex = executor("tiny-llama")
    return st.record_steps(mp, ex, [RAGGED]).lines, [(ex, sum(RAGGED), None, None, "dense")]


@case
def llama_decode_3(mp):
    ex = executor("tiny-llama")
    return st.record_decode(mp, ex, 3).lines, [(ex, 3, None, None, "dense")]


@case
def llama_middle_stage(mp):
    ex = executor("tiny-llama", first=False, last=False)
    return st.record_steps(mp, ex, [RAGGED, [1, 1, 1]]).lines, [(ex, 3, None, None, "dense")]


@case
def llama_deep_prompt(mp):
    ex = executor("tiny-llama", first=False, last=False)
    g = torch.Generator().manual_seed(3)
    p = 0.5 * torch.randn(2, 3, ex.cfg.hidden_size, generator=g)
    rec = st.record_steps(mp, ex, [[6, 3]], prompts=[p, None])
    return rec.lines, [(ex, 9, (None, None), None, "dense")]


def _lora(mp, specs):
    ex = executor("tiny-llama", adapters=specs)
    names = ["", "a", "b"]  # rows on slots -1, 0 and 1
    rec = st.record_steps(mp, ex, [[4, 2, 3], [1, 1, 1]], adapters=names)
    return rec.lines, [(ex, 3, None, (None, None), "dense")]


@case
def llama_lora_gate_up_targeted(mp):
    return _lora(mp, ["synthetic:a:16", f"synthetic:b:8:{ALL7}"])


@case
def llama_lora_gate_up_untargeted(mp):
    return _lora(mp, ["synthetic:a:16", "synthetic:b:8:q_proj,k_proj,v_proj,o_proj,down_proj"])


@case
def mixtral_prefill_70(mp):
    ex = executor("tiny-mixtral")
    return st.record_steps(mp, ex, [[70]]).lines, [(ex, 70, None, None, "dense")]


@case
def mixtral_decode_3(mp):
    ex = executor("tiny-mixtral")
    return st.record_decode(mp, ex, 3).lines, [(ex, 3, None, None, "dense")]


@case
def gpt2_prefill_and_decode(mp):
    ex = executor("tiny-gpt2")
    return st.record_steps(mp, ex, [[9, 4], [1, 1]]).lines, []


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_issues_the_recorded_calls(name, monkeypatch):
    lines, paths = CASES[name](monkeypatch)
    for ex, T, prompt, lora, want in paths:
        assert ex._step_path(T, prompt, lora) == want
    st.assert_matches(name, lines)
