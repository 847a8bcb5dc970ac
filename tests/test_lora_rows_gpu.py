"""The segmented LoRA kernels for steps above 64 rows (csrc/lora_rows.hip) and the executor's use of them.

Shapes (K, N, R): (128, 16, 16) one k-slice per wave and one column tile; (352, 528, 48) 11 slices uneven over
four waves, N no multiple of 256; (4096, 12288, 192) the twelve rank tiles.  Rows: a tile + 1, whole tiles, partial
last tiles.  ``y`` is a column slice of a wider buffer, ``x`` the head of a longer one whose other rows are NaN.
The two bounds are the derived ones of test_lora_gpu.py (they hold for any order of the fp32 additions).
"""
import functools

import pytest
import torch

from src import ops
from src.models.adapters import merged_weights
from src.models.reference_model import reference_forward
from src.runtime.executor import StageExecutor
from tests.test_lora_gpu import stage

pytestmark = pytest.mark.gpu
DEV, S = "cuda", 4
SHAPES = [(128, 16, 16), (352, 528, 48), (4096, 12288, 192)]
TS = [65, 80, 97, 130]
PATTERNS = ["one", "none", "mixed", "cyclic", "runs"]
NAN, PAD = float("nan"), 8  # PAD: columns of the wider buffer on either side of y


@functools.lru_cache(maxsize=None)
def stacks(K, N, R):
    g = torch.Generator(device=DEV).manual_seed(K * 31 + N * 7 + R)
    A = (torch.randn(S, R, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)
    B = (torch.randn(S, N, R, device=DEV, generator=g) * R ** -0.5).to(torch.bfloat16)
    return A, B, torch.tensor([2.0, 0.5, 1.0, 16 / 8 ** 0.5], device=DEV)


def slots_of(T, pattern):
    if pattern in ("one", "none"):
        sl = [2 if pattern == "one" else -1] * T
    elif pattern == "cyclic":  # every row of a tile a different slot than its neighbours
        sl = [m % S for m in range(T)]
    elif pattern == "mixed":   # adapters 0, 1, 3 and base rows; slot 2 unused
        sl = [(0, -1, 3, 1, -1)[(m * 7 + m // 5) % 5] for m in range(T)]
    else:                      # session-like runs of 5 .. 23 rows whose boundaries fall inside tiles
        sl, i = [], 0
        while len(sl) < T:
            sl += [(0, 1, -1, 3)[i % 4]] * (5, 23, 7, 18, 11, 14)[i % 6]
            i += 1
    return torch.tensor(sl[:T], dtype=torch.int32, device=DEV)


def rows(T, K, seed):
    return torch.randn(T, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(torch.bfloat16)


def run_pair(K, N, R, sl, y0, x, A=None, B=None):
    """shrink + expand with everything the ops must not read set to NaN -> (t, y, the wider buffer of y)."""
    T = sl.numel()
    A0, B0, scale = stacks(K, N, R)
    A, B = (A0 if A is None else A).clone(), (B0 if B is None else B).clone()
    for s in set(range(S)) - set(sl.tolist()):  # a slot no row names
        A[s], B[s] = NAN, NAN
    xq = torch.full((T + 16, K), NAN, dtype=torch.bfloat16, device=DEV)
    xq[:T] = x
    xq[:T][sl < 0] = NAN
    t = torch.full((T, R), NAN, dtype=torch.float32, device=DEV)
    wide = torch.full((T, N + 2 * PAD), 3.0, dtype=torch.bfloat16, device=DEV)
    y = wide[:, PAD:PAD + N]
    y.copy_(y0)
    ops.lora_update_rows(xq[:T], y, A, B, scale, sl, t=t)
    return t, y, wide


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K,N,R", SHAPES)
def test_kernels_within_the_derived_bounds_and_read_only_their_rows(K, N, R, T, pattern):
    A, B, scale = stacks(K, N, R)
    sl = slots_of(T, pattern)
    x, y0 = rows(T, K, 1), rows(T, N, 2)
    t, y, wide = run_pair(K, N, R, sl, y0, x)
    live = sl >= 0
    # base rows: t not written (still the NaN fill), y bit-unchanged; so are the columns around y
    assert bool(torch.isnan(t[~live]).all()) and torch.equal(y[~live], y0[~live])
    assert bool((wide[:, :PAD] == 3.0).all()) and bool((wide[:, PAD + N:] == 3.0).all())
    if pattern == "none":
        assert torch.equal(y, y0)
        return
    assert not bool(torch.isnan(t[live]).any()) and not bool(torch.isnan(y[live].float()).any())
    for s in sorted(set(sl[live].tolist())):  # fp64 per slot: sums and sums of magnitudes as two products
        idx = torch.nonzero(sl == s).flatten()
        xs, As, Bs, sc = x[idx].double(), A[s].double(), B[s].double(), scale[s].double()
        t64 = sc * (xs @ As.t())
        bound = 2 * K * 2.0 ** -24 * sc * (xs.abs() @ As.abs().t())
        err = (t[idx].double() - t64).abs()
        print(f"LORA_SHRINK_ROWS {K} {R} {T} {pattern} slot {s}: worst err - bound {(err - bound).max().item():.3e}")
        assert bool((err <= bound).all())
        ts = t[idx].double()  # expand, given the kernel's own t
        y64 = y0[idx].double() + ts @ Bs.t()
        bound = 2.0 ** -8 * y64.abs() + 2 * (R + 2) * 2.0 ** -24 * (y0[idx].double().abs() + ts.abs() @ Bs.abs().t())
        err = (y[idx].double() - y64).abs()
        print(f"LORA_EXPAND_ROWS {N} {R} {T} {pattern} slot {s}: worst err - bound {(err - bound).max().item():.3e}")
        assert bool((err <= bound).all())


def test_a_row_does_not_depend_on_its_neighbours_slots_or_matrices():
    K, N, R, T, m = 352, 528, 48, 97, 70
    x, y0 = rows(T, K, 3), rows(T, N, 4)
    A, B, _ = stacks(K, N, R)
    An, Bn = A.clone(), B.clone()
    An[0], Bn[0] = NAN, NAN  # slot 0: rows 64, 68, 72 and 76 of row 70's tile name it under "cyclic"
    got = []
    for other, mats in (("cyclic", (A, B)), ("runs", (A, B)), ("none", (A, B)), ("cyclic", (An, Bn))):
        sl = slots_of(T, other)
        sl[m] = 1
        t, y, _ = run_pair(K, N, R, sl, y0, x, *mats)
        got.append((t[m].clone(), y[m].clone()))
    assert not bool(torch.isnan(got[0][0]).any()) and not torch.equal(got[0][1], y0[m])
    for t, y in got[1:]:
        assert torch.equal(t, got[0][0]) and torch.equal(y, got[0][1])


def test_uncovered_shapes_launch_nothing():
    for T, N, K, R in ((97, 16, 100, 16), (97, 24, 128, 16), (97, 16, 128, 24), (97, 16, 128, 208), (0, 16, 128, 16)):
        assert not ops.lora_rows_ok(T, N, K, R), (T, N, K, R)
    assert ops.lora_rows_ok(1, 16, 32, 16) and ops.lora_rows_ok(1 << 20, 12288, 4096, 192)
    T = 97
    sl, scale = torch.zeros(T, dtype=torch.int32, device=DEV), torch.ones(S, device=DEV)
    for K, R in ((100, 16), (128, 24), (128, 208)):
        t = torch.full((T, R), 7.0, device=DEV)
        with pytest.raises(RuntimeError, match="no kernel covers"):
            ops.lora_shrink_rows(torch.ones(T, 128, dtype=torch.bfloat16, device=DEV)[:, :K],
                                 torch.ones(S, R, K, dtype=torch.bfloat16, device=DEV), scale, sl, out=t)
        assert bool((t == 7.0).all())
    for N, R in ((24, 16), (16, 24), (16, 208)):
        y = torch.full((T, 32), 7.0, dtype=torch.bfloat16, device=DEV)[:, :N]
        with pytest.raises(RuntimeError, match="no kernel covers"):
            ops.lora_expand_rows(torch.ones(T, R, device=DEV), torch.ones(S, N, R, dtype=torch.bfloat16, device=DEV),
                                 sl, y)
        assert bool((y == 7.0).all())


# ---------------------------------- executor: small-llama with test_lora_gpu.py's adapters ``qv`` and ``all``
KW = dict(kv_cache_bytes=256 << 20, max_sessions=80, max_seq_len=512, use_graphs=False, warmup=False)


@pytest.fixture
def calls(monkeypatch):
    """How often the executor reached each form of the update."""
    n = {"rows": 0, "runs": 0}

    def count(key, op):
        def wrapped(*a, **kw):
            n[key] += 1
            return op(*a, **kw)
        return wrapped
    monkeypatch.setattr(ops, "lora_update_rows", count("rows", ops.lora_update_rows))
    monkeypatch.setattr(ops, "lora_update", count("runs", ops.lora_update))
    return n


def prefill_errors(ex, names, tag):
    """Max |logit - fp32 oracle on merged weights| per session of one ragged prefill step (70, 9 and 20 tokens)."""
    cfg, w = stage("small-llama")
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV) for n in (70, 9, 20)]
    logits = ex.forward([(f"{tag}{i}", len(p)) for i, p in enumerate(seqs)], torch.cat(seqs), adapters=names)
    return [(logits[i].float() - reference_forward([merged_weights(w, ex.adapter_slot(nm))], p)[-1]).abs().max().item()
            for i, (nm, p) in enumerate(zip(names, seqs))]


def test_a_prefill_step_runs_the_kernels_within_twice_the_base_models_error(calls):
    ex = StageExecutor(*stage("small-llama"), DEV, **KW)
    base = max(prefill_errors(ex, ["", "", ""], "b"))
    assert calls == {"rows": 0, "runs": 0}
    errs = prefill_errors(ex, ["all", "qv", ""], "s")
    print(f"LORA_ROWS_ORACLE logit errors {errs} vs base {base:.4f}")
    assert calls["rows"] > 0 and calls["runs"] == 0
    assert max(errs) <= 2 * base, (errs, base)


def test_the_switch_and_pure_decode_steps_keep_the_form_by_runs(calls, monkeypatch):
    cfg, w = stage("small-llama")
    ex = StageExecutor(cfg, w, DEV, **KW)
    names = [("qv", "", "all")[i % 3] for i in range(65)]
    ids = torch.arange(130, device=DEV) % cfg.vocab_size
    lg = ex.forward([(f"d{i}", 2) for i in range(65)], ids, adapters=names)  # 130 rows of prompts
    assert calls["rows"] > 0 and calls["runs"] == 0
    calls.update(rows=0, runs=0)
    ex.forward([(f"d{i}", 1) for i in range(65)], torch.argmax(lg.float(), -1), adapters=names)  # 65 decode rows
    assert calls["rows"] == 0 and calls["runs"] > 0
    calls.update(rows=0, runs=0)
    monkeypatch.setenv("MPAMD_LORA_ROWS", "0")
    off = StageExecutor(cfg, w, DEV, **KW)
    prefill_errors(off, ["all", "qv", ""], "o")
    assert calls["rows"] == 0 and calls["runs"] > 0
