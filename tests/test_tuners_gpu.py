"""The start-up autotuners end to end on the smallest width with a split-K ring form (N = K = 2048,
so every ring form and its rotated variant is a candidate), two timed calls and one round each:
every tuner writes a valid choice for exactly the buckets it was asked for, restores the kernel
mode it forces while timing (also when a timed call raises), and times nothing for shapes it
already holds.  Which kernel wins is a measurement and is not asserted."""
import pytest
import torch

from src import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = K = 2048
IT = dict(iters=2, rounds=1)


@pytest.fixture
def tuning(monkeypatch):
    """Autotuning on, with the choice tables and the run-time bookkeeping put back afterwards."""
    monkeypatch.setenv("MPAMD_GEMM_AUTOTUNE", "1")
    ops.require_native()
    tables = (ops._SK_CHOICE, ops._W8_CHOICE, ops._FP8_CHOICE, ops._QKV_FOLD_CAND)
    saved, runtime = [dict(t) for t in tables], set(ops._TABLE["runtime"])

    def drop(table, keys):
        for k in keys:
            table.pop(k, None)
        return keys

    yield drop
    for t, s in zip(tables, saved):
        t.clear()
        t.update(s)
    ops._TABLE["runtime"].clear()
    ops._TABLE["runtime"].update(runtime)


def _second_call_times_nothing(table, call):
    before, runtime = dict(table), set(ops._TABLE["runtime"])
    call()
    assert table == before and ops._TABLE["runtime"] == runtime


def test_autotune_w8(tuning):
    keys = tuning(ops._W8_CHOICE, [(m, N, K, e) for e in (0, 3) for m in (4, 64)])
    call = lambda: ops.autotune_w8([(N, K, 0), (N, K, 3)], DEV, ms=(4, 64), **IT)  # noqa: E731
    call()
    for k in keys:
        assert ops._base(ops._W8_CHOICE[k]) in ops._W8_KERNELS
    assert ops._W8_MODE == "auto"
    assert all(ops._k4(k) in ops._TABLE["runtime"] for k in keys)
    _second_call_times_nothing(ops._W8_CHOICE, call)


def test_autotune_fp8(tuning, monkeypatch):
    key, = tuning(ops._FP8_CHOICE, [(32, N, K, 0)])
    monkeypatch.setattr(ops, "_FP8_MODE", "pk")  # whatever was set before is what comes back
    call = lambda: ops.autotune_fp8([(N, K, 0)], DEV, ms=(32,), **IT)  # noqa: E731
    call()
    assert ops._FP8_CHOICE[key] in ops._FP8_KERNELS
    assert ops._FP8_MODE == "pk"
    _second_call_times_nothing(ops._FP8_CHOICE, call)


@pytest.mark.parametrize("fp8", [False, True])
def test_autotune_qkv_fold(tuning, fp8):
    keys = tuning(ops._QKV_FOLD_CAND, [(m, N, K, fp8) for m in (16, 64)])
    call = lambda: ops.autotune_qkv_fold(N, K, DEV, fp8=fp8, ms=(16, 64), **IT)  # noqa: E731
    call()
    for k in keys:
        if ops.rwk_split(k[0], N, K, fp8) > 0:
            assert isinstance(ops._QKV_FOLD_CAND[k], bool)
        else:
            assert k not in ops._QKV_FOLD_CAND
    assert any(k in ops._QKV_FOLD_CAND for k in keys)
    assert ops._W8_MODE == "auto"
    _second_call_times_nothing(ops._QKV_FOLD_CAND, call)


def test_autotune_gemm(tuning, monkeypatch):
    keys = tuning(ops._SK_CHOICE, [(m, N, K, 3) for m in (4, 64)])
    monkeypatch.setattr(ops, "_TUNE_POOL_BYTES", 1 << 25)  # a few rotated weight copies, not a GiB
    ops.set_gemm_sk("off")
    call = lambda: ops.autotune_gemm([(N, K, 3)], DEV, ms=(4, 64), **IT)  # noqa: E731
    call()
    for k in keys:
        assert ops._base(ops._SK_CHOICE[k]) in ops._KERNEL_FLAGS
    assert ops._GEMM_SK == "off"
    _second_call_times_nothing(ops._SK_CHOICE, call)


def test_tuner_that_raises_midway_restores_its_mode(tuning, monkeypatch):
    keys = tuning(ops._W8_CHOICE, [(4, N, K, 0)])
    real, calls = ops.linear_w8, []

    def third_call_raises(*a, **kw):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("third call")
        return real(*a, **kw)

    monkeypatch.setattr(ops, "linear_w8", third_call_raises)
    with pytest.raises(RuntimeError, match="third call"):
        ops.autotune_w8([(N, K, 0)], DEV, ms=(4,), **IT)
    assert len(calls) == 3
    assert ops._W8_MODE == "auto"
    assert keys[0] not in ops._W8_CHOICE
