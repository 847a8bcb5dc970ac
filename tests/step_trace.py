"""Launch traces of the stage executor's step function (plain module, like ``tests/gemm_probe.py``).

``recording(monkeypatch)`` replaces the names ``ops`` and ``moe`` INSIDE ``src.runtime.executor`` with
proxies (the ``ops`` package itself is untouched) and yields a ``Recorder``.  Every call the executor
makes to a callable attribute of either appends one line, the op name and its arguments:

* a tensor is ``T<i><shape><dtype>``; ``i`` is a first-seen index keyed on (storage pointer, storage
  offset, shape, stride), so a trace shows WHICH buffer went where - aliasing included - and no
  address.  The recorder keeps every tensor it has seen alive until it is dropped: a freed temporary
  whose address is reused never shares an index;
* a numpy array is ``A<shape><dtype>#<crc32 of its bytes>``;
* tuples and lists are written element by element, keyword arguments sorted by name, an object whose
  ``repr`` would show an address as ``Type(field=..., ...)``, everything else with ``repr``.

A line that names a tensor is a LAUNCH; one that names none (``attention_partition``, ``gemm_policy``,
``packed_numel``, ``rwk_split`` ...) is a host-side QUERY: a pure function of its arguments.
``assert_matches`` holds the launches to the recorded ones line by line, in order, and the queries to the
recorded ones as a multiset: the same questions, the same number of times.  Their place among the launches is
not compared - ``StageExecutor._step_path`` asks all of a step's path questions before the embedding launch,
where the recorded commit asked some of them after it.

The executor is driven through ``forward`` / ``run`` only, so the recorder runs unchanged on any commit.
The committed traces under ``tests/golden/executor_paths/`` were recorded that way on the commit named
in ``tests/golden/executor_paths/README.md``; ``python -m tests.step_trace DIR [cpu|gpu]`` records every
case of ``tests/test_executor_paths.py`` / ``tests/test_executor_paths_gpu.py`` again into ``DIR``.
"""
import collections
import contextlib
import os
import re
import types
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "executor_paths")


_TENSOR = re.compile(r"\bT\d+\(")


def launches(lines):
    """The lines that name a tensor."""
    return [ln for ln in lines if _TENSOR.search(ln)]


class Recorder:
    def __init__(self):
        self.lines = []
        self._ids, self._keep = {}, []

    def fmt(self, v) -> str:
        if isinstance(v, torch.Tensor):
            key = (v.untyped_storage().data_ptr(), v.storage_offset(), tuple(v.shape), tuple(v.stride()))
            if key not in self._ids:
                self._ids[key] = len(self._ids)
                self._keep.append(v)
            return f"T{self._ids[key]}{tuple(v.shape)}{str(v.dtype).replace('torch.', '')}"
        if isinstance(v, np.ndarray):
            return f"A{v.shape}{v.dtype}#{zlib.crc32(np.ascontiguousarray(v).tobytes()):08x}"
        if isinstance(v, (tuple, list)):
            body = ", ".join(self.fmt(x) for x in v)
            return f"({body})" if isinstance(v, tuple) else f"[{body}]"
        r = repr(v)
        if " at 0x" in r:  # an object without a repr of its own (ops.KVF8: codes, scales): by its fields
            names = sorted(vars(v)) if hasattr(v, "__dict__") else list(getattr(type(v), "__slots__", ()))
            return f"{type(v).__name__}(" + ", ".join(f"{k}={self.fmt(getattr(v, k))}" for k in names) + ")"
        return r

    def proxy(self, real, prefix=""):
        return _Proxy(self, real, prefix)

    def launches(self):
        return launches(self.lines)


class _Proxy:
    def __init__(self, rec, real, prefix):
        self.__dict__.update(_rec=rec, _real=real, _prefix=prefix)

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not callable(real) or isinstance(real, (type, types.ModuleType)):
            return real
        rec, label = self._rec, self._prefix + name

        def call(*a, **k):
            rec.lines.append(label + "(" + ", ".join([rec.fmt(x) for x in a] +
                                                     [f"{n}={rec.fmt(x)}" for n, x in sorted(k.items())]) + ")")
            return real(*a, **k)

        return call


@contextlib.contextmanager
def recording(monkeypatch):
    """Record the executor module's ``ops.*`` / ``moe.*`` calls made inside the block."""
    import src.runtime.executor as exm

    rec = Recorder()
    with monkeypatch.context() as mp:
        mp.setattr(exm, "ops", rec.proxy(exm.ops))
        mp.setattr(exm, "moe", rec.proxy(exm.moe, "moe."))
        yield rec


def step_input(ex, T: int, seed: int = 0) -> torch.Tensor:
    """Seeded input of a T-row step: token ids on a first stage, hidden states on a later one."""
    g = torch.Generator().manual_seed(seed)
    if ex.is_first:
        return torch.randint(0, ex.cfg.vocab_size, (T,), generator=g).to(ex.device)
    return (0.1 * torch.randn(T, ex.cfg.hidden_size, generator=g)).to(ex.device, ex.dtype)


def record_steps(monkeypatch, ex, steps, **plan_kw):
    """Record ``ex.forward`` over ``steps``, each a list of tokens per session (sessions "s0", "s1", ...)."""
    with recording(monkeypatch) as rec:
        for k, ntoks in enumerate(steps):
            seqs = [(f"s{i}", n) for i, n in enumerate(ntoks)]
            ex.forward(seqs, step_input(ex, sum(ntoks), seed=k), **plan_kw)
    return rec


def record_decode(monkeypatch, ex, rows: int, steps: int = 1, **plan_kw):
    """An unrecorded 2-token prefill of ``rows`` sessions, then ``steps`` recorded decode steps of all of them."""
    ex.forward([(f"s{i}", 2) for i in range(rows)], step_input(ex, 2 * rows, seed=9), **plan_kw)
    return record_steps(monkeypatch, ex, [[1] * rows] * steps, **plan_kw)


def golden_path(name: str, root: str = GOLDEN) -> str:
    return os.path.join(root, name + ".txt")


def assert_matches(name: str, lines) -> None:
    """``lines`` against the committed trace of case ``name``: launches line by line, queries as a multiset."""
    with open(golden_path(name)) as f:
        want = f.read().splitlines()
    got_l, want_l = launches(lines), launches(want)
    for i, (a, b) in enumerate(zip(got_l, want_l)):
        assert a == b, f"{name}: launch {i} differs from the recorded step\n  now:      {a}\n  recorded: {b}"
    assert len(got_l) == len(want_l), (f"{name}: {len(got_l)} launches, recorded {len(want_l)}; first extra: "
                                       f"{(got_l + want_l)[min(len(got_l), len(want_l))]}")
    got_q, want_q = (collections.Counter(ln for ln in x if not _TENSOR.search(ln)) for x in (lines, want))
    assert got_q == want_q, (f"{name}: host-side queries differ from the recorded step\n  now only:      "
                             f"{dict(got_q - want_q)}\n  recorded only: {dict(want_q - got_q)}")


def write_all(root: str, which: str) -> None:
    import importlib

    import pytest

    os.makedirs(root, exist_ok=True)
    mod = importlib.import_module("tests.test_executor_paths" + ("_gpu" if which == "gpu" else ""))
    for name in sorted(mod.CASES):
        with pytest.MonkeyPatch.context() as mp:
            lines, _ = mod.CASES[name](mp)
        with open(golden_path(name, root), "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{name}: {len(lines)} calls", flush=True)


if __name__ == "__main__":
    import sys

    os.environ.setdefault("MPAMD_GEMM_AUTOTUNE", "0")  # as tests/conftest.py: the committed kernel table
    write_all(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "cpu")
