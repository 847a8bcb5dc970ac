"""The autotuners' one timed section (``ops._time_candidates``), driven on the CPU with stubbed
events: the protocol that decides the committed decode-kernel table.  Per round, candidates run in
mapping order; each gets two warm-up calls, an event, ``iters`` calls over the rotated copies, an
event and a synchronise; the result is each candidate's best round in ms per call."""
import torch

from src import ops


def test_time_candidates_protocol(monkeypatch):
    log = []
    # elapsed ms per (round, candidate), in the order the sections run
    scripted = iter([9.0, 6.0, 3.0, 6.0, 12.0, 1.5])

    class Event:
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            log.append("record")

        def synchronize(self):
            log.append("sync")

        def elapsed_time(self, end):
            assert end is not self
            return next(scripted)

    monkeypatch.setattr(torch.cuda, "Event", Event)
    cands = {name: (lambda i, name=name: log.append((name, i))) for name in ("b", "a", "c")}
    t = ops._time_candidates(cands, iters=3, rounds=2)

    section = lambda n: [(n, 0), (n, 1), "record", (n, 0), (n, 1), (n, 2), "record", "sync"]  # noqa: E731
    assert log == 2 * (section("b") + section("a") + section("c"))
    assert list(t) == ["b", "a", "c"]
    assert t == {"b": 6.0 / 3, "a": 6.0 / 3, "c": 1.5 / 3}
    assert next(scripted, None) is None
