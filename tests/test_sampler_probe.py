"""The sampler oracle (tests/sampler_probe.py) checked on the CPU: the generator's known answers,
agreement with ``reference.sample_probs``, and two conditions on the GPU case set computed from the
oracle alone - few draws are ambiguous, and every listed mistake of a sampler changes the token of
at least 5 unambiguous draws (``pytest -s`` prints both tables)."""
import numpy as np
import pytest
import torch

from src.ops import reference as ref
from tests import sampler_probe as sp


def test_splitmix64_known_answers():
    assert sp.splitmix64(0) == 0xE220A8397B1DCDAF
    assert sp.splitmix64(1) == 0x910A2DEC89025CC1


def test_uniform_is_the_formula_by_hand():
    seed = 0x1234_5678_9ABC_DEF1
    for row in range(70):
        x = (seed * 0x9E3779B97F4A7C15 + row) % 2 ** 64
        x = (x + 0x9E3779B97F4A7C15) % 2 ** 64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        x ^= x >> 31
        want = np.float32(np.float64(x >> 11) / np.float64(2 ** 53))
        got = sp.uniform(seed, row)
        assert got == float(want) and 0.0 <= got <= 1.0
    assert sp.uniform(-1, 3) == sp.uniform(2 ** 64 - 1, 3)  # the seed is read as unsigned
    assert len({sp.uniform(seed, r) for r in range(70)}) == 70
    assert sp.uniform(seed, 5, row_term=False) == sp.uniform(seed, 0)


def _agreement_rows():
    g = torch.Generator().manual_seed(7)
    for i in range(320):
        V = (64, 1000)[i % 2]
        x = (3.0 * torch.randn(V, generator=g)).to(torch.bfloat16)
        if i % 8 == 3:
            x = (x.float() - x.float().max() - 0.5).to(torch.bfloat16)  # all negative
        k = (0, 5, 50, V - 1, V, 1)[(i // 2) % 6]
        tp = (1.0, 0.92, 0.5, 0.0, 0.05)[(i // 3) % 5]
        rp = (1.0, 1.2, 1.5)[(i // 5) % 3]
        T = (0.5, 0.8, 1.5)[(i // 7) % 3]
        top = torch.topk(x.float(), 3).indices.tolist()
        rnd = torch.randint(0, V, (40,), generator=g).tolist()
        hist = [[], rnd[:2] + [top[0]], rnd + [top[1], -1, V, top[0]], rnd[:5] + [top[0]] * 3,
                [top[0], rnd[0]] * 6][(i // 11) % 5]
        yield x, T, tp, k, rp, hist


def test_oracle_agrees_with_reference_sample_probs():
    """Kept set and normalised probabilities of both draw orders against ``reference.sample_probs``
    (what ``sample_row`` feeds to multinomial).  The two orders and torch's topk / sort differ only
    in WHICH of several ids tied at a cut survive, so the set is compared when the cut is not inside
    a tie (of fp32 probabilities) and the sorted probabilities always."""
    n_sets = 0
    for x, T, tp, k, rp, hist in _agreement_rows():
        want = ref.sample_probs(x, T, tp, k, rp, hist)[0].double().numpy()
        ws = np.sort(want[want > 0])[::-1]
        xp = sp.penalise(sp.bf16_values(x), rp, hist, 50)
        for order in ("sorted", "index"):
            d = sp.oracle(x, T, tp, k, rp, hist, order, cap=50)
            got = np.zeros(len(x))
            got[d.ids] = np.diff(d.edges)
            assert abs(d.edges[-1] - 1.0) < 1e-12 and d.edges[0] == 0.0
            if order == "sorted":
                assert len(d.ids) == len(ws)
                np.testing.assert_allclose(np.sort(got)[::-1][:len(ws)], ws, rtol=0, atol=1e-6)
            # the cut sits in a tie when the last kept and the first dropped probability agree to fp32
            kept = np.zeros(len(x), dtype=bool)
            kept[d.ids] = True
            if all(m.all() or (xp[m].min() - xp[~m].max()) / T > 1e-5 for m in (kept, want > 0)):
                assert set(d.ids.tolist()) == set(np.nonzero(want > 0)[0].tolist()), (order, k, tp, rp)
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
                n_sets += 1
            if order == "index":
                assert (np.diff(d.ids) > 0).all()
    assert n_sets >= 500


def test_reference_sample_row_still_draws_from_sample_probs():
    x = torch.randn(64)
    p = ref.sample_probs(x, 0.8, 0.9, 10, 1.3, [1, 2, 2])
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for _ in range(20):
        assert ref.sample_row(x, 0.8, 0.9, 10, 1.3, [1, 2, 2], generator=g1) == int(torch.multinomial(p, 1, generator=g2))
    assert ref.sample_row(x, 0.0, 0.9, 10, 1.3, [1, 2, 2]) == int(torch.argmax(x))


def test_route_small_examples():
    x = np.arange(512, dtype=np.float64)
    assert sp.route(x, 0.0, 5, 50)[0] == "greedy"
    assert sp.route(x, 1.0, 50, 50)[0] == "sorted"
    assert sp.route(x, 1.0, 65, 50)[0] == "index"  # 64 threads own the vectorised 512-wide row
    assert sp.route(x, 1.0, 0, 50)[0] == "index" and sp.route(x, 1.0, 512, 50)[0] == "index"
    assert sp.route(np.zeros(32000), 1.0, 50, 50)[0] == "index"  # every id a candidate
    wide = np.random.default_rng(0).standard_normal(131080)
    assert sp.route(wide, 1.0, 64, 50)[1].startswith("split C=17")
    assert sp.route(wide, 1.0, 64, 300)[1].startswith("fast top-k (workspace")
    assert sp.route(wide, 1.0, 65, 50)[1].startswith("fast top-k (split fallback")


def test_oracle_orders_on_a_tied_row():
    x = torch.tensor([1.0, 3.0, 3.0, 0.0, 3.0, 2.0])
    s = sp.oracle(x, 1.0, 1.0, 2, 1.0, [], "sorted")
    assert s.ids.tolist() == [1, 2]
    i = sp.oracle(x, 1.0, 1.0, 2, 1.0, [], "index")
    assert i.ids.tolist() == [1, 2, 4]  # ties with the k-th value are kept
    p3 = np.exp(3.0) / np.exp(x.double().numpy()).sum()
    s = sp.oracle(x, 1.0, float(np.float32(2.5 * p3)), 0, 1.0, [], "sorted", cut_eps=0.0)
    assert s.ids.tolist() == [1, 2]  # the sorted prefix with cumulative <= p
    i = sp.oracle(x, 1.0, float(np.float32(2.5 * p3)), 0, 1.0, [], "index", cut_eps=0.0)
    assert i.ids.tolist() == [1, 2, 4]  # the tied maxima cross p together and are the first value: kept
    i = sp.oracle(x, 1.0, float(np.float32(3.2 * p3)), 0, 1.0, [], "index", cut_eps=0.0)
    assert i.ids.tolist() == [1, 2, 4]  # the value 2 crosses p and is dropped
    assert sp.acceptable(s, 0.25) == {1} and sp.acceptable(s, 0.5) == {1, 2} and sp.acceptable(s, 1.0) == {1, 2}
    assert sp.outside(s, 0.75, 1) == pytest.approx(0.25) and sp.outside(s, 0.75, 2) == 0.0


def test_cases_cover_the_parameter_grid():
    cs = sp.cases()
    assert sorted({c.R for c in cs.values()}) == [1, 3, 64, 200]
    assert {c.cap for c in cs.values()} == {3, 50, 300}
    rows = [(c, w) for c in cs.values() for w in c.rows]
    ks = {("V-1" if w.top_k == c.V - 1 else "V" if w.top_k == c.V else w.top_k) for c, w in rows}
    assert set(sp.KS) <= ks
    assert {float(np.float32(v)) for v in sp.TOP_PS} <= {w.top_p for _, w in rows}
    assert {float(np.float32(v)) for v in sp.TEMPS} <= {w.temp for _, w in rows}
    sampled = [(c, w) for c, w in rows if w.temp > 0]
    pen = [w for c, w in sampled if w.rep_pen != 1.0 and any(0 <= t < c.V for t in w.history)]
    assert 3 * len(pen) >= len(sampled)
    for c, w in rows:
        assert len(w.history) <= c.cap
    hs = [w.history for c, w in rows]
    assert any(-1 in h for h in hs) and any(c.V in w.history for c, w in rows)
    assert any(len(h) >= 3 and h[-1] == h[-2] == h[-3] for h in hs) and any(not h for h in hs)
    # split widths: k <= 64 rows next to k = 0, 65 and 200 rows
    for name in ("v65536", "v128256", "v131080"):
        paths = {t.path.split(" (")[0].split(" C=")[0] for t in sp.truth(name)}
        assert {"split", "fast top-k", "general", "greedy"} <= paths, paths
        assert {0, 65, 200} <= {w.top_k for w in cs[name].rows}


def test_ambiguous_share_is_capped():
    """A condition on the cases, not a measurement: at most 10% of a case's draws may have more than
    one acceptable id (cases of 1 or 3 rows: none), or the GPU test would accept too much."""
    for name in sp.CASE_NAMES:
        tr = sp.truth(name)
        amb = sum(len(t.ok) > 1 for t in tr)
        print(f"\nAMBIGUOUS {name:16s} {amb:3d} of {len(tr):3d} draws = {amb / len(tr):.3f}", end="")
        assert all(len(t.ok) >= 1 for t in tr)
        assert amb <= 0.10 * len(tr), name


def test_every_mutant_changes_at_least_five_unambiguous_draws():
    counts = {m: 0 for m in sp.MUTANTS}
    for name in sp.CASE_NAMES:
        c = sp.case(name)
        for r, (w, t) in enumerate(zip(c.rows, sp.truth(name))):
            if len(t.ok) != 1:
                continue
            (want,) = t.ok
            for m, fn in sp.MUTANTS.items():
                if sp.mutant_applies(m, c, r):
                    counts[m] += fn(c, r, w, t.order) != want
    for m, n in counts.items():
        print(f"\nMUTANT {m:36s} changes {n:4d} unambiguous draws", end="")
    assert all(n >= 5 for n in counts.values()), counts
