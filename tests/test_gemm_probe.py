"""CPU self-test of the decode-GEMM probes (tests/gemm_probe.py): the builder's conditions hold for
every case of ``shape_set(256)`` (exact values, the sum bound, weight round trips through the fp8 and
fp4 packers), the CPU path of ``ops.linear`` / ``linear_w8`` / ``linear_w4`` and of the grouped MoE ops
passes the comparator, and - what makes the GPU probes worth having - a dense fp64 GEMM with ONE
deliberate mistake is rejected on every output element whose exact value the mistake changes."""
import functools

import pytest
import torch

from src import ops
from tests import gemm_probe as gp

SPECS = gp.shape_set(256)


def test_shape_set_names_every_form_and_epilogue():
    """Every form name has a case for each epilogue it takes (whether it really RUNS there is the GPU
    test's coverage assertion), and the edges the cases aim at are in the set."""
    have = {(s.wt, s.kern, s.epi) for s in SPECS}
    for name in gp.BF16_FORMS:
        for e in gp.FORM_EPIS[ops._base(name)]:
            assert ("bf16", name, e) in have, (name, e)
    for name in gp.W8_FORMS:
        for e in gp.W8_FORM_EPIS[ops._base(name)]:
            assert ("w8", name, e) in have, (name, e)
    assert {("w4", "rw", e) for e in gp.W4_EPIS} <= have
    assert {("bf16", "auto", e) for e in gp.WIDE_EPIS} <= have
    assert len({s.id for s in SPECS}) == len(SPECS)
    # column split: every built width with both remainder edges, and the widths that fall back
    plain = {gp.rw_width(s.N, 0, 256)[1:] for s in SPECS if s.group == "colsplit" and s.epi == 0}
    assert {(1, 0), (2, 1), (2, 255), (3, 1), (4, 1), (5, 1), (6, 1), (6, 0), (8, 1)} <= plain
    glu = {gp.rw_width(s.N, 1, 256)[1:] for s in SPECS if s.group == "colsplit" and s.epi == 1 and s.wt == "w8"}
    assert {(2, 0), (4, 2), (6, 2), (8, 2), (10, 2), (14, 0)} <= glu  # (packed output: even pair counts)
    glu = {gp.rw_width(s.N, 1, 256)[1:] for s in SPECS if s.group == "colsplit" and s.epi == 1 and not s.packed}
    assert {(2, 0), (4, 1), (6, 1), (8, 1), (10, 1)} <= glu
    assert not gp.rw_built(16 * (4 * 256 + 1), 0, 256) and not gp.rw_built(16 * (5 * 256 + 1), 0, 256)
    assert gp.rw_built(32 * 7 * 256, 1, 256, fp8=True) and not gp.rw_built(32 * 7 * 256, 1, 256)
    assert {s.K for s in SPECS if s.group == "ktail"} == {128, 384, 1024, 1152}


def test_builder_conditions_hold_for_every_case():
    """Building a case asserts: sums even and |S| <= 504 on EVERY element, every rounding point exact in
    bf16 (SwiGLU: g and u), rows / residual / weights exact.  No case is left out."""
    keys = list(dict.fromkeys((s.M, s.N, s.K, s.epi) for s in SPECS))
    worst = 0.0
    for M, N, K, epi in keys:
        c = gp.case(M, N, K, epi)
        assert c.expected.shape == (M, c.ncols) and bool(torch.isfinite(c.expected.float()).all())
        if epi == 0:
            worst = max(worst, float((c.expected.double() * torch.exp2(c.w.exp.double())).abs().max()))
    print(f"{len(keys)} cases of {len(SPECS)} specs; largest |S| = {worst:.0f} (bound {gp.SUM_BOUND})")
    assert 0 < worst <= gp.SUM_BOUND


def test_weight_round_trips_through_every_packer():
    seen = list(dict.fromkeys((s.wt, s.N, s.K, s.epi == 1) for s in SPECS))
    for wt, N, K, glu in seen:
        w = gp.weights(N, K, glu)
        assert {"bf16": lambda: w.wp, "w8": lambda: w.w8, "w4": lambda: w.w4}[wt]() is not None  # asserts inside
    w = gp.weights(2048, 1152, True)
    assert sorted(set(w.w.abs().unique().tolist())) == [2.0 ** -6, 2.0 ** -5, 2.0 ** -4, 0.25, 0.5, 1.0]
    print(f"{len(seen)} weights")


def _subset():
    """A few seconds' worth: every weight type, epilogue and layout at one-step and nine-step K, a one-tile
    and a remainder-split N."""
    pick = []
    for s in SPECS:
        if s.M not in (1, 17, 64, 100):
            continue
        if s.group == "ktail" and s.kern in ("rw", "rwk+r") and s.K in (128, 1152):
            pick.append(s)
        elif s.group == "colsplit" and s.kern == "rw" and s.N // 16 in (1, 2, 4, 257, 514, 516):
            pick.append(s)
        elif s.group == "w4" and s.K in (128, 384) and s.N <= 4096:
            pick.append(s)
        elif s.group == "wide" and s.K == 128 and s.N in (2048, 4096):
            pick.append(s)
        elif s.group == "lds" and s.rowmajor and s.kern == "lds22" and s.N == 64:
            pick.append(s)
    return pick


def test_cpu_path_passes_the_comparator():
    specs = _subset()
    assert {s.wt for s in specs} == {"bf16", "w8", "w4"} and {(s.epi, s.packed) for s in specs} >= {
        (0, False), (1, False), (1, True), (2, False), (3, False)}
    for s in specs:
        c = gp.case(s.M, s.N, s.K, s.epi)
        dc = gp.device_case(c, "cpu")
        dw = gp.device_weights(c.w, s.wt, "cpu")
        gp.check(s, c, dc, gp.run(s, c, dc, dw))
    print(f"{len(specs)} specs")


@pytest.mark.parametrize("kind", ["down", "gate_up"])
def test_cpu_moe_path_passes_the_comparator(kind):
    for (H, F, E, routed) in [(256, 128, 4, None), (128, 1152, 8, None), (256, 256, 32, (0, 31)), (256, 256, 1, None),
                              (256, 128, 4, ())]:
        for M in (1, 17):
            c = gp.moe_case(kind, M, H, F, E, routed)
            if kind == "down":
                y = ops.moe_down_w8(gp.moe_act(c), c.w8, c.scale, c.cnt, c.wd, M)
                gp.compare(y, c.expected, None, f"down {H} {F} {E} M={M}")
                if routed == ():
                    assert int(c.cnt.sum()) == 0 and bool((y == 0).all())
            else:
                slab = ops.packed_numel(M, F)
                act = torch.full((E * slab,), 7.0, dtype=torch.bfloat16)
                ops.moe_gate_up_w8(ops.pack_act(c.x), c.w8, c.scale, c.cnt, M, out=act)
                for e in range(E):
                    got = act[e * slab:(e + 1) * slab]
                    if int(c.cnt[e]) > 0:
                        gp.compare(ops.unpack_act(got, M, F), c.expected[e], c.u_zero[e], f"gate_up expert {e}")
                    else:
                        assert bool((got == 7.0).all())


# ------------------------------------------------------------------------------------ deliberate mistakes
MUT_SHAPES = [(50, 2048, 1152), (17, 16 * 257, 128), (64, 2048, 1024)]


@functools.lru_cache(maxsize=None)
def _slices(M, N, K, glu=False):
    """fp64 partial sums [M, N, K/32] of the 32-wide k-slices (their sum over the last axis is the product)."""
    w = gp.weights(N, K, glu)
    x = gp.rows(M, N, K)
    return torch.einsum("mkj,nkj->mnk", x.view(M, K // 32, 32), w.w.view(N, K // 32, 32))


def _judge(acc_bad, M, N, K, epi, what, depends=None):
    """Run the comparator on the mistaken product.  Plain epilogues: rejected exactly where the exact
    value changed (every changed element, nothing else).  Returns (rejected, changed, dependent) counts."""
    c = gp.case(M, N, K, epi)
    acc = _slices(M, N, K, epi == 1).sum(-1)
    out = acc_bad if epi == 0 else acc_bad + c.res.double()
    changed = acc_bad != acc
    rej = gp.rejected(out.to(torch.bfloat16), c.expected)
    assert bool(changed.any()), what
    assert torch.equal(rej, changed), f"{what}: {int(rej.sum())} rejected, {int(changed.sum())} changed"
    dep = int(depends.sum()) if depends is not None else int(changed.sum())
    print(f"{what} M={M} N={N} K={K} epilogue {epi}: {int(rej.sum())} of {dep} dependent elements rejected "
          f"(the others' misread terms cancel exactly)")
    assert int(rej.sum()) >= 0.75 * dep, what
    return int(rej.sum()), dep


def _tile(N, t):
    m = torch.zeros(N, dtype=torch.bool)
    m[16 * t: 16 * t + 16] = True
    return m


@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("M,N,K", MUT_SHAPES)
def test_a_dropped_k_slice_of_one_column_tile_is_rejected(M, N, K, epi):
    P = _slices(M, N, K)
    for t, s in [(0, 0), (N // 16 - 1, K // 32 - 1), (N // 32, K // 64)]:
        bad = P.clone()
        bad[:, 16 * t: 16 * t + 16, s] = 0
        dep = _tile(N, t)[None, :].expand(M, N)
        _judge(bad.sum(-1), M, N, K, epi, f"slice {s} of tile {t} dropped", dep)


@pytest.mark.parametrize("M,N,K", MUT_SHAPES)
def test_the_last_k_slice_counted_twice_is_rejected(M, N, K):
    """The clamped-tail mistake: a dead load's MFMA not skipped."""
    P = _slices(M, N, K)
    _judge(P.sum(-1) + P[..., -1], M, N, K, 0, "last slice twice", torch.ones(M, N, dtype=torch.bool))


@pytest.mark.parametrize("wave", [0, 3])
@pytest.mark.parametrize("M,N,K", MUT_SHAPES)
def test_one_waves_k_slices_left_out_is_rejected(M, N, K, wave):
    P = _slices(M, N, K)
    keep = torch.arange(K // 32) % 4 != wave
    _judge(P[..., keep].sum(-1), M, N, K, 0, f"wave {wave} left out", torch.ones(M, N, dtype=torch.bool))


@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("M,N,K", [s for s in MUT_SHAPES if s[2] >= 1024])
def test_a_split_k_slab_left_out_or_added_twice_is_rejected(M, N, K, twice):
    P = _slices(M, N, K)
    S = 4
    per = K // 32 // S
    for slab in (0, S - 1):
        part = P[..., slab * per: (slab + 1) * per].sum(-1)
        bad = P.sum(-1) + (part if twice else -part)
        _judge(bad, M, N, K, 2, f"slab {slab} of {S} {'twice' if twice else 'left out'}", torch.ones(M, N, dtype=torch.bool))


@pytest.mark.parametrize("what", ["scale", "values"])
@pytest.mark.parametrize("M,N,K", MUT_SHAPES)
def test_scale_or_values_of_the_next_column_tile_are_rejected(M, N, K, what):
    P = _slices(M, N, K)
    acc = P.sum(-1)
    j = gp.channel_exp(N).double()
    for t in (0, 1, N // 16 - 2):
        a, b = slice(16 * t, 16 * t + 16), slice(16 * t + 16, 16 * t + 32)
        bad = acc.clone()
        if what == "scale":  # the fp8 forms' channel scale: every element of the tile is off by 2 or 4
            bad[:, a] = acc[:, a] * torch.exp2(j[a] - j[b])[None, :]
            rej, dep = _judge(bad, M, N, K, 0, f"scale of tile {t} from tile {t + 1}",
                              (_tile(N, t)[None, :] & (acc != 0)))
            assert rej == dep
        else:
            bad[:, a] = acc[:, b]
            _judge(bad, M, N, K, 0, f"values of tile {t} from tile {t + 1}", _tile(N, t)[None, :].expand(M, N))


@pytest.mark.parametrize("M,N,K", [s for s in MUT_SHAPES if s[0] >= 32])
def test_two_swapped_row_tiles_are_rejected(M, N, K):
    acc = _slices(M, N, K).sum(-1)
    bad = acc.clone()
    bad[0:16], bad[16:32] = acc[16:32], acc[0:16]
    dep = torch.zeros(M, N, dtype=torch.bool)
    dep[:32] = True
    _judge(bad, M, N, K, 0, "row tiles 0 and 1 swapped", dep)


@pytest.mark.parametrize("M,N,K", MUT_SHAPES)
def test_a_padding_rows_values_added_into_the_last_row_are_rejected(M, N, K):
    """``row < M`` missing: the (non-zero) row M of the padded tile leaks into row M - 1."""
    acc = _slices(M, N, K).sum(-1)
    pad = gp.rows(1, N + 1, K) @ gp.weights(N, K).w.t()
    bad = acc.clone()
    bad[M - 1] += pad[0]
    dep = torch.zeros(M, N, dtype=torch.bool)
    dep[M - 1] = True
    _judge(bad, M, N, K, 0, "padding row added into the last row", dep)


@pytest.mark.parametrize("M,N,K", [(50, 4096, 1152), (17, 32 * 257, 128)])
def test_swapped_gate_and_up_tiles_are_rejected(M, N, K):
    """SwiGLU under the one-ulp comparator: silu(u) * g instead of silu(g) * u.  Not decidable element by
    element (a zero sum on either side gives 0 both ways, 7 % of the sums at K = 128): the count is stated and
    must be at least three quarters."""
    c = gp.case(M, N, K, 1)
    acc = _slices(M, N, K, True).sum(-1)
    ok = gp.rejected(gp.finish(acc, 1, None)[0], c.expected, c.u_zero)
    assert not bool(ok.any())
    for p in (0, N // 32 - 1):
        bad = acc.clone()
        bad[:, 32 * p: 32 * p + 16], bad[:, 32 * p + 16: 32 * p + 32] = acc[:, 32 * p + 16: 32 * p + 32], acc[:, 32 * p: 32 * p + 16]
        g, u = gp.split_gate_up(bad)
        rej = gp.rejected((gp.silu64(g) * u).to(torch.bfloat16), c.expected, c.u_zero)
        cols = slice(16 * p, 16 * p + 16)
        n = int(rej[:, cols].sum())
        print(f"gate/up pair {p} swapped, M={M} N={N} K={K}: {n} of {M * 16} elements rejected")
        assert n >= 0.75 * M * 16 and int(rej.sum()) == n


@pytest.mark.parametrize("M,N,K", [(50, 4096, 1152), (17, 32 * 257, 128)])
def test_the_smallest_swiglu_mistakes_and_the_one_ulp_bound(M, N, K):
    """One k-slice dropped from a gate or an up tile.  An up change of >= 2 * 2^-j is always rejected
    (relative change >= 2 / 504 > 2 ulp is not guaranteed: stated); a gate change of 1/8 can hide inside
    one ulp where silu is flat - the counts are stated, and must be most of the changed elements."""
    c = gp.case(M, N, K, 1)
    P = _slices(M, N, K, True)
    acc = P.sum(-1)
    for t in (0, 1):  # a gate tile, an up tile
        bad = P.clone()
        bad[:, 16 * t: 16 * t + 16, 0] = 0
        bad = bad.sum(-1)
        g, u = gp.split_gate_up(bad)
        rej = gp.rejected((gp.silu64(g) * u).to(torch.bfloat16), c.expected, c.u_zero)
        ch = gp.split_gate_up((bad != acc).double())
        changed = (ch[0] + ch[1]) > 0
        g0, u0 = gp.split_gate_up(acc)
        visible = changed & ~((u0 == 0) & (u == 0))  # u = 0 before and after: 0 either way
        n, m = int(rej.sum()), int(visible.sum())
        print(f"{'gate' if t == 0 else 'up'} tile slice dropped, M={M} N={N} K={K}: {n} of {m} changed elements rejected")
        assert not bool((rej & ~changed).any()) and n >= 0.5 * m
