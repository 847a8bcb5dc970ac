"""CPU self-test of the probes for the GEMMs above 64 rows (tests/rows_probe.py): the builder's conditions hold
for every case of ``shape_set(256)`` and ``moe_set()``, the CPU forms of the seven op families pass the
comparators, and a fp64 product with ONE deliberate misread - a scale byte from the wrong k-block, row, column
tile or block map, a k-slice dropped or doubled, a pair's row from its neighbour, a slot added twice - is
rejected on every element whose exact value the misread changes.  What escapes (the 32 signs involved cancel)
is counted, printed, and at most one quarter of the affected elements."""
import pytest
import torch

from tests import rows_probe as rp

BF = torch.bfloat16
SPECS = rp.shape_set(256)
MOES = rp.moe_set()


def test_shape_set_reaches_every_branch_of_the_plan():
    assert len(set(SPECS)) == len(SPECS)
    for fam in rp.DENSE:
        mine = [s for s in SPECS if s.fam == fam]
        assert {s.T for s in mine} == {65, 129, 257, 300, 2049} and {s.K for s in mine} == {128, 384, 1152}
        assert {s.epi for s in mine} == {0, 1}
        uneven = {(s.T > 128, s.epi) for s in mine if len(set(rp.dense_plan(s.T, s.N, s.epi, 256)[2:])) == 2}
        assert {(True, 0), (True, 1), (False, 0)} <= uneven
    # the rule itself, on the cases tests/test_w8_rows_gpu.py's docstring states for 256 CUs
    assert rp.dense_plan(2049, 4000, 0, 256) == (16, 10, 16, 15) and rp.dense_plan(2049, 8000, 1, 256) == (32, 26, 16, 14)
    assert rp.dense_plan(65, 16000, 0, 256) == (256, 232, 4, 3) and rp.dense_plan(65, 16384, 1, 256) == (256, 256, 4, 4)
    assert rp.dense_plan(2049, 4096, 0, 256)[2:] == (16, 16) and rp.dense_plan(300, 560, 0, 256) == (32, 3, 2, 1)
    assert rp.uneven_n(2049, 4000, 0, 256) == 4000 and rp.uneven_n(2049, 4096, 0, 256) > 4096


def test_block_maps():
    nat, mx = rp.block("w4mx", 256), rp.block("mx", 256)
    assert nat.tolist() == [k // 32 for k in range(256)]
    # k = 128 kb + 32 s + 8 q + j -> 4 kb + 2 (s >> 1) + (q >> 1): 32 elements a block, every block met
    assert mx[:32].tolist() == [0] * 16 + [1] * 16 and mx[64:96].tolist() == [2] * 16 + [3] * 16 and int(mx[128]) == 4
    assert torch.bincount(mx).tolist() == [32] * 8 and bool((mx != nat).any())


def test_builder_conditions_and_cpu_forms_dense():
    """Building a case asserts exact rows and weights (round trips through both unpackers), both quantizers
    returning x unchanged, |S| <= 504 on EVERY element and bf16-exact sums; the CPU form of every family then
    passes its comparator."""
    worst = 0.0
    for s in SPECS:
        c = rp.case(s.fam, s.T, s.N, s.K, s.epi)
        assert c.expected.shape == (s.T, c.ncols) and bool(torch.isfinite(c.expected.float()).all())
        if s.epi == 0:
            S = c.expected.double() * torch.exp2(2.0 + c.w.exp.double())[None, :] * torch.exp2((torch.arange(s.T) % 3).double())[:, None]
            worst = max(worst, float(S.abs().max()))
        rp.compare(rp.run_dense(c, c.x, rp.carrier(s.fam, c.w)), c.expected, c.u_zero, c.id)
    print(f"{len(SPECS)} dense cases; largest |S| = {worst:.0f} (bound {rp.SUM_BOUND})")
    assert 0 < worst <= rp.SUM_BOUND
    w = rp.weights(True, 2048, 1152, True)
    assert sorted(w.w.abs().unique().tolist()) == [2.0 ** -e for e in range(8, -1, -1)]
    assert sorted(rp.case("mx", 65, 16, 384, 0).x.double().abs().unique().tolist()) == [2.0 ** -e for e in range(4, -1, -1)]


def test_builder_conditions_and_cpu_forms_moe():
    for spec in MOES:
        c = rp.moe_case(*spec)
        o = c.off.tolist()
        if spec[1] == "edge" and c.T == 258:
            assert o == [0, 128, 257, 258, 516]
        if spec[1] == "invalid":
            assert c.P < 2 * c.T and int(c.x.isnan().any(1).sum()) == 1 and bool(c.act_in[c.P:].isnan().all())
        if c.E == 32:
            assert [e for e in range(32) if o[e + 1] > o[e]] == [0, 31] and bool(c.gu[1][1:31].isnan().all())
        assert set(c.w.unique().tolist()) <= {0.25, 0.5, 0.75} and bool((c.w.sum(1) == 1).all())
        act = rp.run_gate_up(c, c.x, c.gu, c.off, c.tok)
        rp.check_moe(c, act, rp.run_down(c, c.act_in, c.dn, c.off, c.tok, c.wsel, c.idx))
    print(f"{len(MOES)} MoE cases")


def test_scale_layout_against_the_torch_form_of_the_slot_order_quantizer():
    """``scale_bytes`` / ``code_rows`` (what the GPU test holds the three quantizers to) against the torch form of
    ``moe_quant_mx_tiled``: codes of magnitude 256, scale bytes 127 - 8 - a - r, padding rows 0 with scale 127."""
    from src import ops
    c = rp.moe_case("tiledmx", "edge", 258, 384, 1152, 4)
    ax, as_ = ops.moe_quant_mx_tiled(c.x, c.off, c.tok)
    o, rexp = c.off.tolist(), []
    for e in range(c.E):
        for p0 in range(o[e], o[e + 1], 128):
            n = min(128, o[e + 1] - p0)
            rexp += [int(c.tok[p]) % 3 for p in range(p0, p0 + n)] + [-1] * (128 - n)
    rexp = torch.tensor(rexp + [-1] * (128 * ax.shape[0] - len(rexp)))
    rows = rp.code_rows(ax, c.H)
    assert bool(((rows[rexp >= 0] & 0x7F) == rp.CODE_256).all()) and bool((rows[rexp < 0] == 0).all())
    assert torch.equal(as_.reshape(-1), rp.scale_bytes("tiledmx", rexp, c.H).reshape(-1))
    assert int((rexp >= 0).sum()) == c.P and len(set(as_.reshape(-1).tolist())) == 6


# ------------------------------------------------------------------------------------ deliberate misreads
MUT = [(mx, T, N, K) for mx in (False, True) for T, N, K in ((300, 560, 512), (130, 2048, 1152))]


def _setup(mx, T, N, K):
    x, acc = rp.dense_product(mx, T, N, K, False)
    w = rp.weights(mx, N, K)
    fam = "mx" if mx else "w4mx"
    return x, w, acc, rp.block(fam, K), rp.case(fam, T, N, K, 0).expected


def _part(x, w, mask, cols=slice(None)):
    """fp64 [T, cols]: the part of the product that comes from the k of ``mask``."""
    return x[:, mask] @ w.w[cols][:, mask].t()


def _judge(bad, acc, expected, dep, what, exact=True):
    """The comparator on a mistaken fp64 result: nothing outside the changed elements is rejected, every
    changed element is (``exact``), and they are at least three quarters of the ``dep`` affected ones."""
    changed = bad != acc
    rej = rp.rejected(bad.to(BF), expected)
    assert bool(changed.any()) and not bool((rej & ~changed).any()), what
    if exact:
        assert torch.equal(rej, changed), f"{what}: {int(rej.sum())} rejected, {int(changed.sum())} changed"
    n, d = int(rej.sum()), int(dep.sum()) if torch.is_tensor(dep) else int(dep)
    print(f"{what}: {n} of {d} affected elements rejected, {d - n} escape (their misread terms cancel)")
    assert not bool((rej & ~dep).any()) if torch.is_tensor(dep) else True
    assert n >= 0.75 * d, what


def _rows(T, N, lo, hi):
    m = torch.zeros(T, N, dtype=torch.bool)
    m[lo:hi] = True
    return m


def _cols(T, N, t):
    m = torch.zeros(T, N, dtype=torch.bool)
    m[:, 16 * t:16 * t + 16] = True
    return m


@pytest.mark.parametrize("mx,T,N,K", MUT)
def test_an_activation_scale_from_the_neighbouring_k_block_is_rejected(mx, T, N, K):
    x, w, acc, blk, expected = _setup(mx, T, N, K)
    for b, nb in ((0, 1), (K // 32 - 1, K // 32 - 2), (5, 4)):
        f = 2.0 ** (b % 3 - nb % 3)
        _judge(acc + (f - 1) * _part(x, w, blk == b), acc, expected, T * N, f"scale of block {b} from block {nb} T={T} N={N} K={K} mx={mx}")


@pytest.mark.parametrize("d", [1, 16, 64])
@pytest.mark.parametrize("mx,T,N,K", MUT)
def test_an_activation_scale_from_a_row_below_is_rejected(mx, T, N, K, d):
    """``as`` is cut in 64-row groups of four 16-row tiles: the next lane, the next byte, the next group."""
    x, w, acc, blk, expected = _setup(mx, T, N, K)
    r = torch.arange(T) % 3
    f = torch.ones(T, dtype=torch.float64)
    f[:T - d] = torch.exp2((r[:T - d] - r[d:]).double())
    assert bool((f[:T - d] != 1).all())
    for b in (0, K // 32 - 1):
        _judge(acc + (f - 1)[:, None] * _part(x, w, blk == b), acc, expected, _rows(T, N, 0, T - d),
               f"scale of block {b} from {d} rows below T={T} N={N} K={K} mx={mx}")


@pytest.mark.parametrize("T,N,K", [m[1:] for m in MUT if not m[0]])
def test_a_weight_block_scale_from_the_next_k_block_or_column_tile_is_rejected(T, N, K):
    """MXFP4 weights: s4 holds one byte per column and natural 32-block."""
    x, w, acc, blk, expected = _setup(False, T, N, K)
    j = rp.channel_exp(N)
    for t, b in ((0, 0), (N // 16 - 2, K // 32 - 2), (N // 32, 7)):
        cols = slice(16 * t, 16 * t + 16)
        part = _part(x, w, blk == b, cols)
        for what, f in (("k-block", 2.0 ** ((b + 1) % 3 - b % 3)), ("column tile", 2.0 ** float(j[16 * t] - j[16 * t + 16]))):
            bad = acc.clone()
            bad[:, cols] += (f - 1) * part
            _judge(bad, acc, expected, _cols(T, N, t), f"weight scale (tile {t}, block {b}) from the next {what} T={T} N={N} K={K}")


@pytest.mark.parametrize("mx,T,N,K", MUT)
def test_a_channel_scale_from_the_next_column_tile_is_rejected(mx, T, N, K):
    x, w, acc, blk, expected = _setup(mx, T, N, K)
    j = rp.channel_exp(N)
    for t in (0, N // 16 - 2):
        cols = slice(16 * t, 16 * t + 16)
        bad = acc.clone()
        bad[:, cols] *= 2.0 ** float(j[16 * t] - j[16 * t + 16])
        _judge(bad, acc, expected, _cols(T, N, t) & (acc != 0), f"channel scale of tile {t} from tile {t + 1} T={T} N={N} K={K}")


@pytest.mark.parametrize("mx,T,N,K", MUT)
def test_the_other_block_map_is_rejected(mx, T, N, K):
    """The activation scales laid out by natural blocks where ``mx_block_quant``'s map belongs, and the
    reverse: every code is 256, so x becomes sign 2^-(a'(k) + r) with the other map's a'.  Every k-block is
    wrong at once, so the mistaken sum need not be a bf16 value: where its rounding lands on the expected value
    (one element in 266240) the mistake is invisible, and counted."""
    x, w, acc, blk, expected = _setup(mx, T, N, K)
    other = rp.k_exp("w4mx" if mx else "mx", K)
    xb = torch.sign(x) * torch.exp2(-(other[None, :] + (torch.arange(T) % 3)[:, None]).double())
    assert bool((xb != x).any())
    _judge(xb @ w.w.t(), acc, expected, T * N, f"the other block map T={T} N={N} K={K} mx={mx}", exact=False)


@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("mx,T,N,K", MUT)
def test_a_dropped_or_doubled_k_slice_is_rejected(mx, T, N, K, twice):
    x, w, acc, blk, expected = _setup(mx, T, N, K)
    for t, s in ((0, 0), (N // 16 - 1, K // 32 - 1), (N // 32, K // 64)):
        cols = slice(16 * t, 16 * t + 16)
        bad = acc.clone()
        bad[:, cols] += (1 if twice else -1) * _part(x, w, torch.arange(K) // 32 == s, cols)
        _judge(bad, acc, expected, _cols(T, N, t), f"slice {s} of tile {t} {'twice' if twice else 'dropped'} T={T} N={N} K={K} mx={mx}")


MOE_MUT = [("tiled", "edge", 258, 256, 256, 4), ("tiledmx", "edge", 258, 384, 1152, 4)]


def _slots(c):
    """fp64 [T, 2, H]: slot j of token t = its j-th valid pair's weighted down row, ascending expert."""
    slots = torch.zeros(c.T, 2, c.H, dtype=torch.float64)
    seen = torch.zeros(c.T, dtype=torch.long)
    for p in range(c.P):
        t = int(c.tok[p])
        slots[t, seen[t]] = float(c.wsel[p]) * c.dn_acc[p]
        seen[t] += 1
    assert bool((seen == 2).all())
    return slots


@pytest.mark.parametrize("spec", MOE_MUT, ids=[s[0] for s in MOE_MUT])
def test_a_slot_added_twice_or_skipped_in_the_combine_is_rejected(spec):
    c = rp.moe_case(*spec)
    slots = _slots(c)
    y = slots.sum(1)
    assert torch.equal(y.to(BF), c.exp_y)
    for j in (0, 1):
        _judge(y + slots[:, j], y, c.exp_y, slots[:, j] != 0, f"{c.id}: slot {j} added twice", exact=False)
        _judge(y - slots[:, j], y, c.exp_y, slots[:, j] != 0, f"{c.id}: slot {j} skipped", exact=False)


@pytest.mark.parametrize("spec", MOE_MUT, ids=[s[0] for s in MOE_MUT])
def test_rows_of_the_next_128_row_slot_of_the_same_expert_are_rejected(spec):
    """Expert 3 owns pairs 258 .. 515: its first row block computed from the rows of its second."""
    c = rp.moe_case(*spec)
    y = _slots(c).sum(1)
    lo = int(c.off[3])
    bad, dep = y.clone(), torch.zeros(c.T, c.H, dtype=torch.bool)
    for p in range(lo, lo + 128):
        t = int(c.tok[p])
        bad[t] += float(c.wsel[p]) * (c.dn_acc[p + 128] - c.dn_acc[p])
        dep[t] = True
    _judge(bad, y, c.exp_y, dep, f"{c.id}: rows of the next slot", exact=False)


@pytest.mark.parametrize("d", [1, -1])
@pytest.mark.parametrize("spec", MOE_MUT, ids=[s[0] for s in MOE_MUT])
def test_a_pairs_row_taken_from_the_neighbouring_pair_is_rejected(spec, d):
    """Gate/up gathers x[tok[p]]: with tok[p + 1] or tok[p - 1] of the same expert the row's sums are another
    token's.  Under the one-ulp SwiGLU comparator the count is stated: an element escapes where both up sums
    are 0, or where the two products happen to agree within an ulp."""
    c = rp.moe_case(*spec)
    o = c.off.tolist()
    for e in (0, 1, 3):
        ps = [p for p in (o[e] + 1, (o[e] + o[e + 1]) // 2, o[e + 1] - 2)]
        for p in ps:
            assert o[e] <= p + d < o[e + 1]
            g, u = rp.split_gate_up(c.gu_acc[p + d:p + d + 1])
            rej = rp.rejected((rp.gp.silu64(g) * u).to(BF), c.exp_act[p:p + 1], c.u_zero[p:p + 1])
            print(f"{c.id}: pair {p} from pair {p + d}: {int(rej.sum())} of {c.F} elements rejected")
            assert int(rej.sum()) >= 0.75 * c.F

