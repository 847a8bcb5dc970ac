"""Exact probes for the GEMMs above 64 rows on the GPU (tests/rows_probe.py: inputs whose every scale byte
matters and whose result every correct kernel reproduces bit for bit, whatever its summation order).

1. every dense case of ``shape_set`` through ``linear_w8_rows`` / ``linear_w4_rows`` / ``linear_mx_rows`` /
   ``linear_w4mx_rows`` and every MoE case of ``moe_set`` through the row-gathered, tiled and tiled-MX op pairs:
   the family's ``*_ok`` predicate first, then two launches bit-identical to each other and to the expected
   bits (SwiGLU: ``gemm_probe``'s derived one-ulp bound; no case needed a recorded deviation);
2. one control per family: a flipped weight sign, an x block with its exponent moved by 1 and (MXFP4) one s4
   byte + 1 are rejected on exactly the column or row they own;
3. unread bytes: every dense launch of 1. reads a strided x with NaN past row T and past column K and writes
   into a sentinel frame; every MoE case holds NaN in the weights and scales of unrouted experts, in the x rows
   of tokens without a valid expert id and in the down rows past the last valid pair, and the tiled forms'
   fp32 workspace is NaN before each call (the combine must not read a slot no pair wrote);
4. the quantizers on probe rows: code magnitude 256 everywhere, ``as`` the layout permutation of
   127 - 8 - a - r, padding rows zero bytes with scale 127;
5. coverage: per family the number of cases, one SwiGLU case and an uneven column split (NBB != NBS by
   ``w8r_plan_blocks``' rule for this device's CU count) in both geometries.
"""
import collections
import copy
import functools

import pytest
import torch

from src import ops
from tests import rows_probe as rp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
NAN = float("nan")
BF = torch.bfloat16
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
SPECS = rp.shape_set(CUS)
MOES = rp.moe_set()
RAN = collections.Counter()


def to_dev(ts):
    return tuple(t.to(DEV) for t in ts)


@functools.lru_cache(maxsize=None)
def dev_weights(fam, N, K, glu):
    return to_dev(rp.carrier(fam, rp.weights(fam in rp.MX_MAP, N, K, glu)))


def framed(T, N):
    buf = torch.full((T + 3, N + 24), SENT, dtype=BF, device=DEV)
    return buf, buf[1:T + 1, 8:8 + N]


def frame_intact(buf, T, N):
    b = buf.clone()
    b[1:T + 1, 8:8 + N] = SENT
    return bool((b == SENT).all())


def strided(x, pad_rows=20, pad_cols=8):
    """x inside a NaN buffer: rows past T and columns past K are NaN, row stride K + 8."""
    T, K = x.shape
    wide = torch.full((T + pad_rows, K + pad_cols), NAN, dtype=BF, device=DEV)
    wide[:T, :K] = x
    return wide[:T, :K]


# ------------------------------------------------------------------------------------ 1. + 3. exact probes
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("fam", rp.DENSE)
def test_exact_probes_dense(fam, epi):
    n = 0
    for s in SPECS:
        if (s.fam, s.epi) != (fam, epi):
            continue
        assert getattr(ops, rp.OK[fam])(s.T, s.N, s.K, epi), f"{s}: not covered"
        c = rp.case(s.fam, s.T, s.N, s.K, s.epi)
        w, x = dev_weights(fam, s.N, s.K, epi == 1), c.x.to(DEV)
        buf, view = framed(s.T, c.ncols)
        assert rp.run_dense(c, strided(x), w, out=view) is view
        y = rp.run_dense(c, x, w)
        rp.compare(y, c.expected.to(DEV), None if c.u_zero is None else c.u_zero.to(DEV), c.id)
        assert torch.equal(view, y), f"{c.id}: two launches differ (or rows past T / columns past K were read)"
        assert frame_intact(buf, s.T, c.ncols), f"{c.id}: a store outside the [T, N'] view"
        n += 1
        RAN[fam] += 1
    print(f"{fam} epilogue {epi}: {n} cases")
    assert n > 0


def moe_dev(c):
    return dict(x=c.x.to(DEV), act_in=c.act_in.to(DEV), gu=to_dev(c.gu), dn=to_dev(c.dn), idx=c.idx.to(DEV), w=c.w.to(DEV))


def moe_grouping(c, d):
    """``ops.moe_group``'s own output, asserted equal to the stable sort of the valid pairs."""
    off, tok, wsel = ops.moe_group(d["idx"], d["w"], c.E)
    P = c.P
    assert torch.equal(off.cpu(), c.off) and torch.equal(tok[:P].cpu(), c.tok[:P]) and torch.equal(wsel[:P].cpu(), c.wsel[:P])
    return off, tok, wsel


def moe_launch(c, d, grp, gu=None, dn=None, x=None):
    off, tok, wsel = grp
    if c.fam != "rows":
        ops._moe_tiled_workspace(2 * c.T * c.H, DEV).fill_(NAN)  # a slot no pair of THIS call writes is never read
    act = torch.full((2 * c.T + 2, c.F), SENT, dtype=BF, device=DEV)
    rp.run_gate_up(c, d["x"] if x is None else x, gu or d["gu"], off, tok, out=act[:2 * c.T])
    buf, view = framed(c.T, c.H)
    rp.run_down(c, d["act_in"], dn or d["dn"], off, tok, wsel, d["idx"], out=view)
    return act, buf, view


@pytest.mark.parametrize("spec", MOES, ids=["-".join(map(str, s)) for s in MOES])
def test_exact_probes_moe(spec):
    fam, kind, T, H, F, E = spec
    ok = ops.moe_rows_ok if fam == "rows" else ops.moe_tiled_ok
    assert ok(T, E, 2, H, F), f"{spec}: not covered"
    c = rp.moe_case(*spec)
    d = moe_dev(c)
    grp = moe_grouping(c, d)
    (act, buf, y), (act2, _, y2) = moe_launch(c, d, grp), moe_launch(c, d, grp)
    P = c.P
    rp.check_moe(c, act, y)
    assert torch.equal(act[:P], act2[:P]) and torch.equal(y, y2), f"{c.id}: two launches differ"
    assert bool((act[P:] == SENT).all()), f"{c.id}: gate/up stored a row past the last valid pair"
    assert frame_intact(buf, T, H), f"{c.id}: a store outside y"
    if kind == "invalid":
        none = ~((c.idx >= 0) & (c.idx < E)).any(1)
        assert int(none.sum()) == 1 and bool((y[none.to(DEV)] == 0).all())
    RAN[fam] += 1


# ------------------------------------------------------------------------------------ 2. controls
def mutated(w, n, k):
    """The probe weight with the sign of element (n, k) flipped, carriers rebuilt."""
    m = copy.copy(w)
    for name in ("bf16", "wp", "w8", "w4"):
        m.__dict__.pop(name, None)
    m.sign, m.w = w.sign.clone(), w.w.clone()
    m.sign[n, k] = -m.sign[n, k]
    m.w[n, k] = -m.w[n, k]
    return m


@pytest.mark.parametrize("fam", rp.DENSE)
def test_one_misread_is_noticed_on_exactly_the_column_or_row_it_owns(fam):
    T, N, K = 129, 560, 384
    assert getattr(ops, rp.OK[fam])(T, N, K, 0)
    c = rp.case(fam, T, N, K, 0)
    x, expected, w = c.x.to(DEV), c.expected.to(DEV), dev_weights(fam, N, K, False)
    assert not bool(rp.rejected(rp.run_dense(c, x, w), expected).any())
    # one weight with the other sign: every row's sum in that column moves by 2 * 2^-(j + 2 + r)
    n0, k0 = 333, 200
    bad = rp.rejected(rp.run_dense(c, x, to_dev(rp.carrier(fam, mutated(c.w, n0, k0)))), expected)
    assert int(bad.sum()) == T and bool(bad[:, n0].all())
    with pytest.raises(AssertionError, match=f"{T} of {T * N} elements rejected"):
        rp.compare(rp.run_dense(c, x, to_dev(rp.carrier(fam, mutated(c.w, n0, k0)))), expected, None, c.id)
    # one x block of one row with its exponent moved by 1 (still an exact MX value: the scale byte - 1)
    t0, b0 = 100, 7
    mask = rp.block(fam, K) == b0
    xm = c.x.clone()
    xm[t0, mask] = (xm[t0, mask].float() * 0.5).to(BF)
    part = c.x[t0, mask].double() @ c.w.w[:, mask].t()
    bad = rp.rejected(rp.run_dense(c, xm.to(DEV), w), expected).cpu()
    own = torch.zeros(T, N, dtype=torch.bool)
    own[t0] = part != 0
    print(f"{fam}: x block {b0} of row {t0} halved: {int(bad.sum())} of {N} elements of the row rejected")
    assert torch.equal(bad, own) and int(bad.sum()) >= 0.75 * N
    if fam in rp.W4:  # one block scale byte + 1: column 16 nt + cc, natural block 4 kb + s doubled
        nt, kb, cc, s = 20, 2, 5, 1
        w4, s4 = c.w.w4
        s4 = s4.clone()
        s4[nt, kb, cc, s] += 1
        mask = rp.block(fam, K) == 4 * kb + s
        part = c.x.double()[:, mask] @ c.w.w[16 * nt + cc, mask]
        bad = rp.rejected(rp.run_dense(c, x, (w4.to(DEV), s4.to(DEV))), expected).cpu()
        own = torch.zeros(T, N, dtype=torch.bool)
        own[:, 16 * nt + cc] = part != 0
        print(f"{fam}: s4[{nt}, {kb}, {cc}, {s}] + 1: {int(bad.sum())} of {T} elements of the column rejected")
        assert torch.equal(bad, own) and int(bad.sum()) >= 0.75 * T


@pytest.mark.parametrize("fam", rp.MOE)
def test_one_misread_is_noticed_on_exactly_the_column_or_row_it_owns_moe(fam):
    c = rp.moe_case(fam, "edge", 258, 256, 256, 4)
    d = moe_dev(c)
    grp = moe_grouping(c, d)
    P, e0, n0, k0 = c.P, 1, 77, 130
    # one down weight of expert 1 with the other sign: column n0 of the tokens routed to expert 1, nothing else
    m = mutated(rp.weights(fam in rp.MX_MAP, c.H, c.F, False, seed=200 + e0), n0, k0)
    dn8 = c.dn[0].clone()
    dn8[e0] = m.w8[0]
    act, _, y = moe_launch(c, d, grp, dn=(dn8.to(DEV), d["dn"][1]))
    assert not bool(rp.rejected(act[:P], c.exp_act[:P].to(DEV), c.u_zero[:P].to(DEV)).any())
    own = torch.zeros(c.T, c.H, dtype=torch.bool)
    own[(c.idx == e0).any(1), n0] = True
    assert torch.equal(rp.rejected(y, c.exp_y.to(DEV)).cpu(), own) and int(own.sum()) == 129
    # one x block of token t0 with its exponent moved by 1: the two pairs of that token, nothing else
    t0, b0 = 200, 3
    mask = rp.block(fam, c.H) == b0
    xm = c.x.clone()
    xm[t0, mask] = (xm[t0, mask].float() * 0.5).to(BF)
    act, _, y = moe_launch(c, d, grp, x=xm.to(DEV))
    bad = rp.rejected(act[:P], c.exp_act[:P].to(DEV), c.u_zero[:P].to(DEV)).cpu()
    pairs = torch.nonzero(c.tok[:P] == t0).squeeze(1)
    print(f"{fam}: x block {b0} of token {t0} halved: {int(bad.sum())} of {2 * c.F} elements of its pairs rejected")
    assert pairs.numel() == 2 and int(bad.sum()) == int(bad[pairs].sum()) and int(bad.sum()) >= 0.5 * 2 * c.F
    assert not bool(rp.rejected(y, c.exp_y.to(DEV)).any())


# ------------------------------------------------------------------------------------ 4. quantizers
@pytest.mark.parametrize("T", [65, 130, 300])
@pytest.mark.parametrize("fam", ["mx", "w4mx"])
def test_quantizers_on_probe_rows(fam, T):
    K = 384
    c = rp.case(fam, T, 16, K, 0)
    quant = ops.quant_mx_rows if fam == "mx" else ops.quant_mxn_rows
    ax, as_ = quant(strided(c.x.to(DEV)))
    rows = rp.code_rows(ax.cpu(), K)
    assert rows.shape[0] == (T + 15) // 16 * 16
    assert bool(((rows[:T] & 0x7F) == rp.CODE_256).all()), "a code whose magnitude is not 256"
    assert bool((rows[T:] == 0).all()), "rows past T must be zero bytes"
    R = (T + 63) // 64 * 64
    rexp = torch.full((R,), -1)
    rexp[:T] = torch.arange(T) % 3
    assert torch.equal(as_.cpu(), rp.scale_bytes(fam, rexp, K)), "as is not the layout permutation of 127 - 8 - a - r"


@pytest.mark.parametrize("kind", ["edge", "invalid"])
def test_slot_order_quantizer_on_probe_rows(kind):
    c = rp.moe_case("tiledmx", kind, 258, 384, 1152, 4)
    d = moe_dev(c)
    off, tok, _ = moe_grouping(c, d)
    o = c.off.tolist()
    for x, t, K, r_of in ((d["x"], tok, c.H, lambda p: int(c.tok[p]) % 3), (d["act_in"], None, c.F, lambda p: p % 3)):
        ax, as_ = ops.moe_quant_mx_tiled(x, off, t)
        rexp = []
        for e in range(c.E):
            for p0 in range(o[e], o[e + 1], 128):
                n = min(128, o[e + 1] - p0)
                rexp += [r_of(p) for p in range(p0, p0 + n)] + [-1] * (128 - n)
        rexp = torch.tensor(rexp)
        live = rexp.numel() // 128
        assert live == sum((o[e + 1] - o[e] + 127) // 128 for e in range(c.E)) and live <= ax.shape[0]
        rows = rp.code_rows(ax[:live].cpu(), K)
        assert bool(((rows[rexp >= 0] & 0x7F) == rp.CODE_256).all()) and bool((rows[rexp < 0] == 0).all())
        assert torch.equal(as_[:live].cpu().reshape(-1), rp.scale_bytes("tiledmx", rexp, K).reshape(-1))
        want = ops._moe_quant_mx_tiled_torch(torch.nan_to_num(x.cpu().float()).to(BF), c.off, None if t is None else c.tok, ax.shape[0])
        assert torch.equal(ax[:live].cpu(), want[0][:live]) and torch.equal(as_[:live].cpu(), want[1][:live])


# ------------------------------------------------------------------------------------ 5. coverage
def test_every_family_has_a_swiglu_case_and_an_uneven_split_in_both_geometries():
    """Runs after the probes (file order); computed from N, T and this device's CU count by ``w8r_plan_blocks``'
    rule (``rows_probe.plan``)."""
    for fam in rp.DENSE:
        mine = [s for s in SPECS if s.fam == fam]
        uneven = collections.Counter(s.T > 128 for s in mine if len(set(rp.dense_plan(s.T, s.N, s.epi, CUS)[2:])) == 2)
        print(f"{fam}: {len(mine)} cases ({RAN[fam]} ran in this session), {sum(s.epi for s in mine)} SwiGLU, uneven splits: "
              f"{uneven[True]} wide, {uneven[False]} narrow")
        assert uneven[True] and uneven[False] and any(s.epi == 1 for s in mine)
    for fam in rp.MOE:
        mine = [s for s in MOES if s[0] == fam]
        n = 0
        for _, _, T, H, F, E in mine:  # the tiled forms: S = 2 T // 128 + E row-block slots, the wide geometry
            n += fam != "rows" and len(set(rp.plan(2 * T // 128 + E, True, 2 * F, 1, CUS)[2:])) == 2
        print(f"{fam}: {len(mine)} cases ({RAN[fam]} ran in this session), each gate/up is SwiGLU; uneven gate/up splits: {n}")
        assert mine and (fam == "rows" or n)
