"""Exact probes for the GEMMs above 64 rows (plain module, CPU only): ``tests/gemm_probe.py``'s +-1 probe with
two exponent patterns on top, so that every scale byte a kernel reads matters and the result stays exact.

Families.  Dense: "w8" ``linear_w8_rows``, "w4" ``linear_w4_rows``, "mx" ``linear_mx_rows``, "w4mx"
``linear_w4mx_rows``.  MoE (gate/up + down): "rows" ``moe_*_w8_rows``, "tiled" ``moe_*_w8_tiled`` with
``moe_combine_tiled``, "tiledmx" ``moe_*_mx_tiled`` with ``moe_quant_mx_tiled``.

Blocks.  ``block(fam, K)[k]`` is the activation-quantization block of k: natural 32-blocks ``k // 32`` (the
blocks MXFP4 weights have; for the bf16-activation families only a k pattern), or ``mx_block_quant``'s map
``4 (k // 128) + 2 sh + qh`` with k = 128 kb + 32 s + 8 q + j, sh = s >> 1, qh = q >> 1 ("mx", "tiledmx").

Values, with a(k) = block(k) % 3, r(t) = t % 3 (t: the row; the pair index p for the MoE down GEMM) and
j = ``gemm_probe.channel_exp``:

* x[t, k] = +-2^-(a(k) + r(t)): as MX e4m3 the code +-256 and the scale byte 127 - 8 - a - r, whichever of the
  two block maps quantizes it (the builder asserts both quantizers return x unchanged);
* w[n, k] = +-2^-(j(n) + 2 - a(k)): e4m3 codes +-2^(a - 2) with channel scale 2^-j, or ``pack_weight_w4`` of the
  bf16 matrix (one e8m0 scale per natural block);
* signs: ``gemm_probe``'s, seeded the same way.

Every product is +-2^-(j + 2 + r), so the correct output is S 2^-(j + 2 + r) with S ``gemm_probe``'s even
integer, |S| <= 504 asserted on EVERY element: the bits do not depend on the summation order or on where a
correct kernel rounds.  An activation scale from another k-block or another row, a weight block scale from
another k-block or column, a channel scale from the next tile each put a factor 2 or 4 on part of S and
change the bits, except where the 32 signs involved cancel (probability 0.14; ``test_rows_probe.py`` counts).

Comparators.  Plain epilogue and MoE down (one bf16 rounding): ``torch.equal`` with bf16(fp64), finite.
SwiGLU: ``gemm_probe``'s derived one-ulp bound (g and u are still bf16 values, so its derivation holds
unchanged).  MoE down: routing weights from {0.25, 0.5, 0.75}; w_a S_a 2^-(ja + 2 + ra) + w_b S_b 2^-(jb + 2 +
rb) needs at most 9 + 2 + 4 bits, so the fp32 combine is exact in any order (asserted on the fp64 sum).

Unrouted experts carry NaN codes and NaN scales, the x rows of tokens without a valid expert id are NaN, and
so are the down input's rows past the last valid pair: an exact, finite result says they were never read.
"""
import functools
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from src import ops
from tests.gemm_probe import (BF, SUM_BOUND, ULP, _exact, _gen, _signs, channel_exp, check_sums,  # noqa: F401
                              compare, finish, rejected, routing, split_gate_up)
from tests import gemm_probe as gp
from tests.test_moe_tiled import edge_routing

DENSE = ("w8", "w4", "mx", "w4mx")
MOE = ("rows", "tiled", "tiledmx")
MX_MAP = ("mx", "tiledmx")
W4 = ("w4", "w4mx")
TS = (65, 129, 257, 300)
MOE_TS = (65, 130, 258)
MOE_SHAPES = ((256, 256, 4), (384, 1152, 4), (256, 256, 32))
CODE_256 = 0x78            # e4m3 magnitude bits of 256
NAN8 = 0x7F                # e4m3 NaN


def block(fam: str, K: int) -> torch.Tensor:
    """int64 [K]: the activation-quantization block of every k under the family's map."""
    k = torch.arange(K)
    if fam in MX_MAP:
        s, q = (k % 128) // 32, (k % 32) // 8
        return 4 * (k // 128) + 2 * (s >> 1) + (q >> 1)
    return k // 32


def k_exp(fam: str, K: int) -> torch.Tensor:
    """a(k) = block(k) % 3."""
    return block(fam, K) % 3


def plan(MB: int, wide: bool, N: int, epi: int, cus: int) -> Tuple[int, int, int, int]:
    """(NB, nbig, NBB, NBS): csrc/gemm_rows_plan.h ``w8r_plan_blocks``' column split for MB row blocks."""
    step = 2 if epi == 1 else 1
    units = N // 16 // step
    cap = (16 if wide else 4) // step
    need = (units + cap - 1) // cap
    want = max(cus // MB, need)
    NB = min(units, want)
    if NB > 8 and NB % 8:
        up, down = (NB + 7) // 8 * 8, NB // 8 * 8
        NB = up if up <= units else down if down >= need else NB
    base, rem = divmod(units, NB)
    return NB, rem or NB, (base + (1 if rem else 0)) * step, base * step


def dense_plan(T: int, N: int, epi: int, cus: int):
    """``w8r_plan``: ceil(T / 128) row blocks, the wide geometry above 128 rows."""
    return plan((T + 127) // 128, T > 128, N, epi, cus)


def uneven_n(T: int, N: int, epi: int, cus: int) -> int:
    """The first weight-row count from N upwards whose column split has groups of two widths (NBB != NBS)."""
    step = 32 if epi == 1 else 16
    while True:
        _, _, nbb, nbs = dense_plan(T, N, epi, cus)
        if nbb != nbs:
            return N
        N += step


# ------------------------------------------------------------------------------------ weights
class Weights(gp.Weights):
    """``gemm_probe.Weights`` with the k pattern: w = +-2^-(j + 2 - a(k)).  The base class' ``sign`` is what its
    fp8 packer turns into e4m3 codes, so it holds the code values +-2^(a - 2) here (``signs``: the +-1)."""

    def __init__(self, fam: str, N: int, K: int, swiglu: bool = False, seed: int = 0):
        super().__init__(N, K, swiglu, seed)
        self.a = k_exp(fam, K)
        self.signs = self.sign
        self.sign = self.signs * torch.exp2(self.a.double() - 2)[None, :]
        self.w = self.sign * torch.exp2(-self.exp.double())[:, None]


@functools.lru_cache(maxsize=None)
def weights(mx_map: bool, N: int, K: int, swiglu: bool = False, seed: int = 0) -> Weights:
    return Weights("mx" if mx_map else "w8", N, K, swiglu, seed)


def carrier(fam: str, w: Weights):
    """The family's weight operands: (w8, channel scales) or (w4, s4); each asserted exact by the base class."""
    return w.w4 if fam in W4 else w.w8


def probe_rows(fam: str, signs: torch.Tensor, rexp: torch.Tensor) -> torch.Tensor:
    """fp64 [R, K] = signs 2^-(a(k) + rexp[row]); asserted to be bf16 values that BOTH block quantizers return
    unchanged."""
    x = signs * torch.exp2(-(k_exp(fam, signs.shape[1])[None, :] + rexp[:, None]).double())
    _exact(x, BF, "probe rows")
    assert torch.equal(ops.mx_block_quant(x.float()).double(), x), "mx_block_quant must return the rows unchanged"
    assert torch.equal(ops.mxn_block_quant(x.float()).double(), x), "mxn_block_quant must return the rows unchanged"
    return x


def row_sums_ok(acc: torch.Tensor, rexp: torch.Tensor, exp: torch.Tensor, what: str) -> None:
    """``check_sums`` on S = acc 2^(j + 2 + r)."""
    check_sums(acc * torch.exp2(2.0 + rexp.double())[:, None], exp, what)


# ------------------------------------------------------------------------------------ dense cases
@dataclass
class Case:
    fam: str
    T: int
    N: int                      # weight rows (2 F for SwiGLU)
    K: int
    epi: int
    x: torch.Tensor             # bf16 [T, K]
    expected: torch.Tensor      # bf16 [T, ncols]
    u_zero: Optional[torch.Tensor]

    @property
    def ncols(self) -> int:
        return self.N // 2 if self.epi == 1 else self.N

    @property
    def w(self) -> Weights:
        return weights(self.fam in MX_MAP, self.N, self.K, self.epi == 1)

    @property
    def id(self) -> str:
        return f"{self.fam}-T{self.T}-N{self.N}-K{self.K}-e{self.epi}"


@functools.lru_cache(maxsize=8)
def dense_product(mx_map: bool, T: int, N: int, K: int, swiglu: bool):
    """(x fp64 [T, K], acc fp64 [T, N]) of a block map, the sum bound asserted."""
    w = weights(mx_map, N, K, swiglu)
    rexp = torch.arange(T) % 3
    x = probe_rows("mx" if mx_map else "w8", _signs((T, K), _gen(2, T, N, K)), rexp)
    acc = x @ w.w.t()
    row_sums_ok(acc, rexp, w.exp, f"T={T} N={N} K={K}")
    return x, acc


def case(fam: str, T: int, N: int, K: int, epi: int) -> Case:
    x, acc = dense_product(fam in MX_MAP, T, N, K, epi == 1)
    expected, u_zero, _ = finish(acc, epi, None, f"{fam} T={T} N={N} K={K} epilogue {epi}")
    return Case(fam, T, N, K, epi, _exact(x, BF, "rows"), expected, u_zero)


@dataclass(frozen=True)
class Spec:
    fam: str
    T: int
    N: int
    K: int
    epi: int


def shape_set(cus: int) -> List[Spec]:
    """Every dense case for a device of ``cus`` compute units: the four row counts that reach each branch of
    ``w8r_plan`` x one, three (odd) and nine k-groups x a one-tile, an odd and a wide N, and the uneven column
    splits of both geometries (a wide one at 2049 rows, a narrow one at 65)."""
    out = []
    for fam in DENSE:
        for epi, Ns in ((0, (16, 560, 2048)), (1, (32, 2048, 4608))):
            out += [Spec(fam, T, N, K, epi) for N in Ns for K in (128, 384, 1152) for T in TS]
        out += [Spec(fam, 2049, uneven_n(2049, 4000, 0, cus), 128, 0), Spec(fam, 2049, uneven_n(2049, 8000, 1, cus), 128, 1),
                Spec(fam, 65, uneven_n(65, 16000, 0, cus), 128, 0)]
    return out


# ------------------------------------------------------------------------------------ MoE cases
def group(idx: torch.Tensor, w: torch.Tensor, E: int):
    """``ops.moe_group``'s result in torch (CPU): the VALID pairs in (expert, token) order - ids outside [0, E)
    are dropped, off[E] counts what is left; the tails of tok / wsel are 0."""
    T, k = idx.shape
    flat = idx.reshape(-1)
    keep = torch.nonzero((flat >= 0) & (flat < E)).squeeze(1)
    order = keep[torch.argsort(flat[keep], stable=True)]
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.bincount(flat[keep], minlength=E), 0)
    tok, wsel = torch.zeros(T * k, dtype=torch.int32), torch.zeros(T * k)
    tok[:order.numel()], wsel[:order.numel()] = (order // k).int(), w.reshape(-1)[order]
    return off, tok, wsel


def probe_routing(kind: str, T: int, E: int):
    """(idx int64 [T, 2], w fp32 [T, 2]), weights from {0.25, 0.5, 0.75} that pair to 1.  "gen":
    ``gemm_probe.routing`` over all experts (E = 32: experts 0 and 31 only); "edge": ``edge_routing``'s ids
    (T = 258: offsets 0, 128, 257, 258, 516); "invalid": the edge ids with ids out of range - token 5 (-1, 3),
    token 130 (1, E), token 200 (-1, E) without a valid pair, the last token (E + 7, 3)."""
    if kind == "gen":
        wd = routing(T, E, (0, E - 1) if E == 32 else tuple(range(E)), seed=T)
        idx = torch.nonzero(wd > 0)[:, 1].view(T, 2)
        return idx, wd.gather(1, idx).float()
    idx = edge_routing(T)[0].clone()
    if kind == "invalid":
        idx[5, 0], idx[T // 2 + 1, 1], idx[T - 58] = -1, E, torch.tensor([-1, E])
        idx[T - 1, 0] = E + 7
    wa = 0.25 * torch.randint(1, 4, (T,), generator=_gen(7, T, E)).float()
    return idx, torch.stack([wa, 1.0 - wa], 1)


@dataclass
class MoeCase:
    fam: str
    kind: str
    T: int
    H: int
    F: int
    E: int
    idx: torch.Tensor           # int64 [T, 2]
    w: torch.Tensor             # fp32 [T, 2]
    off: torch.Tensor           # int32 [E + 1]  (``group``)
    tok: torch.Tensor           # int32 [2 T]
    wsel: torch.Tensor          # fp32 [2 T]
    x: torch.Tensor             # bf16 [T, H], NaN rows for tokens without a valid pair
    act_in: torch.Tensor        # bf16 [2 T, F], NaN rows past the last valid pair
    gu: Tuple[torch.Tensor, torch.Tensor]   # (uint8 [E, 2F/16, H/32, 64, 8], fp32 [E, 2F]); NaN where unrouted
    dn: Tuple[torch.Tensor, torch.Tensor]   # (uint8 [E, H/16, F/32, 64, 8], fp32 [E, H])
    exp_act: torch.Tensor       # bf16 [2 T, F] (rows past off[E]: 0, not compared)
    u_zero: torch.Tensor        # bool [2 T, F]
    exp_y: torch.Tensor         # bf16 [T, H]
    gu_acc: torch.Tensor        # fp64 [2 T, 2 F]: the gate / up sums of every valid pair
    dn_acc: torch.Tensor        # fp64 [2 T, H]: the down product of every valid pair (unweighted)

    @property
    def P(self) -> int:
        return int(self.off[-1])

    @property
    def id(self) -> str:
        return f"{self.fam}-{self.kind}-T{self.T}-H{self.H}-F{self.F}-E{self.E}"


def _stack(ws, routed):
    w8 = torch.stack([w.w8[0] for w in ws])
    sc = torch.stack([w.w8[1] for w in ws])
    for e in range(len(ws)):
        if e not in routed:
            w8[e], sc[e] = NAN8, float("nan")
    return w8, sc


@functools.lru_cache(maxsize=None)
def moe_case(fam: str, kind: str, T: int, H: int, F: int, E: int) -> MoeCase:
    mx = fam in MX_MAP
    idx, w = probe_routing(kind, T, E)
    off, tok, wsel = group(idx, w, E)
    o, tl, P = off.tolist(), tok.long(), int(off[-1])
    routed = [e for e in range(E) if o[e + 1] > o[e]]
    gw = [weights(mx, 2 * F, H, True, seed=100 + e) for e in range(E)]
    dw = [weights(mx, H, F, False, seed=200 + e) for e in range(E)]
    rexp_x, rexp_p = torch.arange(T) % 3, torch.arange(2 * T) % 3
    x = probe_rows(fam, _signs((T, H), _gen(6, T, H, F)), rexp_x)
    a_in = probe_rows(fam, _signs((2 * T, F), _gen(5, T, H, F)), rexp_p)
    exp_act = torch.zeros(2 * T, F, dtype=BF)
    u_zero = torch.zeros(2 * T, F, dtype=torch.bool)
    gu_acc = torch.zeros(2 * T, 2 * F, dtype=torch.float64)
    dn_acc = torch.zeros(2 * T, H, dtype=torch.float64)
    tot = torch.zeros(T, H, dtype=torch.float64)
    for e in routed:
        sl = slice(o[e], o[e + 1])
        gu_acc[sl] = x[tl[sl]] @ gw[e].w.t()
        row_sums_ok(gu_acc[sl], rexp_x[tl[sl]], gw[e].exp, f"moe gate/up expert {e}")
        exp_act[sl], u_zero[sl], _ = finish(gu_acc[sl], 1, None, f"moe gate/up expert {e}")
        dn_acc[sl] = a_in[sl] @ dw[e].w.t()
        row_sums_ok(dn_acc[sl], rexp_p[sl], dw[e].exp, f"moe down expert {e}")
        tot.index_add_(0, tl[sl], wsel[sl, None].double() * dn_acc[sl])
    assert torch.equal(tot.float().double(), tot), "the combined sum must be exact in fp32"
    xb, ab = _exact(x, BF, "rows"), _exact(a_in, BF, "down input")
    valid = ((idx >= 0) & (idx < E)).any(1)
    xb[~valid] = float("nan")
    ab[P:] = float("nan")
    return MoeCase(fam, kind, T, H, F, E, idx, w, off, tok, wsel, xb, ab, _stack(gw, routed), _stack(dw, routed),
                   exp_act, u_zero, tot.to(BF), gu_acc, dn_acc)


def moe_set() -> List[Tuple[str, str, int, int, int, int]]:
    """(fam, kind, T, H, F, E): every shape under general routing, the 128-row block edges on the E = 4
    shapes, ids out of range on the tiled forms (their slot rule counts VALID ids)."""
    out = []
    for fam in MOE:
        for H, F, E in MOE_SHAPES:
            out += [(fam, "gen", T, H, F, E) for T in MOE_TS]
            if E == 4:
                out += [(fam, "edge", T, H, F, E) for T in MOE_TS]
        if fam != "rows":
            out += [(fam, "invalid", 258, H, F, 4) for H, F in ((256, 256), (384, 1152))]
    return out


GATE_UP = {"rows": "moe_gate_up_w8_rows", "tiled": "moe_gate_up_w8_tiled", "tiledmx": "moe_gate_up_mx_tiled"}
DOWN = {"rows": "moe_down_w8_rows", "tiled": "moe_down_w8_tiled", "tiledmx": "moe_down_mx_tiled"}
LINEAR = {"w8": "linear_w8_rows", "w4": "linear_w4_rows", "mx": "linear_mx_rows", "w4mx": "linear_w4mx_rows"}
OK = {"w8": "w8_rows_ok", "w4": "w4_rows_ok", "mx": "mx_rows_ok", "w4mx": "w4mx_rows_ok"}


def run_dense(c: Case, x: torch.Tensor, wops, out=None) -> torch.Tensor:
    return getattr(ops, LINEAR[c.fam])(x, *wops, out=out, epilogue=c.epi)


def run_gate_up(c: MoeCase, x, gu, off, tok, out=None) -> torch.Tensor:
    return getattr(ops, GATE_UP[c.fam])(x, gu[0], gu[1], off, tok, out=out)


def run_down(c: MoeCase, act, dn, off, tok, wsel, idx, out=None) -> torch.Tensor:
    if c.fam == "rows":
        return ops.moe_down_w8_rows(act, dn[0], dn[1], off, tok, wsel, c.T, out=out)
    return getattr(ops, DOWN[c.fam])(act, dn[0], dn[1], off, tok, wsel, idx, c.T, out=out)


def check_moe(c: MoeCase, act: torch.Tensor, y: torch.Tensor) -> None:
    """Both comparators: gate/up on the valid pairs (one ulp), down + combine bit for bit."""
    P = c.P
    compare(act[:P], c.exp_act[:P].to(act.device), c.u_zero[:P].to(act.device), f"{c.id} gate/up")
    compare(y, c.exp_y.to(y.device), None, f"{c.id} down")


# ------------------------------------------------------------------------------------ quantizer layouts
def scale_bytes(fam: str, rexp: torch.Tensor, K: int) -> torch.Tensor:
    """uint8 [R / 64, K / 128, 64, 4], the ``as`` buffer of ``quant_mx_rows`` / ``quant_mxn_rows`` for probe
    rows (``mx_rows_buffers``): byte i of lane 16 b + r of (g, kb) = 127 - 8 - a(4 kb + b) - rexp[64 g + 16 i +
    r]; rows with rexp < 0 are padding (zero rows): scale 127.  R = len(rexp) must be a multiple of 64."""
    R = rexp.numel()
    a = (torch.arange(K // 32) % 3).view(K // 128, 4)                     # [kb, b]: blocks are numbered by the map
    e = 127 - 8 - a[None, :, :] - rexp.view(R, 1, 1)                      # [row, kb, b]
    e = torch.where(rexp.view(R, 1, 1) < 0, torch.full_like(e, 127), e)
    return e.view(R // 64, 4, 16, K // 128, 4).permute(0, 3, 4, 2, 1).reshape(R // 64, K // 128, 64, 4).to(torch.uint8)


def code_rows(ax: torch.Tensor, K: int) -> torch.Tensor:
    """uint8 [tiles * 16, K]: the e4m3 bytes of ``ax`` [tiles, K / 128, 2, 64, 16] by row (the order along K inside
    a row is the fragment's: every byte of a probe row is the code +-256)."""
    t = ax.reshape(-1, K // 128, 2, 4, 16, 16)                            # [mt, kb, h, q, r, byte]
    return t.permute(0, 4, 1, 2, 3, 5).reshape(-1, K)
