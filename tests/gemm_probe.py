"""Decode-GEMM probes whose result is exact in every number format (plain module, CPU only).

The decode GEMM tests on ``randn`` inputs compare a sum of thousands of terms with fp32 under a
tolerance of a few bf16 ulps of that sum: they cannot tell WHICH weights and rows a kernel read.
A GEMM of small integers can.

Inputs (``case``):

* ``x`` [M, K]: +-1.
* ``w`` [N, K]: +-1 * 2^-j(n) with the per-output-channel exponent j = (n // 16) % 3, so a value or
  a scale taken from a neighbouring column tile is off by a factor of 2 or 4.  For the SwiGLU
  epilogue (16-row interleaved gate / up tiles) the gate channels carry another 2^-4.
* residual: even integers in [-8, 8].
* signs seeded per (N, K) for the weight and per (M, N, K) for the rows and the residual.

Exactness.  Every product is +-2^-j, a row sum is S * 2^-j with S an even integer, |S| <= K.  fp32
holds S (<= 2^24) exactly, so ANY summation order gives the same fp32 bits: split-K slabs,
stream-K fix-ups, the 4-wave LDS sums, rotated k walks.  The builder asserts on the fp64 reference
that |S| <= 504 for EVERY element (a condition of the seed, never a mask: K <= 1152 gives a
standard deviation of 34 and peaks near 150 over 64 x 4096 outputs), and that the sum, the sum
plus the residual and every intermediate a kernel may round (``round_bf(acc) + residual``) are
bf16 values (8 significant bits: S / 2 + residual * 2^(j-1) stays an integer below 256).  The
result is then independent of where and how often a correct kernel rounds: expected =
bf16(fp64 result), compared with ``torch.equal`` on the M real rows, and the output must be finite.
Any single misread - a 32-wide k-slice dropped or counted twice, one lane's fragment from the
neighbouring slice, a neighbouring tile's scale, a slab summed twice - changes S by an even
integer >= 2 or the exponent, hence the bits, except where the misread terms happen to cancel
(a sum of 32 random signs is 0 with probability 0.14: ``test_gemm_probe.py`` counts what escapes).

Quantized weights carry the SAME values:

* W8A16 (``Weights.w8``): e4m3 codes of +-1 and per-channel scales 2^-j (2^-(j+4) for gate
  channels).  sum(code * x) = S is exact in fp32 and S * scale only moves the exponent, so the
  scaled accumulator is exactly the bf16 value above (no fp32 rounding at all, a fortiori within
  one fp32 ulp of it).  The builder asserts ``ops.unpack_weight_w8(w8, scale, float32) == w``.
* W4A16 (``Weights.w4``): ``ops.pack_weight_w4`` of the same matrix: a block's amax 2^-j gives the
  e8m0 scale 2^(-j-2) and the e2m1 code of 4.  The builder asserts the same exact round trip
  through ``ops.unpack_weight_w4``.

Epilogues.  0 (plain) and 2 (+ residual): bit equality.  3 (fused-norm producer): the updated
residual is bit-equal, ``ap_out == pack_act(residual)``, ``ss_out`` sums to ``ref.fx_sumsq`` of it
and ``ss_zero`` is cleared (``check_epi3``).  1 (SwiGLU): g = S_g * 2^-(j+4) lies within +-32 in
steps of 1/8, u = S_u * 2^-j; expected = bf16(silu_fp64(g) * u) and the comparator allows ONE bf16
ulp of the expected value, |got - expected| <= 2^-7 |expected|, and an exact 0 where u = 0.  The
bound is derived, not measured: g and u are bf16 values, so the kernel's only inexact steps are
exp (error far below 2^-8 relative), the rounding of silu(g) to bf16 (2^-9 relative, the
reference model's rounding point) and the final rounding (2^-9): the result is within 2^-8 (1 +
2^-9) of the true product, the expected value within 2^-9, together < 2^-7 of it.  The smallest
mistake moves g by 1/8 or u by 2 * 2^-j.

Grouped MoE GEMMs (``moe_case``): E experts' weights and activations of the same kind, general
top-2 routing with weights from {0.25, 0.5, 0.75} that pair to 1.  w_a S_a 2^-ja + w_b S_b 2^-jb
needs at most 14 bits, so the fp32 combine is exact in any order and the down kernel's ONE bf16
rounding gives bf16(fp64) bit for bit (the builder asserts the fp64 result is an fp32 value).
Unrouted experts hold NaN codes, NaN scales and NaN activation slabs.
"""
import contextlib
import dataclasses
import functools
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from src import ops
from src.ops import reference as ref

BF = torch.bfloat16
SUM_BOUND = 504
ULP = 2.0 ** -7           # one bf16 ulp, relative to the expected value (SwiGLU comparator)
GATE_SHIFT = 4            # gate channels: another 2^-4
MS = (1, 13, 16, 17, 50, 64)
WIDE_MS = (65, 100, 128, 129, 200, 256)
BF16_BASES = ("pk", "sk", "lds22", "lds24", "lds42", "rw", "rwk", "rwki", "rwr")
BF16_FORMS = BF16_BASES + tuple(b + "+r" for b in BF16_BASES)
W8_BASES = ("rw", "rwk", "rwki")
W8_FORMS = W8_BASES + tuple(b + "+r" for b in W8_BASES)
# epilogues a form takes: 0 plain, 1 SwiGLU, 2 + residual, 3 fused-norm producer
FORM_EPIS = {"pk": (0, 1, 2, 3), "sk": (0, 1, 2, 3), "lds22": (0, 1, 2, 3), "lds24": (0, 1, 2, 3),
             "lds42": (0, 1, 2, 3), "rw": (0, 1, 2, 3), "rwk": (0, 2, 3), "rwki": (0, 2, 3), "rwr": (0, 2, 3)}
W8_FORM_EPIS = {"rw": (0, 1, 3), "rwk": (0, 3), "rwki": (0, 3)}
W4_EPIS = (0, 1, 3)
WIDE_EPIS = (0, 1)


def _gen(*key) -> torch.Generator:
    h = 0x5DEECE66D
    for v in key:
        h = (h * 1000003 + int(v) + 0x9E3779B9) % (2 ** 62)
    return torch.Generator().manual_seed(h)


def _signs(shape, gen) -> torch.Tensor:
    return torch.randint(0, 2, shape, generator=gen, dtype=torch.int8).double() * 2 - 1


def _exact(x: torch.Tensor, dtype, what: str) -> torch.Tensor:
    y = x.to(dtype)
    assert torch.equal(y.double(), x), f"{what} must be exact in {dtype}"
    return y


def channel_exp(N: int, swiglu: bool = False) -> torch.Tensor:
    """int64 [N]: the exponent j of output channel n's weights +-2^-j: (n // 16) % 3, + 4 on the gate
    tiles (even 16-row tiles) of an interleaved gate / up weight."""
    t = torch.arange(N) // 16
    j = t % 3
    if swiglu:
        j = j + GATE_SHIFT * (t % 2 == 0)
    return j


# ------------------------------------------------------------------------------------ weights
class Weights:
    """One probe weight [N, K] (fp64, exact) and its carriers, each built once and asserted exact."""

    def __init__(self, N: int, K: int, swiglu: bool = False, seed: int = 0):
        assert N % (32 if swiglu else 16) == 0 and K % 32 == 0
        self.N, self.K, self.swiglu = N, K, swiglu
        self.exp = channel_exp(N, swiglu)
        self.sign = _signs((N, K), _gen(1, N, K, int(swiglu), seed))
        self.w = self.sign * torch.exp2(-self.exp.double())[:, None]

    @functools.cached_property
    def bf16(self) -> torch.Tensor:
        """Row-major bf16 [N, K]."""
        return _exact(self.w, BF, "probe weights")

    @functools.cached_property
    def wp(self) -> torch.Tensor:
        """``ops.pack_weight`` of the bf16 weight (the fragment layout of the decode GEMMs)."""
        wp = ops.pack_weight(self.bf16)
        assert torch.equal(ops.unpack_weight(wp), self.bf16)
        return wp

    @functools.cached_property
    def w8(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(codes uint8 [N/16, K/32, 64, 8], scales fp32 [N]): e4m3 codes of +-1, scales 2^-j."""
        N, K = self.N, self.K
        assert K % 64 == 0
        q = self.sign.float().to(torch.float8_e4m3fn).view(torch.uint8)
        wq = q.view(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 64, 64, 16)
        w8 = ops.w8_from_fp8(wq.contiguous())
        scale = torch.exp2(-self.exp.float()).contiguous()
        assert torch.equal(ops.unpack_weight_w8(w8, scale, torch.float32).double(), self.w), \
            "probe weights must be exact through the fp8 packer"
        return w8, scale

    @functools.cached_property
    def w4(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``ops.pack_weight_w4`` of the same matrix: e2m1 codes of +-4, e8m0 scales 2^(-j-2)."""
        w4, s4 = ops.pack_weight_w4(self.bf16)
        assert torch.equal(ops.unpack_weight_w4(w4, s4, torch.float32).double(), self.w), \
            "probe weights must be exact through the MXFP4 packer"
        return w4, s4


@functools.lru_cache(maxsize=None)
def weights(N: int, K: int, swiglu: bool = False, seed: int = 0) -> Weights:
    return Weights(N, K, swiglu, seed)


# ------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    M: int
    N: int                      # weight rows (2 F for the SwiGLU epilogue)
    K: int
    epi: int
    x: torch.Tensor             # bf16 [M, K], +-1
    res: Optional[torch.Tensor]  # bf16 [M, N] (epilogues 2, 3)
    expected: torch.Tensor      # bf16 [M, ncols]
    u_zero: Optional[torch.Tensor] = None  # bool [M, F] (epilogue 1): the up sum is 0
    ss: Optional[torch.Tensor] = None      # int64 [M] (epilogue 3): ref.fx_sumsq of the new residual

    @property
    def ncols(self) -> int:
        return self.N // 2 if self.epi == 1 else self.N

    @property
    def w(self) -> Weights:
        return weights(self.N, self.K, self.epi == 1)


def rows(M: int, N: int, K: int) -> torch.Tensor:
    """fp64 [M, K] of +-1, seeded per (M, N, K)."""
    return _signs((M, K), _gen(2, M, N, K))


def residual(M: int, N: int, K: int) -> torch.Tensor:
    """fp64 [M, N] of even integers in [-8, 8]."""
    return torch.randint(-4, 5, (M, N), generator=_gen(3, M, N, K)).double() * 2


def check_sums(acc: torch.Tensor, exp: torch.Tensor, what: str = "") -> None:
    """The builder's condition on the fp64 product [M, N]: every integer sum S = acc * 2^j is even
    and |S| <= 504, for EVERY element."""
    S = acc * torch.exp2(exp.double())[None, :]
    assert torch.equal(S, torch.round(S / 2) * 2), f"{what}: sums of +-1 over an even K are even integers"
    worst = float(S.abs().max())
    assert worst <= SUM_BOUND, f"{what}: |sum| = {worst} > {SUM_BOUND}: change the seed, do not mask"


def silu64(g: torch.Tensor) -> torch.Tensor:
    return g * torch.sigmoid(g)


def split_gate_up(y: torch.Tensor):
    """[M, 2F] with 16-column interleaved gate / up tiles -> (g [M, F], u [M, F])."""
    M, F2 = y.shape
    v = y.view(M, F2 // 32, 2, 16)
    return v[:, :, 0].reshape(M, F2 // 2), v[:, :, 1].reshape(M, F2 // 2)


def finish(acc: torch.Tensor, epi: int, res: Optional[torch.Tensor], what: str = ""):
    """(expected bf16, u_zero, ss) of an fp64 product [M, N] under an epilogue; asserts that every
    rounding point of a correct kernel is exact (or, for SwiGLU, that g and u are)."""
    _exact(acc, BF, f"{what}: the sums")
    if epi == 1:
        g, u = split_gate_up(acc)
        assert float(g.abs().max()) <= 32.0
        return (silu64(g) * u).to(BF), u == 0, None
    if epi == 0:
        return acc.to(BF), None, None
    out = _exact(acc + res, BF, f"{what}: sum + residual")
    return out, None, (ref.fx_sumsq(out) if epi == 3 else None)


@functools.lru_cache(maxsize=4)
def _product(M: int, N: int, K: int, swiglu: bool) -> torch.Tensor:
    w = weights(N, K, swiglu)
    acc = rows(M, N, K) @ w.w.t()
    check_sums(acc, w.exp, f"M={M} N={N} K={K}")
    return acc


@functools.lru_cache(maxsize=None)
def case(M: int, N: int, K: int, epi: int) -> Case:
    acc = _product(M, N, K, epi == 1)
    res = residual(M, N, K) if epi >= 2 else None
    expected, u_zero, ss = finish(acc, epi, res, f"M={M} N={N} K={K} epilogue {epi}")
    return Case(M, N, K, epi, _exact(rows(M, N, K), BF, "rows"),
                None if res is None else _exact(res, BF, "residual"), expected, u_zero, ss)


# ------------------------------------------------------------------------------------ comparator
def rejected(out: torch.Tensor, expected: torch.Tensor, u_zero: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bool [M, ncols]: the comparator rejects this element.  Plain: not finite or other bits than the
    expected bf16 value (+0 and -0 are the same value).  SwiGLU (``u_zero`` given): not finite, more
    than one bf16 ulp (2^-7 relative) from the expected value, or not 0 where the up sum is 0."""
    o = out.detach().double().reshape(expected.shape)
    e = expected.to(o.device).double()
    bad = ~torch.isfinite(o)
    if u_zero is None:
        return bad | (o != e)
    return bad | ((o - e).abs() > ULP * e.abs()) | (u_zero.to(o.device) & (o != 0))


def compare(out: torch.Tensor, expected: torch.Tensor, u_zero: Optional[torch.Tensor] = None, what: str = "") -> None:
    """The comparator on the M real rows of a row-major output [M, ncols]."""
    bad = rejected(out, expected, u_zero)
    if bool(bad.any()):
        o = out.detach().double().reshape(expected.shape).cpu()
        idx = torch.nonzero(bad.cpu())
        first = [(int(r), int(n), float(o[r, n]), float(expected[r, n])) for r, n in idx[:6].tolist()]
        cols = sorted({int(n) // 16 for n in idx[:, 1].tolist()})
        raise AssertionError(f"{what}: {len(idx)} of {bad.numel()} elements rejected; rows "
                             f"{sorted({int(r) for r in idx[:, 0].tolist()})[:8]}, column tiles {cols[:8]}"
                             f"{'...' if len(cols) > 8 else ''}; (row, col, got, expected): {first}")


def check_epi3(c: Case, res_out, ap_out, ss_out, ss_zero, what: str = "") -> None:
    """Epilogue 3: the updated residual, its packed copy, the row statistics and the cleared buffer."""
    compare(res_out, c.expected, None, what)
    M, N = c.M, c.N
    assert torch.equal(ap_out.cpu()[: ops.packed_numel(M, N)], ref.pack_act(res_out.cpu())), \
        f"{what}: ap_out is not pack_act(residual)"
    assert torch.equal(ss_out.view(ref.SS_SHARDS, -1).sum(0)[:M].cpu(), c.ss), f"{what}: ss_out"
    assert int(ss_zero.abs().sum()) == 0, f"{what}: ss_zero was not cleared"


# ------------------------------------------------------------------------------------ column split
def rw_width(N: int, epi: int, cus: int) -> Tuple[int, int, int]:
    """(G, ntb, rem) of the balanced ring form's column split: units (tiles, or gate / up tile pairs)
    over G = min(cus, units) workgroups, ``rem`` (or all, when 0) of them ``ntb`` tiles wide."""
    step = 2 if epi == 1 else 1
    units = N // 16 // step
    G = min(units, cus)
    base, rem = divmod(units, G)
    return G, (base + (1 if rem else 0)) * step, rem


def rw_built(N: int, epi: int, cus: int, fp8: bool = False) -> bool:
    """Whether the ring form is built for this width (M <= 128): 1/1, 2/1, 3/2, 4/3, 6/6, 8/7; SwiGLU
    2/2, 4/2, 6/4, 8/6 and, fp8 weights only, 14/14."""
    _, ntb, rem = rw_width(N, epi, cus)
    if epi == 1:
        return (ntb == 2 and not rem) or ntb in (4, 6, 8) or (ntb == 14 and fp8 and not rem)
    return ntb in (1, 2, 3, 4, 8) or (ntb == 6 and not rem)


# ------------------------------------------------------------------------------------ shapes
@dataclass(frozen=True)
class Spec:
    group: str
    wt: str            # "bf16" | "w8" | "w4"
    kern: str          # the forced form; "auto": ops.linear's own choice (65..256 rows)
    M: int
    N: int             # weight rows: 2 F for SwiGLU
    K: int
    epi: int
    packed: bool = False     # SwiGLU output in the packed activation layout
    rowmajor: bool = False   # x handed over row-major (ops.linear packs it, or takes hipBLASLt)

    @property
    def id(self) -> str:
        return (f"{self.group}-{self.wt}-{self.kern}-M{self.M}-N{self.N}-K{self.K}-e{self.epi}"
                f"{'p' if self.packed else ''}{'-rm' if self.rowmajor else ''}")


def _epi_variants(epis, wt: str):
    """(epilogue, packed) pairs: bf16 SwiGLU runs row-major and packed, fp8 / fp4 weights packed only."""
    out = []
    for e in epis:
        if e == 1:
            out += [(1, True)] if wt != "bf16" else [(1, False), (1, True)]
        else:
            out.append((e, False))
    return out


def shape_set(cus: int) -> List[Spec]:
    """Every probe case for a device of ``cus`` compute units (see the module's test files)."""
    C = cus
    out: List[Spec] = []

    def add(group, wt, kerns, Ms, Ns, Ks, epis, rowmajor=False):
        for kern in kerns:
            for N in Ns:
                for K in Ks:
                    for e, packed in _epi_variants(epis, wt):
                        n = 2 * N if e == 1 else N   # SwiGLU: N output columns = 2 N weight rows
                        if e == 3 and n % 32:
                            # the producer's packed copy lives in 32-column groups: an odd tile count has
                            # none (the ops reject it), its edge runs with one tile more
                            n += 16
                        if packed and (n // 2) % 32:
                            n += 32  # the same for a packed SwiGLU output: an even count of gate / up pairs
                        for M in Ms:
                            out.append(Spec(group, wt, kern, M, n, K, e, packed, rowmajor))

    # ring depth and tail: 1, 3, 8 and 9 k-steps per wave
    KT = (128, 384, 1024, 1152)
    add("ktail", "bf16", BF16_FORMS, MS, (2048,), KT, (0, 1, 2, 3))
    add("ktail", "w8", W8_FORMS, MS, (2048,), KT, (0, 1, 3))
    # column split, plain: widths 1/1 (G = 1, 2, C), 2/1 with n_big = 1 and C - 1, 3/2, 4/3, 5 (falls
    # back), 6 with a remainder (falls back), 6/6, 8/7
    NP = tuple(16 * t for t in (1, 2, C, C + 1, 2 * C - 1, 2 * C + 1, 3 * C + 1, 4 * C + 1, 5 * C + 1, 6 * C, 7 * C + 1))
    add("colsplit", "bf16", ("rw", "rw+r"), MS, NP, (128,), (0, 2, 3))
    add("colsplit", "w8", ("rw", "rw+r"), MS, NP, (128,), (0, 3))
    # column split, SwiGLU: pairs 1, C (2/2), C + 1 (4/2), 2C + 1 (6/4), 3C + 1 (8/6), 4C + 1 (falls back);
    # fp8 also 7C (14/14)
    NS = tuple(16 * t for t in (1, C, C + 1, 2 * C + 1, 3 * C + 1, 4 * C + 1))
    add("colsplit", "bf16", ("rw", "rw+r"), MS, NS, (128,), (1,))
    add("colsplit", "w8", ("rw", "rw+r"), MS, NS + (16 * 7 * C,), (128,), (1,))
    # split-K ring: one step per wave (falls back), then K = 256 / 512 (the first K that splits is
    # asserted to be among them by the GPU test) - 512 gives the in-launch combine a width >= 2
    KS = (128, 256, 512)
    add("splitk", "bf16", ("rwk", "rwk+r", "rwki", "rwki+r"), MS, (2048,), KS, (0, 2, 3))
    add("splitk", "w8", ("rwk", "rwk+r", "rwki", "rwki+r"), MS, (2048,), KS, (0, 3))
    # row-split ring: 2 and 4 row tiles
    add("rwr", "bf16", ("rwr", "rwr+r"), (17, 32, 50, 64), (2048,), (128, 1152), (0, 2, 3))
    # stream-K: 32 k-slices (the fewest the form takes) and one chunk more; 2 tiles fall back
    add("sk", "bf16", ("sk", "sk+r"), MS, (32, 2048), (1024, 1280), (0, 1, 2, 3))
    # shared-A: 2 and 6 k-groups of 64 (fewer than, and no multiple of, the 2 / 4 k-splits).  K = 192 is
    # no multiple of the decode GEMMs' 128: ops.linear takes it row-major on the hipBLASLt path
    LF = ("lds22", "lds24", "lds42", "lds22+r", "lds24+r", "lds42+r")
    add("lds", "bf16", LF, MS, (64, 128, 2048), (128, 384), (0, 1, 2, 3))
    add("lds", "bf16", ("lds22", "lds24", "lds42"), MS, (64, 128, 2048), (192,), (0, 2), rowmajor=True)
    # one-group-per-workgroup: one tile, C + 1 tiles
    add("pk", "bf16", ("pk", "pk+r"), MS, (16, 16 * (C + 1)), (128,), (0, 1, 2, 3))
    # 65..256 rows through ops.linear's own choice (rwk, rw or t2d)
    add("wide", "bf16", ("auto",), WIDE_MS, (2048, 16 * (C + 1)), (128, 1024), (0,))
    # (the tiled form's plain epilogue is only picked where its split-K variant applies too: N % 1024 == 0
    # and K >= 256 - 192 tiles split 2 / 1 over its column groups)
    add("wide", "bf16", ("auto",), WIDE_MS, (3072,), (1024,), (0,))
    out.extend(Spec("wide", "bf16", "auto", M, 2 * N, K, 1, True)
               for N in (2048, 16 * (C + 2)) for K in (128, 1024) for M in WIDE_MS)  # (packed: even pairs)
    # W4A16
    add("w4", "w4", ("rw",), MS, (16, 2048, 16 * (C + 1)), (128, 384, 1152), W4_EPIS)
    return list(dict.fromkeys(out))


# ------------------------------------------------------------------------------------ grouped MoE
@dataclass
class MoeCase:
    kind: str                   # "down" | "gate_up"
    M: int
    E: int
    N: int                      # weight rows of each expert: H (down) or 2 F (gate / up)
    K: int
    x: torch.Tensor             # bf16: down [E, M, K] (NaN slabs where unrouted), gate_up [M, K]
    w8: torch.Tensor            # uint8 [E, N/16, K/32, 64, 8] (NaN codes where unrouted)
    scale: torch.Tensor         # fp32 [E, N] (NaN where unrouted)
    wd: torch.Tensor            # fp32 [M, E] dense routing matrix
    cnt: torch.Tensor           # int32 [E]
    expected: torch.Tensor      # bf16: down [M, N]; gate_up [E, M, N / 2] (zeros where unrouted)
    u_zero: Optional[torch.Tensor] = None  # gate_up: bool [E, M, N / 2]


def routing(M: int, E: int, routed: Tuple[int, ...], seed: int = 0) -> torch.Tensor:
    """fp64 [M, E]: every row routes to two distinct experts of ``routed`` with weights from {0.25, 0.5,
    0.75} that pair to 1 (one routed expert: weight 1); every routed expert gets at least one row
    when M allows."""
    wd = torch.zeros(M, E, dtype=torch.float64)
    gen = _gen(4, M, E, len(routed), seed)
    if len(routed) == 1:
        wd[:, routed[0]] = 1.0
        return wd
    for r in range(M):
        a = routed[(2 * r) % len(routed)]
        b = routed[(2 * r + 1 + int(torch.randint(0, len(routed) - 1, (1,), generator=gen))) % len(routed)]
        wa = 0.25 * (1 + int(torch.randint(0, 3, (1,), generator=gen)))
        wd[r, a], wd[r, b] = wa, 1.0 - wa
    return wd


def _nan_unrouted(w8, scale, cnt):
    for e, c in enumerate(cnt.tolist()):
        if c == 0:
            w8[e] = 0x7F    # e4m3 NaN
            scale[e] = float("nan")


@functools.lru_cache(maxsize=None)
def moe_case(kind: str, M: int, H: int, F: int, E: int, routed: Optional[Tuple[int, ...]] = None) -> MoeCase:
    """``kind`` "down": y [M, H] = sum_e wd[:, e] (act[e] @ down[e]^T); "gate_up": act[e] = SwiGLU(x @
    gate_up[e]^T).  ``routed``: the experts that get tokens (default all; () = nothing routed)."""
    routed = tuple(range(E)) if routed is None else tuple(routed)
    N, K = (H, F) if kind == "down" else (2 * F, H)
    ws = [weights(N, K, kind == "gate_up", seed=100 + e) for e in range(E)]
    w8 = torch.stack([w.w8[0] for w in ws])
    scale = torch.stack([w.w8[1] for w in ws])
    wd = routing(M, E, routed, seed=N + K) if routed else torch.zeros(M, E, dtype=torch.float64)
    cnt = (wd > 0).sum(0).to(torch.int32)
    _nan_unrouted(w8, scale, cnt)
    routed = tuple(e for e in range(E) if int(cnt[e]) > 0)  # (one row: two experts, whatever was offered)
    if kind == "down":
        x = torch.stack([_signs((M, K), _gen(5, M, N, K, e)) for e in range(E)])
        tot = torch.zeros(M, N, dtype=torch.float64)
        for e in routed:
            acc = x[e] @ ws[e].w.t()
            check_sums(acc, ws[e].exp, f"moe down expert {e}")
            tot += wd[:, e : e + 1] * acc
        assert torch.equal(tot.float().double(), tot), "the combined sum must be exact in fp32"
        xb = _exact(x, BF, "expert activations")
        for e in range(E):
            if e not in routed:
                xb[e] = float("nan")
        return MoeCase(kind, M, E, N, K, xb, w8, scale, wd.float(), cnt, tot.to(BF))
    x = _signs((M, K), _gen(6, M, N, K))
    exp = torch.zeros(E, M, N // 2, dtype=BF)
    uz = torch.zeros(E, M, N // 2, dtype=torch.bool)
    for e in routed:
        acc = x @ ws[e].w.t()
        check_sums(acc, ws[e].exp, f"moe gate/up expert {e}")
        exp[e], uz[e], _ = finish(acc, 1, None, f"moe gate/up expert {e}")
    return MoeCase(kind, M, E, N, K, _exact(x, BF, "rows"), w8, scale, wd.float(), cnt, exp, uz)


def moe_act(c: MoeCase) -> torch.Tensor:
    """The down kernel's input: E packed activations (padding rows 0)."""
    return torch.cat([ref.pack_act(c.x[e]) for e in range(c.E)])


# ------------------------------------------------------------------------------------ launches
@contextlib.contextmanager
def forced(spec: Spec):
    """The spec's form forced wherever it applies (``ops.set_gemm_sk`` / ``ops._W8_MODE``), put back after."""
    if spec.wt == "bf16" and spec.kern != "auto":
        prev = ops._GEMM_SK
        ops.set_gemm_sk(spec.kern)
        try:
            yield
        finally:
            ops.set_gemm_sk(prev)
    elif spec.wt == "w8":
        prev = ops._W8_MODE
        ops._W8_MODE = spec.kern
        try:
            yield
        finally:
            ops._W8_MODE = prev
    else:
        yield


def device_case(c: Case, device, pad: float = 0.0) -> dict:
    """A case's tensors on ``device``: rows row-major and packed (padding rows of the last 16-row
    tile = ``pad``), residual, expected."""
    full = torch.full((((c.M + 15) // 16) * 16, c.K), pad, dtype=BF)
    full[: c.M] = c.x
    mv = lambda t: None if t is None else t.to(device)
    return dict(x=mv(c.x), xp=mv(ref.pack_act(full)), res=mv(c.res), expected=mv(c.expected), u_zero=mv(c.u_zero))


def device_weights(w: Weights, wt: str, device) -> dict:
    if wt == "bf16":
        return dict(w=w.bf16.to(device), wp=w.wp.to(device))
    if wt == "w8":
        return dict(w8=tuple(t.to(device) for t in w.w8))
    return dict(w4=tuple(t.to(device) for t in w.w4))


def run(spec: Spec, c: Case, dc: dict, dw: dict, out=None, res=None) -> dict:
    """One launch of a spec through ``ops.linear`` / ``linear_w8`` / ``linear_w4``.  ``out``: the
    caller's output buffer (epilogues 0 - 2); ``res``: the residual buffer epilogue 3 updates in
    place (default: a fresh copy)."""
    M, epi, dev = c.M, c.epi, dc["xp"].device
    r = {}
    if epi == 3:
        res = dc["res"].clone() if res is None else res
        r = dict(ap=torch.zeros(ops.packed_numel(M, c.N), dtype=BF, device=dev), sso=ops.norm_stats_buffer(dev)[0],
                 ssz=ops.norm_stats_buffer(dev)[0] + 7)
        kw = dict(out=res, residual=res, ap_out=r["ap"], ss_out=r["sso"], ss_zero=r["ssz"])
    elif epi == 2:
        kw = dict(out=out, residual=dc["res"])
    else:
        kw = dict(out=out)
    with forced(spec):
        if spec.wt == "bf16" and spec.rowmajor:
            y = ops.linear(dc["x"], dw["w"], wp=dw["wp"], epilogue=epi, out_packed=spec.packed, **kw)
        elif spec.wt == "bf16":
            y = ops.linear(dc["xp"], None, wp=dw["wp"], a_rows=M, epilogue=epi, out_packed=spec.packed, **kw)
        elif spec.wt == "w8":
            y = ops.linear_w8(dc["xp"], *dw["w8"], M, epilogue=epi, out_packed=spec.packed, **kw)
        else:
            y = ops.linear_w4(dc["xp"], *dw["w4"], M, epilogue=epi, out_packed=spec.packed, **kw)
    r["y"] = y
    return r


def rows_of(spec: Spec, c: Case, y: torch.Tensor) -> torch.Tensor:
    """The M real rows [M, ncols] of a launch's output (unpacked when it is packed)."""
    return ops.unpack_act(y, c.M, c.ncols) if spec.packed else y


def check(spec: Spec, c: Case, dc: dict, r: dict, what: str = "") -> None:
    what = what or spec.id
    if c.epi == 3:
        c3 = dataclasses.replace(c, expected=dc["expected"])
        check_epi3(c3, r["y"], r["ap"], r["sso"], r["ssz"], what)
    else:
        compare(rows_of(spec, c, r["y"]), dc["expected"], dc["u_zero"], what)
