"""Attention probes whose expected output is known in closed form (plain module, CPU only).

The attention tests on ``randn`` inputs compare an average over ~n/e keys under a tolerance as
large as that average's spread: they cannot tell WHICH keys a kernel read.  A probe can.  For one
sequence (page size 64, head dim D):

* "special" key positions (the tiling edges a test aims at, at most D - 1 of them, the first
  invisible position included) hold distinct rows of the D x D Sylvester-Hadamard matrix (row 0
  skipped): entries +-1, exact in bf16, mutually orthogonal.  Every other visible position is
  background, K = +-0.25 at random.  K is the same for every kv head.
* V is random multiples of 0.5 in [-2, 2] (per kv head); special rows differ pairwise in >= D/4
  channels.
* every cache position after the trap - the rest of the last page and one more valid page that
  the block table names - holds NaN (bytes 0xFF in an fp8 cache).  The block table holds valid
  page ids only, so a kernel that reads too far meets NaN, never unmapped memory.
* each (query row, head) is one probe with gain g = 4 (D = 128) or 8 (D = 64), scale 1/sqrt(D):
    single    q = g (K[a] + K[trap])          -> V[a]; a visible trap gives (V[a] + V[trap]) / 2
    pair      q = g (K[a] + K[b])             -> (V[a] + V[b]) / 2; a key counted twice or a wrong
                                                 (m, l) combine gives 2/3 : 1/3
    weighted  q = g K[a] + (g - 0.125) K[b]   -> w V[a] + (1 - w) V[b], w = sigmoid(0.125 sqrt(D))
  The target logit is g sqrt(D) (45 / 64) above every orthogonal key and >= 34 above any
  background key, so all other keys together weigh < 1e-12.

Every q, K and V value is exact in bf16 and through the fp8 KV cache (``KVF8``), which the builder
asserts.  ``compare`` is the comparator: finite everywhere and |out - expected| <= 2^-6, absolute.
The bound is derived, not measured: the bf16 output (|out| <= 2) costs <= 2^-8; P rounds to bf16,
so after normalisation a two-key weight is off by <= 2^-10, times |V[a] - V[b]| <= 4 is <= 2^-8;
together ~2^-7, doubled.  The smallest single-key mistake (a key counted twice in a pair) moves a
channel by >= 0.5 / 6 = 0.083.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from src import ops

PAGE = 64
BOUND = 2.0 ** -6
BF = torch.bfloat16


def gain(D: int) -> float:
    return 4.0 if D == 128 else 8.0


def hadamard(D: int) -> torch.Tensor:
    """D x D Sylvester-Hadamard matrix (D a power of two), float64 +-1."""
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < D:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == D
    return h


@dataclass(frozen=True)
class Probe:
    kind: str          # "single" | "pair" | "weighted"
    a: int
    b: int = -1        # second key of a pair (unused for a single)

    @property
    def keys(self) -> Tuple[int, ...]:
        return (self.a,) if self.kind == "single" else (self.a, self.b)


def weighted_w(D: int) -> float:
    """Weight of key a in a weighted pair: softmax of logits g sqrt(D) and (g - 0.125) sqrt(D)."""
    return 1.0 / (1.0 + math.exp(-0.125 * math.sqrt(D)))


@dataclass
class Seq:
    """One sequence of a case, dense (position-major) for references and mutations."""
    N: int                    # tokens the cache holds before the trap (trap at position N)
    K: torch.Tensor           # [L, D] float64, NaN after the trap
    V: torch.Tensor           # [nkv, L, D] float64, NaN after the trap
    pages: List[int]
    rows: List[int] = field(default_factory=list)  # flat query rows of this sequence


@dataclass
class Case:
    nh: int
    nkv: int
    D: int
    scale: float
    q: torch.Tensor             # bf16 [T, (nh + 2 nkv) D]: q strided inside a qkv row
    k_cache: torch.Tensor       # bf16 [P, nkv, 64, D]
    v_cache: torch.Tensor
    block_tables: torch.Tensor  # int32 [S, maxp], valid page ids only
    q_seq: torch.Tensor         # int32 [T]
    q_ctx: torch.Tensor         # int32 [T]
    expected: torch.Tensor      # float64 [T, nh D] closed form (zeros on rows that are no probes)
    probe_rows: torch.Tensor    # bool [T]
    probes: List[Optional[List[Probe]]]  # per row: nh probes, or None (random q, not compared)
    seqs: List[Seq]
    poison: torch.Tensor        # bool [P, 64]: cache positions that hold NaN
    # RoPE-fused decode cases (rope_case) only
    positions: Optional[torch.Tensor] = None
    slots: Optional[torch.Tensor] = None
    cos: Optional[torch.Tensor] = None
    sin: Optional[torch.Tensor] = None
    k_after: Optional[torch.Tensor] = None   # the caches the launch must leave behind
    v_after: Optional[torch.Tensor] = None
    stale_v: Optional[List[torch.Tensor]] = None  # per sequence [nkv, D]: V of the stale slot N - 1

    @property
    def T(self) -> int:
        return self.q.shape[0]

    def to(self, device):
        """Tensors for a launch on ``device`` (fresh copies: a launch may write the caches)."""
        mv = lambda x: None if x is None else x.clone().to(device)
        return dict(q=mv(self.q), k_cache=mv(self.k_cache), v_cache=mv(self.v_cache),
                    block_tables=mv(self.block_tables), q_seq=mv(self.q_seq), q_ctx=mv(self.q_ctx),
                    positions=mv(self.positions), slots=mv(self.slots), cos=mv(self.cos), sin=mv(self.sin))

    def f8(self, device="cpu"):
        """(K, V) as fp8 caches: the same values exactly; poison = byte 0xFF in codes and scales."""
        res = []
        for c in (self.k_cache, self.v_cache):
            kv = ops.KVF8.from_dense(torch.nan_to_num(c, nan=0.0))
            dq = kv.dequant()
            ok = ~self.poison[:, None, :, None].expand_as(c)
            assert torch.equal(dq[ok], c[ok]), "probe values must be exact through the fp8 KV cache"
            kv.codes[self.poison[:, None, :].expand_as(kv.scales)] = 0xFF
            kv.scales[self.poison[:, None, :].expand_as(kv.scales)] = 0xFF
            assert kv.dequant(torch.float32)[~ok].isnan().all()
            res.append(ops.KVF8(kv.codes.to(device), kv.scales.to(device)))
        return tuple(res)


def _exact_bf16(x: torch.Tensor) -> torch.Tensor:
    y = x.to(BF)
    ok = ~x.isnan()  # (the poison stays NaN)
    assert torch.equal(y.double()[ok], x.double()[ok]) and y.isnan()[~ok].all(), "probe values must be exact in bf16"
    return y


def _build(nh, nkv, D, seq_specs, seed) -> Case:
    """``seq_specs``: per sequence (N, specials, rows); rows = [(ctx, probes | None)], probes one
    per head (``_heads``).  The trap N and every probe's keys and trap must be special."""
    gen = torch.Generator().manual_seed(seed)
    H = hadamard(D)
    g = gain(D)
    rep = nh // nkv
    scale = 1.0 / math.sqrt(D)
    # the pages up to the trap's, and one more valid page of nothing but NaN
    npages = [math.ceil((N + 1) / PAGE) + 1 for N, _, _ in seq_specs]
    P = sum(npages) + 3
    perm = torch.randperm(P, generator=gen).tolist()
    poison_page = perm[sum(npages)]
    kc = torch.full((P, nkv, PAGE, D), float("nan"), dtype=torch.float64)
    vc = torch.full((P, nkv, PAGE, D), float("nan"), dtype=torch.float64)
    bt = torch.full((len(seq_specs), max(npages)), poison_page, dtype=torch.int32)
    seqs, qs, q_seq, q_ctx, exp, probes_all = [], [], [], [], [], []
    used = 0
    for si, (N, specials, rows) in enumerate(seq_specs):
        specials = sorted(set(specials) | {N})
        assert specials[0] >= 0 and specials[-1] == N and len(specials) <= D - 1, (len(specials), D)
        L = npages[si] * PAGE
        K = torch.full((L, D), float("nan"), dtype=torch.float64)
        V = torch.full((nkv, L, D), float("nan"), dtype=torch.float64)
        K[: N + 1] = (torch.randint(0, 2, (N + 1, D), generator=gen).double() - 0.5) * 0.5
        hrow = (torch.randperm(D - 1, generator=gen)[: len(specials)] + 1).tolist()
        for pos, r in zip(specials, hrow):
            K[pos] = H[r]
        V[:, : N + 1] = torch.randint(-4, 5, (nkv, N + 1, D), generator=gen).double() * 0.5
        sv = V[:, specials]  # special rows pairwise different in >= D/4 channels (per kv head)
        ndiff = (sv[:, :, None, :] != sv[:, None, :, :]).sum(-1)
        ndiff += torch.eye(len(specials), dtype=ndiff.dtype) * D
        assert int(ndiff.min()) >= D // 4
        pages = perm[used : used + npages[si]]
        used += npages[si]
        bt[si, : npages[si]] = torch.tensor(pages, dtype=torch.int32)
        for j, pg in enumerate(pages):
            kc[pg] = K[j * PAGE : (j + 1) * PAGE].unsqueeze(0).expand(nkv, PAGE, D)
            vc[pg] = V[:, j * PAGE : (j + 1) * PAGE]
        seq = Seq(N, K, V, pages)
        sp = set(specials)
        for c, plist in rows:
            assert 1 <= c <= N
            t = len(qs)
            seq.rows.append(t)
            q_seq.append(si)
            q_ctx.append(c)
            e = torch.zeros(nh, D, dtype=torch.float64)
            if plist is None:
                qrow = torch.randn(nh, D, generator=gen).to(BF).double()
                probes_all.append(None)
            else:
                assert c in sp, "the trap of a probe row must be a special position"
                qrow = torch.zeros(nh, D, dtype=torch.float64)
                assert len(plist) == nh
                mine = []
                for h, pr in enumerate(plist):
                    assert all(0 <= k < c and k in sp for k in pr.keys) and len(set(pr.keys)) == len(pr.keys), (pr, c)
                    va = V[h // rep, pr.a]
                    if pr.kind == "single":
                        qrow[h] = g * (K[pr.a] + K[c])
                        e[h] = va
                    elif pr.kind == "pair":
                        qrow[h] = g * (K[pr.a] + K[pr.b])
                        e[h] = (va + V[h // rep, pr.b]) / 2
                    else:
                        qrow[h] = g * K[pr.a] + (g - 0.125) * K[pr.b]
                        w = weighted_w(D)
                        e[h] = w * va + (1 - w) * V[h // rep, pr.b]
                    mine.append(pr)
                probes_all.append(mine)
            kvpart = torch.randn(2 * nkv, D, generator=gen).to(BF).double()
            qs.append(torch.cat([qrow, kvpart], 0).reshape(-1))
            exp.append(e.reshape(-1))
        seqs.append(seq)
    poison = kc[:, 0, :, 0].isnan()
    assert torch.equal(poison, vc[:, 0, :, 0].isnan()) and bool(poison[poison_page].all())
    return Case(nh, nkv, D, scale, _exact_bf16(torch.stack(qs)), _exact_bf16(kc), _exact_bf16(vc), bt,
                torch.tensor(q_seq, dtype=torch.int32), torch.tensor(q_ctx, dtype=torch.int32), torch.stack(exp),
                torch.tensor([p is not None for p in probes_all]), probes_all, seqs, poison)


def _heads(nh: int, j: int, cycle: List[Probe], fixed: List[Probe] = ()) -> List[Probe]:
    """The nh probes of a sequence's j-th row: ``fixed`` on the first heads of every row, then the
    row's share of ``cycle`` (row j goes on where row j - 1 stopped)."""
    fixed = list(fixed)[:nh]
    cycle = cycle or fixed
    m = nh - len(fixed)
    return fixed + [cycle[(j * m + i) % len(cycle)] for i in range(m)]


# ------------------------------------------------------------------------------------ decode
DECODE_CTXS = (1, 2, 63, 64, 65, 129, 257, 1000, 4097)
PART_SIZES = (64, 128, 256, 2048)


def decode_edges(n: int, D: int, part_sizes) -> List[int]:
    """Key positions in [0, n) at the tiling edges of the decode kernels."""
    tpi = 64 // (D // 8)
    e = {0, 1, tpi - 1, tpi, 31, 32, 63, 64, 65, 127, 128, 129, 255, 256, 257, n - 2, n - 1}
    for ps in part_sizes:
        last = ps * ((n - 1) // ps)
        e |= {ps - 1, ps, ps + 1, last - 1, last, last + 1}
    return sorted(x for x in e if 0 <= x < n)


def _decode_probes(n: int, D: int, part_sizes) -> List[Probe]:
    edges = decode_edges(n, D, part_sizes)
    pairs = [(0, n - 1), (n - 2, n - 1), (63, 64)]
    for ps in part_sizes:
        last = ps * ((n - 1) // ps)
        pairs += [(last - 1, last), (ps - 1, ps)]
    seen, ok = set(), []
    for a, b in pairs:
        if 0 <= a < b < n and (a, b) not in seen:
            seen.add((a, b))
            ok.append((a, b))
    out = [Probe("pair", a, b) for a, b in ok]
    out += [Probe("weighted", a, b) for a, b in ok[:3]] + [Probe("weighted", b, a) for a, b in ok[:1]]
    # singles: the ends first, then the far edges (the long-context code) before the near ones
    first = [x for x in (n - 1, 0, n - 2) if 0 <= x < n]
    rest = [x for x in reversed(edges) if x not in first]
    return out + [Probe("single", a) for a in dict.fromkeys(first + rest)]


def decode_case(nh, nkv, D, ctxs=DECODE_CTXS, rows=None, short_ctx=False, seed=0) -> Case:
    """One launch of several sequences, ``rows`` query rows each (q_seq repeated, q_ctx = n); every
    (row, head) aims at another edge, for every partition of ``decode_partitions``.  ``short_ctx``:
    q_ctx = n for a cache that holds 2 n + 70 tokens (prefill-as-decode: the trap is real data); its
    heads go on in the probe list where the plain case's rows * nh heads stopped, so that the two
    cases of a shape with few heads cover the whole list between them."""
    rows = rows or (3 if nh <= 12 else 2)
    parts = sorted({ps for ps, _ in decode_partitions(len(ctxs) * rows, nkv, max(ctxs))})
    specs = []
    for n in ctxs:
        pl = _decode_probes(n, D, parts)
        if short_ctx:
            k = (rows * nh) % len(pl)
            pl = pl[k:] + pl[:k]
        sp = {k for p in pl for k in p.keys}
        specs.append((2 * n + 70 if short_ctx else n, sp | {n}, [(n, _heads(nh, j, pl)) for j in range(rows)]))
    return _build(nh, nkv, D, specs, seed)


def decode_partitions(T: int, nkv: int, max_ctx: int):
    """(part_size, num_parts): the default of ``attention_partition`` first, then 64- / 128- / 256- /
    2048-token slices, each with enough slices to cover ``max_ctx``."""
    res = [tuple(ops.attention_partition(T, nkv, max_ctx))]
    for ps in PART_SIZES:
        p = (ps, math.ceil(max_ctx / ps))
        if p not in res:
            res.append(p)
    return res


# ------------------------------------------------------------------------------------ prefill
PREFILL_ROWS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64)


def _prefill_probes(c: int):
    """(fixed, cycle) probes of a row with context c.  Fixed, on every probe row: singles at the
    diagonal c - 1, c - 2 and key 0.  Cycled over the other heads: singles at the largest multiples
    of 16 / 32 / 64 below c (the 64 one is the first key of the last 64-token step) and those minus 1;
    pairs across the same edges."""
    tg = [c - 1, c - 2, 0]
    mult = [m * ((c - 1) // m) for m in (16, 32, 64)]
    for x in mult:
        tg += [x, x - 1]
    tg = [x for x in dict.fromkeys(tg) if 0 <= x < c]
    pairs = [(0, c - 1), (c - 2, c - 1)] + [(x - 1, x) for x in dict.fromkeys(mult)]
    pairs = [(a, b) for a, b in dict.fromkeys(pairs) if 0 <= a < b < c]
    nfix = len(dict.fromkeys(x for x in (c - 1, c - 2, 0) if 0 <= x < c))
    out = [Probe("single", a) for a in tg[nfix:]] + [Probe("pair", a, b) for a, b in pairs]
    if pairs:
        out += [Probe("weighted", *pairs[0]), Probe("weighted", pairs[-1][1], pairs[-1][0])]
    return [Probe("single", a) for a in tg[:nfix]], out


def prefill_case(nh, nkv, D, ntoks, prefix, row_idx=PREFILL_ROWS, seed=0) -> Case:
    """Chunked causal prefill: sequence i has ``prefix[i]`` cached tokens and ``ntoks[i]`` query rows
    (row j sees ctx = prefix + j + 1; its trap, position ctx, is the chunk's next token, really in
    the cache).  Rows ``row_idx`` (and the last) are probes - together they must fit the D - 1
    special positions of a sequence; the other rows keep random q."""
    specs = []
    for n, pre in zip(ntoks, prefix):
        N = pre + n
        sp, chosen = {N}, {}
        for j in dict.fromkeys([n - 1] + [r for r in row_idx if 0 <= r < n]):
            c = pre + j + 1
            fixed, cyc = _prefill_probes(c)
            sp |= {k for p in fixed + cyc for k in p.keys} | {c}
            assert len(sp) <= D - 1, f"probe row {j}: more than {D - 1} special positions, drop a row"
            chosen[j] = _heads(nh, j, cyc, fixed)
        assert n - 1 in chosen
        specs.append((N, sp, [(pre + j + 1, chosen.get(j)) for j in range(n)]))
    return _build(nh, nkv, D, specs, seed)


def qctx_lists(case: Case):
    """(ntoks per sequence, in flat order) of a case, for ``query_blocks`` / ``fa_blocks``."""
    return [len(s.rows) for s in case.seqs]


# ------------------------------------------------------------------------------------ RoPE-fused decode
ROPE_CTXS = (1, 64, 65, 129, 257, 1000)


def _unrotate_quarter(x: torch.Tensor) -> torch.Tensor:
    """x' with rotate_half(x', cos = 0, sin = 1) = [-x'2, x'1] = x, i.e. x' = [x2, -x1]."""
    h = x.shape[-1] // 2
    return torch.cat([x[..., h:], -x[..., :h]], -1)


def rope_case(nh, nkv, D, ctxs=ROPE_CTXS, quarter=False, seed=0) -> Case:
    """A RoPE-fused decode step: one query per sequence, its own token n - 1 the last of the context.
    The qkv row carries the new token's k (the Hadamard row of n - 1) and v; its cache slot holds a
    stale trap, the same K row with another V.  The rotary table is the identity (cos 1, sin 0), or
    with ``quarter`` a quarter turn (cos 0, sin 1) with q and the new k pre-rotated the other way:
    either way the rotated values are the exact probe."""
    specs = []
    for n in ctxs:
        pl = [Probe("single", n - 1)]
        if n >= 2:
            pl += [Probe("pair", 0, n - 1), Probe("weighted", 0, n - 1), Probe("weighted", n - 1, 0)]
        if n >= 3:
            pl += [Probe("pair", n - 2, n - 1), Probe("weighted", n - 2, n - 1)]
        specs.append((n, {k for p in pl for k in p.keys} | {n}, [(n, _heads(nh, 0, pl))]))
    case = _build(nh, nkv, D, specs, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    T = case.T
    qkv = case.q.double().view(T, nh + 2 * nkv, D).clone()
    case.k_after, case.v_after = case.k_cache.clone(), case.v_cache.clone()
    case.stale_v, slots = [], []
    for t, (seq, n) in enumerate(zip(case.seqs, ctxs)):
        qkv[t, nh : nh + nkv] = seq.K[n - 1]
        qkv[t, nh + nkv :] = seq.V[:, n - 1]
        while True:
            stale = torch.randint(-4, 5, (nkv, D), generator=gen).double() * 0.5
            if int((stale != seq.V[:, n - 1]).sum(-1).min()) >= D // 4:
                break
        case.stale_v.append(stale)
        pg, off = seq.pages[(n - 1) // PAGE], (n - 1) % PAGE
        case.v_cache[pg, :, off] = stale.to(BF)
        slots.append(pg * PAGE + off)
    if quarter:
        qkv[:, : nh + nkv] = _unrotate_quarter(qkv[:, : nh + nkv])
    case.q = _exact_bf16(qkv.reshape(T, -1))
    case.positions = case.q_ctx.long() - 1
    case.slots = torch.tensor(slots, dtype=torch.int64)
    tab = torch.zeros(max(ctxs) + 1, D // 2, dtype=torch.float32)
    case.cos, case.sin = (tab, tab + 1) if quarter else (tab + 1, tab)
    return case


# ------------------------------------------------------------------------------------ comparator
def deviation(out: torch.Tensor, case: Case) -> torch.Tensor:
    """[T, nh] largest |out - expected| per (row, head); inf where the output is not finite."""
    o = out.detach().cpu().double().reshape(case.T, case.nh, case.D)
    d = (o - case.expected.view(case.T, case.nh, case.D)).abs().amax(-1)
    return torch.where(torch.isfinite(o).all(-1), d, torch.full_like(d, float("inf")))


def rejected(out: torch.Tensor, case: Case) -> torch.Tensor:
    """bool [T, nh]: the comparator rejects this (row, head)."""
    return deviation(out, case) > BOUND


def compare(out: torch.Tensor, case: Case, what: str = "") -> float:
    """The comparator: the whole output finite, every probe row within 2^-6 of the closed form
    (absolute, no relative term).  Returns the largest deviation seen."""
    o = out.detach().cpu().double().reshape(case.T, -1)
    assert torch.isfinite(o).all(), f"{what}: non-finite output (a kernel read past the context)"
    dev = deviation(out, case)[case.probe_rows]
    worst = float(dev.max())
    if worst > BOUND:
        rows = torch.nonzero(case.probe_rows).flatten().tolist()
        bad = [(rows[i], h, case.probes[rows[i]][h], int(case.q_ctx[rows[i]]), round(float(dev[i, h]), 4))
               for i, h in torch.nonzero(dev > BOUND).tolist()[:8]]
        raise AssertionError(f"{what}: |out - expected| = {worst:.4f} > 2^-6; (row, head, probe, ctx, dev): {bad}")
    return worst
