"""fp64 inverse-CDF oracle of the token sampler (plain module, numpy / torch on the CPU).

``ops.sample`` is deterministic: row r draws with u = ``uniform(seed_r, r)`` - splitmix64 of
``seed * 0x9E3779B97F4A7C15 + r``, its top 53 bits scaled to [0, 1) and rounded to fp32 - by an
inverse CDF over a defined order of the ids that survive the repetition penalty, top-k and top-p.
``oracle`` computes those ids and the fp64 edges of their intervals; ``acceptable`` says which ids
a correct fp32 kernel may return for a given u; ``route`` says which of the kernel's two draw
orders a row takes.  ``cases`` builds the inputs of tests/test_sampler_probe_gpu.py, and
tests/test_sampler_probe.py checks the oracle itself (and, through ``MUTANTS``, that the cases
would catch a wrong sampler).

Which row takes which order (``route``; decided in csrc/sampling.hip at the places named):

* temperature <= 0: greedy, the first maximum of the raw logits (``sample_kernel`` before the
  penalty; ``sample_split_merge_kernel`` from the chunk records).
* ``mp_sample`` launches the split kernels when V >= 65536, V <= 64 chunks of 8192 and the history
  capacity is <= 256.  There a row with 0 < k <= 64 is drawn by ``sample_split_merge_kernel`` in
  "sorted" order, unless some chunk finds more than 512 candidates at its k-th thread maximum
  (``sample_split_chunk_kernel``: record word 4 = -1); every other sampled row is left at -1 for
  ``sample_kernel(only_unset = 1)``.
* ``sample_kernel`` (one workgroup per row; LDS row for V <= 34816, workspace row above; 16-byte
  loads when V % 8 == 0, scalar loads otherwise) takes its fast path, "sorted" order, when
  0 < k < V and at most 1024 values reach tau, a lower bound of the k-th largest value taken from
  the per-thread maxima: for k <= 64 the k-th largest of the union of every wave's four largest
  thread maxima (no bound at all when fewer than k of those exist), otherwise the k-th largest
  thread maximum.  When fewer than k threads own a value (k > 1024; k > V / 8 for a narrow
  vectorised row) or more than 1024 values reach tau (large k, or many ties at the k-th value),
  and for k <= 0 or k >= V, it takes the general path: "index" order.

"sorted": top-k = the first k ids by (value desc, index asc); top-p keeps the sorted prefix with
cumulative full-softmax mass <= p, always the first id; the draw runs over the sorted order.
"index": ids tied with the k-th value are all kept; top-p drops the first VALUE (with all its
ties) whose descending cumulative mass exceeds p and everything below it, never the maximum; the
draw runs in index order.

eps, the bound on the fp32 error of the kernel's CDF (d = 2^-24, the unit roundoff; p_i the
softmax probability of id i, a_i = (x_i - m) / T its exponent; the common factor 1 / Z cancels in
the draw, which normalises by the sum of the kept probabilities):
* exponent: (x_i - m) * inv_t carries <= 3 d relative error (subtraction, reciprocal, product), a
  relative error 3 d |a_i| of p_i; summed over ids, 3 d sum p_i |a_i| <= 3 d ln V <= 36 d
  (sum p_i |a_i| is at most the entropy, V <= 151936).
* a penalised logit x' = x / rp^c (powf <= 2 ulp, one or two divisions) is off by <= 6 d |x'|; the
  cases keep |x'| / T <= 40 for every id with mass, so <= 240 d, on the penalised ids only.
* ``__expf(a)`` = v_exp_f32(a * log2 e): the product's rounding is a relative error d |a| of the
  result, the instruction adds 1 ulp: (|a_i| + 2) d, summed <= 14 d.
* scans: a prefix of the fast and the split path goes through <= 12 additions, of the general path
  through <= ceil(V / 1024) - 1 = 148 sequential and 12 tree additions, each <= d of a partial sum
  <= the total; prefix and total together <= 2 * 160 d = 320 d.
* u * total: d.
Sum <= 611 d = 2^-14.7; EPS = 2^-14 = 1024 d.  The same terms plus the normaliser (<= 170 d) bound
the error of the cumulative mass that top-p compares with p, so a cut within EPS of p may fall
either way and ``acceptable`` takes the union over those cuts.  (The general path's top-p sums
masses with LDS atomics, bin by bin; a bin of n values has a worst case of n d times its mass, which
only the many-tiny-ids tail of a flat row could bring near EPS - the wide general-path cases use
peaked rows.)  Rows marked ``exact`` - a few ids tied at the maximum, every other logit >= 100
below - have probabilities that are exact powers of two in fp32 and fp64 alike (exp(0) = 1, the
rest flushes to 0), so their cut is compared without slack: they are what tells a top-p ``<``
from ``<=``.

The oracle works in the logit domain with fp64 penalties.  The kernel's penalised logit is an fp32
quotient, and bf16 / 1.2 lands on another bf16 value often enough to matter (11.625 / 1.2f rounds to
9.6875 exactly, a tie the index then breaks, where fp64 says 9.68749962 < 9.6875): where another
logit lies within TIE_TOL = 2^-21 (relative) of a penalised one, ``oracle`` adds the draws with the
penalised logit nudged above and below it, and ``acceptable`` takes their union too.  The kernel's
general path ranks fp32 probabilities, where distinct logits far below the maximum can collapse
into one value; the cases keep every top-k / top-p boundary among ids with distinct probabilities,
or ties in the logits."""
import functools
import itertools
import math
from collections import Counter
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

EPS = 2.0 ** -14
TIE_TOL = 2.0 ** -21  # relative slack of a penalised logit (the kernel's is within 6 * 2^-24 of the fp64 one)
M64 = (1 << 64) - 1
SEED_MUL = 0x9E3779B97F4A7C15
T_MIN = float(np.float32(1e-5))

# the dispatch constants of csrc/sampling.hip that ``route`` mirrors
SB, CAND = 1024, 1024
SPLIT_MIN, SPLIT_CH, SPLIT_NT, SPLIT_KMAX, SPLIT_CAND, SPLIT_MAXC = 65536, 8192, 256, 64, 512, 64
LDS_MAX_V = 136 * 1024 // 4  # 34816


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniform(seed: int, row: int, row_term: bool = True) -> float:
    """The kernel's u01 of (seed, launch row): exact integers, then one rounding to fp32."""
    r = splitmix64(((seed & M64) * SEED_MUL + (row if row_term else 0)) & M64)
    return float(np.float32((r >> 11) * 2.0 ** -53))


def bf16_values(logits_row) -> np.ndarray:
    return torch.as_tensor(logits_row).detach().to(torch.bfloat16).double().numpy().copy()


def penalise(x: np.ndarray, rp: float, history, cap: int, last_three=True, always_divide=False,
             count_once=False) -> np.ndarray:
    """Repetition penalty over the last ``cap`` ids (header comment of sampling.hip)."""
    x = x.copy()
    h = [int(t) for t in history][-cap:]
    if rp == 1.0 or not h:
        return x
    V = len(x)
    for tok, cnt in Counter(h).items():
        if not 0 <= tok < V:
            continue
        e = 1 if count_once else cnt
        if last_three and len(h) >= 3 and h[-1] == h[-2] == h[-3] == tok:
            e += 3
        pen = rp ** e
        x[tok] = x[tok] / pen if (x[tok] > 0 or always_divide) else x[tok] * pen
    return x


def _kth_largest(v: np.ndarray, k: int) -> float:
    return float(np.partition(v, len(v) - k)[len(v) - k])


def route(xp: np.ndarray, temp: float, k: int, cap: int) -> Tuple[str, str]:
    """(order, path) of a row with penalised logits ``xp``, mirroring ``mp_sample``'s dispatch."""
    V = len(xp)
    if temp <= 0:
        return "greedy", "greedy"
    C = -(-V // SPLIT_CH)
    split = V >= SPLIT_MIN and C <= SPLIT_MAXC and cap <= SPLIT_NT
    where = "lds" if V <= LDS_MAX_V else "workspace"
    if split and 0 < k <= SPLIT_KMAX and k < V:
        ok = True
        for c in range(C):
            ch = xp[c * SPLIT_CH:(c + 1) * SPLIT_CH]
            n = len(ch)
            nmax = min(SPLIT_NT, n)
            pad = np.full(-(-n // SPLIT_NT) * SPLIT_NT, -np.inf)
            pad[:n] = ch
            tmax = pad.reshape(-1, SPLIT_NT).max(0)[:nmax]  # thread t owns t, t + 256, ...
            tau = _kth_largest(tmax, min(k, n, nmax))
            if int((ch >= tau).sum()) > SPLIT_CAND:
                ok = False
                break
        if ok:
            return "sorted", f"split C={C}" + (" (C > 16 merge)" if C > 16 else "")
        where = "split chunk degenerate -> " + where
    elif split:
        where = "split fallback -> " + where
    if not 0 < k < V:
        return "index", f"general ({where})"
    vec = V % 8 == 0
    if vec:  # thread t owns the 8-wide pieces t, t + 1024, ...
        pad = np.full(-(-V // (SB * 8)) * SB * 8, -np.inf)
        pad[:V] = xp
        tmax = pad.reshape(-1, SB, 8).max((0, 2))
    else:
        pad = np.full(-(-V // SB) * SB, -np.inf)
        pad[:V] = xp
        tmax = pad.reshape(-1, SB).max(0)
    load = "16-B loads" if vec else "scalar loads"
    if k <= 64:
        u = np.sort(tmax.reshape(16, 64), axis=1)[:, -4:].reshape(-1)  # -inf stands for "no element"
        tau = _kth_largest(u, k)
    else:
        owned = tmax[tmax > -np.inf]
        if len(owned) < k:
            return "index", f"general: fewer thread maxima than k ({where}, {load})"
        tau = _kth_largest(owned, k)
    if int((xp >= tau).sum()) > CAND:
        return "index", f"general: > 1024 candidates ({where}, {load})"
    return "sorted", f"fast top-k ({where}, {load})"


@dataclass
class Draw:
    """Kept ids in draw order with the fp64 edges of their intervals (``edges[j] .. edges[j + 1]``
    belongs to ``ids[j]``); ``variants`` lists (ids, edges) for every top-p cut within the slack of
    p, the nominal one first."""
    ids: np.ndarray
    edges: np.ndarray
    variants: List[Tuple[np.ndarray, np.ndarray]]
    top: int  # the most likely kept id: what the kernel returns when rounding pushes u past the end

    def token(self, u: float) -> int:
        """The id whose exact interval holds u (-1: nothing kept)."""
        if len(self.ids) == 0:
            return -1
        j = int(np.searchsorted(self.edges[1:], u, side="right"))
        return int(self.ids[min(j, len(self.ids) - 1)])


def _variant(ids, P):
    q = P[ids]
    c = np.cumsum(q)
    return ids, np.concatenate([[0.0], c / c[-1]])


def oracle(logits_row, temp, top_p, top_k, rep_pen, history, order, cap=50, cut_eps=EPS, tie_tol=None, k_delta=0,
           p_strict=False, keep_first=True, last_three=True, always_divide=False, count_once=False) -> Draw:
    """``cut_eps`` / ``tie_tol``: the slack of a top-p cut and of a penalised logit (0: the nominal draw
    only).  The keyword arguments after them switch on the deliberately wrong variants of ``MUTANTS``."""
    x = bf16_values(logits_row)
    V = len(x)
    if temp <= 0 or order == "greedy":
        i = int(np.argmax(x))
        ids = np.array([i])
        e = np.array([0.0, 1.0])
        return Draw(ids, e, [(ids, e)], i)
    rp = float(np.float32(rep_pen))
    xp = penalise(x, rp, history, cap, last_three, always_divide, count_once)
    core = dict(temp=temp, top_p=top_p, top_k=top_k, order=order, cut_eps=cut_eps, k_delta=k_delta, p_strict=p_strict,
                keep_first=keep_first)
    d = _draw(xp, **core)
    tie_tol = (TIE_TOL if cut_eps > 0 else 0.0) if tie_tol is None else tie_tol
    if tie_tol > 0 and rp != 1.0:
        # A penalised logit is an fp32 quotient in the kernel (bf16 / 1.2 often lands on another bf16 value, where
        # fp32 rounding makes a tie or decides the order): with another logit within tie_tol of it, either order.
        near = [t for t in sorted({int(t) for t in list(history)[-cap:] if 0 <= int(t) < V})
                if int((np.abs(xp - xp[t]) <= tie_tol * abs(xp[t])).sum()) > 1]
        n = len(near)
        combos = list(itertools.product((-1.0, 1.0), repeat=n)) if n <= 3 else [(-1.0,) * n, (1.0,) * n]
        for signs in combos if n else []:
            x2 = xp.copy()
            for t, sg in zip(near, signs):
                x2[t] += sg * 2 * tie_tol * abs(xp[t])
            d.variants += _draw(x2, **core).variants
    return d


def _draw(xp, temp, top_p, top_k, order, cut_eps, k_delta, p_strict, keep_first) -> Draw:
    V = len(xp)
    t = max(float(np.float32(temp)), T_MIN)
    p = np.exp((xp - xp.max()) / t)
    P = p / p.sum()
    k = top_k + k_delta if 0 < top_k < V else top_k
    tp = float(np.float32(top_p))
    top = int(np.argmax(xp))
    # cand: the ids that survive top-k, by (value desc, index asc) - a stable sort of what reaches the k-th value
    if 0 < k < V:
        pool = np.nonzero(xp >= _kth_largest(xp, k))[0]
        pool = pool[np.argsort(-xp[pool], kind="stable")]
        cand = pool[:k] if order == "sorted" else pool
    elif order == "sorted" or 0.0 < tp < 1.0:
        cand = np.argsort(-xp, kind="stable")
    else:  # every id, drawn in index order
        ids, e = _variant(np.arange(V), P)
        return Draw(ids, e, [(ids, e)], top)
    if order == "sorted":
        ends = np.arange(1, len(cand) + 1)
    else:
        xv = xp[cand]
        ends = np.concatenate([np.nonzero(xv[1:] != xv[:-1])[0] + 1, [len(cand)]])  # ends of tie groups
    if 0.0 < tp < 1.0:
        cg = np.cumsum(P[cand])[ends - 1]

        def groups(bound):
            n = int((cg < bound).sum() if p_strict else (cg <= bound).sum())
            return max(n, 1) if keep_first else n

        nom = groups(tp)
        cuts = [nom] + [g for g in range(groups(tp - cut_eps), groups(tp + cut_eps) + 1) if g != nom]
        kept = [cand[:ends[g - 1]] if g > 0 else cand[:0] for g in cuts]
    else:
        kept = [cand]
    if order != "sorted":
        kept = [np.sort(ids) for ids in kept]
    if len(kept[0]) == 0:
        return Draw(kept[0], np.array([0.0]), [], -1)
    variants = [_variant(ids, P) for ids in kept]
    return Draw(variants[0][0], variants[0][1], variants, top)


def acceptable(draw: Draw, u: float, eps: float = EPS) -> set:
    """Every id the kernel may return: those whose interval, widened by eps on both sides, holds u,
    over every cut variant; the most likely id too when u is within eps of 1 (the kernel's fallback
    when rounding leaves u behind the last interval)."""
    ok = set()
    for ids, e in draw.variants:
        m = (u >= e[:-1] - eps) & (u <= e[1:] + eps)
        ok.update(int(i) for i in ids[m])
    if u >= 1.0 - eps and draw.top >= 0:
        ok.add(draw.top)
    return ok


def outside(draw: Draw, u: float, tok: int) -> float:
    """Distance of u from ``tok``'s unwidened interval (0 inside; the nearest over the variants)."""
    best = math.inf
    for ids, e in draw.variants:
        for j in np.nonzero(ids == tok)[0]:
            best = min(best, max(e[j] - u, u - e[j + 1], 0.0))
    return best


# ------------------------------------------------------------------------------------- cases
KS = [-1, 0, 1, 5, 50, 64, 65, 200, 2000, "V-1", "V"]
TOP_PS = [0.0, 1e-6, 0.5, 0.92, 1.0, 1.5]
TEMPS = [0.0, 1e-6, 0.5, 0.8, 1.5]
PENS = [1.0, 1.2, 1.5]
HISTS = ["empty", "short", "full", "last3", "repeat"]


@dataclass
class Row:
    temp: float
    top_p: float
    top_k: int
    rep_pen: float
    history: List[int]
    seed: int
    exact: bool = False  # probabilities are exact powers of two: the top-p cut has no slack
    note: str = ""


@dataclass
class Case:
    name: str
    V: int
    cap: int
    logits: torch.Tensor            # bf16 [R, V], contiguous
    rows: List[Row]
    buf_width: int = 0              # > 0: the launch passes a [:, off:off + V] view of a buf_width-wide buffer
    buf_off: int = 0
    _truth: Optional[list] = field(default=None, repr=False)

    @property
    def R(self):
        return len(self.rows)


# name, V, rows, history capacity, (buffer width, column offset) of a strided view
SPECS = [
    ("v50", 50, 64, 50, (56, 0)),
    ("v512", 512, 64, 50, None),
    ("v512_r1", 512, 1, 3, None),
    ("v1001", 1001, 200, 50, (1016, 8)),
    ("v32000", 32000, 64, 50, None),
    ("v32000_strided", 32000, 3, 3, (32776, 8)),
    ("v34816", 34816, 3, 50, None),
    ("v34824", 34824, 3, 3, None),
    ("v50257", 50257, 64, 50, (50264, 0)),
    ("v65528", 65528, 3, 50, None),
    ("v65536", 65536, 64, 3, None),
    ("v128256", 128256, 64, 50, None),
    ("v131080", 131080, 64, 50, None),
    ("v131080_r1", 131080, 1, 50, None),
    ("v151936", 151936, 3, 3, None),
    ("v128256_cap300", 128256, 3, 300, None),
]
CASE_NAMES = [s[0] for s in SPECS]
VERIFY_CASES = ["v512", "v131080"]
# (k, top-p, temperature, penalty, history) of the 3-row and 1-row cases
SMALL = {
    1: [(50, 0.92, 0.8, 1.2, "full")],
    3: [(50, 0.92, 0.8, 1.2, "full"), (0, 0.92, 0.8, 1.5, "last3"), (200, 1.0, 1.5, 1.0, "short")],
    "v151936": [(64, 0.92, 0.8, 1.2, "full"), (65, 0.5, 0.5, 1.5, "last3"), (0, 0.92, 0.8, 1.0, "empty")],
    "v128256_cap300": [(50, 0.92, 0.8, 1.2, "full"), (5, 0.5, 0.5, 1.5, "last3"), (0, 0.92, 1.5, 1.2, "repeat")],
    "v34824": [(200, 0.92, 0.8, 1.5, "last3"), (0, 0.5, 0.5, 1.2, "full"), (5, 1.0, 1.5, 1.0, "short")],
}
EXACT_CASES = {"v512", "v32000", "v131080"}     # their last 6 rows are ``exact`` rows
TIE_CASES = {"v32000": None, "v128256": 3}      # row 57: ~2000 ids tie at the maximum (in one chunk)


def _cycle(values, R, g):
    out = []
    while len(out) < R:
        out += [values[i] for i in torch.randperm(len(values), generator=g).tolist()]
    return out[:R]


def _rand_ids(g, V, n, avoid=()):
    out = []
    while len(out) < n:
        t = int(torch.randint(0, V, (1,), generator=g))
        if t not in avoid:
            out.append(t)
    return out


def _history(kind, x, V, cap, g):
    """Histories of every shape; they hold ids of the top 5 (inside any top-k), random ids (positive
    and negative logits) and the ids -1 and V, which the sampler must ignore."""
    top = torch.topk(x.float(), 5).indices.tolist()
    if kind == "empty":
        return []
    if kind == "short":
        return [top[1], -1] if cap <= 3 else [top[1], -1, V]
    if kind == "last3":
        pre = _rand_ids(g, V, min(cap - 3, 4), avoid=top[:1])
        return pre + [top[0]] * 3
    if kind == "repeat":
        if cap <= 3:
            return [top[0], V, top[0]]
        other = _rand_ids(g, V, 3, avoid=top[:1])
        return [top[0], other[0], top[0], top[0], other[1], top[0], -1, top[0], other[2]][:cap]
    h = _rand_ids(g, V, cap)  # full
    for pos, t in zip(torch.randperm(cap, generator=g).tolist(), [top[0], top[2], -1, V, top[0]]):
        h[pos] = t
    if h[-1] == h[-2] == h[-3]:
        h[-2] = -1
    return h


def _bf(v: float) -> float:
    return float(torch.tensor(v).to(torch.bfloat16))


def _argmax_row(x, V, cap, rp, neg, r, g):
    """A row whose draw is the arg-max of the penalised logits (temperature 1e-6 or k = 1), with the
    two leading ids A and B placed so that the penalty rules decide between them: B wins by a clear
    gap, and A wins if the rule under test is wrong.  Returns (history, note)."""
    A, B = _rand_ids(g, V, 2) if V > 2 else (0, 1)
    while B == A:
        B = _rand_ids(g, V, 1)[0]
    m = float(x.float().max())
    fill = [t for t in _rand_ids(g, V, 4, avoid=(A, B))]
    if neg:  # negative logits are multiplied: A = -0.25 falls behind B, and passes it if divided
        x[A], x[B] = -0.25, -0.25 * rp ** 0.5
        return ([A, V, -1] if cap > 3 else [A, -1]), "penalty multiplies a negative logit"
    xb = m + 2.0
    x[B] = xb
    if r % 2 == 0:  # last three equal: rp**6 in all, rp**3 without the rule
        x[A] = xb * rp ** 4.5
        return fill[:min(cap - 3, 2)] + [A, A, A], "last-three rule"
    if cap <= 3:  # A counted twice (rp**2), once if ids are counted once
        x[A] = xb * rp ** 1.5
        return [A, fill[0], A], "count penalty"
    x[A] = xb * rp ** 2.0  # A counted three times
    return [A, fill[0], A, fill[1], A, fill[2]], "count penalty"


def _build(name, V, R, cap, view) -> Case:
    g = torch.Generator().manual_seed(20240 + V * 7 + R * 131 + cap)
    if R >= 11:
        params = list(zip(_cycle(KS, R, g), _cycle(TOP_PS, R, g), _cycle(TEMPS, R, g), _cycle(PENS, R, g),
                          _cycle(HISTS, R, g)))
    else:
        params = SMALL.get(name, SMALL[R])
    logits = torch.empty(R, V, dtype=torch.bfloat16)
    rows = []
    n_exact = 6 if name in EXACT_CASES else 0
    for r, (k, tp, T, rp, hk) in enumerate(params):
        k = V - 1 if k == "V-1" else V if k == "V" else k
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=g))
        if r % 9 == 4:
            seed = -seed  # the kernel reads the seed as unsigned
        note = ""
        exact = False
        if r >= R - n_exact:
            # four ids tie at the maximum (two of them in one chunk of a split row), the rest >= 102 below,
            # log-uniform so that few values tie at any top-k bound: probabilities 1/4 each, exactly
            x = (-100.0 * torch.exp(5.0 * torch.rand(V, generator=g))).to(torch.bfloat16)
            ties = sorted({V // 9, V // 9 + 17, V // 2 + 3, V - 5})
            x[ties] = 2.0
            k, tp, T, rp, hist, exact = 50, 0.5, (0.5, 0.8, 1.5)[r % 3], 1.0, [], True
            note = "exact quarters, top-p 0.5"
        elif name in TIE_CASES and r == 57:
            x = (3.0 * torch.randn(V, generator=g)).clamp(max=4.0).to(torch.bfloat16)
            ch = TIE_CASES[name]
            pool = torch.randperm(V if ch is None else SPLIT_CH, generator=g)[:2000] + (0 if ch is None else ch * SPLIT_CH)
            x[pool] = 5.0
            k, tp, T, rp, hist = 50, 1.0, 0.8, 1.0, []
            note = "2000 ids tie at the maximum"
        else:
            general = not 0 < k <= 1024 or k >= V
            scale = 6.0 * max(T, 0.5) / 0.8 if (V >= 32000 and general and T >= 0.5) else 3.0
            x = (scale * torch.randn(V, generator=g)).to(torch.bfloat16)
            neg = r % 4 == 1
            if neg:  # every logit negative: the penalty multiplies
                x = (x.float() - x.float().max() - 1.0).to(torch.bfloat16)
            arg = T > 0 and (T < 1e-3 or k == 1)
            if arg and rp != 1.0 and V > 8:
                hist, note = _argmax_row(x, V, cap, rp, neg, r, g)
            else:
                hist = _history(hk, x, V, cap, g)
                if 0 < T < 1e-3:  # a clear top-1 gap of the penalised row
                    A = _rand_ids(g, V, 1, avoid=[t for t in hist if rp != 1.0])[0]
                    x[A] = float(x.float().max()) + 4.0
        logits[r] = x
        rows.append(Row(float(np.float32(T)), float(np.float32(tp)), int(k), float(np.float32(rp)),
                        [int(t) for t in hist][-cap:], seed, exact, note))
    bw, off = view if view else (0, 0)
    return Case(name, V, cap, logits, rows, bw, off)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    spec = {s[0]: s for s in SPECS}[name]
    return _build(*spec)


def cases() -> Dict[str, Case]:
    """The named GPU cases, generated from fixed seeds on the CPU."""
    return {n: case(n) for n in CASE_NAMES}


@dataclass
class Truth:
    u: float
    order: str
    path: str
    draw: Draw
    ok: set  # acceptable ids


def truth(name: str) -> List[Truth]:
    """The oracle of every row of a case (computed once and kept on the case)."""
    c = case(name)
    if c._truth is None:
        out = []
        for r, row in enumerate(c.rows):
            xp = penalise(bf16_values(c.logits[r]), row.rep_pen, row.history, c.cap)
            order, path = route(xp, row.temp, row.top_k, c.cap)
            d = oracle(c.logits[r], row.temp, row.top_p, row.top_k, row.rep_pen, row.history, order, c.cap,
                       cut_eps=0.0 if row.exact else EPS)
            u = uniform(row.seed, r)
            out.append(Truth(u, order, path, d, acceptable(d, u)))
        c._truth = out
    return c._truth


# ----------------------------------------------------------------------------------- mutants
def _other(order):
    return {"sorted": "index", "index": "sorted"}.get(order, order)


def _nb(c: Case, r: int) -> Row:
    return c.rows[(r + 1) % c.R]


# name -> (case, row index, row, order) -> the token a sampler with that mistake would return
MUTANTS = {
    "top-k keeps k+1": lambda c, r, w, o: _mut(c, r, w, o, k_delta=1),
    "top-k keeps k-1": lambda c, r, w, o: _mut(c, r, w, o, k_delta=-1),
    "top-p uses <": lambda c, r, w, o: _mut(c, r, w, o, p_strict=True),
    "top-p forgets the first": lambda c, r, w, o: _mut(c, r, w, o, keep_first=False),
    "no last-three rule": lambda c, r, w, o: _mut(c, r, w, None, last_three=False),
    "penalty always divides": lambda c, r, w, o: _mut(c, r, w, None, always_divide=True),
    "penalty counts each id once": lambda c, r, w, o: _mut(c, r, w, None, count_once=True),
    "uniform without the row term": lambda c, r, w, o: _mut(c, r, w, o, u=uniform(w.seed, r, row_term=False)),
    "uniform from the neighbour's seed": lambda c, r, w, o: _mut(c, r, w, o, u=uniform(_nb(c, r).seed, r)),
    "neighbour's temperature": lambda c, r, w, o: _mut(c, r, w, None, temp=_nb(c, r).temp),
    "neighbour's top-p": lambda c, r, w, o: _mut(c, r, w, o, top_p=_nb(c, r).top_p),
    "neighbour's top-k": lambda c, r, w, o: _mut(c, r, w, None, top_k=_nb(c, r).top_k),
    "neighbour's history": lambda c, r, w, o: _mut(c, r, w, None, history=_nb(c, r).history),
    "draw order swapped": lambda c, r, w, o: _mut(c, r, w, _other(o)),
}


def mutant_applies(name: str, c: Case, r: int) -> bool:
    """False where the mistake cannot change row r's draw (saves the oracle run)."""
    w, nb = c.rows[r], _nb(c, r)
    if name == "neighbour's temperature":
        return nb.temp != w.temp
    if w.temp <= 0:
        return False
    pen = w.rep_pen != 1.0
    if name.startswith("top-k"):
        return 0 < w.top_k < c.V
    if name.startswith("top-p"):
        return 0.0 < w.top_p < 1.0
    if name in ("no last-three rule", "penalty always divides", "penalty counts each id once"):
        return pen and any(0 <= t < c.V for t in w.history)
    if name == "neighbour's history":
        return pen and nb.history != w.history
    if name == "neighbour's top-p":
        return nb.top_p != w.top_p
    if name == "neighbour's top-k":
        return nb.top_k != w.top_k
    return True


def _mut(c, r, w, order, u=None, temp=None, top_p=None, top_k=None, history=None, **flags) -> int:
    temp = w.temp if temp is None else temp
    top_k = w.top_k if top_k is None else top_k
    history = w.history if history is None else history
    if temp <= 0:
        order = "greedy"
    elif order is None or order == "greedy":  # the order the wrong sampler's own dispatch would take
        xp = penalise(bf16_values(c.logits[r]), w.rep_pen, history, c.cap, **{k: v for k, v in flags.items() if k in (
            "last_three", "always_divide", "count_once")})
        order = route(xp, temp, top_k, c.cap)[0]
    d = oracle(c.logits[r], temp, w.top_p if top_p is None else top_p, top_k, w.rep_pen, history, order, c.cap,
               cut_eps=0.0, **flags)
    return d.token(uniform(w.seed, r) if u is None else u)
