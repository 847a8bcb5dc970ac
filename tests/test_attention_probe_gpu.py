"""Closed-form probes (tests/attn_probe.py) through every attention entry point at the boundaries of
its tiling: unlike the randn comparisons of test_kernels_gpu.py these tell WHICH keys a kernel read.
A lost key, a visible key past the context, a key counted twice, a wrong (m, l) combine across
split-K slices or a stale cache slot read for the new token each move a probed channel by >= 0.083;
the comparator allows 2^-6 = 0.0156 (derived in attn_probe.py: bf16 output + bf16 P), absolute.

Boundaries probed, per kernel (every context of a case sits in ONE launch):
* flash-decoding kernel (``paged_attention``, bf16 and fp8 cache; 4 shapes): contexts 1, 2, 63, 64,
  65, 129, 257, 1000, 4097; keys 0, 1, TPI - 1, TPI, 31 .. 257 around every power of two, PS - 1,
  PS, PS + 1, the start of the last slice +- 1, n - 2, n - 1, the trap n; pairs across (0, n - 1),
  (63, 64), every slice end, (n - 2, n - 1); partitions default / 64 / 128 / 256 / 2048; the
  in-launch combine and the reduce kernel; packed output; q_ctx below what the cache holds, through
  the same partitions and combines (its heads continue the probe list of the plain case).
* ``paged_attention_rope`` (bf16 and fp8) and ``attention_mfma_rope``: contexts 1, 64, 65, 129, 257,
  1000 (token ctx - 1 in the first, a middle and the last slice, and on a page's first slot), single
  n - 1, pairs (0, n - 1) and (n - 2, n - 1), identity and quarter-turn rotary tables, a stale trap
  in the new token's slot, the caches after the launch bit for bit.
* ``attention_mfma``: GQA decode blocks on the contexts above (one slice, 128- and 256-token slices,
  the default, packed), the one-block and the grouped (superblock) prefill kernels on chunked
  prompts: rows 0, 1, 15, 16, 17, 31, 32, 33, 63, 64 and the last; keys c - 1 (diagonal), c - 2,
  0, the multiples of 16 / 32 / 64 below c and those - 1; the trap is the chunk's next token; NaN
  after the last token (the "tokens past the context are zeroed" claim).
* ``attention_fa``: 4 and 8 waves; the context in 1, 2 (the op's own split) and 3 parts; causal block
  pairing on the unsplit form, blocks of two sequences in one workgroup included; probe rows at the
  32-row wave, the workgroup block and the 64-token step boundaries; the same keys (the multiple of 64 is the first
  key of the last step; key 0 with background after it and key c - 1 with background before it are
  the two directions of the lazy rescale).

Largest |out - closed form| measured on an MI355X over all probes of all cases, next to the derived
bound 2^-6 = 0.015625 (``pytest -s`` prints them again as PROBE_DEV lines):
    paged_attention (reduce kernel and in-launch combine), bf16 and fp8 cache   0.003795
    paged_attention_rope, bf16 and fp8 cache                                    0.003795
    attention_mfma_rope                                                         0.003795
    attention_mfma: GQA decode, one-block prefill, grouped prefill              0.003795
    attention_fa                                                                0.008328
0.003795 is the bf16 rounding of the output alone (a weighted pair's value between 1 and 2); the FA
kernel adds the bf16 rounding of P in the numerator against an unrounded row sum l."""
import functools
import math

import pytest
import torch

from src import ops
from tests import attn_probe as ap

pytestmark = pytest.mark.gpu
DEV = "cuda"

_SEEN = {}  # kernel -> largest deviation from the closed form in this run


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"
    yield
    for k, v in sorted(_SEEN.items()):
        print(f"\nPROBE_DEV {k} {v:.6f}", end="")


def _note(kernel, dev):
    _SEEN[kernel] = max(_SEEN.get(kernel, 0.0), dev)


@functools.lru_cache(maxsize=None)
def _decode(nh, nkv, D, short=False):
    return ap.decode_case(nh, nkv, D, rows=3 if nh <= 16 else 2, short_ctx=short)


@functools.lru_cache(maxsize=None)
def _rope(nh, nkv, D, quarter):
    return ap.rope_case(nh, nkv, D, quarter=quarter)


@functools.lru_cache(maxsize=None)
def _prefill(nh, nkv, D, ntoks, prefix, fa):
    rows = ap.PREFILL_ROWS
    if fa:  # wave (32 rows), workgroup block (4 / 8 waves) and 64-token step boundaries first
        tpw = 32 // (nh // nkv)
        rows = [0, 1]
        for m in (4, 8, 1, 2):
            rows += [m * tpw - 1, m * tpw]
        for n, pre in zip(ntoks, prefix):
            rows += [j for j in range(n) if (pre + j + 1) % 64 in (0, 1)]
    return ap.prefill_case(nh, nkv, D, list(ntoks), list(prefix), row_idx=tuple(rows))


@functools.lru_cache(maxsize=None)
def _f8(case_fn, *key):
    return case_fn(*key).f8(DEV)


def _args(a):
    return a["q"], a["k_cache"], a["v_cache"], a["block_tables"], a["q_seq"], a["q_ctx"]


def _unpack(out, case, packed):
    return ops.unpack_act(out, case.T, case.nh * case.D) if packed else out


FD_SHAPES = [(8, 2, 128), (32, 8, 128), (12, 12, 64), (8, 2, 64)]


def _run_flash_decoding(case, kc, vc, f8, inlaunch, monkeypatch):
    """Every partition (the op's default, then 64 / 128 / 256 / 2048-token slices; 128 packed)."""
    nh, nkv = case.nh, case.nkv
    a = case.to(DEV)
    q, _, _, bt, q_seq, q_ctx = _args(a)
    if not f8:
        kc, vc = a["k_cache"], a["v_cache"]
    monkeypatch.setattr(ops, "ATTN_INLAUNCH_REDUCE", inlaunch)
    parts = ap.decode_partitions(case.T, nkv, max(ap.DECODE_CTXS))
    assert parts[0] == tuple(ops.attention_partition(case.T, nkv, int(q_ctx.max())))
    what = f"paged_attention{'_f8' if f8 else ''} {'in-launch' if inlaunch else 'reduce'}"
    for ps, np_ in [("default", 0)] + parts:
        if np_ == 0:  # chosen by the op itself
            out = ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, case.scale)
        else:
            packed = ps == 128
            out = _unpack(ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, case.scale, part_size=ps,
                                              num_parts=np_, packed=packed), case, packed)
        _note(what, ap.compare(out, case, f"{what} part {ps} x {np_}"))
    if inlaunch:
        assert int(ops.attention_counters(DEV).abs().sum()) == 0


@pytest.mark.parametrize("nh,nkv,D", FD_SHAPES)
@pytest.mark.parametrize("f8", [False, True])
@pytest.mark.parametrize("inlaunch", [False, True])
def test_flash_decoding_probes(nh, nkv, D, f8, inlaunch, monkeypatch):
    kc, vc = _f8(_decode, nh, nkv, D) if f8 else (None, None)
    _run_flash_decoding(_decode(nh, nkv, D), kc, vc, f8, inlaunch, monkeypatch)


@pytest.mark.parametrize("nh,nkv,D", FD_SHAPES)
@pytest.mark.parametrize("f8", [False, True])
@pytest.mark.parametrize("inlaunch", [False, True])
def test_flash_decoding_ctx_below_cache(nh, nkv, D, f8, inlaunch, monkeypatch):
    """Prefill-as-decode: q_ctx = n of a cache that holds 2 n + 70 tokens, the trap is real later data.
    Its heads go on in the probe list where the plain case stopped, over the same partitions."""
    kc, vc = _f8(_decode, nh, nkv, D, True) if f8 else (None, None)
    _run_flash_decoding(_decode(nh, nkv, D, True), kc, vc, f8, inlaunch, monkeypatch)


def _check_cache_after(case, kc, vc, f8):
    """The new token's slot holds the new k / v bit for bit, every other slot is unchanged (the
    poison included)."""
    ka, va = (kc.dequant(), vc.dequant()) if f8 else (kc, vc)
    ok = ~case.poison[:, None, :, None].expand_as(case.k_after)
    for got, want, name in ((ka.cpu(), case.k_after, "k"), (va.cpu(), case.v_after, "v")):
        assert torch.equal(got[ok], want[ok]), f"{name} cache after the launch"
        assert got[~ok].isnan().all(), f"{name} cache: a poisoned slot was written"
    if f8:
        pz = case.poison[:, None, :].expand_as(kc.scales.cpu())
        for c in (kc, vc):
            assert (c.codes.cpu()[pz] == 0xFF).all() and (c.scales.cpu()[pz] == 0xFF).all()


@pytest.mark.parametrize("nh,nkv,D", FD_SHAPES)
@pytest.mark.parametrize("f8", [False, True])
@pytest.mark.parametrize("quarter,parts,inlaunch", [(False, None, False), (False, (64, 16), False), (False, (64, 16), True),
                                                    (False, (256, 4), False), (False, (128, 8), True),
                                                    (True, (64, 16), False), (True, None, False)])
def test_paged_attention_rope_probes(nh, nkv, D, f8, quarter, parts, inlaunch, monkeypatch):
    case = _rope(nh, nkv, D, quarter)
    a = case.to(DEV)
    q, kc, vc, bt, q_seq, q_ctx = _args(a)
    if f8:
        kc, vc = (ops.KVF8(c.codes.clone(), c.scales.clone()) for c in _f8(_rope, nh, nkv, D, quarter))
    monkeypatch.setattr(ops, "ATTN_INLAUNCH_REDUCE", inlaunch)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else {}
    out = ops.paged_attention_rope(q, kc, vc, bt, q_seq, q_ctx, a["positions"], a["cos"], a["sin"], a["slots"], nh,
                                   nkv, case.scale, **kw)
    what = f"paged_attention_rope{'_f8' if f8 else ''}"
    _note(what, ap.compare(out, case, f"{what} {parts} quarter={quarter} inlaunch={inlaunch}"))
    assert torch.equal(q.cpu(), case.q), "the fused op must not modify qkv"
    _check_cache_after(case, kc, vc, f8)
    if inlaunch:
        assert int(ops.attention_counters(DEV).abs().sum()) == 0


MFMA_SHAPES = [(32, 8, 128), (16, 4, 128), (12, 12, 64)]


@pytest.mark.parametrize("nh,nkv,D", MFMA_SHAPES)
@pytest.mark.parametrize("quarter,parts", [(False, None), (False, (128, 8)), (False, (256, 4)), (True, None),
                                           (True, (128, 8))])
def test_attention_mfma_rope_probes(nh, nkv, D, quarter, parts):
    case = _rope(nh, nkv, D, quarter)
    a = case.to(DEV)
    q, kc, vc, bt, q_seq, q_ctx = _args(a)
    qb = torch.from_numpy(ops.query_blocks([1] * case.T, nh // nkv)).to(DEV)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else {}
    out = ops.attention_mfma_rope(q, kc, vc, bt, q_seq, q_ctx, qb, a["positions"], a["cos"], a["sin"], a["slots"],
                                  nh, nkv, case.scale, **kw)
    _note("attention_mfma_rope", ap.compare(out, case, f"attention_mfma_rope {parts} quarter={quarter}"))
    assert torch.equal(q.cpu(), case.q), "the fused op must not modify qkv"
    _check_cache_after(case, kc, vc, False)


@pytest.mark.parametrize("nh,nkv,D", MFMA_SHAPES)
def test_attention_mfma_decode_probes(nh, nkv, D):
    case = _decode(nh, nkv, D)
    a = case.to(DEV)
    q, kc, vc, bt, q_seq, q_ctx = _args(a)
    qb = torch.from_numpy(ops.query_blocks([1] * case.T, nh // nkv)).to(DEV)
    n = max(ap.DECODE_CTXS)
    for kw in ({}, dict(part_size=128 * math.ceil(n / 128), num_parts=1), dict(part_size=128, num_parts=math.ceil(n / 128)),
               dict(part_size=256, num_parts=math.ceil(n / 256)),
               dict(part_size=256, num_parts=math.ceil(n / 256), packed=True)):
        out = _unpack(ops.attention_mfma(q, kc, vc, bt, q_seq, q_ctx, qb, nh, nkv, case.scale, **kw), case,
                      kw.get("packed", False))
        _note("attention_mfma decode", ap.compare(out, case, f"attention_mfma decode {kw}"))


PREFILLS = [((130,), (0,)), ((300, 17), (64, 5)), ((64,), (200,))]


@pytest.mark.parametrize("nh,nkv,D", MFMA_SHAPES)
@pytest.mark.parametrize("ntoks,prefix", PREFILLS)
@pytest.mark.parametrize("split", [False, True])
def test_attention_mfma_prefill_probes(nh, nkv, D, ntoks, prefix, split):
    case = _prefill(nh, nkv, D, ntoks, prefix, False)
    a = case.to(DEV)
    qb = torch.from_numpy(ops.query_blocks(ntoks, nh // nkv)).to(DEV)
    sb = torch.from_numpy(ops.query_superblocks(ntoks, nh // nkv)).to(DEV)
    ctx = max(p + n for p, n in zip(prefix, ntoks))
    kw = dict(part_size=128, num_parts=math.ceil(ctx / 128)) if split else {}
    out = ops.attention_mfma(*_args(a), qb, nh, nkv, case.scale, superblocks=sb, **kw)
    _note("attention_mfma grouped prefill", ap.compare(out, case, f"grouped prefill {kw}"))
    out = ops.attention_mfma(*_args(a), qb, nh, nkv, case.scale, **kw)
    _note("attention_mfma prefill", ap.compare(out, case, f"one-block prefill {kw}"))


@pytest.mark.parametrize("nh,nkv", [(32, 8), (8, 4), (32, 32)])
@pytest.mark.parametrize("ntoks,prefix", [((130,), (0,)), ((129, 256), (0, 63)), ((300,), (64,))])
@pytest.mark.parametrize("waves,parts,pair", [(4, 1, False), (8, 1, False), (4, None, False), (8, None, False),
                                             (4, 3, False), (8, 3, False), (4, 1, True), (8, 1, True)])
def test_attention_fa_probes(nh, nkv, ntoks, prefix, waves, parts, pair):
    """``parts`` 1: the whole context in one part (up to six 64-token steps of the lazy rescale), the only
    form that pairs blocks - with ``pair`` every prompt but the 8-wave 130-token MHA one has >= 2 blocks,
    and ([129, 256], [0, 63]) pairs blocks of different sequences.  None: the op's own split (1 part for
    the 130-token prompt, 2 for the others).  3: three parts."""
    D = 128
    case = _prefill(nh, nkv, D, ntoks, prefix, True)
    a = case.to(DEV)
    fb = torch.from_numpy(ops.fa_blocks(ntoks, nh // nkv, waves)).to(DEV)
    if pair:
        assert parts == 1 and (fb.shape[1] >= 2 or (waves, nh // nkv, ntoks) == (8, 1, (130,)))
    out = ops.attention_fa(*_args(a), fb, nh, nkv, case.scale, waves=waves, num_parts=parts, pair=pair)
    _note("attention_fa", ap.compare(out, case, f"attention_fa waves={waves} parts={parts} pair={pair}"))
