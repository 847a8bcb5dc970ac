"""Every decode kernel whose argument list was reordered for kernarg preload (docs/KERNARG_PRELOAD.md),
at the smallest shapes that still tell a misplaced argument.

GEMMs: the exact small-integer probes of tests/gemm_probe.py (their own comparators: bit equality,
one bf16 ulp for SwiGLU) with M in {1, 17, 64}, every form forced through ``ops.set_gemm_sk`` as the
candidate tests do, each plain and with the rotated k walk (``+r``: a non-zero ``rot``).  M, N, K, the
split count and the strides all differ, so a swapped pair of them moves whole tiles.

* balanced ring (``rw``): N 1024 x K 512 with epilogues 0, 1 (packed SwiGLU) and 3; one workgroup per
  column tile there, so the same three epilogues also run at 16 (C + 1) columns (C + 1 gate / up pairs for
  SwiGLU), which splits into two widths (2 / 1, SwiGLU 4 / 2): ``n_big`` matters;
* split-K ring: N 2048 x K 512, as partials only (``ops.linear_partials``, summed here), with the reduce
  launch (``rwk``) and with the in-launch combine (``rwki``), epilogues 0, 2 and 3;
* row-split ring (``rwr``): N 4096 x K 256 (the packed activation has twice the kernel's row tiles);
* shared-A form (the lm_head kernel): N 2064 x K 256, a ragged last tile: no shared-A geometry divides 129
  tiles, so the launch falls to the one-group kernel (also reordered); the shared-A kernel itself runs the
  same probe at N 2048;
* stream-K: N 2048 x K 1024.

Attention: T = 3 sessions of contexts {1, 63, 130}, D 128, ``nh`` 4 with ``nkv`` 4 and 2, pages of 16 and
64 tokens, a block table wider than the pages in use, bf16 and fp8 cache, window 0 and 48, one and two
context slices; the plain kernel, the fused RoPE + KV write and the folded qkv partial slabs, against
``ops.reference`` on the CPU at the attention tolerance of the existing tests (2e-2), and the new token's
K / V in its page slot after the RoPE forms.  The GQA MFMA decode kernel runs the same case at ``nh`` 16.
"""
import functools
import math

import pytest
import torch

from src import ops
from src.ops import reference as ref
from tests import gemm_probe as gp

pytestmark = pytest.mark.gpu
DEV = "cuda"
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
MS = (1, 17, 64)


# ------------------------------------------------------------------------------------ GEMMs
@functools.lru_cache(maxsize=None)
def _weights(N, K, glu):
    return gp.device_weights(gp.weights(N, K, glu), "bf16", DEV)


@functools.lru_cache(maxsize=None)
def _case(M, N, K, epi):
    c = gp.case(M, N, K, epi)
    return c, gp.device_case(c, DEV)


def _probe(kern, M, N, K, epi, packed=False):
    s = gp.Spec("kernarg", "bf16", kern, M, N, K, epi, packed)
    c, dc = _case(M, N, K, epi)
    r = gp.run(s, c, dc, _weights(N, K, epi == 1))
    gp.check(s, c, dc, r)


def _rw_runs(N, epi):
    """The balanced ring form is built for this column split (else the launch falls back)."""
    return gp.rw_built(N, epi, CUS)


@pytest.mark.parametrize("rot", ["", "+r"])
@pytest.mark.parametrize("M", MS)
def test_balanced_ring(M, rot):
    two_widths = 16 * (CUS + 1)
    for N in (1024, two_widths):
        for epi, packed in ((0, False), (1, True), (3, False)):
            n = 2 * N if epi == 1 else N          # SwiGLU: N output columns = 2 N weight rows
            if epi == 3 and n % 32:
                n += 16                            # the producer's packed copy lives in 32-column groups
            if packed and (n // 2) % 32:
                n += 32
            assert _rw_runs(n, epi), (n, epi)
            _probe("rw" + rot, M, n, 512, epi, packed)
    G, ntb, rem = gp.rw_width(two_widths, 0, CUS)
    assert rem and rem != G, "two widths: n_big workgroups of ntb tiles, the rest one narrower"


@pytest.mark.parametrize("rot", ["", "+r"])
@pytest.mark.parametrize("M", MS)
def test_split_k_ring(M, rot):
    N, K = 2048, 512
    S = ops.rwk_split(M, N, K)
    assert S >= 2, S
    for kern in ("rwk", "rwki"):
        for epi in (0, 2, 3):
            _probe(kern + rot, M, N, K, epi)
    # partials only: the fp32 slabs sum (exactly: small integers) to the expected bits
    c, dc = _case(M, N, K, 0)
    part = ops.linear_partials(dc["xp"], M, wp=_weights(N, K, False)["wp"], rot=bool(rot))
    assert part.shape == (S, M, N)
    gp.compare(part.sum(0).to(gp.BF), dc["expected"], None, f"partials M{M}{rot}")


@pytest.mark.parametrize("rot", ["", "+r"])
@pytest.mark.parametrize("M", MS)
def test_row_split_ring(M, rot):
    for epi in (0, 2, 3):
        _probe("rwr" + rot, M, 4096, 256, epi)   # (M = 1: one row tile does not split, the launch falls back)


@pytest.mark.parametrize("rot", ["", "+r"])
@pytest.mark.parametrize("M", MS)
def test_shared_a_and_one_group_forms(M, rot):
    for kern in ("lds22", "lds24", "lds42"):
        _probe(kern + rot, M, 2064, 256, 0)      # ragged: 129 tiles -> the one-group kernel
        for epi in (0, 1, 3):
            _probe(kern + rot, M, 4096 if epi == 1 else 2048, 256, epi)
    _probe("pk" + rot, M, 2064, 256, 0)
    _probe("pk" + rot, M, 2064 + 16, 256, 3)


@pytest.mark.parametrize("M", MS)
def test_stream_k(M):
    for epi in (0, 1, 3):
        _probe("sk", M, 4096 if epi == 1 else 2048, 1024, epi)


# ------------------------------------------------------------------------------------ attention
CTXS = (1, 63, 130)
D = 128
TOL = dict(atol=2e-2, rtol=2e-2)   # the attention tolerance of test_kernels_gpu.py / test_attention_window_gpu.py


@functools.lru_cache(maxsize=None)
def _attn_case(nh, nkv, page, seed=0):
    """Random caches with shuffled pages; the block table has 3 columns more than any session uses (they
    point at a real page full of large values, as does everything past a session's last page)."""
    g = torch.Generator().manual_seed(seed + 17 * nkv + page)
    npg = [math.ceil(c / page) for c in CTXS]
    P = sum(npg) + 2
    perm = torch.randperm(P, generator=g).tolist()
    kc = torch.randn(P, nkv, page, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(P, nkv, page, D, generator=g).to(torch.bfloat16)
    kc[perm[-1]] = 8.0
    vc[perm[-1]] = 100.0
    bt = torch.full((len(CTXS), max(npg) + 3), perm[-1], dtype=torch.int32)
    used, slots = 0, []
    for i, n in enumerate(npg):
        bt[i, :n] = torch.tensor(perm[used:used + n], dtype=torch.int32)
        slots.append(int(bt[i, (CTXS[i] - 1) // page]) * page + (CTXS[i] - 1) % page)
        used += n
    qkv = torch.randn(len(CTXS), (nh + 2 * nkv) * D, generator=g).to(torch.bfloat16)
    q_ctx = torch.tensor(CTXS, dtype=torch.int32)
    cos, sin = ops.rope_cos_sin(D, max(CTXS) + 1, 10000.0, "cpu")
    return dict(qkv=qkv, kc=kc, vc=vc, bt=bt, q_seq=torch.arange(len(CTXS), dtype=torch.int32), q_ctx=q_ctx,
                pos=q_ctx.long() - 1, slots=torch.tensor(slots, dtype=torch.int64), cos=cos.float(), sin=sin.float())


def _caches(c, f8, dev):
    if f8:
        k, v = ops.KVF8.from_dense(c["kc"]), ops.KVF8.from_dense(c["vc"])
        return ops.KVF8(k.codes.to(dev), k.scales.to(dev)), ops.KVF8(v.codes.to(dev), v.scales.to(dev))
    return c["kc"].clone().to(dev), c["vc"].clone().to(dev)


def _dense(cache, f8):
    return (cache.dequant() if f8 else cache).float().cpu()


def _reference(c, nh, nkv, f8, rope, window):
    """(expected output, expected K cache, expected V cache) from ops.reference on the CPU."""
    kr, vr = _caches(c, f8, "cpu")
    q = c["qkv"].clone()
    if rope:
        (ref.rope_kv_write_f8 if f8 else ref.rope_kv_write)(q, c["pos"], c["cos"], c["sin"], kr, vr, c["slots"], nh, nkv)
    want = (ref.paged_attention_f8 if f8 else ref.paged_attention)(q, kr, vr, c["bt"], c["q_seq"], c["q_ctx"], nh, nkv,
                                                                   1 / math.sqrt(D), window=window)
    return want.float(), _dense(kr, f8), _dense(vr, f8)


def _check_caches(c, kc, vc, k_want, v_want, f8, what):
    """Every slot but the new tokens' is bit for bit what it was; the new token's V is exact (bf16: a copy;
    fp8: the row quantizer is exact arithmetic) and its rotated K within the attention tolerance, or for
    the fp8 cache within one e4m3 step (2^-3 relative: a last-bit difference of the bf16 rotation can move
    a code by one) of the reference's."""
    page = c["kc"].shape[2]
    new = torch.zeros(c["kc"].shape, dtype=torch.bool)
    for s in c["slots"].tolist():
        new[s // page, :, s % page, :] = True
    k_got, v_got = _dense(kc, f8), _dense(vc, f8)
    assert torch.equal(k_got[~new], k_want[~new]) and torch.equal(v_got[~new], v_want[~new]), f"{what}: old slots"
    assert torch.equal(v_got[new], v_want[new]), f"{what}: new token's V"
    torch.testing.assert_close(k_got[new], k_want[new], atol=2e-2, rtol=2.0 ** -3 if f8 else 2e-2,
                               msg=lambda m: f"{what}: new token's K: {m}")


def _fold_slabs(qkv):
    """Two fp32 split-K slabs that sum to ``qkv`` exactly (1/4 and 3/4 of a bf16 value are fp32 values,
    and so is their sum): the fold must give the RoPE form's result on ``qkv``."""
    x = qkv.float()
    return torch.stack([0.25 * x, 0.75 * x]).contiguous()


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("nkv", [4, 2])
def test_flash_decoding_kernel(nkv, page, f8):
    nh = 4
    c = _attn_case(nh, nkv, page)
    d = {k: v.to(DEV) for k, v in c.items()}
    meta = (d["bt"], d["q_seq"], d["q_ctx"])
    ropeargs = (d["pos"], d["cos"], d["sin"], d["slots"])
    sc = 1 / math.sqrt(D)
    assert d["bt"].shape[1] == math.ceil(max(CTXS) / page) + 3
    for window in (0, 48):
        for ps, np_ in ((192, 1), (128, 2)):
            kw = dict(part_size=ps, num_parts=np_, max_ctx=max(CTXS), window=window)
            what = f"nkv{nkv} page{page} f8={f8} window{window} parts {ps}x{np_}"
            want, _, _ = _reference(c, nh, nkv, f8, False, window)
            kc, vc = _caches(c, f8, DEV)
            out = ops.paged_attention(d["qkv"], kc, vc, *meta, nh, nkv, sc, **kw)
            torch.testing.assert_close(out.float().cpu(), want, msg=lambda m: f"plain {what}: {m}", **TOL)
            want, k_want, v_want = _reference(c, nh, nkv, f8, True, window)
            for form in ("rope", "fold"):
                kc, vc = _caches(c, f8, DEV)
                if form == "fold":
                    qkv = torch.full_like(d["qkv"], float("nan"))   # never read on the fold path
                    part = (_fold_slabs(d["qkv"]), None, 1.0, 0.0)
                else:
                    qkv, part = d["qkv"], None
                out = ops.paged_attention_rope(qkv, kc, vc, *meta, *ropeargs, nh, nkv, sc, qkv_part=part, **kw)
                torch.testing.assert_close(out.float().cpu(), want, msg=lambda m: f"{form} {what}: {m}", **TOL)
                # the new token's K / V landed in its page slot, and nowhere else
                _check_caches(c, kc, vc, k_want, v_want, f8, f"{form} {what}")


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page", [32, 64])
def test_mfma_decode_kernel(page, f8):
    """The GQA MFMA decode kernel (heads per kv head >= 4; pages of a multiple of 32 tokens; slices of a
    multiple of 128)."""
    nh, nkv = 16, 4
    c = _attn_case(nh, nkv, page)
    d = {k: v.to(DEV) for k, v in c.items()}
    meta = (d["bt"], d["q_seq"], d["q_ctx"])
    ropeargs = (d["pos"], d["cos"], d["sin"], d["slots"])
    qb = torch.from_numpy(ops.query_blocks([1] * len(CTXS), nh // nkv)).to(DEV)
    sc = 1 / math.sqrt(D)
    plain = ops.attention_mfma_f8 if f8 else ops.attention_mfma
    fused = ops.attention_mfma_rope_f8 if f8 else ops.attention_mfma_rope
    for window in (0, 48):
        for ps, np_ in ((256, 1), (128, 2)):
            kw = dict(part_size=ps, num_parts=np_, max_ctx=max(CTXS), window=window)
            what = f"mfma page{page} f8={f8} window{window} parts {ps}x{np_}"
            want, _, _ = _reference(c, nh, nkv, f8, False, window)
            kc, vc = _caches(c, f8, DEV)
            out = plain(d["qkv"], kc, vc, *meta, qb, nh, nkv, sc, **kw)
            torch.testing.assert_close(out.float().cpu(), want, msg=lambda m: f"plain {what}: {m}", **TOL)
            want, k_want, v_want = _reference(c, nh, nkv, f8, True, window)
            kc, vc = _caches(c, f8, DEV)
            out = fused(d["qkv"], kc, vc, *meta, qb, *ropeargs, nh, nkv, sc, **kw)
            torch.testing.assert_close(out.float().cpu(), want, msg=lambda m: f"rope {what}: {m}", **TOL)
            _check_caches(c, kc, vc, k_want, v_want, f8, f"rope {what}")
