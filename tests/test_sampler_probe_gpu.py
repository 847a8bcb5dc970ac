"""Every draw of ``ops.sample`` against the fp64 inverse-CDF oracle of tests/sampler_probe.py.

One launch per case; every row of a case has its own logits, temperature, top-p, top-k, penalty,
history and seed, and the id it returns must be one the oracle accepts: an id whose fp64 interval,
widened by EPS = 2^-14 (derived in sampler_probe.py from the fp32 roundings of the kernel's CDF),
holds the row's uniform.  The histogram tests of test_kernels_gpu.py cannot see a top-k of k + 1,
a top-p ``<``, a neighbour's parameter or a wrong penalty on a sampled row; tests/
test_sampler_probe.py shows that each of those changes at least 5 draws checked here.

Cases and the path of ``mp_sample``'s dispatch each one reaches (read from the dispatch, which
``sampler_probe.route`` mirrors; rows x history capacity):
    v50              64 x 50   LDS row, scalar loads ([:, :50] of 56 columns); k >= V -> general; k = 5: fewer non-empty wave maxima than k
    v512, v512_r1    64 x 50, 1 x 3   LDS, 16-B loads; k <= 64 fast top-k, k = 65 / 200 / 511: 64 owning threads < k -> general
    v1001            200 x 50  LDS, scalar loads ([:, 8:1009] of 1016 columns); fast top-k up to k = 1000, general
    v32000           64 x 50   LDS, 16-B loads; fast top-k, general, 2000 tied maxima -> > 1024 candidates -> general
    v32000_strided   3 x 3     the same through a [:, 8:32008] view of a 32776-wide buffer
    v34816 / v34824  3 x 50, 3 x 3   the last LDS width / the first workspace width
    v50257           64 x 50   workspace row, scalar loads, a [:, :50257] view of a 50264-wide buffer
    v65528 / v65536  3 x 50, 64 x 3  one workgroup below the split threshold / split, 8 chunks, fallback rows
    v128256          64 x 50   split, 16 chunks, short last chunk; a chunk with > 512 candidates -> fallback -> general
    v131080 (_r1)    64 x 50, 1 x 50  split, 17 chunks, 8-wide last chunk, the C > 16 merge
    v151936          3 x 3     split, 19 chunks
    v128256_cap300   3 x 300   history wider than 256: no split, one workgroup with a workspace row
In the split cases k <= 64 rows (split kernels) sit next to k = 0 / 65 / 200 / 2000 / V - 1 / V rows, which
the one-workgroup kernel draws afterwards over the split records' workspace, and greedy rows.

Measured on an MI355X, per case: draws with more than one acceptable id, and the largest distance by
which a returned id lay outside its unwidened fp64 interval (``pytest -s`` prints both as
SAMPLER_PROBE lines), next to the derived EPS = 2^-14 = 6.1e-5:
    case              ambiguous   outside        case              ambiguous   outside
    v50               1 of  64    0              v50257            0 of  64    0
    v512              0 of  64    0              v65528            0 of   3    0
    v512_r1           0 of   1    0              v65536            1 of  64    0
    v1001             2 of 200    0              v128256           1 of  64    0
    v32000            1 of  64    0              v131080           0 of  64    0
    v32000_strided    0 of   3    0              v131080_r1        0 of   1    0
    v34816            0 of   3    0              v151936           0 of   3    0
    v34824            0 of   3    0              v128256_cap300    0 of   3    0
    sample_verify: v512 0 of 64, 0; v131080 0 of 64, 0
Every one of the 668 draws (and the 128 through ``sample_verify``) lay inside its unwidened fp64 interval: none needed the EPS slack.  The first
run had one draw outside, by 0.0145 (v32000 row 2: k = 65, T = 1.5, penalty 1.2 on id 1418, logit 11.625):
the kernel's fp32 quotient 11.625 / 1.2f is exactly 9.6875, the logit of id 27700, and the index breaks that
tie in favour of 1418, while the fp64 quotient is just below 9.6875.  The kernel follows its fp32 arithmetic
(as ``reference.sample_row`` does); the oracle now takes both orders of such a near-tie (TIE_TOL).
"""
import functools

import numpy as np
import pytest
import torch

from src import ops
from tests import sampler_probe as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Device tensors of a case: the logits (through the case's strided view), the per-row parameters
    and the histories inside a [R + 2, cap] tensor whose first and last row are sentinels."""
    c = sp.case(name)
    R, V, cap = c.R, c.V, c.cap
    if c.buf_width:
        buf = torch.full((R, c.buf_width), float("nan"), dtype=torch.bfloat16, device=DEV)  # NaN around the view
        logits = buf[:, c.buf_off:c.buf_off + V]
        logits.copy_(c.logits)
        assert not logits.is_contiguous()
    else:
        logits = c.logits.to(DEV)
    assert logits.data_ptr() % 16 == 0 and logits.stride(0) % 8 == 0
    rec = np.full((R + 2, cap), SENTINEL, dtype=np.int32)
    ln = np.full(R + 2, SENTINEL, dtype=np.int32)
    for r, w in enumerate(c.rows):
        rec[r + 1, :len(w.history)] = w.history
        ln[r + 1] = len(w.history)
    par = (_dev([w.temp for w in c.rows], np.float32), _dev([w.top_p for w in c.rows], np.float32),
           _dev([w.top_k for w in c.rows], np.int32), _dev([w.rep_pen for w in c.rows], np.float32))
    return logits, par, rec, ln, _dev([w.seed for w in c.rows], np.int64)


def _check_ids(name, got, what):
    """Every id is acceptable; returns (ambiguous draws, largest distance outside the fp64 interval)."""
    c, tr = sp.case(name), sp.truth(name)
    bad, worst = [], 0.0
    for r, (t, tok) in enumerate(zip(tr, got)):
        if tok not in t.ok:
            w = c.rows[r]
            bad.append(f"row {r}: got {tok}, acceptable {sorted(t.ok)[:8]}, u={t.u!r} T={w.temp} p={w.top_p} k={w.top_k} "
                       f"rp={w.rep_pen} hist={w.history[-6:]} {t.path} {w.note}; outside by {sp.outside(t.draw, t.u, tok)}")
        elif not (t.u >= 1.0 - sp.EPS and tok == t.draw.top):  # (the end-of-range fallback has no interval)
            worst = max(worst, sp.outside(t.draw, t.u, tok))
    amb = sum(len(t.ok) > 1 for t in tr)
    print(f"\nSAMPLER_PROBE {what:24s} {name:16s} ambiguous {amb:3d} of {len(tr):3d}  outside <= {worst:.3e}", end="")
    assert not bad, f"{name} ({what}): {len(bad)} of {len(tr)} draws not acceptable\n" + "\n".join(bad[:12])
    assert worst <= sp.EPS


@pytest.mark.parametrize("name", sp.CASE_NAMES)
def test_every_draw_is_acceptable(name):
    c = sp.case(name)
    R, cap = c.R, c.cap
    logits, par, rec, ln, seeds = _inputs(name)
    # without the history update: histories and sentinels untouched
    recent, rlen = torch.from_numpy(rec).to(DEV), torch.from_numpy(ln).to(DEV)
    out = ops.sample(logits, *par, recent[1:R + 1], rlen[1:R + 1], seeds)
    got = out.cpu().tolist()
    assert np.array_equal(recent.cpu().numpy(), rec) and np.array_equal(rlen.cpu().numpy(), ln)
    _check_ids(name, got, "sample")
    # with it, on fresh copies: the same ids, each appended to its row, a full row drops its oldest id
    recent, rlen = torch.from_numpy(rec).to(DEV), torch.from_numpy(ln).to(DEV)
    out2 = ops.sample(logits, *par, recent[1:R + 1], rlen[1:R + 1], seeds, update_history=True)
    assert out2.cpu().tolist() == got
    want_rec, want_ln = rec.copy(), ln.copy()
    for r, w in enumerate(c.rows):
        h = (w.history + [got[r]])[-cap:]
        want_rec[r + 1, :len(h)] = h
        want_ln[r + 1] = min(len(w.history) + 1, cap)
    assert np.array_equal(rlen.cpu().numpy(), want_ln)
    assert np.array_equal(recent.cpu().numpy(), want_rec)  # slots past a row's length and the sentinel rows too
    if c.buf_width:  # the launch wrote nothing around the view
        buf = logits._base if logits._base is not None else logits
        assert torch.equal(logits.cpu(), c.logits)
        assert buf.isnan().sum().item() == R * (c.buf_width - c.V)


@pytest.mark.parametrize("name", sp.VERIFY_CASES)
def test_sample_verify_draws_are_acceptable(name):
    """The same rows as one-row sessions without drafts: ``sample_verify``'s expanded seeds must give
    session s the uniform of launch row s, and its own tests only tie it to ``ops.sample``."""
    c = sp.case(name)
    R = c.R
    logits, par, rec, ln, seeds = _inputs(name)
    recent, rlen = torch.from_numpy(rec).to(DEV), torch.from_numpy(ln).to(DEV)
    tokens, count = ops.sample_verify(logits, _dev(np.arange(R + 1), np.int32), _dev(np.full(R, -1), np.int32), *par,
                                      recent[1:R + 1], rlen[1:R + 1], seeds)
    assert count.cpu().tolist() == [1] * R
    assert np.array_equal(recent.cpu().numpy(), rec) and np.array_equal(rlen.cpu().numpy(), ln)
    _check_ids(name, tokens.cpu().tolist(), "sample_verify")


def test_binding_refuses_unaligned_rows():
    c = sp.case("v32000_strided")
    _, par, rec, ln, seeds = _inputs(c.name)
    recent, rlen = torch.from_numpy(rec[1:4].copy()).to(DEV), torch.from_numpy(ln[1:4].copy()).to(DEV)
    buf = torch.zeros(3, 1008, dtype=torch.bfloat16, device=DEV)
    ops.sample(buf[:, 8:1000], *par, recent, rlen, seeds)  # 16-B aligned base, stride a multiple of 8
    with pytest.raises(RuntimeError, match="16-B aligned"):
        ops.sample(buf[:, 1:1001], *par, recent, rlen, seeds)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.sample(torch.zeros(3, 1001, dtype=torch.bfloat16, device=DEV), *par, recent, rlen, seeds)
