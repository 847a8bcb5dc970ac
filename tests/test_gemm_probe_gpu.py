"""Exact decode-GEMM probes on the GPU (tests/gemm_probe.py: small-integer inputs whose result every
kernel form must reproduce bit for bit, whatever its summation order).

1. every case of ``shape_set`` through ``ops.linear`` (form forced with ``set_gemm_sk``), ``linear_w8``
   (``_W8_MODE``) and ``linear_w4``: two launches bit-identical to each other and to the expected bits; a
   forced form that does not cover a shape falls back and must still be exact; a shape no kernel of a
   weight type covers must raise (a missing kernel is an error, never a quiet detour);
2. NaN in the padding rows of the packed activation changes nothing (bf16, W8A16, W4A16, MX, W8A8);
3. stores stay inside the output: a sentinel frame around a row-major view, a sentinel tail and
   sentinel padding rows around a packed SwiGLU output;
4. the workspace's control words (arrival counters, zero fragment) are zero after every launch that
   uses it;
5. the grouped MoE kernels on exact inputs: down + combine bit-equal under general top-2 routing,
   E = 1 and E = 32, nothing routed, NaN in everything an unrouted expert owns.

What the project's dispatch makes of some of the cases (``which`` says it per case, from the dry-run
predicates; the tallies are printed):

* the packed activation layout has no place for half a 32-column group, so a fused-norm producer or
  a packed SwiGLU output with an odd column-tile count is rejected by the ops
  (``test_packed_copies_need_whole_32_column_groups``); those edges run with one tile more;
* fp8 and fp4 weights have no second kernel to fall back to: a column split the ring form is not
  built for (5 wide, 6 with a remainder, SwiGLU 10) raises, and the test asserts that it does;
* K = 192 is no multiple of the decode GEMMs' 128-deep groups: ``ops.linear`` takes it row-major on
  the hipBLASLt path (still exact); the shared-A forms' odd group count runs at K = 384;
* 129..256 rows with the plain epilogue reach the tiled form only where its split-K variant applies
  too (N % 1024 == 0, K >= 256); elsewhere ``ops.linear`` raises for a packed activation;
* the SwiGLU outputs met the derived one-ulp bound everywhere: no bound had to be recorded.
"""
import collections
import functools

import pytest
import torch

from src import ops
from tests import gemm_probe as gp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
NAN = float("nan")  # (one object: a key of the lru_caches below)
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
SPECS = gp.shape_set(CUS)
GROUPS = list(dict.fromkeys((s.group, s.wt, s.kern) for s in SPECS))
FORMS = [("bf16", k) for k in gp.BF16_FORMS] + [("w8", k) for k in gp.W8_FORMS] + [("w4", "rw")]
# csrc/gemm_kernels.h: the workspace starts with SK_MAX_GROUPS arrival counters and SK_ZERO_BYTES of zeros
# (the stream-K slabs and, from gemm_slab_offset() on, the split-K slabs follow: scratch, never cleared)
WS_CONTROL_BYTES = 4 * (1 << 15) + 4096
NO_KERNEL = "no fp8-weight kernel covers|no MXFP4-weight kernel covers|need the native decode GEMM"


@functools.lru_cache(maxsize=None)
def dev_weights(wt, N, K, glu):
    return gp.device_weights(gp.weights(N, K, glu), wt, DEV)


@functools.lru_cache(maxsize=None)
def dev_case(M, N, K, epi, pad=0.0):
    c = gp.case(M, N, K, epi)
    return c, gp.device_case(c, DEV, pad)


def operands(s, pad=0.0):
    c, dc = dev_case(s.M, s.N, s.K, s.epi, pad)
    return c, dc, dev_weights(s.wt, s.N, s.K, s.epi == 1)


def _inlaunch(M, N, K, fp8):
    """Sufficient for the in-launch combine of ``rwki``: it needs column groups >= 2 tiles wide, and the
    grid (tiles / width) x splits is at most one workgroup per CU."""
    return (N // 16) * ops.rwk_split(M, N, K, fp8) > CUS


def which(s):
    """The kernel a spec really runs, from the project's dry-run predicates: a form name, "pk" (the
    fallback of the bf16 forms), "sk?" (stream-K or its fallback: not decidable from outside),
    "hipblaslt" (row-major x no decode GEMM takes) or None (nothing covers it: the op raises)."""
    M, N, K, e = s.M, s.N, s.K, s.epi
    tiles = N // 16
    if s.wt == "w4":
        return "w4" if ops.w4_gemm_ok(M, N, K, e) else None
    base = ops._base(s.kern)
    if s.wt == "w8":
        if base in ("rwk", "rwki") and e != 1 and N % 2048 == 0 and ops.rwk_split(M, N, K, True) >= 2:
            return "rwki" if base == "rwki" and _inlaunch(M, N, K, True) else "rwk"
        return "rw" if gp.rw_built(N, e, CUS, fp8=True) else None
    if not ops.native_gemm_ok(M, N, K, e, s.packed):
        return "hipblaslt" if s.rowmajor and not s.packed and e != 3 else None
    if s.kern == "auto":
        if ops.t2d_rows(M) and ops.t2d_ok(M, N, K, e, s.packed):
            return "t2d"
        if not s.packed and ops._covered("rwk", M, N, K, e) and ops.rwk_split(M, N, K) >= 2:
            return "rwk"
        assert torch.ops.mpamd.gemm_rw_ok(M, N, K, e, int(s.packed)), s
        return "rw"
    if base == "pk" or not ops._covered(s.kern, M, N, K, e):
        return "pk"
    if base == "sk":
        return "sk" if tiles % 4 == 0 and K // 32 >= 32 else "sk?"
    if base == "rw":
        return "rw" if gp.rw_built(N, e, CUS) else "pk"
    if base in ("rwk", "rwki"):
        if ops.rwk_split(M, N, K) < 2:
            return "pk"
        return "rwki" if base == "rwki" and _inlaunch(M, N, K, False) else "rwk"
    if base == "rwr":
        return "rwr" if CUS % 16 == 0 and (2 * tiles) % CUS == 0 and 2 * tiles // CUS in (1, 2, 4) else "pk"
    return base  # the shared-A forms: ops._covered is the launcher's own condition


def uses_workspace(s):
    return s.kern == "auto" or ops._base(s.kern) in ("sk", "rwk", "rwki")


def assert_workspace_clean(what):
    ws = ops.gemm_workspace(DEV)
    assert int(torch.ops.mpamd.gemm_slab_offset()) > WS_CONTROL_BYTES
    assert int(ws[:WS_CONTROL_BYTES].view(torch.int32).abs().sum()) == 0, f"{what}: counters / zero fragment not zero"


def same_bits(s, c, r1, r2):
    assert torch.equal(gp.rows_of(s, c, r1["y"]), gp.rows_of(s, c, r2["y"])), f"{s.id}: two launches differ"
    if c.epi == 3:
        assert torch.equal(r1["ap"], r2["ap"]) and torch.equal(r1["sso"].sum(0), r2["sso"].sum(0)), s.id


# ------------------------------------------------------------------------------------ 1. exact probes
@pytest.mark.parametrize("group,wt,kern", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_exact_probes(group, wt, kern):
    tally = collections.Counter()
    for s in SPECS:
        if (s.group, s.wt, s.kern) != (group, wt, kern):
            continue
        c, dc, dw = operands(s)
        k = which(s)
        tally[str(k)] += 1
        if k is None:
            with pytest.raises(RuntimeError, match=NO_KERNEL):
                gp.run(s, c, dc, dw)
            continue
        r1 = gp.run(s, c, dc, dw)
        if uses_workspace(s):
            assert_workspace_clean(s.id)
        r2 = gp.run(s, c, dc, dw)
        if uses_workspace(s):
            assert_workspace_clean(s.id)
        gp.check(s, c, dc, r1)
        same_bits(s, c, r1, r2)
    label = "w4" if wt == "w4" else ops._base(kern)
    ran = sum(v for k_, v in tally.items() if k_ == label or (kern == "auto" and k_ != "None"))
    print(f"{group} {wt} {kern}: {sum(tally.values())} cases, forced form ran in {ran}; by kernel {dict(tally)}")


def test_one_flipped_weight_is_noticed_on_exactly_its_column():
    """Control: the comparison is live on the GPU path - one weight of 2048 x 1152 with the other sign
    moves every row's sum in that column by 2 * 2^-j, and nothing else."""
    s = gp.Spec("control", "bf16", "rw", 17, 2048, 1152, 0)
    c, dc, _ = operands(s)
    w = c.w.bf16.clone()
    w[777, 1000] = -w[777, 1000]
    with gp.forced(s):
        y = ops.linear(dc["xp"], None, wp=ops.pack_weight(w.to(DEV)), a_rows=s.M)
    bad = gp.rejected(y, dc["expected"])
    assert int(bad.sum()) == s.M and bool(bad[:, 777].all())
    with pytest.raises(AssertionError, match="17 of 34816 elements rejected"):
        gp.compare(y, dc["expected"], None, s.id)


def test_every_form_really_runs_for_each_epilogue_it_takes():
    """Guards against a fallback quietly making this file test ``pk``: per form name and epilogue, at
    least one case where the dry-run predicates say the form itself ran."""
    ran = collections.Counter((s.wt, s.kern, s.epi, which(s)) for s in SPECS)
    cases = collections.Counter((s.wt, s.kern) for s in SPECS)
    for wt, name in FORMS:
        base = ops._base(name)
        epis = {"bf16": gp.FORM_EPIS, "w8": gp.W8_FORM_EPIS}[wt][base] if wt != "w4" else gp.W4_EPIS
        label = "w4" if wt == "w4" else base
        n = sum(v for (w, k, e, l), v in ran.items() if (w, k) == (wt, name) and l == label)
        print(f"{wt} {name}: {cases[(wt, name)]} cases, the form ran in {n}")
        for e in epis:
            assert ran[(wt, name, e, label)] > 0, f"{wt} {name} epilogue {e}: no case where it really runs"
    wide = collections.Counter((which(s), s.epi) for s in SPECS if s.kern == "auto")
    print(f"wide rows: {dict(wide)}")
    for s in SPECS:
        if s.kern == "auto":
            print(f"wide M={s.M} N={s.N} K={s.K} epilogue {s.epi}: {which(s)}")
    assert wide[("t2d", 0)] and wide[("t2d", 1)] and wide[("rw", 0)] and wide[("rw", 1)]
    # the first K at which the split-K ring splits N = 2048 is one of the split-K group's
    for fp8 in (False, True):
        first = next(K for K in range(128, 4097, 128) if ops.rwk_split(64, 2048, K, fp8) >= 2)
        print(f"rwk_split(64, 2048, K, fp8={fp8}) first reaches 2 at K = {first} (S = {ops.rwk_split(64, 2048, first, fp8)})")
        assert first in {s.K for s in SPECS if s.group == "splitk"}


def test_the_ring_width_table_matches_the_launchers_dry_run():
    """``gp.rw_built`` (which column-split cases the ring form really runs) against the exported dry run
    of the same launcher at 65 rows, for every plain / packed-SwiGLU column count of the set."""
    for N, e in sorted({(s.N, s.epi) for s in SPECS if s.group == "colsplit" and s.epi in (0, 1)}):
        if e == 1 and (N // 2) % 32:
            continue
        assert gp.rw_built(N, e, CUS) == bool(torch.ops.mpamd.gemm_rw_ok(65, N, 128, e, int(e == 1))), (N, e)


# ------------------------------------------------------------------------------------ 2. padding rows
PAD_MS = (1, 13, 17, 50)
PAD_WIDE = (70, 100, 130, 200)


@pytest.mark.parametrize("wt,kern", FORMS + [("bf16", "auto")], ids=[f"{w}-{k}" for w, k in FORMS] + ["bf16-auto"])
def test_nan_in_the_padding_rows_changes_nothing(wt, kern):
    N, K = 2048, 1024
    for M in (PAD_WIDE if kern == "auto" else PAD_MS):
        s = gp.Spec("pad", wt, kern, M, N, K, 0)
        c, dz, dw = operands(s)
        _, dn, _ = operands(s, NAN)
        assert bool(gp.ref.unpack_act(dn["xp"], 16 * ((M + 15) // 16), K)[M:].isnan().all())
        y0, y1 = gp.run(s, c, dz, dw)["y"], gp.run(s, c, dn, dw)["y"]
        assert bool(torch.isfinite(y1.float()).all()), f"{s.id}: a padding row was read"
        assert torch.equal(y0, y1), s.id
        gp.compare(y1, dz["expected"], None, s.id)


def test_nan_in_the_padding_rows_changes_nothing_mx_and_w8a8():
    N, K = 2048, 1024
    assert ops.fp8_gemm_ok(64, N, K)
    w8, scale = dev_weights("w8", N, K, False)["w8"]
    wq = ops.fp8_from_w8(w8).contiguous()
    for M in PAD_MS:
        c, dz = dev_case(M, N, K, 0)
        _, dn = dev_case(M, N, K, 0, NAN)
        ys = [ops.linear_mx(*ops.quant_mx(d["xp"], M, K), w8, scale, M) for d in (dz, dn)]
        assert bool(torch.isfinite(ys[1].float()).all()) and torch.equal(ys[0], ys[1]), f"MX M={M}"
        gp.compare(ys[1], dz["expected"], None, f"MX M={M}")  # +-1 is exact as MX e4m3 too
        prev = ops._FP8_MODE
        try:
            for kind in ("auto", "pk", "rw", "rwk"):
                ops.set_fp8_kernel(kind)
                ys = [ops.linear_fp8(*ops.quant_act_fp8(d["xp"], M, K), wq, scale, M) for d in (dz, dn)]
                assert bool(torch.isfinite(ys[1].float()).all()) and torch.equal(ys[0], ys[1]), f"W8A8 {kind} M={M}"
        finally:
            ops.set_fp8_kernel(prev)


# ------------------------------------------------------------------------------------ 3. stores
def _framed(M, N):
    buf = torch.full((M + 2, N + 16), SENT, dtype=torch.bfloat16, device=DEV)
    return buf, buf[1:M + 1, :N]


def _frame_intact(buf, M, N):
    b = buf.clone()
    b[1:M + 1, :N] = SENT
    return bool((b == SENT).all())


@pytest.mark.parametrize("wt,kern", FORMS + [("bf16", "auto")], ids=[f"{w}-{k}" for w, k in FORMS] + ["bf16-auto"])
def test_stores_stay_inside_the_output(wt, kern):
    wide = kern == "auto"
    table = gp.WIDE_EPIS if wide else gp.W4_EPIS if wt == "w4" else \
        {"bf16": gp.FORM_EPIS, "w8": gp.W8_FORM_EPIS}[wt][ops._base(kern)]
    done = collections.Counter()
    for N, K in ((32, 128), (16 * (CUS + 2), 128), (2048, 1024)):
        for M in ((65, 200) if wide else (1, 17, 64)):
            for e in (x for x in table if x != 1):  # row-major: a view of a sentinel-filled [M + 2, N + 16] buffer
                s = gp.Spec("store", wt, kern, M, N, K, e)
                if which(s) is None:
                    continue
                c, dc, dw = operands(s)
                buf, view = _framed(M, N)
                if e == 3:
                    view.copy_(dc["res"])
                    plain = gp.run(s, c, dc, dw)
                    r = gp.run(s, c, dc, dw, res=view)
                    same_bits(s, c, plain, r)
                else:
                    plain = gp.run(s, c, dc, dw)
                    r = gp.run(s, c, dc, dw, out=view)
                    assert r["y"].data_ptr() == view.data_ptr()
                assert torch.equal(view, plain["y"]), s.id
                assert _frame_intact(buf, M, N), f"{s.id}: a store outside the [M, N] view"
                gp.check(s, c, dc, r)
                done[which(s)] += 1
            if 1 not in table:
                continue
            # packed SwiGLU: packed_numel(M, F) + 1024 sentinel elements, F = N
            s = gp.Spec("store", wt, kern, M, 2 * N, K, 1, True)
            if which(s) is None:
                continue
            c, dc, dw = operands(s)
            n = ops.packed_numel(M, N)
            buf = torch.full((n + 1024,), SENT, dtype=torch.bfloat16, device=DEV)
            plain = gp.run(s, c, dc, dw)
            r = gp.run(s, c, dc, dw, out=buf)
            assert bool((buf[n:] == SENT).all()), f"{s.id}: a store past the packed output"
            assert bool((ops.unpack_act(buf, 16 * ((M + 15) // 16), N)[M:] == SENT).all()), f"{s.id}: padding rows stored"
            assert torch.equal(gp.rows_of(s, c, buf), gp.rows_of(s, c, plain["y"])), s.id
            gp.check(s, c, dc, r)
            done[which(s)] += 1
    print(f"{wt} {kern}: {dict(done)}")
    assert sum(done.values()) > 0


def test_packed_copies_need_whole_32_column_groups():
    """The packed layout has no place for half a 32-column group: the ops reject a fused-norm producer
    or a packed SwiGLU output with an odd column-tile count instead of storing past the buffer."""
    M, K = 17, 128
    c, dc, dw = operands(gp.Spec("reject", "bf16", "rw", M, 48, K, 2))
    ap = torch.zeros(ops.packed_numel(M, 48), dtype=torch.bfloat16, device=DEV)
    ss = ops.norm_stats_buffer(DEV)[0]
    with pytest.raises(RuntimeError, match="ap: the packed copy needs N % 32 == 0"):
        ops.linear(dc["xp"], None, wp=dw["wp"], a_rows=M, epilogue=3, out=dc["res"].clone(), residual=dc["res"].clone(),
                   ap_out=ap, ss_out=ss, ss_zero=ss.clone())
    dw = dev_weights("bf16", 96, K, True)
    out = torch.zeros(ops.packed_numel(M, 48) + 1024, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="packed y: the packed output needs N / 2 % 32 == 0"):
        torch.ops.mpamd.gemm(dc["xp"], dw["wp"], out, None, 1, M, 3, None, None, None, None, None, None, 1.0 / K, 0.0)
    assert int(out.abs().sum()) == 0


# ------------------------------------------------------------------------------------ 5. grouped MoE
MOE_SHAPES = [(256, 128, 4), (128, 1152, 8), (6144, 128, 4)]
MOE_EDGES = [(256, 256, 1, None), (256, 256, 32, (0, 31))]
MOE_MS = (1, 17, 64)


def _moe_dev(c):
    return dict(w8=c.w8.to(DEV), scale=c.scale.to(DEV), cnt=c.cnt.to(DEV), wd=c.wd.to(DEV))


def _down(H, F, E, M, routed=None):
    assert ops.moe_w8_ok(M, E, H, F)
    c = gp.moe_case("down", M, H, F, E, routed)
    d = _moe_dev(c)
    act = gp.moe_act(c).to(DEV)
    buf, view = _framed(M, H)
    ys = [ops.moe_down_w8(act, d["w8"], d["scale"], d["cnt"], d["wd"], M, out=o) for o in (None, view)]
    gp.compare(ys[0], c.expected.to(DEV), None, f"down H={H} F={F} E={E} M={M} routed {c.cnt.tolist()}")
    assert torch.equal(ys[0], ys[1]) and _frame_intact(buf, M, H)
    return c, ys[0]


def _gate_up(H, F, E, M, routed=None):
    assert ops.moe_w8_ok(M, E, H, F)
    c = gp.moe_case("gate_up", M, H, F, E, routed)
    d = _moe_dev(c)
    xp = gp.ref.pack_act(c.x).to(DEV)
    slab = ops.packed_numel(M, F)
    acts = []
    for _ in range(2):
        act = torch.full((E * slab + 1024,), SENT, dtype=torch.bfloat16, device=DEV)
        ops.moe_gate_up_w8(xp, d["w8"], d["scale"], d["cnt"], M, out=act)
        acts.append(act)
    assert torch.equal(acts[0], acts[1])
    act = acts[0]
    assert bool((act[E * slab:] == SENT).all()), "a store past the last slab"
    for e in range(E):
        got = act[e * slab:(e + 1) * slab]
        if int(c.cnt[e]) > 0:
            gp.compare(ops.unpack_act(got, M, F), c.expected[e].to(DEV), c.u_zero[e].to(DEV),
                       f"gate/up H={H} F={F} E={E} M={M} expert {e}")
            assert bool((ops.unpack_act(got, 16 * ((M + 15) // 16), F)[M:] == SENT).all()), f"expert {e}: padding rows stored"
        else:
            assert bool((got == SENT).all()), f"unrouted expert {e} was written"
    return c


@pytest.mark.parametrize("M", MOE_MS)
@pytest.mark.parametrize("H,F,E", MOE_SHAPES)
def test_moe_down_with_general_routing_is_bit_exact(H, F, E, M):
    c, _ = _down(H, F, E, M)
    assert int((c.cnt > 0).sum()) >= 2 and bool(((c.wd > 0).sum(1) == 2).all())


@pytest.mark.parametrize("M", MOE_MS)
@pytest.mark.parametrize("H,F,E", MOE_SHAPES)
def test_moe_gate_up_meets_the_swiglu_expectation(H, F, E, M):
    _gate_up(H, F, E, M)


@pytest.mark.parametrize("M", MOE_MS)
@pytest.mark.parametrize("H,F,E,routed", MOE_EDGES)
def test_moe_with_one_expert_and_with_the_first_and_last_of_32(H, F, E, routed, M):
    c, _ = _down(H, F, E, M, routed)
    assert [e for e in range(E) if int(c.cnt[e]) > 0] == list(routed or range(E))
    _gate_up(H, F, E, M, routed)


@pytest.mark.parametrize("M", MOE_MS)
def test_moe_with_nothing_routed(M):
    """``cnt`` all zero, every weight, scale and activation slab NaN: down returns exact zeros, gate/up
    leaves every slab at its sentinel."""
    for H, F, E in ((256, 128, 4), (256, 256, 32)):
        c, y = _down(H, F, E, M, ())
        assert int(c.cnt.sum()) == 0 and bool(c.scale.isnan().all()) and bool((y == 0).all())
        _gate_up(H, F, E, M, ())
