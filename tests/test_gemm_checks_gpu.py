"""Host-side argument checks of the decode GEMM ops (ops/csrc/bindings.cpp): ``gemm``, ``gemm_w8``,
``gemm_w4`` and ``gemm_mx`` each reject one bad argument at a time with the message the op has always
raised, before any kernel is launched; one valid call per op gives the bits of ``ops.linear*``.

The rejections use M = 16, N = 32, K = 256, the smallest shape every check accepts (the row-count
rules need their own buffers for 65 rows, the W4 SwiGLU rule a 16-column weight).  The valid calls use
the smallest shapes the launchers cover: the one-group bf16 kernel at that shape, the W8A16 ring at
1024 x 1024, the MXFP4 ring at 256 x 512 and the MX split-K ring at 2048 x 2048."""
import re

import pytest
import torch

from src import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, N, K = 16, 32, 256


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device=DEV)


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8, device=DEV)


def _args(op, M=M, N=N, K=K):
    """Valid keyword arguments of ``torch.ops.mpamd.<op>`` (epilogue 0, packed activation)."""
    a = dict(y=_bf(M, N), residual=None, epilogue=0, M=M, flags=1, ap=None, ss_out=None, ss_zero=None, ss_in=None,
             inv_k=1.0 / K, eps=0.0)
    if op == "gemm":
        a.update(x=_bf(ops.packed_numel(M, K)), wp=_bf(N // 16, K // 32, 64, 8), workspace=None, gate=None)
    elif op == "gemm_w8":
        a.update(x=_bf(ops.packed_numel(M, K)), wq=_u8(N // 16, K // 32, 64, 8),
                 wsc=torch.ones(N, dtype=torch.float32, device=DEV), workspace=None, flags=1 | 128)
    elif op == "gemm_w4":
        a.update(x=_bf(ops.packed_numel(M, K)), w4=_u8(N // 16, K // 128, 64, 16), s4=_u8(N // 16, K // 128, 16, 4))
    else:
        a.update(ax=_u8(ops.packed_numel(M, K)), as_=_u8(2 * K), wq=_u8(N // 16, K // 32, 64, 8),
                 wsc=torch.ones(N, dtype=torch.float32, device=DEV), workspace=ops.gemm_workspace(DEV),
                 flags=1 | 256)
    return a


def _short_workspace():
    return _u8(int(torch.ops.mpamd.gemm_workspace_bytes()) - 1)


def _epi3(a, **kw):
    """Epilogue-3 arguments: the residual stream (also the output) and its packed copy."""
    res = _bf(a["M"], a["y"].shape[1])
    return dict(epilogue=3, y=res, residual=res, ap=_bf(ops.packed_numel(a["M"], res.shape[1])), **kw)


X = {"gemm": "x", "gemm_w8": "x", "gemm_w4": "x", "gemm_mx": "ax"}
X_SHORT = {"gemm": "packed x too small", "gemm_w8": "packed x too small", "gemm_w4": "packed x too small",
           "gemm_mx": "ax size"}
EPI3_NO_AP = {"gemm": "epilogue 3 needs ap (and ss_out outside ablations)",
              "gemm_w8": "epilogue 3 needs residual and ap", "gemm_w4": "epilogue 3 needs residual and ap",
              "gemm_mx": "epilogue 3 needs residual and ap"}
WEIGHT = {"gemm": ("wp", "wp must be a packed weight [N/16, K/32, 64, 8] (ops.pack_weight)"),
          "gemm_w8": ("wq", "wq must be an fp8 weight uint8 [N/16, K/32, 64, 8] (ops.pack_weight_w8)"),
          "gemm_w4": ("w4", "w4 must be an MXFP4 weight uint8 [N/16, K/128, 64, 16] (ops.pack_weight_w4)"),
          "gemm_mx": ("wq", "wq must be an fp8 weight uint8 [N/16, K/32, 64, 8] (ops.pack_weight_w8)")}


def _bad_cases(op):
    """(message, changed arguments) pairs: each violates exactly one check of ``op``."""
    a = _args(op)
    x, (wname, wmsg) = X[op], WEIGHT[op]
    cases = [
        ("y shape", dict(y=_bf(M - 1, N))),
        (X_SHORT[op], {x: a[x][:-1]}),
        ("residual shape", dict(residual=_bf(M - 1, N))),
        ("ap: packed [ceil(M/16)*16*N]", dict(ap=_bf(2 * ops.packed_numel(M, N))[::2])),
        ("ap: packed [ceil(M/16)*16*N]", dict(ap=_bf(ops.packed_numel(M, N) - 1))),
        (EPI3_NO_AP[op], _epi3(a) | dict(ap=None)),
        (wmsg, {wname: a[wname].view(N // 16, -1, 32, 16)}),
    ]
    if op != "gemm_w4":
        cases.append(("gemm workspace too small (ops.gemm_workspace)", dict(workspace=_short_workspace())))
    if op in ("gemm_w8", "gemm_mx"):
        cases.append(("wsc: fp32 [N] column scales", dict(wsc=a["wsc"][:-1])))
    if op in ("gemm", "gemm_w8", "gemm_w4"):  # the packed (SwiGLU) output
        cases += [("packed y", dict(flags=a["flags"] | 2, y=_bf(ops.packed_numel(M, N)))),
                  ("packed y", dict(flags=a["flags"] | 2, epilogue=1, y=_bf(ops.packed_numel(M, N // 2) - 1)))]
    if op == "gemm":
        cases += [("residual epilogue needs residual", dict(epilogue=2)),
                  ("epilogue", dict(epilogue=4, residual=_bf(M, N)))]
    else:  # the op-named rules
        big = _args(op, M=65)
        if op == "gemm_mx":
            rows = "gemm_mx: 1 <= M <= 64, K % 128 == 0"
            cases.append(("gemm_mx: epilogue 0 or 3", dict(epilogue=2, residual=_bf(M, N))))
        else:
            rows = f"{op}: 0 <= M <= 64"
            cases.append((f"{op}: epilogue 0, 3 or packed SwiGLU", dict(epilogue=2, residual=_bf(M, N))))
        cases.append((rows, big))
    if op == "gemm_w4":
        n16 = _args(op, N=16)
        cases += [("s4 must be the e8m0 block scales uint8 [N/16, K/128, 16, 4] (ops.pack_weight_w4)",
                   dict(s4=a["s4"].view(N // 16, -1, 8, 8))),
                  ("gemm_w4: SwiGLU needs N % 32 == 0",
                   n16 | dict(epilogue=1, flags=3, y=_bf(ops.packed_numel(M, 8))))]
    return cases


@pytest.mark.parametrize("op", ["gemm", "gemm_w8", "gemm_w4", "gemm_mx"])
def test_one_bad_argument_is_rejected_with_its_message(op):
    ops.require_native()
    fn = getattr(torch.ops.mpamd, op)
    for msg, change in _bad_cases(op):
        with pytest.raises(RuntimeError, match=re.escape("mpamd: " + msg) + r"(\n|$)"):
            fn(**(_args(op) | change))


def test_launcher_return_codes_before_any_launch():
    """Calls that pass every binding check and are refused by the launchers (``mp_gemm_*``) before a
    kernel is launched: each keeps its return code, which the op raises as it always has."""
    ops.require_native()
    ws = ops.gemm_workspace(DEV)
    partials = 1 | 256 | 16384  # packed A | split-K ring | partial slabs only
    wide = dict(y=_bf(M, 1024), workspace=ws, flags=partials)
    cases = [
        # a row-major x: only the packed-activation kernels are built
        ("gemm", dict(x=_bf(M, K), flags=0), "gemm launch failed with code -4"),
        # SwiGLU over an odd number of column tiles (N = 48: three)
        ("gemm", _args("gemm", N=48) | dict(epilogue=1, y=_bf(M, 24)), "gemm launch failed with code -2"),
        # N = 1024 has no split-K geometry, and nothing else writes partial slabs
        ("gemm", _args("gemm", N=1024) | wide, "gemm launch failed with code -6"),
        ("gemm_w8", _args("gemm_w8", N=1024) | wide, "gemm_w8 launch failed with code -6"),
        # K = 64 is no multiple of the 128 a wave group walks
        ("gemm", _args("gemm", K=64), "gemm launch failed with code -1"),
        ("gemm_mx", _args("gemm_mx", N=1024), "gemm_mx: no split-K geometry for M=16 N=1024 K=256"),
    ]
    for op, change, msg in cases:
        with pytest.raises(RuntimeError, match=re.escape("mpamd: " + msg) + r"(\n|$)"):
            getattr(torch.ops.mpamd, op)(**(_args(op) | change))


def _operands(n, k):
    torch.manual_seed(n + k)
    x = torch.randn(M, k, device=DEV).to(torch.bfloat16)
    w = torch.randn(n, k, device=DEV) * 0.02
    return ops.pack_act(x), w


def test_gemm_valid_call_equals_linear():
    xp, w = _operands(N, K)
    wp = ops.pack_weight(w.to(torch.bfloat16))
    ops.set_gemm_sk("off")  # the one-group kernel: flags = packed activation only, no workspace
    a = _args("gemm") | dict(x=xp, wp=wp)
    torch.ops.mpamd.gemm(**a)
    assert torch.equal(a["y"], ops.linear(xp, None, wp=wp, a_rows=M))


def test_gemm_w8_valid_call_equals_linear_w8(monkeypatch):
    n = k = 1024
    xp, w = _operands(n, k)
    wq, wsc = ops.pack_weight_fp8(w)
    w8 = ops.w8_from_fp8(wq)
    monkeypatch.setattr(ops, "_W8_MODE", "rw")  # flags = packed activation | ring
    a = _args("gemm_w8", N=n, K=k) | dict(x=xp, wq=w8, wsc=wsc)
    torch.ops.mpamd.gemm_w8(**a)
    assert torch.equal(a["y"], ops.linear_w8(xp, w8, wsc, M))


def test_gemm_w4_valid_call_equals_linear_w4():
    n, k = 256, 512
    xp, w = _operands(n, k)
    w4, s4 = ops.pack_weight_w4(w)
    a = _args("gemm_w4", N=n, K=k) | dict(x=xp, w4=w4, s4=s4)
    torch.ops.mpamd.gemm_w4(**a)
    assert torch.equal(a["y"], ops.linear_w4(xp, w4, s4, M))


def test_gemm_mx_valid_call_equals_linear_mx():
    n = k = 2048
    xp, w = _operands(n, k)
    wq, wsc = ops.pack_weight_fp8(w)
    w8 = ops.w8_from_fp8(wq)
    ax, as_ = ops.quant_mx(xp, M, k)
    a = _args("gemm_mx", N=n, K=k) | dict(ax=ax, as_=as_, wq=w8, wsc=wsc)
    torch.ops.mpamd.gemm_mx(**a)
    assert torch.equal(a["y"], ops.linear_mx(ax, as_, w8, wsc, M))
