"""W8A8-MX tiled MoE ops (ops.moe_quant_mx_tiled / moe_gate_up_mx_tiled / moe_down_mx_tiled) - the torch forms
CPU tensors take, against a direct fp64 computation over ops.mx_block_quant, and the executor's switch
MPAMD_MOE_TILED_MX on a CPU stage.  The kernels: tests/test_moe_tiled_mx_gpu.py.
"""
import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.ops.reference import GU_BLOCK
from src.runtime.executor import StageExecutor

from .test_moe_fp8 import _stage
from .test_moe_tiled import E, F, H, edge_routing, weights


@pytest.mark.parametrize("gather", [True, False])
def test_quantizer_torch_form_dequantizes_to_mx_block_quant_in_slot_order(gather):
    """Bytes x 2^(scale - 127), read back through the fragment and scale map, are mx_block_quant of each slot's
    rows; rows past an expert's last pair and the slots past the last block are zero bytes with scale 127."""
    idx, w = edge_routing()
    off, tok, _ = ops.moe_group(idx, w, E)
    x = torch.randn(idx.shape[0], H, generator=torch.Generator().manual_seed(1))
    x[:, :32] *= 2.0 ** 20  # blocks with their own scales
    rows = x[tok.long()]
    ax, as_ = ops.moe_quant_mx_tiled(x, off, tok) if gather else ops.moe_quant_mx_tiled(rows, off)
    S, nkb = 516 // 128 + E, H // 128
    assert ax.shape == (S, 8, nkb, 2, 64, 16) and as_.shape == (S, 2, nkb, 64, 4) and ax.dtype == as_.dtype == torch.uint8
    # ax [S, mt, kb, sh, (qh, ql, r), (sl, j)] -> [S, mt, r, kb, sh, sl, qh, ql, j]; as [S, g, kb, (sh, qh, r), i]
    q = ax.view(torch.float8_e4m3fn).float().view(S, 8, nkb, 2, 2, 2, 16, 2, 8).permute(0, 1, 6, 2, 3, 7, 4, 5, 8)
    sc = as_.view(S, 2, nkb, 2, 2, 16, 4).permute(0, 1, 6, 5, 2, 3, 4).reshape(S, 8, 16, nkb, 2, 1, 2, 1, 1)
    got = (q * torch.exp2(sc.float() - 127)).reshape(S, 128, H)
    want = torch.zeros(S, 128, H)
    for s, (p0, n) in enumerate([(0, 128), (128, 128), (256, 1), (257, 1), (258, 128), (386, 128), (514, 2)]):
        want[s, :n] = ops.mx_block_quant(rows[p0:p0 + n])
    assert torch.equal(got, want)
    assert bool((ax[7:] == 0).all()) and bool((as_[7:] == 127).all()) and bool((as_[2, :, :, 1:16] == 127).all())


def test_gemm_torch_forms_equal_fp64_over_mx_block_quant():
    gu8, gus, dn8, dns = weights()
    idx, w = edge_routing()
    T = idx.shape[0]
    off, tok, wsel = ops.moe_group(idx, w, E)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(1))
    act_in = torch.randn(2 * T, F, generator=torch.Generator().manual_seed(2))
    act = ops.moe_gate_up_mx_tiled(x, gu8, gus, off, tok)
    y = ops.moe_down_mx_tiled(act_in, dn8, dns, off, tok, wsel, idx, T)
    want_act, want_y = torch.zeros(2 * T, F, dtype=torch.float64), torch.zeros(T, H, dtype=torch.float64)
    o = off.tolist()
    for e in range(E):
        sl = slice(o[e], o[e + 1])
        gu = ops.mx_block_quant(x[tok[sl].long()]).double() @ ops.unpack_weight_w8(gu8[e], gus[e], torch.float64).t()
        g, u = gu.view(-1, F // GU_BLOCK, 2, GU_BLOCK).unbind(2)
        want_act[sl] = (g * torch.sigmoid(g) * u).reshape(-1, F)
        ye = ops.mx_block_quant(act_in[sl]).double() @ ops.unpack_weight_w8(dn8[e], dns[e], torch.float64).t()
        want_y.index_add_(0, tok[sl].long(), ye * wsel[sl, None].double())
    torch.testing.assert_close(act.double(), want_act, atol=1e-5, rtol=1e-4)  # fp32 round-off of the torch forms
    torch.testing.assert_close(y.double(), want_y, atol=1e-5, rtol=1e-4)
    assert not torch.equal(act, ops.moe_gate_up_w8_tiled(x, gu8, gus, off, tok))


def test_cpu_executor_reads_the_switch_and_keeps_dequantizing(monkeypatch):
    """A CPU stage dequantizes everywhere and never takes the tiled route, so the MX switch - which acts on the
    steps of that route only - is read and changes nothing."""
    cfg = resolve_model("tiny-mixtral")
    ids = torch.randint(0, cfg.vocab_size, (90,), generator=torch.Generator().manual_seed(1))
    calls, logits = [], []
    for name in ("moe_gate_up_mx_tiled", "moe_down_mx_tiled"):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **kw: (calls.append(_n), _f(*a, **kw))[1])
    for on in (False, True):
        if on:
            monkeypatch.setenv("MPAMD_MOE_TILED", "65")
            monkeypatch.setenv("MPAMD_MOE_TILED_MX", "1")
        ex = StageExecutor(cfg, _stage(cfg, quant_type="fp8"), "cpu", dtype=torch.float32, kv_cache_bytes=16 << 20,
                           max_sessions=4, max_seq_len=256)
        assert ex._moe_tiled_mx is on
        logits.append(ex.forward([("a", 90)], ids))
    assert not calls and torch.equal(logits[0], logits[1])
