"""The packed-QKV window attention (window_attn_qkv.hip, 1..64 tokens, bf16,
D = 32) through `ops.window_attention_qkv`, against the float64 oracle of
rowops_oracle.py.

The bound is that of test_window_attn_mfma_gpu.py (derivation there): the
oracle's plus U_BF16_STORE times the first-order terms of the two operand
roundings, P in out and dv, dS in dq and dk; dbias gets no widening."""

import pytest
import torch

import rowops_oracle as ro
from test_window_attn_mfma_gpu import _reference

pytestmark = pytest.mark.gpu

from flreid_amd import ops


def _group():
    return ops.require_extension("window_attn_qkv_bwd").window_attn_qkv_group()


def _cases():                # (BW, H, N, D, nW or None)
    return [
        (9, 3, 49, 32, 4),       # production window, odd head count, one valid
                                 # row / column in the last tile, BW % nW != 0
        (2, 1, 64, 32, 1),       # four full tiles
        (3, 2, 16, 32, None),    # one tile, no mask (window 4)
        (5, 2, 36, 32, 2),       # the last tile holds exactly one key quad
        (1, 1, 1, 32, None),     # a single token
        (2 * _group() + 1, 1, 49, 32, 3),   # two full runs and a one-window
                                            # tail: idle waves in the reduction
    ]


def _pack(q, k, v):
    """[BW, H, N, D] x 3 -> [BW, N, 3·H·D], last axis (q|k|v, head, d)."""
    bw, h, n, d = q.shape
    return torch.stack((q, k, v)).permute(1, 3, 0, 2, 4).reshape(
        bw, n, 3 * h * d).contiguous()


def _run(inp, grad: bool):
    bw, h, n, d = inp.q.shape
    qkv = _pack(inp.q, inp.k, inp.v).cuda().requires_grad_(grad)
    bias = inp.bias.cuda().requires_grad_(grad)
    mask = None if inp.mask is None else inp.mask.cuda()

    def heads(t):            # [BW, N, H·D] -> [BW, H, N, D]
        return t.view(bw, n, h, d).transpose(1, 2).cpu()

    if not grad:
        with torch.no_grad():
            return {"out": heads(ops.window_attention_qkv(
                qkv, h, bias, mask, inp.scale))}
    out = ops.window_attention_qkv(qkv, h, bias, mask, inp.scale)
    out.backward(inp.do.transpose(1, 2).reshape(bw, n, h * d).cuda())
    assert out.dtype == qkv.grad.dtype == torch.bfloat16
    assert bias.grad.dtype == torch.float32
    dq, dk, dv = qkv.grad.view(bw, n, 3, h, d).permute(2, 0, 3, 1, 4).cpu()
    return {"out": heads(out.detach()), "dq": dq, "dk": dk, "dv": dv,
            "dbias": bias.grad.cpu()}


@pytest.mark.parametrize("index", range(6))
def test_window_attention_qkv_within_bound(index):
    """out by the no-grad route and by the autograd route, and the latter's
    dQ, dK, dV (unpacked from dqkv) and dbias."""
    case = _cases()[index]
    inp, ref = ro.cached(("window_qkv", case), lambda: _reference(case))
    assert ops.window_attention_qkv_route(case[2], case[3], inp.q.dtype,
                                          0.0) == "packed"
    for grad in (False, True):
        got = _run(inp, grad)
        ratios = {n: ro.worst_ratio(got[n], *ref[n]) for n in got}
        print(case, "autograd" if grad else "no-grad",
              {n: round(r, 4) for n, r in ratios.items()})
        assert all(r <= 1.0 for r in ratios.values()), (case, grad, ratios)


def test_window_attention_qkv_backward_keeps_ds_and_copies_out_of_memory():
    """The backward allocates dqkv and one [N, N] dS partial per group of
    windows: no dq / dk / dv, no restacked copy, no [BW, H, N, N] fp32 dS."""
    bw, h, n, d, _nw = case = (256, 3, 49, 32, 2)
    inp = ro.window_inputs(case, torch.bfloat16)
    qkv = _pack(inp.q, inp.k, inp.v).cuda().requires_grad_(True)
    bias = inp.bias.cuda().requires_grad_(True)
    out = ops.window_attention_qkv(qkv, h, bias, inp.mask.cuda(), inp.scale)
    do = inp.do.transpose(1, 2).reshape(bw, n, h * d).cuda().contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out.backward(do)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    limit = qkv.numel() * 2 + bw * h * n * n * 4 // 2
    print("backward peak growth", growth, "limit", limit)
    assert growth < limit
    assert bias.grad is not None and qkv.grad is not None
