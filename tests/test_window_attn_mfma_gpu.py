"""The MFMA window attention (window_attn_mfma.hip, 65..144 tokens, bf16,
D = 32) through `ops.window_attention`, against the float64 oracle of
rowops_oracle.py.

The bound is the oracle's plus the first-order cost of the two operand
roundings the kernel's design has: P is rounded to bf16 as the operand of
P V and P^T dO, dS as the operand of dS K and dS^T Q.  U_BF16_STORE = 2^-8
covers a 2^-9 rounding with the oracle's usual factor 2.  dbias is summed
from the unrounded fp32 dS and gets no widening."""

import numpy as np
import pytest
import torch

import rowops_oracle as ro

pytestmark = pytest.mark.gpu

from flreid_amd import ops

CASES = [                    # (BW, H, N, D, nW or None)
    (9, 2, 144, 32, 4),      # full tiles, odd tile count, BW % nW != 0, one
                             # window past a group of 8
    (3, 1, 81, 32, None),    # ws 9: one valid row / column in the last tile
    (5, 2, 100, 32, 2),      # ws 10, short group
    (2, 1, 65, 32, 1),       # first N past the VALU limit
    (17, 1, 80, 32, 3),      # exactly five tiles; groups of 8, 8 and 1
    (1, 1, 121, 32, 1),      # ws 11, single window
]


def _reference(case):
    """-> (inputs, {name: (ref64, widened bound)})."""
    inp = ro.window_inputs(case, torch.bfloat16)
    ref = ro.window_reference(inp)
    q, k, v, do = (t.double() for t in (inp.q, inp.k, inp.v, inp.do))
    scale = float(np.float32(inp.scale))
    s = scale * (q @ k.transpose(-1, -2)) + inp.bias.double()
    if inp.mask is not None:
        w = torch.arange(q.shape[0]) % inp.mask.shape[0]
        s = s + inp.mask.double()[w].unsqueeze(1)
    p = torch.softmax(s, -1)
    dp = do @ v.transpose(-1, -2)
    ds = (p * (dp - (dp * p).sum(-1, keepdim=True))).abs()
    extra = {"out": p @ v.abs(),
             "dv": p.transpose(-1, -2) @ do.abs(),
             "dq": scale * (ds @ k.abs()),
             "dk": scale * (ds.transpose(-1, -2) @ q.abs()),
             "dbias": 0.0}
    return inp, {name: (r, b + ro.U_BF16_STORE * extra[name])
                 for name, (r, b) in ref.items()}


def _run(inp, grad: bool):
    q, k, v = (t.cuda().requires_grad_(grad) for t in (inp.q, inp.k, inp.v))
    bias = inp.bias.cuda().requires_grad_(grad)
    mask = None if inp.mask is None else inp.mask.cuda()
    if not grad:
        with torch.no_grad():
            return {"out": ops.window_attention(q, k, v, bias, mask,
                                                inp.scale).cpu()}
    out = ops.window_attention(q, k, v, bias, mask, inp.scale)
    out.backward(inp.do.cuda())
    got = {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad,
           "dbias": bias.grad}
    for name in ("out", "dq", "dk", "dv"):
        assert got[name].dtype == torch.bfloat16, name
    assert got["dbias"].dtype == torch.float32
    return {name: t.cpu() for name, t in got.items()}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_window_attention_mfma_within_bound(case):
    """out by the no-grad route and by the autograd route, and the latter's
    dQ, dK, dV and dbias."""
    inp, ref = ro.cached(("window_mfma", case), lambda: _reference(case))
    assert ops.window_attention_route(case[2], case[3], inp.q.dtype,
                                      0.0) == "mfma"
    for grad in (False, True):
        got = _run(inp, grad)
        ratios = {n: ro.worst_ratio(got[n], *ref[n]) for n in got}
        print(case, "autograd" if grad else "no-grad",
              {n: round(r, 4) for n, r in ratios.items()})
        assert all(r <= 1.0 for r in ratios.values()), (case, grad, ratios)


def test_window_attention_mfma_backward_keeps_ds_out_of_memory():
    """The backward allocates the three gradients, a dO copy and one [N, N]
    dS partial per group of windows: less than a [BW, H, N, N] fp32 dS."""
    bw, h, n, d, _nw = case = (128, 1, 144, 32, 2)
    inp = ro.window_inputs(case, torch.bfloat16)
    q, k, v = (t.cuda().requires_grad_(True) for t in (inp.q, inp.k, inp.v))
    bias = inp.bias.cuda().requires_grad_(True)
    out = ops.window_attention(q, k, v, bias, inp.mask.cuda(), inp.scale)
    do = inp.do.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out.backward(do)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("backward peak growth", growth, "of", bw * h * n * n * 4)
    assert growth < bw * h * n * n * 4
    assert bias.grad is not None and q.grad is not None
