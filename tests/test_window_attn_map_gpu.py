"""The map-addressed shifted-window attention (window_attn_map.hip, windows
of up to 64 tokens, bf16, D = 32) through `ops.shifted_window_attention_qkv`,
against the float64 oracle of rowops_oracle.py on window-order inputs.

The inputs are drawn in window order, brought to the feature map with
window_reverse + roll(+shift), and the results brought back with roll(-shift)
+ window_partition, so the kernel's addressing and its in-register shift mask
are checked against the model's own partition and `_build_mask` formula.  The
bound is that of test_window_attn_mfma_gpu.py (derivation there)."""

import numpy as np
import pytest
import torch

import rowops_oracle as ro

pytestmark = pytest.mark.gpu

from flreid_amd import ops
from flreid_amd.models.swin import window_partition, window_reverse

CASES = [                    # (B, Hi, Wi, ws, shift, H)
    (2, 14, 14, 7, 3, 3),    # production window: the four label patterns,
                             # ragged last tile, odd heads, second image base
    (1, 14, 21, 7, 3, 1),    # Hi != Wi: swapped strides or nWy / nWx
    (2, 14, 14, 7, 0, 2),    # unshifted instances: no mask, no wrap
    (3, 8, 8, 4, 2, 2),      # NT = 1; 12 windows: a full run across an image
                             # boundary and a 4-window tail
    (1, 16, 8, 8, 4, 1),     # NT = 4 full tiles; Wi == ws: a window that is
                             # first and last column and wraps inside itself
    (2, 12, 18, 6, 3, 1),    # NT = 3: the zero tile of an odd NT, with labels
    (1, 7, 7, 7, 0, 1),      # the map is one window (stage 3)
]


def _swin_mask(hi, wi, ws, shift):
    """SwinBlock._build_mask for an (hi, wi) map."""
    if shift == 0:
        return None
    img = torch.zeros(1, hi, wi, 1)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    windows = window_partition(img, ws).squeeze(-1)          # [nW, N]
    diff = windows.unsqueeze(1) - windows.unsqueeze(2)
    return diff.masked_fill(diff != 0, -100.0).masked_fill(diff == 0, 0.0)


def _reference(case):
    """-> (inputs, {name: (ref64, widened bound)}), in window order."""
    b, hi, wi, ws, shift, h = case
    nw = (hi // ws) * (wi // ws)
    inp = ro.window_inputs((b * nw, h, ws * ws, 32, None), torch.bfloat16)
    inp.mask = _swin_mask(hi, wi, ws, shift)
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
    return inp, {name: (r, bd + ro.U_BF16_STORE * extra[name])
                 for name, (r, bd) in ref.items()}


def _run(case, inp, grad: bool):
    b, hi, wi, ws, shift, h = case
    bw, _, n, d = inp.q.shape

    def to_map(win):         # [BW, N, X] -> [B, Hi, Wi, X]
        return torch.roll(window_reverse(win, ws, hi, wi), (shift, shift),
                          (1, 2)).contiguous()

    def to_win(x):           # and back
        return window_partition(torch.roll(x, (-shift, -shift), (1, 2)), ws)

    def heads(t):            # [BW, N, H·D] -> [BW, H, N, D]
        return t.view(bw, n, h, d).transpose(1, 2)

    packed = torch.stack((inp.q, inp.k, inp.v)).permute(
        1, 3, 0, 2, 4).reshape(bw, n, 3 * h * d)     # (q|k|v, head, d)
    qkv = to_map(packed).cuda().requires_grad_(grad)
    bias = inp.bias.cuda().requires_grad_(grad)
    mask = None if inp.mask is None else inp.mask.cuda()
    args = (qkv, h, ws, shift, bias, mask, inp.scale)
    if not grad:
        with torch.no_grad():
            out = ops.shifted_window_attention_qkv(*args)
        return {"out": heads(to_win(out.cpu()))}
    out = ops.shifted_window_attention_qkv(*args)
    out.backward(to_map(inp.do.transpose(1, 2).reshape(bw, n, h * d)).cuda())
    assert out.shape == (b, hi, wi, h * d)
    assert out.dtype == qkv.grad.dtype == torch.bfloat16
    assert bias.grad.dtype == torch.float32
    dq, dk, dv = to_win(qkv.grad.cpu()).view(bw, n, 3, h, d).permute(
        2, 0, 3, 1, 4)
    return {"out": heads(to_win(out.detach().cpu())), "dq": dq, "dk": dk,
            "dv": dv, "dbias": bias.grad.cpu()}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_shifted_window_attention_qkv_within_bound(case):
    """out by the no-grad route and by the autograd route, and the latter's
    dQ, dK, dV (unpacked from the map-order dqkv) and dbias."""
    b, hi, wi, ws, shift, h = case
    inp, ref = ro.cached(("window_map", case), lambda: _reference(case))
    assert ops.shifted_window_attention_qkv_route(
        ws * ws, 32, inp.q.dtype, 0.0, hi, wi, ws, shift) == "map"
    for grad in (False, True):
        got = _run(case, inp, grad)
        ratios = {n: ro.worst_ratio(got[n], *ref[n]) for n in got}
        print(case, "autograd" if grad else "no-grad",
              {n: round(r, 4) for n, r in ratios.items()})
        assert all(r <= 1.0 for r in ratios.values()), (case, grad, ratios)
