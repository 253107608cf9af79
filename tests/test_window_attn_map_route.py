"""Which path `ops.shifted_window_attention_qkv` gives a qkv feature map to,
and that the "windows" path is the sequence the model ran before."""

import pytest
import torch

from flreid_amd import ops
from flreid_amd.models.swin import window_partition, window_reverse

BF16, F32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("n, d, dtype, drop_p, hi, wi, ws, shift, route", [
    (49, 32, BF16, 0.0, 56, 56, 7, 3, "map"),
    (49, 32, BF16, 0.0, 7, 7, 7, 0, "map"),
    (64, 32, BF16, 0.0, 16, 8, 8, 7, "map"),
    (1, 32, BF16, 0.0, 3, 5, 1, 0, "map"),
    (49, 32, F32, 0.0, 56, 56, 7, 3, "windows"),
    (49, 64, BF16, 0.0, 56, 56, 7, 3, "windows"),
    (81, 32, BF16, 0.0, 18, 18, 9, 4, "windows"),
    (49, 32, BF16, 0.0, 56, 55, 7, 3, "windows"),      # wi % ws != 0
    (49, 32, BF16, 0.0, 55, 56, 7, 3, "windows"),      # hi % ws != 0
    (49, 32, BF16, 0.0, 56, 56, 7, 7, "windows"),      # shift >= ws
    (49, 32, BF16, 0.1, 56, 56, 7, 3, "windows"),
])
def test_shifted_window_attention_qkv_route(n, d, dtype, drop_p, hi, wi, ws,
                                            shift, route):
    assert ops.shifted_window_attention_qkv_route(
        n, d, dtype, drop_p, hi, wi, ws, shift) == route


@pytest.mark.parametrize("shift", [0, 2])
def test_shifted_window_attention_qkv_cpu_is_the_windows_sequence(shift):
    g = torch.Generator().manual_seed(0)
    b, hi, wi, ws, h, d = 2, 8, 12, 4, 2, 8
    n, c, nw = ws * ws, h * d, (hi // ws) * (wi // ws)
    qkv = torch.randn(b, hi, wi, 3 * c, generator=g)
    bias = torch.randn(h, n, n, generator=g)
    mask = None
    if shift:
        mask = torch.where(torch.rand(nw, n, n, generator=g) < 0.3, -100.0,
                           0.0)
    go = torch.randn(b, hi, wi, c, generator=g)

    def old(x, bs):
        if shift:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        win = ops.window_attention_qkv(window_partition(x, ws), h, bs, mask,
                                       d ** -0.5, None)
        x = window_reverse(win, ws, hi, wi)
        if shift:
            x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
        return x

    def new(x, bs):
        return ops.shifted_window_attention_qkv(x, h, ws, shift, bs, mask,
                                                d ** -0.5, None)

    got = []
    for fn in (old, new):
        x = qkv.clone().requires_grad_(True)
        bs = bias.clone().requires_grad_(True)
        out = fn(x, bs)
        out.backward(go)
        got.append((out.detach(), x.grad, bs.grad))
    for a, e in zip(*got):
        assert torch.equal(a, e)
