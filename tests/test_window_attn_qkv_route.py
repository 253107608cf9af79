"""Which path `ops.window_attention_qkv` gives a packed projection output to,
and that the "unpacked" path is the sequence the model ran before."""

import pytest
import torch

from flreid_amd import ops


@pytest.mark.parametrize("n, d, dtype, drop_p, route", [
    (49, 32, torch.bfloat16, 0.0, "packed"),
    (64, 32, torch.bfloat16, 0.0, "packed"),
    (49, 32, torch.float32, 0.0, "unpacked"),
    (49, 64, torch.bfloat16, 0.0, "unpacked"),
    (65, 32, torch.bfloat16, 0.0, "unpacked"),
    (49, 32, torch.bfloat16, 0.1, "unpacked"),
])
def test_window_attention_qkv_route(n, d, dtype, drop_p, route):
    assert ops.window_attention_qkv_route(n, d, dtype, drop_p) == route


def test_window_attention_qkv_cpu_is_the_unpacked_sequence():
    g = torch.Generator().manual_seed(0)
    bn, n, h, d, nw = 6, 16, 2, 8, 3
    c = h * d
    qkv = torch.randn(bn, n, 3 * c, generator=g)
    bias = torch.randn(h, n, n, generator=g)
    mask = torch.where(torch.rand(nw, n, n, generator=g) < 0.3, -100.0, 0.0)
    go = torch.randn(bn, n, c, generator=g)

    def old(x, b):
        q, k, v = x.view(bn, n, 3, h, d).permute(2, 0, 3, 1, 4).unbind(0)
        out = ops.window_attention(q, k, v, b, mask, d ** -0.5, None)
        return out.transpose(1, 2).reshape(bn, n, c)

    def new(x, b):
        return ops.window_attention_qkv(x, h, b, mask, d ** -0.5, None)

    got = []
    for fn in (old, new):
        x = qkv.clone().requires_grad_(True)
        b = bias.clone().requires_grad_(True)
        out = fn(x, b)
        out.backward(go)
        got.append((out.detach(), x.grad, b.grad))
    for a, b in zip(*got):
        assert torch.equal(a, b)
