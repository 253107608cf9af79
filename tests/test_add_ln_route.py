"""`ops.add_layer_norm` off the GPU: the route function's answers, the CPU
path (the reference composition, bit for bit) and the Swin block's switch."""

import pytest
import torch

from flreid_amd import ops
from flreid_amd.models.swin import SwinBlock
from flreid_amd.ops import reference as ref

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


@pytest.mark.parametrize("c, x, branch, out, want", [
    (8, F32, BF16, BF16, "kernel"),
    (96, F32, BF16, BF16, "kernel"),
    (96, F32, None, BF16, "kernel"),
    (96, BF16, BF16, F32, "kernel"),
    (1536, F32, F32, F32, "kernel"),
    (1544, F32, BF16, BF16, "eager"),
    (100, F32, BF16, BF16, "eager"),
    (0, F32, BF16, BF16, "eager"),
    (96, F16, None, F16, "eager"),
    (96, F32, F16, BF16, "eager"),
    (96, BF16, F32, BF16, "eager"),     # the sum would be promoted to fp32
])
def test_add_layer_norm_route(c, x, branch, out, want):
    assert ops.add_layer_norm_route(c, x, branch, out) == want


@pytest.mark.parametrize("out_dtype", [None, BF16])
@pytest.mark.parametrize("with_branch", [False, True])
def test_cpu_path_is_the_reference_composition(with_branch, out_dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 96, generator=g)
    branch = torch.randn(3, 5, 96, generator=g).bfloat16() \
        if with_branch else None
    w, b = torch.randn(96, generator=g), torch.randn(96, generator=g)
    s = x if branch is None else x + branch
    y = torch.nn.functional.layer_norm(s, (96,), w, b, 1e-5)
    y = y if out_dtype is None else y.to(out_dtype)
    for fn in (ops.add_layer_norm, ref.add_layer_norm):
        got = fn(x, branch, w, b, 1e-5, out_dtype)
        if with_branch:
            assert torch.equal(got[0], s)
            got = got[1]
        assert got.dtype == y.dtype and torch.equal(got, y)


def test_cpu_swin_block_ignores_the_switch(monkeypatch):
    torch.manual_seed(0)
    blk = SwinBlock(96, (14, 14), 3, window_size=7, shift=3)
    x = torch.randn(2, 196, 96)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("FLREID_SWIN_ADD_LN", flag)
        outs.append(blk(x))
    assert torch.equal(outs[0], outs[1])
