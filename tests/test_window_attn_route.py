"""Which kernel `ops.window_attention` gives a window shape to."""

import pytest
import torch

from flreid_amd import ops

BF16, F32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("n,d,dtype,drop_p,route", [
    (49, 32, BF16, 0.0, "valu"),
    (64, 64, F32, 0.0, "valu"),
    (65, 8, F32, 0.0, "eager"),
    (144, 32, F32, 0.0, "eager"),
    (144, 64, BF16, 0.0, "eager"),
    (145, 32, BF16, 0.0, "eager"),
    (144, 32, BF16, 0.1, "eager"),
    (65, 32, BF16, 0.0, "mfma"),
    (144, 32, BF16, 0.0, "mfma"),
])
def test_window_attention_route(n, d, dtype, drop_p, route):
    assert ops.window_attention_route(n, d, dtype, drop_p) == route
