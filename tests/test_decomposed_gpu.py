"""Fused FedWeIT composition kernels (ops/csrc/decomposed.hip) vs the fp64
reference expression (MI355X only).

Exact cases draw every operand from small integers and halves, so every
product and partial sum is exactly representable in fp32 and summation
order cannot matter: the kernels must match the fp64 reference bit for bit.
mask values of exactly ±0.5 sit ON the threshold (λ = 0.5); the strict `>`
must zero them."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from flreid_amd import ops
from flreid_amd.models.decomposed import (DecomposedConv2d,
                                          DecomposedLayerNorm,
                                          DecomposedLinear)
from flreid_amd.ops import reference as ref

LAM = 0.5
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension must be built in-tree"


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _exact_inputs(shape, kb, cl):
    g = torch.Generator().manual_seed(1000 * kb + sum(shape) + int(cl))

    def ri(sh, lo, hi):
        return torch.randint(lo, hi + 1, sh, generator=g).float()

    sw, aw = ri(shape, -2, 2), ri(shape, -2, 2)
    aw_kb = ri(shape + (kb,), -2, 2)
    mask = ri((shape[0],), -2, 2) / 2
    mask[0], mask[-1] = 0.5, -0.5          # exactly at the threshold
    atten = ri((kb,), -2, 2) / 2
    go = ri(shape, -1, 1)
    if cl:
        sw, aw, go = _cl(sw), _cl(aw), _cl(go)
    return sw, mask, aw, aw_kb, atten, go


@functools.lru_cache(maxsize=None)
def _random_inputs(shape, kb, cl):
    g = torch.Generator().manual_seed(7 + kb + sum(shape))
    sw, aw = (torch.randn(shape, generator=g) for _ in range(2))
    aw_kb = torch.randn(*shape, kb, generator=g)
    mask = torch.randn(shape[0], generator=g)
    atten = torch.randn(kb, generator=g)
    go = torch.randn(shape, generator=g)
    if cl:
        sw, aw, go = _cl(sw), _cl(aw), _cl(go)
    return sw, mask, aw, aw_kb, atten, go


def _reference64(inp, training):
    """(θ, d_aw, d_mask, d_atten) in fp64 on the CPU."""
    sw, mask, aw, aw_kb, atten, go = (t.double() for t in inp)
    mask, aw, atten = (t.clone().requires_grad_(True)
                       for t in (mask, aw, atten))
    theta = ref.decomposed_compose(sw, mask, aw, aw_kb, atten, LAM, LAM,
                                   training)
    d_aw, d_mask, d_atten = torch.autograd.grad(theta, (aw, mask, atten), go)
    return theta.detach(), d_aw, d_mask, d_atten


def _fused(inp, training, out_dtype=None, needs=(True, True, True),
           backward=True):
    """(θ, d_aw, d_mask, d_atten) from the fused route, moved to the CPU;
    needs = requires_grad of (aw, mask, atten)."""
    sw, mask, aw, aw_kb, atten, go = (t.cuda() for t in inp)
    aw.requires_grad_(needs[0])
    mask.requires_grad_(needs[1])
    atten.requires_grad_(needs[2])
    theta = ops.decomposed_compose(sw, mask, aw, aw_kb, atten, LAM, LAM,
                                   training, out_dtype)
    assert "DecomposedComposeFn" in type(theta.grad_fn).__name__, \
        "fused route not taken"
    assert theta.stride() == sw.stride()
    grads = [None, None, None]
    if backward:
        theta.backward(go.to(theta.dtype))
        grads = [None if t.grad is None else t.grad.cpu()
                 for t in (aw, mask, atten)]
    return (theta.detach().cpu(), *grads)


EXACT_CASES = [
    ((7, 10), 3, False),          # tail, inner not a multiple of 4
    ((33, 130), 5, False),
    ((4, 4), 1, False),
    ((8, 12, 1, 1), 5, False),
    ((5, 6, 3, 3), 5, False),
    ((5, 6, 3, 3), 5, True),
    ((16, 70, 3, 3), 2, True),    # c-tile remainder
    ((64, 256, 3, 3), 5, True),   # several tiles per row, multi-block partials
    ((300, 2048), 7, False),      # several chunks per row
    ((33, 130), 9, False),        # generic (non-templated) KB loop
    ((5, 8, 3, 3), 9, True),      # generic KB loop, channels-last
    ((3, 6, 5, 5), 4, True),      # more than one tap tile per row (S > 16)
    ((3, 8, 5, 5), 4, True),      # the same with C % 4 == 0
]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape,kb,cl", EXACT_CASES)
def test_exact(shape, kb, cl, training):
    inp = _exact_inputs(shape, kb, cl)
    want = _reference64(inp, training)
    got = _fused(inp, training)
    for name, g, w in zip(("theta", "d_aw", "d_mask", "d_atten"), got, want):
        assert g.dtype == torch.float32
        assert torch.equal(g, w.float()), name


def test_threshold_is_strict():
    inp = _exact_inputs((7, 10), 3, False)
    theta, d_aw, d_mask, _ = _fused(inp, True)
    sw, mask, aw, aw_kb, atten, go = inp
    # rows 0 / -1 carry |mask| == λ exactly: pruned, no gradient
    assert d_mask[0] == 0 and d_mask[-1] == 0
    kb = (atten * aw_kb).sum(-1)
    assert torch.equal(theta[0], aw[0] + kb[0])
    assert torch.equal(d_aw, go * (aw != 0))


@pytest.mark.parametrize("needs", [(False, False, True), (True, False, False)])
@pytest.mark.parametrize("shape,kb,cl", [((33, 130), 5, False),
                                         ((16, 70, 3, 3), 2, True)])
def test_skip_flags(shape, kb, cl, needs):
    inp = _exact_inputs(shape, kb, cl)
    want = _reference64(inp, True)
    got = _fused(inp, True, needs=needs)
    for need, g, w in zip(needs, got[1:], want[1:]):
        if need:
            assert torch.equal(g, w.float())
        else:
            assert g is None


@pytest.mark.parametrize("shape,kb,cl", [((33, 130), 5, False),
                                         ((300, 2048), 7, False),
                                         ((5, 6, 3, 3), 5, True),
                                         ((64, 256, 3, 3), 5, True)])
def test_bf16_output(shape, kb, cl):
    inp = _exact_inputs(shape, kb, cl)
    f32 = _fused(inp, True)
    b16 = _fused(inp, True, out_dtype=torch.bfloat16)
    assert b16[0].dtype == torch.bfloat16
    # RNE of the fp32 θ, bit for bit
    assert torch.equal(b16[0].view(torch.int16),
                       f32[0].bfloat16().view(torch.int16))
    # dθ ∈ {−1, 0, 1} is exact in bf16: same gradients either way
    for a, b in zip(b16[1:], f32[1:]):
        assert a.dtype == torch.float32
        assert torch.equal(a, b)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape,kb,cl", [((33, 130), 5, False),
                                         ((16, 70, 3, 3), 2, True)])
def test_random_within_rounding_bound(shape, kb, cl, training):
    inp = _random_inputs(shape, kb, cl)
    theta64, d_aw64, d_mask64, d_atten64 = _reference64(inp, training)
    theta, d_aw, d_mask, d_atten = _fused(inp, training)
    sw, mask, aw, aw_kb, atten, go = (t.double() for t in inp)
    if training:
        mask_t = mask * (mask.abs() > LAM)
        aw_t = aw * (aw.abs() > LAM)
    else:
        mask_t, aw_t = mask, aw
    bshape = (-1,) + (1,) * (sw.dim() - 1)
    # θ and d_aw: at most KB+2 rounded terms per element
    mag = ((mask_t.view(bshape) * sw).abs() + aw_t.abs()
           + (atten * aw_kb).abs().sum(-1))
    assert ((theta.double() - theta64).abs() <= (kb + 3) * EPS * mag).all()
    assert ((d_aw.double() - d_aw64).abs() <= (kb + 3) * EPS * go.abs()).all()
    # reductions: worst-case bound over their n summands (sanity only)
    n_row = sw[0].numel()
    mag_m = (go * sw).abs().flatten(1).sum(1)
    assert ((d_mask.double() - d_mask64).abs() <= n_row * EPS * mag_m).all()
    mag_a = (go.unsqueeze(-1) * aw_kb).abs().flatten(0, -2).sum(0)
    assert ((d_atten.double() - d_atten64).abs()
            <= sw.numel() * EPS * mag_a).all()


@pytest.mark.parametrize("shape,kb,cl", [((300, 2048), 7, False),
                                         ((64, 256, 3, 3), 5, True)])
def test_backward_is_deterministic(shape, kb, cl):
    inp = _random_inputs(shape, kb, cl)
    a = _fused(inp, True)
    b = _fused(inp, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _module_run(layer, x, go):
    layer.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    y = layer(x)
    y.backward(go)
    grads = {n: p.grad.clone() for n, p in layer.named_parameters()
             if p.grad is not None}
    return y.detach(), x.grad, grads


def _check_module(layer, x, monkeypatch):
    layer.train()
    assert "DecomposedComposeFn" in type(
        layer.composed_weight().grad_fn).__name__
    go = torch.randn_like(layer(x))
    y, dx, grads = _module_run(layer, x, go)
    monkeypatch.setenv("FLREID_NO_FUSED_DECOMPOSE", "1")
    assert "DecomposedComposeFn" not in type(
        layer.composed_weight().grad_fn).__name__
    y0, dx0, grads0 = _module_run(layer, x, go)
    assert set(grads) == set(grads0) >= {"mask", "aw", "atten", "bias"}
    assert torch.allclose(y, y0, atol=1e-4, rtol=1e-4)
    assert torch.allclose(dx, dx0, atol=1e-4, rtol=1e-4)
    for n in grads:
        assert torch.allclose(grads[n], grads0[n], atol=1e-4, rtol=1e-4), n


def test_module_conv3x3_channels_last(monkeypatch):
    torch.manual_seed(0)
    k, c, kb = 6, 8, 5
    sw = _cl(torch.randn(k, c, 3, 3) * 0.2)
    layer = DecomposedConv2d(
        shared_weight=sw, padding=1, bias=torch.randn(k) * 0.1,
        mask=torch.rand(k), adaptive=_cl(torch.randn(k, c, 3, 3) * 0.2),
        knowledge_base=torch.randn(k, c, 3, 3, kb) * 0.2,
        atten=torch.randn(kb) * 0.5, lambda_l1=0.05, lambda_mask=0.1,
        kb_cnt=kb).cuda()
    assert layer.sw.is_contiguous(memory_format=torch.channels_last)
    assert layer.aw.is_contiguous(memory_format=torch.channels_last)
    _check_module(layer, torch.randn(2, c, 6, 5, device="cuda"), monkeypatch)


def test_module_linear(monkeypatch):
    torch.manual_seed(1)
    n, k, kb = 10, 24, 5
    layer = DecomposedLinear(
        shared_weight=torch.randn(n, k) * 0.2, bias=torch.randn(n) * 0.1,
        mask=torch.rand(n), adaptive=torch.randn(n, k) * 0.2,
        knowledge_base=torch.randn(n, k, kb) * 0.2,
        atten=torch.randn(kb) * 0.5, lambda_l1=0.05, lambda_mask=0.1,
        kb_cnt=kb).cuda()
    _check_module(layer, torch.randn(3, k, device="cuda"), monkeypatch)


def test_fallback_one_dim_weight():
    torch.manual_seed(2)
    d, kb = 16, 3
    layer = DecomposedLayerNorm(
        shared_weight=torch.randn(d), bias=torch.zeros(d),
        mask=torch.rand(d), adaptive=torch.randn(d),
        knowledge_base=torch.randn(d, kb), atten=torch.randn(kb),
        lambda_l1=0.05, lambda_mask=0.1, kb_cnt=kb).cuda().train()
    theta = layer.composed_weight()
    assert "DecomposedComposeFn" not in type(theta.grad_fn).__name__
    want = ref.decomposed_compose(layer.sw, layer.mask, layer.aw, layer.aw_kb,
                                  layer.atten, 0.05, 0.1, True)
    assert torch.equal(theta, want)
    assert layer(torch.randn(4, d, device="cuda")).shape == (4, d)


def test_fallback_mismatched_layout():
    torch.manual_seed(3)
    k, c, kb = 6, 8, 2
    layer = DecomposedConv2d(
        shared_weight=torch.randn(k, c, 3, 3), padding=1,
        mask=torch.rand(k), adaptive=_cl(torch.randn(k, c, 3, 3)),
        knowledge_base=torch.randn(k, c, 3, 3, kb), atten=torch.randn(kb),
        lambda_l1=0.05, lambda_mask=0.1, kb_cnt=kb).cuda().train()
    assert layer.sw.is_contiguous()
    assert not layer.aw.is_contiguous()
    theta = layer.composed_weight()
    assert "DecomposedComposeFn" not in type(theta.grad_fn).__name__
    want = ref.decomposed_compose(layer.sw, layer.mask, layer.aw, layer.aw_kb,
                                  layer.atten, 0.05, 0.1, True)
    assert torch.equal(theta, want)
