"""The routes of the FedSTIL adaptive layers, pinned down (MI355X only).

Characterisation: every combination of layer shape, live / composed θ,
autocast, input dtype, FLREID_NO_FUSED_1X1, FLREID_CLASSIFIER_GEMM and
frozen / trainable atten runs forward + backward with the extension wrapped
in a recorder; the sequence of bindings it called and the dtypes that came
out must equal ROUTES below.  Then bit-equality tests of the one linear
autograd function and of the composition kernel against host arithmetic."""

import contextlib
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from flreid_amd import ops
from flreid_amd.models.adaptive import (AdaptiveConv2d, AdaptiveLinear,
                                        live_theta_scope)

BF16 = torch.bfloat16


class _Recorder:
    """The extension, with the name of every binding called kept in order."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def call(*args, **kwargs):
            self.calls.append(name)
            return fn(*args, **kwargs)
        return call


@pytest.fixture()
def rec(monkeypatch):
    """Records the bindings and, as F.linear / F.conv2d, the library calls
    made through torch.nn.functional (the fallbacks; the lib conv engine)."""
    assert torch.cuda.is_available()
    recorder = _Recorder(ops.require_extension("compose2"))
    monkeypatch.setattr(ops, "_EXT", recorder)    # put back at teardown
    for name in ("linear", "conv2d"):
        def call(*args, _fn=getattr(F, name), _name="F." + name, **kwargs):
            recorder.calls.append(_name)
            return _fn(*args, **kwargs)
        monkeypatch.setattr(F, name, call)
    return recorder


# ---------------------------------------------------------------------------
# 1. characterisation
# ---------------------------------------------------------------------------

# conv input [2, 32, 4, 4] channels-last, K = 32; linear M = 32, N = 96,
# K = 64 (three N tiles and two K tiles of the K2 kernel)
LAYERS = {
    "linear2d": None, "linear3d": None,
    # kernel, stride, padding, bias
    "conv3x3": (3, 1, 1, False), "conv1x1": (1, 1, 0, False),
    "conv3x3s2": (3, 2, 1, False), "conv1x1bias": (1, 1, 0, True),
}


def _build(kind, atten_trainable):
    torch.manual_seed(0)
    if LAYERS[kind] is None:
        layer = AdaptiveLinear(global_weight=torch.randn(96, 64) * 0.1,
                               atten_default=0.9,
                               atten_trainable=atten_trainable)
        x = torch.randn(*((32, 64) if kind == "linear2d" else (2, 16, 64)))
    else:
        ksz, stride, padding, bias = LAYERS[kind]
        w = (torch.randn(32, 32, ksz, ksz) * 0.1).to(
            memory_format=torch.channels_last)
        layer = AdaptiveConv2d(
            global_weight=w, stride=stride, padding=padding,
            adaptive_bias=torch.zeros(32) if bias else None,
            atten_default=0.9, atten_trainable=atten_trainable)
        x = torch.randn(2, 32, 4, 4).to(memory_format=torch.channels_last)
    return layer.cuda(), x.cuda()


def _name(dtype):
    return {None: "-", torch.float32: "f32", BF16: "bf16"}[dtype]


def _grad_dtype(t):
    return None if t is None or t.grad is None else t.grad.dtype


def _run(kind, live, autocast, x_dtype, atten_trainable, rec):
    """'<bindings> | y dx daw dlive datten dbias', or 'raises' where the
    library fallback is handed an input and a weight of different dtypes."""
    layer, x = _build(kind, atten_trainable)
    x = x.to(x_dtype).requires_grad_(True)
    with contextlib.ExitStack() as stack:
        if live:
            buf = torch.empty_like(layer.global_weight, dtype=BF16)
            stack.enter_context(live_theta_scope([layer], [buf]))
        rec.calls.clear()
        try:
            with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                y = layer(x)
        except RuntimeError as e:
            if "same" not in str(e):      # only the dtype check of the library
                raise
            return " ".join(rec.calls + ["| raises"])
        y.backward(torch.ones_like(y))
        live_grad = layer._live.grad.dtype \
            if live and layer._live.grad is not None else None
    grads = (y.dtype, _grad_dtype(x), _grad_dtype(layer.adaptive_weight),
             live_grad, _grad_dtype(layer.global_weight_atten),
             _grad_dtype(layer.adaptive_bias))
    return " ".join(rec.calls + ["|"] + [_name(d) for d in grads])


AXES = list(itertools.product(
    ("live", "composed"), ("autocast", "plain"), ("x32", "x16"),
    ("1x1", "no1x1"), ("k2", "lib"), ("frozen", "trainable")))


def characterise(kind, rec, monkeypatch):
    got = {}
    for theta, cast, xd, fused, gemm, atten in AXES:
        monkeypatch.setenv("FLREID_NO_FUSED_1X1", "01"[fused == "no1x1"])
        monkeypatch.setenv("FLREID_CLASSIFIER_GEMM", gemm)
        got[(theta, cast, xd, fused, gemm, atten)] = _run(
            kind, theta == "live", cast == "autocast",
            torch.float32 if xd == "x32" else BF16, atten == "trainable", rec)
    return got


# Generated once on the commit before the routes were unified (all 384 cases,
# then merged mechanically into rows); the only change since is that the
# standalone composition reads compose2.  A row is "θ autocast x-dtype
# FLREID_NO_FUSED_1X1 FLREID_CLASSIFIER_GEMM atten", "*" matching either
# value; the FIRST matching row of a layer is the one that holds.  Outcome:
# bindings and F.* library calls in call order | dtype of y, x.grad,
# adaptive_weight.grad, _live.grad, atten.grad, adaptive_bias.grad.
ROUTES = {
    "linear2d": [
        ("live      plain     x32       *         *         *",
         "F.linear | raises"),
        ("live      *         x16       *         k2        *",
         "theta_linear_fwd | bf16 bf16 - bf16 - -"),
        ("live      *         x16       *         *         *",
         "| bf16 bf16 - bf16 - -"),
        ("*         *         x16       *         *         frozen",
         "adaptive_linear_fwd compose2 | bf16 bf16 f32 - - -"),
        ("composed  *         *         *         *         frozen",
         "adaptive_linear_fwd compose2 | bf16 f32 f32 - - -"),
        ("live      *         *         *         k2        *",
         "theta_linear_fwd | bf16 f32 - bf16 - -"),
        ("live      *         *         *         *         *",
         "| bf16 f32 - bf16 - -"),
        ("*         autocast  x32       *         *         *",
         "compose2 F.linear | bf16 f32 f32 - f32 -"),
        ("*         autocast  *         *         *         *",
         "compose2 F.linear | bf16 bf16 f32 - f32 -"),
        ("*         *         x32       *         *         *",
         "compose2 F.linear | f32 f32 f32 - f32 -"),
        ("*         *         *         *         *         *",
         "compose2 F.linear | raises"),
    ],
    "linear3d": [
        ("live      *         x16       *         *         *",
         "F.linear | bf16 bf16 - bf16 - -"),
        ("live      autocast  *         *         *         *",
         "F.linear | bf16 f32 - bf16 - -"),
        ("live      *         *         *         *         *",
         "F.linear | raises"),
        ("*         plain     x16       *         *         *",
         "compose2 F.linear | raises"),
        ("*         plain     *         *         *         frozen",
         "compose2 F.linear | f32 f32 f32 - - -"),
        ("*         plain     *         *         *         *",
         "compose2 F.linear | f32 f32 f32 - f32 -"),
        ("*         *         x32       *         *         frozen",
         "compose2 F.linear | bf16 f32 f32 - - -"),
        ("*         *         x32       *         *         *",
         "compose2 F.linear | bf16 f32 f32 - f32 -"),
        ("*         *         *         *         *         frozen",
         "compose2 F.linear | bf16 bf16 f32 - - -"),
        ("*         *         *         *         *         *",
         "compose2 F.linear | bf16 bf16 f32 - f32 -"),
    ],
    "conv3x3": [
        ("live      *         x16       *         *         *",
         "F.conv2d conv3x3_tile F.conv2d | bf16 bf16 - bf16 - -"),
        ("live      autocast  *         *         *         *",
         "F.conv2d conv3x3_tile F.conv2d | bf16 f32 - bf16 - -"),
        ("live      *         *         *         *         *",
         "F.conv2d | raises"),
        ("*         *         x16       *         *         frozen",
         "compose2 F.conv2d conv3x3_tile F.conv2d | bf16 bf16 f32 - - -"),
        ("*         autocast  x16       *         *         *",
         "compose2 F.conv2d | bf16 bf16 f32 - f32 -"),
        ("*         *         x16       *         *         *",
         "compose2 F.conv2d | raises"),
        ("*         autocast  *         *         *         frozen",
         "compose2 F.conv2d conv3x3_tile F.conv2d | bf16 f32 f32 - - -"),
        ("*         autocast  *         *         *         *",
         "compose2 F.conv2d | bf16 f32 f32 - f32 -"),
        ("*         *         *         *         *         frozen",
         "compose2 F.conv2d | f32 f32 f32 - - -"),
        ("*         *         *         *         *         *",
         "compose2 F.conv2d | f32 f32 f32 - f32 -"),
    ],
    "conv1x1": [
        ("live      plain     x32       *         *         *",
         "F.conv2d | raises"),
        ("live      *         x16       1x1       *         *",
         "| bf16 bf16 - bf16 - -"),
        ("live      *         x16       *         *         *",
         "F.conv2d | bf16 bf16 - bf16 - -"),
        ("live      *         *         1x1       *         *",
         "| bf16 f32 - bf16 - -"),
        ("live      *         *         *         *         *",
         "F.conv2d | bf16 f32 - bf16 - -"),
        ("*         autocast  x32       *         *         trainable",
         "compose2 F.linear | bf16 f32 f32 - f32 -"),
        ("*         autocast  *         *         *         trainable",
         "compose2 F.linear | bf16 bf16 f32 - f32 -"),
        ("*         *         x32       *         *         trainable",
         "compose2 F.linear | f32 f32 f32 - f32 -"),
        ("*         *         *         *         *         trainable",
         "compose2 F.linear | raises"),
        ("*         plain     x32       *         *         *",
         "compose2 F.linear | f32 f32 f32 - - -"),
        ("*         *         x16       1x1       *         *",
         "compose2 | bf16 bf16 f32 - - -"),
        ("*         plain     *         *         *         *",
         "compose2 F.linear | raises"),
        ("*         *         x16       *         *         *",
         "compose2 F.linear | bf16 bf16 f32 - - -"),
        ("*         *         *         1x1       *         *",
         "compose2 | bf16 f32 f32 - - -"),
        ("*         *         *         *         *         *",
         "compose2 F.linear | bf16 f32 f32 - - -"),
    ],
    "conv3x3s2": [
        ("live      *         x16       *         *         *",
         "F.conv2d | bf16 bf16 - bf16 - -"),
        ("live      autocast  *         *         *         *",
         "F.conv2d | bf16 f32 - bf16 - -"),
        ("live      *         *         *         *         *",
         "F.conv2d | raises"),
        ("*         plain     x16       *         *         *",
         "compose2 F.conv2d | raises"),
        ("*         plain     *         *         *         frozen",
         "compose2 F.conv2d | f32 f32 f32 - - -"),
        ("*         plain     *         *         *         *",
         "compose2 F.conv2d | f32 f32 f32 - f32 -"),
        ("*         *         x32       *         *         frozen",
         "compose2 F.conv2d | bf16 f32 f32 - - -"),
        ("*         *         x32       *         *         *",
         "compose2 F.conv2d | bf16 f32 f32 - f32 -"),
        ("*         *         *         *         *         frozen",
         "compose2 F.conv2d | bf16 bf16 f32 - - -"),
        ("*         *         *         *         *         *",
         "compose2 F.conv2d | bf16 bf16 f32 - f32 -"),
    ],
    "conv1x1bias": [
        ("live      plain     x32       *         *         *",
         "F.conv2d | raises"),
        ("live      *         x16       1x1       *         *",
         "| bf16 bf16 - bf16 - f32"),
        ("live      plain     *         *         *         *",
         "F.conv2d | raises"),
        ("live      *         x16       *         *         *",
         "F.conv2d | bf16 bf16 - bf16 - f32"),
        ("live      *         *         1x1       *         *",
         "| bf16 f32 - bf16 - f32"),
        ("live      *         *         *         *         *",
         "F.conv2d | bf16 f32 - bf16 - f32"),
        ("*         autocast  x32       *         *         trainable",
         "compose2 F.linear | bf16 f32 f32 - f32 f32"),
        ("*         autocast  *         *         *         trainable",
         "compose2 F.linear | bf16 bf16 f32 - f32 f32"),
        ("*         *         x32       *         *         trainable",
         "compose2 F.linear | f32 f32 f32 - f32 f32"),
        ("*         *         *         *         *         trainable",
         "compose2 F.linear | raises"),
        ("*         plain     x32       *         *         *",
         "compose2 F.linear | f32 f32 f32 - - f32"),
        ("*         *         x16       1x1       *         *",
         "compose2 | bf16 bf16 f32 - - f32"),
        ("*         plain     *         *         *         *",
         "compose2 F.linear | raises"),
        ("*         *         x16       *         *         *",
         "compose2 F.linear | bf16 bf16 f32 - - f32"),
        ("*         *         *         1x1       *         *",
         "compose2 | bf16 f32 f32 - - f32"),
        ("*         *         *         *         *         *",
         "compose2 F.linear | bf16 f32 f32 - - f32"),
    ],
}


def _expected(kind, case):
    for row, outcome in ROUTES[kind]:
        if all(r in ("*", c) for r, c in zip(row.split(), case)):
            return outcome
    raise KeyError((kind, case))


@pytest.mark.parametrize("kind", list(LAYERS))
def test_routes(kind, rec, monkeypatch):
    got = characterise(kind, rec, monkeypatch)
    wrong = {case: (out, _expected(kind, case)) for case, out in got.items()
             if out != _expected(kind, case)}
    assert not wrong, "\n".join(
        f"{' '.join(c)}: got '{g}', expected '{w}'"
        for c, (g, w) in wrong.items())


# ---------------------------------------------------------------------------
# 2. the one linear autograd function, bit for bit
# ---------------------------------------------------------------------------

def _linear_inputs(bias=True):
    torch.manual_seed(1)
    m, n, k = 32, 96, 64
    x = torch.randn(m, k, device="cuda").bfloat16().requires_grad_(True)
    gw = torch.randn(n, k, device="cuda") * 0.1
    atten = torch.rand(k, device="cuda")
    aw = (torch.randn(n, k, device="cuda") * 0.02).requires_grad_(True)
    b = torch.randn(n, device="cuda").requires_grad_(True) if bias else None
    g = torch.randn(m, n, device="cuda").bfloat16()
    return x, gw, atten, aw, b, g


@pytest.mark.parametrize("bias", (False, True))
def test_lib_engine_composed_is_compose2_plus_gemm(bias):
    ext = ops.require_extension("compose2")
    x, gw, atten, aw, b, g = _linear_inputs(bias)
    y = ops.adaptive_linear(x, gw, atten, aw, b, engine="lib")
    theta = ops.compose_theta_bf16(ext, gw, atten, aw)
    want = x.detach() @ theta.t()
    if bias:
        want = want + b.detach().to(BF16)
    assert y.dtype == BF16 and torch.equal(y, want)
    y.backward(g)
    assert aw.grad.dtype == torch.float32
    assert torch.equal(aw.grad, (g.t() @ x.detach()).float())
    assert torch.equal(x.grad, g @ theta)
    if bias:
        assert torch.equal(b.grad, g.sum(0).float())


@pytest.mark.parametrize("bias", (False, True))
def test_k2_engine_ready_theta_equals_composing(bias):
    """The bf16-load prologue of the K2 tile loop sums in the composing
    prologue's order: same θ, same bits."""
    ext = ops.require_extension("compose2")
    x, gw, atten, aw, b, g = _linear_inputs(bias)
    theta = ops.compose_theta_bf16(ext, gw, atten, aw).requires_grad_(True)
    y_ready = ops.adaptive_linear(x, theta, None, None, b, engine="k2")
    y_comp = ops.adaptive_linear(x, gw, atten, aw, b, engine="k2")
    assert y_ready.dtype == BF16 and y_comp.dtype == BF16
    assert torch.equal(y_ready, y_comp)
    # θ recomposed in the composing route's backward is the same θ
    dx_ready, = torch.autograd.grad(y_ready, x, g)
    dx_comp, = torch.autograd.grad(y_comp, x, g)
    assert torch.equal(dx_ready, g @ theta.detach())
    assert torch.equal(dx_comp, dx_ready)


@pytest.mark.parametrize("engine", ("k2", "lib"))
def test_ready_theta_weight_gradient_stays_bf16(engine, rec):
    x, gw, atten, aw, b, g = _linear_inputs()
    theta = ops.compose_theta_bf16(rec, gw, atten, aw).requires_grad_(True)
    rec.calls.clear()
    y = ops.adaptive_linear(x, theta, None, None, b, engine=engine)
    y.backward(g)
    assert rec.calls == (["theta_linear_fwd"] if engine == "k2" else [])
    assert theta.grad.dtype == BF16
    assert torch.equal(theta.grad, g.t() @ x.detach())


def test_composing_k2_route_needs_fp32_weights(rec):
    """The composing K2 kernel reads gw / aw as fp32: bf16 weights are out
    of regime and launch nothing."""
    x, gw, atten, aw, b, _g = _linear_inputs()
    rec.calls.clear()
    assert ops.adaptive_linear(x, gw.bfloat16(), atten,
                               aw.detach().bfloat16(), b) is None
    assert rec.calls == []


# ---------------------------------------------------------------------------
# 3. the composition kernel against host arithmetic
# ---------------------------------------------------------------------------

def _host_fma_f32(a, g, w):
    """fl32(a·g + w) with ONE rounding, for fp32-representable inputs: the
    product is exact in fp64; the fp64 sum is rounded to odd (TwoSum error
    term), after which the cast to fp32 rounds as the exact sum would."""
    a, g, w = (t.double().cpu().numpy() for t in (a, g, w))
    p = a * g
    s = p + w
    bb = s - p
    err = (p - (s - bb)) + (w - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return torch.from_numpy(s.astype(np.float32))


@pytest.mark.parametrize("dtype", (torch.float32, BF16))
@pytest.mark.parametrize("shape", ((33, 7), (48, 64), (6, 5, 3, 7)))
def test_adaptive_compose_is_one_fma(shape, dtype, rec):
    torch.manual_seed(2)
    gw = torch.randn(*shape, device="cuda").to(dtype)
    aw = (torch.randn(*shape, device="cuda") * 0.1).to(dtype)
    if len(shape) == 4:
        gw = gw.to(memory_format=torch.channels_last)
    atten = torch.rand(shape[-1], device="cuda")
    rec.calls.clear()
    out = ops.adaptive_compose(gw, atten, aw)
    assert len(rec.calls) == 1
    assert out.dtype == dtype and out.shape == gw.shape and out.is_contiguous()
    want = _host_fma_f32(atten.expand(shape), gw, aw).to(dtype)
    assert torch.equal(out.cpu(), want)


def test_compose_theta_bf16_of_bf16_weights_is_adaptive_compose():
    """compose2's bf16 → bf16 case rounds as the standalone composition."""
    ext = ops.require_extension("compose2")
    torch.manual_seed(3)
    gw = torch.randn(96, 64, device="cuda").bfloat16()
    aw = (torch.randn(96, 64, device="cuda") * 0.1).bfloat16()
    atten = torch.rand(64, device="cuda")
    assert torch.equal(ops.compose_theta_bf16(ext, gw, atten, aw),
                       ops.adaptive_compose(gw, atten, aw).to(BF16))
