"""The conv oracle (tests/conv_oracle.py) is sound and sharp — on the CPU.

Sound: torch's own fp32 conv agrees with it exactly on grid inputs and
within the bound on full-mantissa inputs.  Sharp: each of a list of
deliberately wrong convs — the mistakes a hand-written kernel's edge code
can make — is rejected by BOTH checks.  The GPU tests of the hand kernels
(test_conv3x3_hand_gpu.py) apply the same two checks."""

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import conv_oracle as co

# (n, C, H, W, K): odd batch, C != K both ways, widths 7 and 8, C crossing 128
SHAPES = [(3, 96, 16, 7, 32), (3, 160, 14, 8, 96)]
KINDS = ["grid", "full"]


def _inputs(kind, shape):
    return (co.grid_inputs if kind == "grid" else co.full_inputs)(*shape,
                                                                   seed=11)


_REFS = {}


def _case(kind, shape):
    key = (kind, shape)
    if key not in _REFS:
        inp = _inputs(kind, shape)
        _REFS[key] = (inp, co.reference(inp.x, inp.dy, inp.gw, inp.atten,
                                        inp.aw, exact=(kind == "grid")))
    return _REFS[key]


def _theta32(inp, atten_view=(1, 1, 1, 3), flip_atten=False):
    """theta the way an fp32 kernel makes it: fp32 compose, one bf16 round."""
    a = inp.atten.flip(0) if flip_atten else inp.atten
    return (a.view(*atten_view) * inp.gw + inp.aw).bfloat16().float()


def _fp32_conv(inp, theta=None, unflipped_dgrad=False):
    """torch's fp32 conv on the bf16-rounded operands -> (out, dx, dw) in
    fp32, before the final store."""
    th = _theta32(inp) if theta is None else theta
    x, dy = inp.x.float(), inp.dy.float()
    out = F.conv2d(x, th, padding=1)
    if unflipped_dgrad:
        dx = F.conv2d(dy, th.transpose(0, 1).contiguous(), padding=1)
    else:
        dx = conv2d_input(x.shape, th, dy, padding=1)
    dw = conv2d_weight(x, th.shape, dy, padding=1)
    return out, dx, dw


def _accepts(kind, ref, out=None, dx=None, dw=None, store=co.round_bf16):
    """Apply the check of `kind` to whichever results are given; out and dx
    go through the bf16 store first.  Returns {name: passed}."""
    res = {}
    for name, got, r64, bnd in (("out", out, ref.out, ref.bound_out),
                                ("dx", dx, ref.dx, ref.bound_dx)):
        if got is None:
            continue
        got16 = store(got.double()).to(torch.bfloat16)
        if kind == "grid":
            res[name] = torch.equal(got16, co.to_bf16(r64))
        else:
            res[name] = co.worst_ratio(got16, r64, bnd()) <= 1.0
    if dw is not None:
        if kind == "grid":
            res["dw"] = torch.equal(dw.float(), ref.dw.float())
        else:
            res["dw"] = co.worst_ratio(dw, ref.dw, ref.bound_dw()) <= 1.0
    return res


def test_round_bf16_matches_torch_cast():
    """The bit-pattern rounding is torch's own fp32 -> bf16 cast on fp32
    values, ties included, and truncation never rounds away from zero."""
    g = torch.Generator().manual_seed(5)
    t = torch.randn(4096, generator=g)
    ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0, 0.0])
    t = torch.cat([t, ties])
    assert torch.equal(co.round_bf16(t.double()).float(), t.bfloat16().float())
    tr = co.trunc_bf16(t.double())
    assert bool((tr.abs() <= t.double().abs()).all())
    assert torch.equal(tr.to(torch.bfloat16).double(), tr)
    assert co.bf16_ulp_distance(torch.tensor([1.0, -1.0]).bfloat16(),
                                torch.tensor([1.0078125, -1.0]).bfloat16()) == 1


@pytest.mark.parametrize("shape", SHAPES)
def test_grid_inputs_are_on_their_grids(shape):
    inp, ref = _case("grid", shape)
    for t, scale, lim in ((inp.x.float(), 2 ** 8, 128),
                          (inp.dy.float(), 2 ** 8, 128),
                          (inp.gw, 2 ** 4, 8), (inp.aw, 2 ** 6, 32),
                          (ref.theta, 2 ** 6, 64)):
        s = t.double() * scale
        assert torch.equal(s, s.round()) and float(s.abs().max()) <= lim
    assert len(set(inp.atten.tolist())) == 3
    # the final store is really exercised: most outputs are not bf16 values
    share = float((co.round_bf16(ref.out) != ref.out).double().mean())
    assert share > 0.9, share


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_conv_is_exact_on_grid_inputs(shape):
    inp, ref = _case("grid", shape)
    out, dx, dw = _fp32_conv(inp)
    # exact before the store, hence bit-equal after it
    assert torch.equal(out.double(), ref.out)
    assert torch.equal(dx.double(), ref.dx)
    assert torch.equal(dw.double(), ref.dw)
    assert _accepts("grid", ref, out, dx, dw) == \
        {"out": True, "dx": True, "dw": True}


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_conv_is_within_bound_on_full_inputs(shape):
    inp, ref = _case("full", shape)
    out, dx, dw = _fp32_conv(inp)
    ratios = {
        "out": co.worst_ratio(co.to_bf16(out.double()), ref.out,
                              ref.bound_out()),
        "dx": co.worst_ratio(co.to_bf16(dx.double()), ref.dx, ref.bound_dx()),
        "dw": co.worst_ratio(dw, ref.dw, ref.bound_dw())}
    print("fp32 conv error/bound", shape, ratios)
    assert all(r <= 1.0 for r in ratios.values()), ratios
    # ... and the bound is not slack: the bf16 store alone comes close to it
    assert ratios["out"] > 0.5 and ratios["dx"] > 0.5, ratios


def _mutants(inp):
    """name -> the results a kernel with that one mistake would produce
    (only the ops the mistake reaches)."""
    n, c, h, w = inp.x.shape
    k = inp.gw.shape[0]
    out, dx, dw = _fp32_conv(inp)
    th = _theta32(inp)
    m = {}

    o, d, _ = _fp32_conv(inp, theta=_theta32(inp, flip_atten=True))
    m["atten in reversed tap order"] = dict(out=o, dx=d)

    o, d, _ = _fp32_conv(inp, theta=_theta32(inp, atten_view=(1, 1, 3, 1)))
    m["atten along kernel height"] = dict(out=o, dx=d)

    _, d, _ = _fp32_conv(inp, unflipped_dgrad=True)
    m["theta unflipped in dgrad"] = dict(dx=d)

    # the kernel writes a flat [K][9][C] buffer; with C and K exchanged the
    # same bytes are laid out [C][9][K]
    assert c != k
    flat = dw.permute(1, 2, 3, 0).contiguous().view(-1)
    m["C and K swapped in the dW layout"] = dict(
        dw=flat.view(k, 3, 3, c).permute(0, 3, 1, 2))

    # centre tap missing at the last image column only
    centre = torch.zeros_like(th)
    centre[:, :, 1, 1] = th[:, :, 1, 1]
    o = out.clone()
    o[..., w - 1] -= F.conv2d(inp.x.float(), centre, padding=1)[..., w - 1]
    m["one tap dropped at the last column"] = dict(out=o)

    x, dy = inp.x.float(), inp.dy.float()
    m["last 32-channel tile omitted"] = dict(
        out=F.conv2d(x[:, :c - 32], th[:, :c - 32], padding=1),
        dx=conv2d_input(x.shape, th[:k - 32], dy[:, :k - 32], padding=1)
        if k > 32 else torch.zeros_like(dx))

    m["output truncated to bf16"] = dict(out=out, dx=dx, store=co.trunc_bf16)
    return m


MUTANTS = ["atten in reversed tap order", "atten along kernel height",
           "theta unflipped in dgrad", "C and K swapped in the dW layout",
           "one tap dropped at the last column", "last 32-channel tile omitted",
           "output truncated to bf16"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_wrong_convs_are_rejected(kind, shape):
    inp, ref = _case(kind, shape)
    mutants = _mutants(inp)
    assert sorted(mutants) == sorted(MUTANTS)
    for name in MUTANTS:
        verdict = _accepts(kind, ref, **mutants[name])
        assert verdict and not any(verdict.values()), (name, kind, verdict)


@pytest.mark.parametrize("case", co.HAND_CASES,
                         ids=lambda c: "x".join(map(str, c)))
def test_every_hand_kernel_case_is_a_valid_oracle_case(case):
    """The cases the GPU tests run satisfy the oracle's preconditions (the
    exactness conditions on grid inputs, the near-tie share of theta on
    full-mantissa inputs), and an ideal kernel — float64 accumulation of the
    fp32-composed theta, one bf16 store — passes both checks on them.  So a
    failure on the GPU is the kernel's."""
    n, c, h, w, k = case
    for mode in co.HAND_MODES:
        inp, ref = co.hand_case("grid", case, mode)   # asserts exactness
        inp, ref = co.hand_case("full", case, mode)   # asserts tie share
        th = co.theta_fp32_path(inp.gw,
                                inp.atten if mode == "adaptive" else None,
                                None if mode == "plain" else inp.aw)
        x64, dy64 = inp.x.double(), inp.dy.double()
        out = co.to_bf16(F.conv2d(x64, th, padding=1))
        dx = co.to_bf16(conv2d_input(x64.shape, th, dy64, padding=1))
        assert co.worst_ratio(out, ref.out, ref.bound_out()) <= 1.0
        assert co.worst_ratio(dx, ref.dx, ref.bound_dx()) <= 1.0


def test_hand_kernel_cases_cover_the_edge_code():
    cases = co.HAND_CASES
    # wgrad M: one chunk (empty split), 2 + 1 chunks, tails, aligned
    assert {n * h * w for (n, c, h, w, k) in cases} >= \
        {48, 192, 240, 336, 672, 256}
    assert {h * w // 16 for (n, c, h, w, k) in cases} == set(range(1, 9))
    assert {w for (n, c, h, w, k) in cases} >= {1, 3, 5, 6, 7}
    assert {c for (n, c, h, w, k) in cases} >= {32, 64, 96, 160}
    assert {k for (n, c, h, w, k) in cases} >= {32, 64, 96}
    assert any(c > k for (n, c, h, w, k) in cases)
    assert any(c < k for (n, c, h, w, k) in cases)
    assert any(n % 2 for (n, c, h, w, k) in cases)
