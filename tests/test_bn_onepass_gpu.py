"""One-launch train BatchNorm (ops/csrc/bn_onepass.hip) against the two-launch
pair (ops/csrc/bn_train.hip): same bits on every output, a float64 sanity
check for both, and hipGraph capture + replay."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from flreid_amd import ops

pytestmark = pytest.mark.gpu

# [64,512,8,4]: S=512, 4 rows/stripe; [64,2048,8,4]: S=128, 16 rows/stripe;
# [64,2048]: BNNeck, 1 row/stripe; [3,64,5,7]: M=105, nslab=7, S=112 — stripes
# with one row and with none; [2,128,1,1]: M=2, the smallest legal M.
SHAPES = [(64, 512, 8, 4), (64, 2048, 8, 4), (64, 2048), (3, 64, 5, 7),
          (2, 128, 1, 1)]
STEPS = 2


def _inputs(shape, seed):
    """x and dy for STEPS train steps, on the CPU: bf16 values with exact
    zeros and negatives."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(STEPS):
        x = torch.randn(shape, generator=g)
        x[torch.rand(shape, generator=g) < 0.1] = 0.0
        dy = torch.randn(shape, generator=g)
        dy[torch.rand(shape, generator=g) < 0.1] = 0.0
        out.append((x.bfloat16(), dy.bfloat16()))
    return out


def _params(c, seed):
    """gamma, beta, running_mean, running_var.  Every 4th channel has
    gamma = beta = 0, so its pre-ReLU output is exactly 0 on every row: the
    `<= 0` edge of the ReLU mask, once in every 4-channel quad and therefore
    in every channel group of either kernel family.  Some gammas are
    negative."""
    g = torch.Generator().manual_seed(seed + 1000)
    gamma = torch.empty(c).uniform_(0.5, 1.5, generator=g)
    beta = torch.empty(c).uniform_(-1, 1, generator=g)
    gamma[1::8] *= -1
    gamma[::4] = 0.0
    beta[::4] = 0.0
    rm = torch.empty(c).uniform_(-1, 1, generator=g)
    rv = torch.empty(c).uniform_(0.5, 2.0, generator=g)
    return gamma, beta, rm, rv


def _module(shape, seed):
    c = shape[1]
    bn = (nn.BatchNorm2d(c) if len(shape) == 4 else nn.BatchNorm1d(c))
    gamma, beta, rm, rv = _params(c, seed)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta)
        bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    return bn.cuda().train()


def _to_dev(t):
    t = t.cuda()
    return t.to(memory_format=torch.channels_last) if t.dim() == 4 else t


class _Spy:
    """Stands in for the extension and records which launchers ran."""

    def __init__(self, ext):
        self._ext, self.called = ext, []

    def __getattr__(self, name):
        self.called.append(name)
        return getattr(self._ext, name)


def _run(shape, relu, onepass, monkeypatch, seed=0):
    """STEPS chained train steps; every output of every step."""
    monkeypatch.setenv("FLREID_BN_ONEPASS", "1" if onepass else "0")
    spy = _Spy(ops._load_extension())
    monkeypatch.setattr(ops, "require_extension", lambda *_a, **_k: spy)
    bn = _module(shape, seed)
    res = []
    for x, dy in _inputs(shape, seed):
        x = _to_dev(x).requires_grad_(True)
        bn.zero_grad()
        y = ops.bn_train_2d(x, bn, relu=relu)
        assert y is not None, "fused path did not engage"
        _x, _g, _b, smean, sinv = y.grad_fn.saved_tensors   # freed by backward
        smean, sinv = smean.clone(), sinv.clone()
        y.backward(_to_dev(dy))
        res.append({
            "y": y.detach().clone(), "save_mean": smean,
            "save_invstd": sinv,
            "running_mean": bn.running_mean.clone(),
            "running_var": bn.running_var.clone(),
            "num_batches_tracked": bn.num_batches_tracked.clone(),
            "dx": x.grad.clone(), "dgamma": bn.weight.grad.clone(),
            "dbeta": bn.bias.grad.clone()})
    torch.cuda.synchronize()
    return res, spy.called


@pytest.fixture(scope="module")
def two_launch():
    """The two-launch results, computed once per (shape, relu)."""
    cache = {}

    def get(shape, relu):
        if (shape, relu) not in cache:
            mp = pytest.MonkeyPatch()
            try:
                cache[(shape, relu)] = _run(shape, relu, False, mp)
            finally:
                mp.undo()
        return cache[(shape, relu)]
    return get


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_onepass_bits_equal_two_launch(shape, relu, two_launch, monkeypatch):
    ref, ref_calls = two_launch(shape, relu)
    assert "bn_train_fwd" in ref_calls and "bn_train_bwd" in ref_calls
    assert not [n for n in ref_calls if n.startswith("bn_onepass_f")
                or n.startswith("bn_onepass_b")]

    c = shape[1]
    m = int(torch.Size(shape).numel()) // c
    assert ops.bn_onepass_applies(m, c, torch.bfloat16), \
        "every shape of this test is inside the one-launch regime"
    got, calls = _run(shape, relu, True, monkeypatch)
    assert calls.count("bn_onepass_fwd") == STEPS
    assert calls.count("bn_onepass_bwd") == STEPS
    assert "bn_train_fwd" not in calls and "bn_train_bwd" not in calls

    # the ReLU mask's `<= 0` edge is there: an exact-zero output in every
    # 4-channel quad, and negatives elsewhere
    if relu:
        y0 = ref[0]["y"].float()
        flat = y0.permute(0, 2, 3, 1).reshape(-1, c) if y0.dim() == 4 else y0
        assert (flat[:, ::4] == 0).all()
    else:
        assert (ref[0]["y"] < 0).any() and (ref[0]["y"] == 0).any()

    for step, (a, b) in enumerate(zip(got, ref)):
        for k in b:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
            assert torch.equal(a[k], b[k]), (
                step, k, (a[k].double() - b[k].double()).abs().max())
    assert int(got[-1]["num_batches_tracked"]) == STEPS


def _fp64(shape, relu, seed=0):
    c = shape[1]
    gamma, beta, rm, rv = (t.double() for t in _params(c, seed))
    gamma.requires_grad_(True), beta.requires_grad_(True)
    res = []
    for x, dy in _inputs(shape, seed):
        x = x.double().requires_grad_(True)
        y = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
        if relu:
            y = torch.relu(y)
        dx, dg, db = torch.autograd.grad(y, [x, gamma, beta], dy.double())
        res.append({"y": y.detach(), "running_mean": rm.clone(),
                    "running_var": rv.clone(), "dx": dx, "dgamma": dg,
                    "dbeta": db})
    return res


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_onepass_matches_fp64(shape, relu, monkeypatch):
    """Both GPU paths could be wrong together: float64 on the CPU, at the
    bf16 tolerances of test_bn_train_fused_matches_torch."""
    got, _ = _run(shape, relu, True, monkeypatch)
    atol = 5e-2
    for step, (a, b) in enumerate(zip(got, _fp64(shape, relu))):
        def close(k, atol, rtol):
            d = a[k].detach().double().cpu()
            assert torch.allclose(d, b[k], atol=atol, rtol=rtol), (
                step, k, (d - b[k]).abs().max())
        close("y", atol, 5e-2)
        close("running_mean", atol, 1e-2)
        close("running_var", atol, 1e-2)
        close("dx", atol * 10, 5e-2)
        close("dgamma", atol * 10, 5e-2)
        close("dbeta", atol * 10, 5e-2)


def test_onepass_graph_capture_replays(monkeypatch):
    """The head step is replayed from a hipGraph (runtime/hipgraph.py): one
    eager warm-up step, the capture with its replay, one more replay — and
    every step meets the eager chain, running stats included."""
    from flreid_amd.runtime.hipgraph import GraphedStep
    monkeypatch.setenv("FLREID_BN_ONEPASS", "1")
    shape = (64, 512, 8, 4)
    x_cpu, dy_cpu = _inputs(shape, 0)[0]
    n_steps = 3

    def make():
        bn = _module(shape, 0)

        def step(x, dy):
            x = x.detach().requires_grad_(True)
            bn.weight.grad = bn.bias.grad = None
            y = ops.bn_train_2d(x, bn, relu=True)
            y.backward(dy)
            return y.detach(), x.grad, bn.weight.grad, bn.bias.grad

        def snap(outs):
            return [o.clone() for o in outs] + [
                bn.running_mean.clone(), bn.running_var.clone(),
                bn.num_batches_tracked.clone()]
        return step, snap

    x, dy = _to_dev(x_cpu), _to_dev(dy_cpu)

    step, snap = make()
    eager = [snap(step(x, dy)) for _ in range(n_steps)]

    step, snap = make()
    gs = GraphedStep(step)
    got = [snap(gs.warmup(x, dy)), snap(gs.capture(x, dy)), snap(gs(x, dy))]
    torch.cuda.synchronize()
    assert int(got[-1][-1]) == n_steps
    for i, (g, want) in enumerate(zip(got, eager)):
        for j, (a, b) in enumerate(zip(g, want)):
            assert torch.equal(a, b), (i, j)
