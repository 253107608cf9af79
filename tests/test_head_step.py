"""head_step_reference (the fp64 ground truth of the one-pass FedSTIL head
update) against the chain it replaces, on CPU: torch.optim.Adam (non-fused,
fp32) fed dw + λ·sign(aw − aw0), then ref.adaptive_compose for θ."""

import pytest
import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref

EPS32 = float(torch.finfo(torch.float32).eps)

# Largest error measured here over every case below, in units of
# eps32 · max|reference| per tensor (an fp32 ulp at the tensor's scale):
#   aw 0.80, exp_avg 0.78, exp_avg_sq 1.93, θ 1.00, drift 2.59 (an fp32 sum
#   of 15-1300 terms).  The asserts allow 4× these.
MEASURED_ULPS = {"aw": 0.80, "m": 0.78, "v": 1.93, "theta": 1.00,
                 "drift": 2.59}


def _ulps(got, want):
    scale = EPS32 * float(want.abs().max().clamp_min(1e-30))
    return float((got.double() - want).abs().max()) / scale


def _case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    aw0 = torch.randn(shape, generator=g) * 0.05
    aw = aw0.clone()
    # both signs of drift, and exact ties aw == aw0 on a third of the weights
    delta = torch.randn(shape, generator=g) * 1e-3
    delta[torch.rand(shape, generator=g) < 1 / 3] = 0.0
    aw += delta
    gw = torch.randn(shape, generator=g) * 0.05
    atten = torch.rand(shape[-1], generator=g)
    dws = [torch.randn(shape, generator=g) * 1e-2 for _ in range(3)]
    return aw, aw0, gw, atten, dws


@pytest.mark.parametrize("shape", [(7, 12), (3, 5), (8, 4, 3, 3), (20, 65)])
@pytest.mark.parametrize("lam,wd", [(0.0, 0.0), (1e-4, 1e-5), (1e-4, 0.0)])
def test_reference_matches_torch_adam(shape, lam, wd):
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    aw, aw0, gw, atten, dws = _case(shape, seed=sum(shape))
    lam32 = torch.tensor(lam, dtype=torch.float32)

    p = torch.nn.Parameter(aw.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps,
                           weight_decay=wd, foreach=False, fused=False)
    a64, m64, v64 = aw.double(), torch.zeros(shape).double(), \
        torch.zeros(shape).double()
    worst = dict.fromkeys(MEASURED_ULPS, 0.0)
    for k, dw in enumerate(dws, start=1):
        drift32 = ref.l1_drift([(p.detach(), aw0)])
        p.grad = dw + lam32 * torch.sign(p.detach() - aw0)
        opt.step()
        theta32 = ref.adaptive_compose(gw, atten, p.detach())

        a64, m64, v64, th64, drift64 = ref.head_step_reference(
            a64, aw0, dw, m64, v64, k, lr, b1, b2, wd, eps, lam, gw, atten)
        st = opt.state[p]
        for name, got, want in (("aw", p.detach(), a64),
                                ("m", st["exp_avg"], m64),
                                ("v", st["exp_avg_sq"], v64),
                                ("theta", theta32, th64),
                                ("drift", drift32.reshape(1),
                                 drift64.reshape(1))):
            worst[name] = max(worst[name], _ulps(got, want))
    print("head_step_reference vs torch Adam, ulps:", shape, lam, wd, worst)
    for name, bound in MEASURED_ULPS.items():
        assert worst[name] <= 4 * bound, (name, worst[name])


def test_cpu_op_runs_the_reference():
    """ops.head_step on CPU tensors: in-place update from the reference,
    step advanced, drift in the partials."""
    shape = (6, 8)
    aw, aw0, gw, atten, dws = _case(shape, seed=3)
    m, v = torch.zeros(shape), torch.zeros(shape)
    step = torch.zeros(())
    theta = torch.empty(shape, dtype=torch.bfloat16)
    row = {"aw": aw.clone(), "aw0": aw0, "dw": dws[0], "m": m, "v": v,
           "step": step, "gw": gw, "atten": atten, "theta": theta}
    partials = torch.zeros(ops.head_step_partials([row]),
                           dtype=torch.float64)
    a64, m64, v64, th64, d64 = ref.head_step_reference(
        aw, aw0, dws[0], m, v, 1, 1e-3, 0.9, 0.999, 1e-5, 1e-8, 1e-4, gw,
        atten)
    ops.head_step([row], partials, 1e-3, 0.9, 0.999, 1e-5, 1e-8, 1e-4)
    assert float(step) == 1.0
    assert torch.equal(row["aw"], a64.float())
    assert torch.equal(m, m64.float()) and torch.equal(v, v64.float())
    assert torch.equal(theta, th64.to(torch.bfloat16))
    assert float(partials.sum()) == float(d64)


def test_empty_table_raises():
    with pytest.raises(ValueError):
        ops.head_step([], torch.zeros(1, dtype=torch.float64), 1e-3, 0.9,
                      0.999, 0.0, 1e-8, 0.0)
