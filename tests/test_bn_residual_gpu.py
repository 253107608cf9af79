"""relu(bn(x) + identity) inside the BN kernels (ops/csrc/bn_onepass.hip train,
ops/csrc/elementwise.hip eval) against the chain this tree builds from its own
unfused ops: bn, then `+ identity`, then ReLU, with autograd through it.
Everything is compared with torch.equal; there is no tolerance."""

import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from flreid_amd import ops
from flreid_amd.models.resnet import Bottleneck

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
STEPS = 2

# One shape per instantiation bn_onepass_config returns — [64,512,8,4] (the
# 8-channel 1024-thread tile, 4 rows per stripe), [64,2048,8,4] (16 channels,
# 16 rows per stripe), [2,64,1,1] (one row per stripe; M = 2, the smallest) —
# of which the first two are the head-epoch shapes; [2,64,5,3]: M = 30, ragged
# stripes; [2,64,17,16]: M = 544 at C = 64 is outside the one-launch regime.
IN_REGIME = [(2, 64, 1, 1), (2, 64, 5, 3), (64, 512, 8, 4), (64, 2048, 8, 4)]
OUTSIDE = (2, 64, 17, 16)
CONFIG = {(2, 64, 1, 1): 5, (2, 64, 5, 3): 5, (64, 512, 8, 4): 2,
          (64, 2048, 8, 4): 4}


def _cl(t):
    t = t.cuda()
    return t.to(memory_format=torch.channels_last) if t.dim() == 4 else t


def _bn(c, seed, dim=4):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(c) if dim == 4 else nn.BatchNorm1d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.empty(c).uniform_(0.5, 1.5, generator=g))
        bn.bias.copy_(torch.empty(c).uniform_(-0.5, 0.5, generator=g))
        bn.weight[1::8] *= -1
        bn.running_mean.copy_(torch.empty(c).uniform_(-1, 1, generator=g))
        bn.running_var.copy_(torch.empty(c).uniform_(0.5, 2.0, generator=g))
    return bn.cuda()


def _train_inputs(shape, seed):
    """Per step: x, the identity's source r, and dz — finite bf16 with exact
    zeros, so that bn(x) + identity straddles zero."""
    g = torch.Generator().manual_seed(seed)
    steps = []
    for _ in range(STEPS):
        ts = []
        for _k in range(3):
            t = torch.randn(shape, generator=g)
            t[torch.rand(shape, generator=g) < 0.05] = 0.0
            ts.append(_cl(t.to(BF16)))
        steps.append(ts)
    return steps


class _Spy:
    """Stands in for the extension and records which launchers ran."""

    def __init__(self, ext):
        self._ext, self.called = ext, []

    def __getattr__(self, name):
        self.called.append(name)
        return getattr(self._ext, name)


def _add_relu(x, bn, identity, fused):
    """What a residual block does with its last BN."""
    if fused:
        z = ops.bn_train_2d(x, bn, residual=identity)
        if z is not None:
            return z
    y = ops.bn_train_2d(x, bn)
    assert y is not None, "fused train BN did not engage"
    return F.relu(y + identity)


def _run_train(shape, downsample, fused, monkeypatch):
    """STEPS chained steps.  The identity is a leaf (the block input) or, with
    `downsample`, the output of a second train BN."""
    monkeypatch.setenv("FLREID_BN_ONEPASS", "1")
    monkeypatch.delenv("FLREID_BN_RESIDUAL", raising=False)
    spy = _Spy(ops._load_extension())
    monkeypatch.setattr(ops, "require_extension", lambda *_a, **_k: spy)
    c = shape[1]
    bn, bn_ds = _bn(c, 1).train(), _bn(c, 2).train()
    res = []
    for x, r, dz in _train_inputs(shape, 0):
        x = x.clone().requires_grad_(True)
        r = r.clone().requires_grad_(True)
        bn.zero_grad(), bn_ds.zero_grad()
        identity = ops.bn_train_2d(r, bn_ds) if downsample else r
        assert identity is not None
        z = _add_relu(x, bn, identity, fused)
        z.backward(dz)
        out = {"z": z.detach().clone(), "dx": x.grad.clone(),
               "dres": r.grad.clone(), "dgamma": bn.weight.grad.clone(),
               "dbeta": bn.bias.grad.clone(),
               "running_mean": bn.running_mean.clone(),
               "running_var": bn.running_var.clone(),
               "num_batches_tracked": bn.num_batches_tracked.clone()}
        if downsample:
            out["ds_dgamma"] = bn_ds.weight.grad.clone()
            out["ds_dbeta"] = bn_ds.bias.grad.clone()
        res.append(out)
    torch.cuda.synchronize()
    return res, spy.called


def _assert_same(got, ref):
    for step, (a, b) in enumerate(zip(got, ref)):
        for k in b:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
            assert torch.equal(a[k], b[k]), (
                step, k, (a[k].double() - b[k].double()).abs().max())
    assert int(got[-1]["num_batches_tracked"]) == STEPS


def _assert_mask_tested(ref):
    for r in ref:
        share = float((r["z"] == 0).float().mean())
        assert 0.10 < share < 0.90, share
        for k in ("z", "dx", "dres"):
            assert torch.isfinite(r[k].float()).all(), k


@pytest.mark.parametrize("downsample", [False, True],
                         ids=["block_input", "downsample_bn"])
@pytest.mark.parametrize("shape", IN_REGIME,
                         ids=lambda s: "x".join(map(str, s)))
def test_train_residual_bits_equal_chain(shape, downsample, monkeypatch):
    c = shape[1]
    m = int(torch.Size(shape).numel()) // c
    assert ops._load_extension().bn_onepass_config(m, c) == CONFIG[shape]

    ref, ref_calls = _run_train(shape, downsample, False, monkeypatch)
    assert "bn_onepass_res_fwd" not in ref_calls
    _assert_mask_tested(ref)

    got, calls = _run_train(shape, downsample, True, monkeypatch)
    assert calls.count("bn_onepass_res_fwd") == STEPS
    assert calls.count("bn_onepass_res_bwd") == STEPS
    _assert_same(got, ref)


def test_train_residual_outside_regime_falls_back(monkeypatch):
    c = OUTSIDE[1]
    m = int(torch.Size(OUTSIDE).numel()) // c
    assert not ops.bn_onepass_applies(m, c, BF16)
    x, r, _dz = _train_inputs(OUTSIDE, 0)[0]
    assert ops.bn_train_2d(x, _bn(c, 1).train(), residual=r) is None

    ref, _ = _run_train(OUTSIDE, True, False, monkeypatch)
    _assert_mask_tested(ref)
    got, calls = _run_train(OUTSIDE, True, True, monkeypatch)
    assert "bn_onepass_res_fwd" not in calls
    assert "bn_train_fwd" in calls
    _assert_same(got, ref)


def test_train_residual_declines_and_rejects(monkeypatch):
    shape = (2, 64, 5, 3)
    x, r, _dz = _train_inputs(shape, 0)[0]
    bn = _bn(64, 1).train()
    with pytest.raises(ValueError):
        ops.bn_train_2d(x, bn, relu=True, residual=r)
    assert ops.bn_train_2d(x, bn, residual=r.float()) is None
    assert ops.bn_train_2d(x, bn, residual=r.contiguous()) is None
    assert ops.bn_train_2d(x, bn, residual=r[:1]) is None
    monkeypatch.setenv("FLREID_BN_RESIDUAL", "0")
    assert ops.bn_train_2d(x, bn, residual=r) is None


def test_train_residual_graph_capture_replays(monkeypatch):
    """One eager warm-up step, the capture with its replay, one more replay,
    each on fresh inputs — and every step meets the eager chain."""
    from flreid_amd.runtime.hipgraph import GraphedStep
    monkeypatch.setenv("FLREID_BN_ONEPASS", "1")
    monkeypatch.delenv("FLREID_BN_RESIDUAL", raising=False)
    shape = (64, 512, 8, 4)
    g = torch.Generator().manual_seed(7)
    batches = [[_cl(torch.randn(shape, generator=g).to(BF16))
                for _k in range(3)] for _ in range(3)]

    def make(fused):
        bn = _bn(shape[1], 1).train()

        def step(x, r, dz):
            x = x.detach().requires_grad_(True)
            r = r.detach().requires_grad_(True)
            bn.weight.grad = bn.bias.grad = None
            z = _add_relu(x, bn, r, fused)
            z.backward(dz)
            return z.detach(), x.grad, r.grad, bn.weight.grad, bn.bias.grad

        def snap(outs):
            return [o.clone() for o in outs] + [
                bn.running_mean.clone(), bn.running_var.clone(),
                bn.num_batches_tracked.clone()]
        return step, snap

    step, snap = make(False)
    eager = [snap(step(*b)) for b in batches]

    step, snap = make(True)
    gs = GraphedStep(step)
    got = [snap(gs.warmup(*batches[0])), snap(gs.capture(*batches[1])),
           snap(gs(*batches[2]))]
    torch.cuda.synchronize()
    assert int(got[-1][-1]) == len(batches)
    for i, (a_step, b_step) in enumerate(zip(got, eager)):
        for j, (a, b) in enumerate(zip(a_step, b_step)):
            assert torch.equal(a, b), (i, j)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bottleneck_switch_off_matches_fused(training, monkeypatch):
    """FLREID_BN_RESIDUAL=0 is the three-kernel sequence; the default route
    gives the same block output and gradients."""
    torch.manual_seed(0)
    blk = Bottleneck(256, 64).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2.0)
    blk.train(training)
    # bf16 like the cached features the head epoch trains on: the identity
    # then has the dtype of the autocast conv output
    x0 = _cl(torch.randn(8, 256, 8, 4).to(BF16))
    dz = _cl(torch.randn(8, 256, 8, 4).to(BF16))

    def run(switch):
        if switch is None:
            monkeypatch.delenv("FLREID_BN_RESIDUAL", raising=False)
        else:
            monkeypatch.setenv("FLREID_BN_RESIDUAL", switch)
        b = copy.deepcopy(blk)
        x = x0.clone().requires_grad_(training)
        # the frozen forwards run without autograd, like prototype capture
        with torch.autocast("cuda", dtype=BF16), \
                torch.set_grad_enabled(training):
            z = b(x)
        outs = {"z": z.detach().clone()}
        if training:
            z.backward(dz)
            outs["dx"] = x.grad.clone()
            for n, p in b.named_parameters():
                outs["grad " + n] = p.grad.clone()
        for n, t in b.named_buffers():
            outs["buf " + n] = t.clone()
        return outs

    calls = []
    for name in ("bn_train_2d", "bn_eval_2d"):
        real = getattr(ops, name)

        def spy(*a, _real=real, **k):
            out = _real(*a, **k)
            if k.get("residual") is not None:
                calls.append(out is not None)
            return out
        monkeypatch.setattr(ops, name, spy)

    # The library convolutions are not reproducible from call to call until
    # they are told to be and have chosen their algorithms: without this the
    # switched-off block differs from itself in the conv weight gradients.
    with torch.backends.cudnn.flags(enabled=True, benchmark=False,
                                    deterministic=True):
        run("0")
        del calls[:]
        ref = run("0")
        assert calls == [False]
        got = run(None)
        assert calls == [False, True], "the fused route did not engage"
    share = float((ref["z"] == 0).float().mean())
    assert 0.10 < share < 0.90, share
    assert ref.keys() == got.keys()
    assert not [k for k in ref if not torch.equal(got[k], ref[k])]


# ---------------------------------------------------------------- eval kernel

def _eval_raw(x, bn, res, wide):
    """The eval launcher itself: wide = 0 keeps the one-element-per-thread
    kernel whatever the layout."""
    ext = ops.require_extension("bn_eval test")
    if x.dim() == 2:
        nhwc, hw = True, 1
    else:
        nhwc = x.is_contiguous(memory_format=torch.channels_last)
        assert nhwc or x.is_contiguous()
        hw = x.shape[2] * x.shape[3]
    out = torch.empty_like(x)
    ext.bn_eval_res(x.data_ptr(), res.data_ptr() if res is not None else 0,
                    out.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                    bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                    x.numel(), x.shape[1], hw, float(bn.eps), int(nhwc), 0,
                    wide, 1 if x.dtype == BF16 else 0,
                    torch.cuda.current_stream().cuda_stream)
    return out


def _offset_cl(shape, dtype, g):
    """Channels-last tensor that starts one element into its buffer."""
    n, c, h, w = shape
    buf = torch.randn(n * h * w * c + 8, generator=g).to(dtype).cuda()
    return buf[1:1 + n * h * w * c].view(n, h, w, c).permute(0, 3, 1, 2)


EVAL_CASES = {
    # numel 6720 is no multiple of the 2048 (bf16) / 1024 (fp32) block span
    "cl_bf16": ((3, 64, 5, 7), BF16, "cl"),
    "cl_fp32": ((3, 64, 5, 7), torch.float32, "cl"),
    "c24": ((4, 24, 4, 4), BF16, "cl"),            # C no power of two
    "c20": ((4, 20, 4, 4), BF16, "cl"),            # C % 8 != 0: scalar
    "nchw": ((3, 64, 5, 7), BF16, "nchw"),         # scalar
    "rows": ((64, 2048), BF16, "2d"),
    "unaligned": ((3, 64, 5, 7), BF16, "offset"),  # scalar
}


@pytest.mark.parametrize("case", list(EVAL_CASES))
def test_eval_wide_and_residual_bits(case, monkeypatch):
    monkeypatch.delenv("FLREID_BN_RESIDUAL", raising=False)
    shape, dtype, layout = EVAL_CASES[case]
    g = torch.Generator().manual_seed(3)
    if layout == "offset":
        x, res = _offset_cl(shape, dtype, g), _offset_cl(shape, dtype, g)
        assert x.data_ptr() % 16 != 0
        assert x.is_contiguous(memory_format=torch.channels_last)
    else:
        x = torch.randn(shape, generator=g).to(dtype).cuda()
        res = torch.randn(shape, generator=g).to(dtype).cuda()
        if layout == "cl":
            x, res = _cl(x), _cl(res)
    bn = _bn(shape[1], 4, dim=len(shape)).eval()

    scalar = _eval_raw(x, bn, None, 0)
    # float64 sanity check of the reference itself
    c_view = (1, -1) + (1,) * (x.dim() - 2)
    want = ((x.double() - bn.running_mean.double().view(c_view))
            / torch.sqrt(bn.running_var.double().view(c_view) + bn.eps)
            * bn.weight.double().view(c_view) + bn.bias.double().view(c_view))
    tol = 2.0 ** -7 if dtype == BF16 else 1e-5
    assert ((scalar.double() - want).abs() <= tol * (1 + want.abs())).all()

    chain = F.relu(scalar + res)
    share = float((chain == 0).float().mean())
    assert 0.10 < share < 0.90, share

    # the launcher's own choice (wide where it applies) against scalar
    assert torch.equal(_eval_raw(x, bn, None, 1), scalar)
    assert torch.equal(_eval_raw(x, bn, res, 1), chain)
    assert torch.equal(_eval_raw(x, bn, res, 0), chain)
    # and through the op
    for relu in (False, True):
        got = ops.bn_eval_2d(x, bn, relu=relu)
        assert torch.equal(got, F.relu(scalar) if relu else scalar)
    got = ops.bn_eval_2d(x, bn, residual=res)
    assert got is not None and got.stride() == x.stride()
    assert torch.equal(got, chain)


def test_eval_residual_declines(monkeypatch):
    monkeypatch.delenv("FLREID_BN_RESIDUAL", raising=False)
    bn = _bn(64, 4).eval()
    x = _cl(torch.randn(2, 64, 4, 4).to(BF16))
    r = _cl(torch.randn(2, 64, 4, 4).to(BF16))
    with pytest.raises(ValueError):
        ops.bn_eval_2d(x, bn, relu=True, residual=r)
    assert ops.bn_eval_2d(x, bn, residual=r.float()) is None
    assert ops.bn_eval_2d(x, bn, residual=r.contiguous()) is None
    assert ops.bn_eval_2d(x, bn, residual=r.clone().requires_grad_(True)) \
        is None
    monkeypatch.setenv("FLREID_BN_RESIDUAL", "0")
    assert ops.bn_eval_2d(x, bn, residual=r) is None
