"""Routing of train BatchNorm between the one-launch kernels, the two-launch
pair and torch — host logic only, no GPU."""

import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from flreid_amd import ops
from flreid_amd.models.resnet import Bottleneck, EvalFusedBatchNorm2d

BF16 = torch.bfloat16


def test_flagship_shapes_are_inside_the_regime(monkeypatch):
    monkeypatch.delenv("FLREID_BN_ONEPASS", raising=False)
    if not ops.extension_available():
        # without the extension nothing fused runs at all
        assert not ops.bn_onepass_applies(2048, 512, BF16)
        return
    for m, c in ((2048, 512), (2048, 2048), (64, 2048), (105, 64), (2, 128)):
        assert ops.bn_onepass_applies(m, c, BF16), (m, c)


def test_switch_and_out_of_regime_take_the_two_launch_pair(monkeypatch):
    monkeypatch.setenv("FLREID_BN_ONEPASS", "0")
    assert not ops.bn_onepass_applies(2048, 512, BF16)
    monkeypatch.setenv("FLREID_BN_ONEPASS", "1")
    # 64 rows per stripe (M = 8192, S = 128) do not fit in registers
    assert not ops.bn_onepass_applies(8192, 512, BF16)
    assert not ops.bn_onepass_applies(16384, 128, BF16)
    # fp32 stays on the pair; so do the shapes the pair itself refuses
    assert not ops.bn_onepass_applies(2048, 512, torch.float32)
    assert not ops.bn_onepass_applies(2048, 48, BF16)
    assert not ops.bn_onepass_applies(1, 512, BF16)


def test_cpu_and_non_channels_last_decline():
    bn = nn.BatchNorm2d(64).train()
    x = torch.randn(4, 64, 4, 4)
    assert ops.bn_train_2d(x, bn) is None
    assert ops.bn_train_2d(x.to(memory_format=torch.channels_last), bn) is None


def test_eval_mode_never_reaches_the_train_kernels(monkeypatch):
    def boom(*_a, **_k):
        raise AssertionError("train BN called in eval mode")
    monkeypatch.setattr(ops, "bn_train_2d", boom)
    bn = EvalFusedBatchNorm2d(64).eval()
    x = torch.randn(2, 64, 4, 4)
    assert torch.equal(bn(x), nn.BatchNorm2d.forward(bn, x))


def test_bottleneck_cpu_is_the_plain_composition():
    torch.manual_seed(0)
    blk = Bottleneck(64, 16).train()
    ref = copy.deepcopy(blk)
    x = torch.randn(4, 64, 6, 5, requires_grad=True)
    x_ref = x.detach().clone().requires_grad_(True)

    out = blk(x)

    def bn(m, t):
        m.num_batches_tracked += 1
        return F.batch_norm(t, m.running_mean, m.running_var, m.weight,
                            m.bias, True, m.momentum, m.eps)
    o = F.relu(bn(ref.bn1, ref.conv1(x_ref)))
    o = F.relu(bn(ref.bn2, ref.conv2(o)))
    o = bn(ref.bn3, ref.conv3(o))
    want = F.relu(o + x_ref)

    assert torch.equal(out, want)
    g = torch.randn_like(want)
    out.backward(g)
    want.backward(g)
    assert torch.equal(x.grad, x_ref.grad)
    for (n, p), (_n, q) in zip(blk.named_parameters(),
                               ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, b), (_n, q) in zip(blk.named_buffers(), ref.named_buffers()):
        assert torch.equal(b, q), n
