"""The residual blocks on the CPU: handing the identity to the last BatchNorm
falls through there, so Bottleneck and BasicBlock stay the plain composition —
same outputs, gradients, buffers and state-dict keys.  No GPU."""

import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from flreid_amd import ops
from flreid_amd.models.resnet import (BasicBlock, Bottleneck,
                                      EvalFusedBatchNorm2d, conv1x1)


def _bn(m, t, training):
    if training:
        m.num_batches_tracked += 1
    return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias,
                        training, m.momentum, m.eps)


def _plain(blk, x, training):
    identity = x
    if blk.downsample is not None:
        identity = _bn(blk.downsample[1], blk.downsample[0](x), training)
    o = F.relu(_bn(blk.bn1, blk.conv1(x), training))
    if isinstance(blk, Bottleneck):
        o = F.relu(_bn(blk.bn2, blk.conv2(o), training))
        o = _bn(blk.bn3, blk.conv3(o), training)
    else:
        o = _bn(blk.bn2, blk.conv2(o), training)
    return F.relu(o + identity)


def _make(kind, downsample):
    torch.manual_seed(0)
    cout = 64 if kind is Bottleneck else 16
    ds = None
    if downsample:
        ds = nn.Sequential(conv1x1(32, cout), EvalFusedBatchNorm2d(cout))
    blk = kind(32 if downsample else cout, 16, downsample=ds)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2.0)
    return blk, (32 if downsample else cout)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("downsample", [False, True], ids=["plain", "ds"])
@pytest.mark.parametrize("kind", [Bottleneck, BasicBlock],
                         ids=["bottleneck", "basic"])
def test_block_cpu_is_the_plain_composition(kind, downsample, training):
    blk, cin = _make(kind, downsample)
    blk.train(training)
    ref = copy.deepcopy(blk)
    x = torch.randn(4, cin, 6, 5, requires_grad=True)
    x_ref = x.detach().clone().requires_grad_(True)

    out = blk(x)
    want = _plain(ref, x_ref, training)
    assert torch.equal(out, want)
    assert 0.1 < float((out == 0).float().mean()) < 0.9

    g = torch.randn_like(want)
    out.backward(g)
    want.backward(g)
    assert torch.equal(x.grad, x_ref.grad)
    for (n, p), (_n, q) in zip(blk.named_parameters(),
                               ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, b), (_n, q) in zip(blk.named_buffers(), ref.named_buffers()):
        assert torch.equal(b, q), n


def test_residual_entry_declines_on_cpu_and_state_dict_is_unchanged():
    bn = EvalFusedBatchNorm2d(16)
    x, r = torch.randn(2, 16, 3, 3), torch.randn(2, 16, 3, 3)
    for training in (True, False):
        bn.train(training)
        assert bn(x, residual=r) is None
        assert ops.bn_train_2d(x, bn, residual=r) is None
        assert ops.bn_eval_2d(x, bn, residual=r) is None
    assert int(bn.num_batches_tracked) == 0
    assert sorted(bn.state_dict()) == sorted(nn.BatchNorm2d(16).state_dict())
    keys = set(Bottleneck(64, 16).state_dict())
    assert {"bn3.weight", "bn3.running_mean", "conv3.weight"} <= keys
    assert not [k for k in keys if "relu" in k or "residual" in k]


def test_a_swapped_in_norm_layer_keeps_the_plain_sequence():
    blk = Bottleneck(64, 16).eval()
    blk.bn3 = nn.BatchNorm2d(64).eval()
    x = torch.randn(2, 64, 4, 4)
    assert torch.equal(blk(x), _plain(blk, x, False))
