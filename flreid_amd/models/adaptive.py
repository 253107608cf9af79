"""FedSTIL additive-decomposition layers (ref:methods/fedstil.py:24-225).

θ = global_weight_atten ⊙ global_weight + adaptive_weight, with the attention
vector broadcast over the LAST weight dimension
(ref:methods/fedstil.py:66-67,84-92).  Only `adaptive_weight` (and bias)
train; `global_weight` is the federated state and `global_weight_atten` is a
fixed mixing vector (it becomes a learnable stacked attention in the
fedstil-atten variant — ref:methods/fedstil_atten.py).

`init_training_weights()` (no args) is the dispatch-time re-initialisation:
atten resets to `atten_default` and adaptive_weight to (1−atten)·W_glob, so
the composed weight right after dispatch equals the dispatched global weight
(ref:methods/fedstil.py:53-82, applied at ref:methods/fedstil.py:879-911).
`initial_*` snapshots anchor the round's L1 drift regulariser
(ref:methods/fedstil.py:639-644).

On GPU the composition runs through the fused HIP compose2 kernel
(flreid_amd.ops.adaptive_compose) so θ is produced in one pass; the backward
for adaptive_weight is identity and atten (when learnable) reduces over all
dims but the last.  The Linear and Conv2d forwards only name the layer's
shape; which kernels run is decided in ops.conv3x3_try and
ops.adaptive_linear alone.
"""

from __future__ import annotations

import contextlib
import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn import Parameter

from flreid_amd import ops


def live_theta_enabled() -> bool:
    return os.environ.get("FLREID_LIVE_THETA", "1") != "0"


class _LiveThetaFn(torch.autograd.Function):
    """adaptive_weight → the leaf's live bf16 θ.  Forward hands out the
    buffer; backward stashes the incoming bf16 dθ for the head_step kernel
    (dθ IS d(adaptive_weight): identity composition) and returns no
    gradient, so adaptive_weight.grad stays None."""

    @staticmethod
    def forward(ctx, aw, live):
        ctx.live = live
        return live.theta.detach()

    @staticmethod
    def backward(ctx, g):
        live = ctx.live
        if g.dtype != torch.bfloat16:
            g = g.to(torch.bfloat16)
        if not ops.same_layout(g, live.theta):
            # e.g. an NCHW-ordered conv2d_weight result for a channels-last θ
            g = torch.empty_like(live.theta).copy_(g)
        live.grad = g if live.grad is None else live.grad + g
        return None, None


class LiveTheta:
    """θ = atten ⊙ gw + aw of one adaptive leaf in bf16, alive for exactly
    one head epoch (live_theta_scope): composed at epoch start, kept current
    by the head_step kernel after every update, dropped at epoch end.
    Every consumer (F.conv2d, F.linear, the 3×3 and 1×1 routes, the
    classifier GEMM) sees an ordinary bf16 weight; `grad` is the bf16 dθ the
    last backward left for the kernel."""

    def __init__(self, theta: torch.Tensor):
        self.theta = theta
        self.grad: Optional[torch.Tensor] = None

    def __call__(self, adaptive_weight: torch.Tensor) -> torch.Tensor:
        return _LiveThetaFn.apply(adaptive_weight, self)


@contextlib.contextmanager
def live_theta_scope(leaves, buffers):
    """Attach a freshly composed live θ to every leaf for the length of one
    head epoch; detached on exit, exceptions included.  Nothing outside the
    scope ever reads the buffers (herding, validation, uploads and dispatch
    re-inits go through composed_weight), so a stale θ cannot be observed."""
    ext = ops.require_extension("compose2")
    try:
        for leaf, buf in zip(leaves, buffers):
            ops.compose_theta_bf16(ext, leaf.global_weight,
                                   leaf.global_weight_atten,
                                   leaf.adaptive_weight, out=buf)
            leaf._live = LiveTheta(buf)
        yield
    finally:
        for leaf in leaves:
            leaf._live = None


class AdaptiveBase(nn.Module):
    """Holds the decomposed parameter set; subclasses implement forward."""

    _live: Optional[LiveTheta] = None     # set only inside live_theta_scope

    def __init__(self, global_weight: torch.Tensor,
                 global_weight_atten: Optional[torch.Tensor] = None,
                 adaptive_weight: Optional[torch.Tensor] = None,
                 adaptive_bias: Optional[torch.Tensor] = None,
                 atten_default: float = 0.80, atten_trainable: bool = False,
                 **kwargs):
        super().__init__()
        self.atten_default = atten_default
        self.atten_trainable = atten_trainable
        self.global_weight = Parameter(torch.empty(0), requires_grad=False)
        self.global_weight_atten = Parameter(torch.empty(0), requires_grad=False)
        self.adaptive_weight = Parameter(torch.empty(0))
        self.adaptive_bias = Parameter(torch.empty(0)) if adaptive_bias is not None else None
        self.initial_global_weight_atten = Parameter(torch.empty(0), requires_grad=False)
        self.initial_adaptive_weight = Parameter(torch.empty(0), requires_grad=False)
        self.init_training_weights(global_weight, global_weight_atten,
                                   adaptive_weight, adaptive_bias)

    @staticmethod
    def _assign(param: Parameter, value: torch.Tensor) -> None:
        """In-place when shapes match (keeps optimizer state and captured
        hipGraph pointers valid across per-round re-inits); rebind otherwise
        (clearing any stale gradient of the old shape)."""
        if param.data.shape == value.shape:
            param.data.copy_(value)
        else:
            param.data = value.detach().clone().to(param.device)
            param.grad = None

    @torch.no_grad()
    def init_training_weights(self, global_weight=None, global_weight_atten=None,
                              adaptive_weight=None, adaptive_bias=None) -> None:
        if global_weight is None:
            global_weight = self.global_weight.data
        self._assign(self.global_weight, global_weight.detach())
        self.global_weight.requires_grad = False

        if global_weight_atten is None:
            global_weight_atten = torch.ones(
                self.global_weight.data.shape[-1],
                device=self.global_weight.device) * self.atten_default
        self._assign(self.global_weight_atten, global_weight_atten.detach())
        self._assign(self.initial_global_weight_atten, global_weight_atten.detach())
        self.global_weight_atten.requires_grad = self.atten_trainable

        if adaptive_weight is None:
            adaptive_weight = (1.0 - self.global_weight_atten.data) * self.global_weight.data
        self._assign(self.adaptive_weight, adaptive_weight.detach())
        self._assign(self.initial_adaptive_weight, adaptive_weight.detach())
        self.adaptive_weight.requires_grad = True

        if self.adaptive_bias is not None and adaptive_bias is not None:
            self._assign(self.adaptive_bias, adaptive_bias.detach())
            self.adaptive_bias.requires_grad = True

    def composed_weight(self) -> torch.Tensor:
        return ops.adaptive_compose(self.global_weight, self.global_weight_atten,
                                    self.adaptive_weight)

    def _weights(self):
        """(weight, atten, aw) as the ops routes take them: the live bf16 θ
        with (None, None) during a head epoch — read, not composed — else
        the decomposed parameters."""
        if self._live is not None:
            return self._live(self.adaptive_weight), None, None
        return (self.global_weight, self.global_weight_atten,
                self.adaptive_weight)

    def drift_pairs(self):
        """(current, round-start) pairs for the L1 drift regulariser."""
        return [(self.global_weight_atten, self.initial_global_weight_atten),
                (self.adaptive_weight, self.initial_adaptive_weight)]


class AdaptiveLinear(AdaptiveBase):
    def forward(self, data: torch.Tensor) -> torch.Tensor:
        weight, atten, aw = self._weights()
        # the K2 GEMM (compose-in-prologue, or the tile loop on the live θ);
        # None off-GPU, for 3-D input or when atten trains
        y = ops.adaptive_linear(data, weight, atten, aw, self.adaptive_bias)
        if y is not None:
            return y
        theta = weight if atten is None else self.composed_weight()
        return F.linear(data, theta, self.adaptive_bias)


def _is_one(v) -> bool:
    return v == 1 or v == (1, 1) or v == [1, 1]


def _is_zero(v) -> bool:
    return v == 0 or v == (0, 0) or v == [0, 0]


class AdaptiveConv2d(AdaptiveBase):
    def __init__(self, global_weight, stride=1, padding=0, **kwargs):
        super().__init__(global_weight, **kwargs)
        self.stride = stride
        self.padding = padding

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        weight, atten, aw = self._weights()
        bias = self.adaptive_bias
        k, c, kh, kw = weight.shape
        if ((kh, kw) == (3, 3) and _is_one(self.stride)
                and _is_one(self.padding) and bias is None):
            # K1: θ composed to bf16 in one pass (or the live θ as it is),
            # then the hand-written or the library conv by ops' policy
            y = ops.conv3x3_try(data, weight, atten, aw)
            if y is not None:
                return y
        if ((kh, kw) == (1, 1) and _is_one(self.stride)
                and _is_zero(self.padding) and data.is_cuda):
            # pointwise conv == GEMM over N·H·W; on channels-last input the
            # [NHW, C] view is free.  Default route: compose2 to bf16 + bf16
            # library GEMMs fwd/bwd (FLREID_NO_FUSED_1X1=1 disables it)
            b, _, h, w = data.shape
            xv = data.permute(0, 2, 3, 1).reshape(-1, c)
            y = ops.adaptive_linear(
                xv, weight.view(k, c), atten,
                aw.view(k, c) if aw is not None and aw.numel() else None,
                bias, engine="lib")
            if y is None and atten is not None:
                # the composed fallback stays a GEMM on the view; the live
                # one below is the conv (other library call, other bits)
                y = F.linear(xv, self.composed_weight().view(k, c), bias)
            if y is not None:
                return y.view(b, h, w, -1).permute(0, 3, 1, 2)
        theta = weight if atten is None else self.composed_weight()
        return F.conv2d(data, theta, bias, stride=self.stride,
                        padding=self.padding)


class AdaptiveBatchNorm2d(AdaptiveBase):
    """Completeness parity with ref:methods/fedstil.py:131-198 (the reference
    ships this but keeps BatchNorm out of its transform LUT)."""

    def __init__(self, global_weight, running_mean=None, running_var=None,
                 num_batches_tracked=None, track_running_stats=False,
                 momentum=0.1, eps=1e-5, **kwargs):
        super().__init__(global_weight, **kwargs)
        self.register_buffer("running_mean", running_mean)
        self.register_buffer("running_var", running_var)
        self.register_buffer("num_batches_tracked", num_batches_tracked)
        self.track_running_stats = track_running_stats
        self.momentum = momentum
        self.eps = eps

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        training = self.training or (self.running_mean is None and self.running_var is None)
        use_stats = not self.training or self.track_running_stats
        return F.batch_norm(
            data,
            self.running_mean if use_stats else None,
            self.running_var if use_stats else None,
            self.composed_weight(), self.adaptive_bias,
            training, self.momentum or 0.0, self.eps)


class AdaptiveLayerNorm(AdaptiveBase):
    def __init__(self, global_weight, normalized_shape: Tuple[int, ...] = None,
                 eps: float = 1e-5, **kwargs):
        super().__init__(global_weight, **kwargs)
        self.normalized_shape = normalized_shape or tuple(global_weight.shape)
        self.eps = eps

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        return F.layer_norm(data, self.normalized_shape, self.composed_weight(),
                            self.adaptive_bias, self.eps)


ADAPTIVE_TYPES = (AdaptiveLinear, AdaptiveConv2d, AdaptiveBatchNorm2d, AdaptiveLayerNorm)


def convert_to_adaptive(net: nn.Module, atten_default: float = 0.80,
                        atten_trainable: bool = False) -> int:
    """Rewrite every fully-trainable Linear/Conv2d leaf into its adaptive
    counterpart (ref:methods/fedstil.py:290-347; BN/LN stay untouched like the
    reference's LUT).  Returns the number of converted leaves."""
    count = 0
    for name, module in list(net.named_modules()):
        if isinstance(module, (nn.Linear, nn.Conv2d)):
            if not all(p.requires_grad for p in module.parameters()):
                continue
            if isinstance(module, nn.Linear):
                new = AdaptiveLinear(
                    global_weight=module.weight, adaptive_bias=module.bias,
                    atten_default=atten_default, atten_trainable=atten_trainable)
            else:
                new = AdaptiveConv2d(
                    global_weight=module.weight, adaptive_bias=module.bias,
                    atten_default=atten_default, atten_trainable=atten_trainable,
                    stride=module.stride, padding=module.padding)
            parent = net
            parts = name.split(".")
            for p in parts[:-1]:
                parent = getattr(parent, p)
            setattr(parent, parts[-1], new)
            count += 1
    return count


def adaptive_leaves(net: nn.Module):
    """[(qualname, module)] of adaptive leaves, in module order."""
    return [(n, m) for n, m in net.named_modules() if isinstance(m, ADAPTIVE_TYPES)]


def non_adaptive_leaves(net: nn.Module):
    """Leaves that are NOT adaptive (the 'pre-trained' frozen set,
    ref:methods/fedstil.py:421-433)."""
    out = []
    for n, m in net.named_modules():
        if len(list(m.children())) == 0 and not isinstance(m, ADAPTIVE_TYPES) and n:
            out.append((n, m))
    return out


# ---------------------------------------------------------------------------
# FedSTIL-atten stacked variant (ref:methods/fedstil_atten.py)
# ---------------------------------------------------------------------------

class StackedAttenBase(nn.Module):
    """θ = Σ_k atten_k · W_glob[..., k] + W_adapt.

    The server CONCATENATES client uploads along a new last dim instead of
    averaging, and the per-slot attention is LEARNABLE; `adaptive_weight`
    persists across dispatch re-inits while `atten` is re-initialised to
    `atten_default` sized to the current stack depth
    (ref:methods/fedstil_atten.py:46-90)."""

    def __init__(self, global_weight: torch.Tensor,
                 adaptive_bias: Optional[torch.Tensor] = None,
                 atten_default: float = 0.0, **kwargs):
        super().__init__()
        self.atten_default = atten_default
        self.atten_trainable = True
        self.global_weight = Parameter(torch.empty(0), requires_grad=False)
        self.global_weight_atten = Parameter(torch.empty(0))
        self.adaptive_weight = Parameter(torch.empty(0))
        self.adaptive_bias = Parameter(torch.empty(0)) if adaptive_bias is not None else None
        self.initial_global_weight_atten = Parameter(torch.empty(0), requires_grad=False)
        self.initial_adaptive_weight = Parameter(torch.empty(0), requires_grad=False)
        # the constructor always receives a RAW module weight: add the stack
        # dim unconditionally (re-inits via init_training_weights pass
        # already-stacked tensors)
        self.init_training_weights(global_weight.unsqueeze(-1),
                                   adaptive_bias=adaptive_bias)

    _assign = staticmethod(AdaptiveBase._assign)

    @torch.no_grad()
    def init_training_weights(self, global_weight=None, global_weight_atten=None,
                              adaptive_weight=None, adaptive_bias=None) -> None:
        if global_weight is None:
            global_weight = self.global_weight.data
        self._assign(self.global_weight, global_weight.detach())
        self.global_weight.requires_grad = False

        k = self.global_weight.shape[-1]
        if global_weight_atten is None:
            global_weight_atten = torch.ones(k, device=self.global_weight.device) \
                                  * self.atten_default
        self._assign(self.global_weight_atten, global_weight_atten.detach())
        self._assign(self.initial_global_weight_atten, global_weight_atten.detach())
        self.global_weight_atten.requires_grad = True

        if self.adaptive_weight.numel() == 0:   # created once, then persists
            if adaptive_weight is None:
                adaptive_weight = ((1.0 - self.global_weight_atten.data)
                                   * self.global_weight.data).sum(dim=-1)
            self._assign(self.adaptive_weight, adaptive_weight.detach())
        elif adaptive_weight is not None:
            self._assign(self.adaptive_weight, adaptive_weight.detach())
        self.adaptive_weight.requires_grad = True
        self._assign(self.initial_adaptive_weight, self.adaptive_weight.detach())

        if self.adaptive_bias is not None and adaptive_bias is not None:
            self._assign(self.adaptive_bias, adaptive_bias.detach())
            self.adaptive_bias.requires_grad = True

    def composed_weight(self) -> torch.Tensor:
        return (self.global_weight_atten * self.global_weight).sum(dim=-1) \
               + self.adaptive_weight

    def drift_pairs(self):
        return [(self.global_weight_atten, self.initial_global_weight_atten),
                (self.adaptive_weight, self.initial_adaptive_weight)]


class StackedAttenLinear(StackedAttenBase):
    def forward(self, data: torch.Tensor) -> torch.Tensor:
        return F.linear(data, self.composed_weight(), self.adaptive_bias)


class StackedAttenConv2d(StackedAttenBase):
    def __init__(self, global_weight, stride=1, padding=0, **kwargs):
        super().__init__(global_weight, **kwargs)
        self.stride = stride
        self.padding = padding

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        return F.conv2d(data, self.composed_weight(), self.adaptive_bias,
                        stride=self.stride, padding=self.padding)


ADAPTIVE_TYPES = ADAPTIVE_TYPES + (StackedAttenLinear, StackedAttenConv2d)


def convert_to_stacked(net: nn.Module, atten_default: float = 0.0) -> int:
    count = 0
    for name, module in list(net.named_modules()):
        if isinstance(module, (nn.Linear, nn.Conv2d)):
            if not all(p.requires_grad for p in module.parameters()):
                continue
            if isinstance(module, nn.Linear):
                new = StackedAttenLinear(global_weight=module.weight,
                                         adaptive_bias=module.bias,
                                         atten_default=atten_default)
            else:
                new = StackedAttenConv2d(global_weight=module.weight,
                                         adaptive_bias=module.bias,
                                         atten_default=atten_default,
                                         stride=module.stride,
                                         padding=module.padding)
            parent = net
            parts = name.split(".")
            for p in parts[:-1]:
                parent = getattr(parent, p)
            setattr(parent, parts[-1], new)
            count += 1
    return count
