"""Swin Transformer ReID backbones (capability parity with
ref:models/swin_transformer.py).

From-scratch Swin v1 (tiny/small/base/large) with the ReID head of the
reference wrapper: input resized to 224², 4 stages of shifted-window blocks,
LN + token avgpool, BNNeck head, dual train/eval outputs
(ref:models/swin_transformer.py:604-700).

MI355X notes: where `ops.shifted_window_attention_qkv_route` says "map" (GPU,
extension built, bf16 — the autocast dtype counts —, head dim 32, windows of
up to 64 tokens that tile the map, no attention dropout) a block is
norm1 → qkv on the feature map → window_attn_map.hip → proj → + shortcut:
the kernel reads qkv from the map and writes its result to it in image
order, so roll, window_partition, window_reverse and the second roll are its
addressing, and it forms the shift mask from region labels (`attn_mask` is
passed on but not read there).  Every other configuration runs roll /
partition / attention / reverse / roll as before:
the per-window attention runs through
flreid_amd.ops.window_attention_qkv (K3 in SURVEY.md §2.9) on the qkv
projection output as it lies.  On GPU `ops.window_attention_qkv_route` gives
bf16 windows of up to 64 tokens at head dim 32 without attention dropout (49
tokens at 224² / window 7 under autocast) to the packed MFMA kernel
(window_attn_qkv.hip): no q / k / v copies, the result ready for `proj`, one
dqkv in the backward.  Everything else is split into q, k, v and goes through
`ops.window_attention` — eager composition on CPU; on GPU
`ops.window_attention_route` picks the kernel: windows of up to 64 tokens and
head dim up to 64 take the fused VALU kernel (window_attn.hip, fp32 or bf16),
bf16 windows of 65..144 tokens at head dim 32 (144 tokens at 384² / window
12) the MFMA kernel (window_attn_mfma.hip), the rest the eager chain.
The row passes around the attention go through `ops.add_layer_norm`
(add_ln.hip) on the GPU: `norm1`, and the residual add fused with `norm2`,
each one pass that hands the next Linear its rows in the autocast dtype.
Only a plain nn.LayerNorm takes that route, and FLREID_SWIN_ADD_LN=0 turns
it off; the CPU runs the separate operations.
Staged execution (`stage_of`/`run_stages`) mirrors models/resnet.py so
FedSTIL's head-only training path works unchanged (stages: stem, layers.0-3,
head).
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from flreid_amd import ops
from flreid_amd.tools.winit import weights_init_classifier, weights_init_kaiming


def window_partition(x: torch.Tensor, ws: int) -> torch.Tensor:
    """[B, H, W, C] -> [B·nW, ws·ws, C]"""
    b, h, w, c = x.shape
    x = x.view(b, h // ws, ws, w // ws, ws, c)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, c)


def window_reverse(win: torch.Tensor, ws: int, h: int, w: int) -> torch.Tensor:
    """[B·nW, ws·ws, C] -> [B, H, W, C]"""
    b = win.shape[0] // ((h // ws) * (w // ws))
    x = win.view(b, h // ws, w // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, -1)


class DropPath(nn.Module):
    def __init__(self, p: float = 0.0):
        super().__init__()
        self.p = p

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.p == 0.0 or not self.training:
            return x
        keep = 1.0 - self.p
        mask = torch.rand(x.shape[0], *([1] * (x.dim() - 1)),
                          device=x.device, dtype=x.dtype) < keep
        return x * mask / keep


class WindowAttention(nn.Module):
    """W-MSA with relative position bias (ref:models/swin_transformer.py:208-286)."""

    def __init__(self, dim: int, window_size: int, num_heads: int,
                 qkv_bias: bool = True, attn_drop: float = 0.0,
                 proj_drop: float = 0.0):
        super().__init__()
        self.dim = dim
        self.window_size = window_size
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5

        n = 2 * window_size - 1
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros(n * n, num_heads))
        coords = torch.stack(torch.meshgrid(
            torch.arange(window_size), torch.arange(window_size),
            indexing="ij")).flatten(1)                       # [2, ws*ws]
        rel = coords[:, :, None] - coords[:, None, :]        # [2, N, N]
        rel = rel.permute(1, 2, 0) + (window_size - 1)
        index = rel[..., 0] * n + rel[..., 1]                # [N, N]
        self.register_buffer("relative_position_index", index)

        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None,
                shift: int = 0):
        """x [b·nW, n, c]: the windows, already rolled and partitioned, or
        x [b, h, w, c]: the feature map in image order, whose windows are
        those of a roll by -`shift`; the result has x's form.  `mask` is the
        block's shift mask in both (None without a shift)."""
        n = self.window_size * self.window_size
        bias = self.relative_position_bias_table[
            self.relative_position_index.view(-1)].view(n, n, -1)
        bias = bias.permute(2, 0, 1).contiguous()            # [h, n, n]
        dropout = self.attn_drop if self.training else None
        if x.dim() == 4:
            out = ops.shifted_window_attention_qkv(
                self.qkv(x), self.num_heads, self.window_size, shift,
                bias * 1.0, mask, self.scale, dropout)       # [b, h, w, c]
        else:
            out = ops.window_attention_qkv(
                self.qkv(x), self.num_heads, bias * 1.0, mask, self.scale,
                dropout)                                     # [bn, n, c]
        return self.proj_drop(self.proj(out))


class SwinBlock(nn.Module):
    def __init__(self, dim: int, input_resolution: Tuple[int, int],
                 num_heads: int, window_size: int = 7, shift: int = 0,
                 mlp_ratio: float = 4.0, qkv_bias: bool = True,
                 drop: float = 0.0, attn_drop: float = 0.0,
                 drop_path: float = 0.0):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.window_size = min(window_size, *input_resolution)
        self.shift = 0 if self.window_size >= min(input_resolution) and shift else shift
        if min(input_resolution) <= self.window_size:
            self.shift = 0

        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, self.window_size, num_heads, qkv_bias,
                                    attn_drop, drop)
        self.drop_path = DropPath(drop_path)
        self.norm2 = nn.LayerNorm(dim)
        hidden = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(),
                                 nn.Dropout(drop), nn.Linear(hidden, dim),
                                 nn.Dropout(drop))

        if self.shift > 0:
            self.register_buffer("attn_mask", self._build_mask(), persistent=False)
        else:
            self.attn_mask = None

    def _build_mask(self) -> torch.Tensor:
        """Shifted-window cross-region mask (ref:models/swin_transformer.py:333-356)."""
        h, w = self.input_resolution
        ws, sh = self.window_size, self.shift
        img_mask = torch.zeros(1, h, w, 1)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None)):
            for wslice in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None)):
                img_mask[:, hs, wslice, :] = cnt
                cnt += 1
        windows = window_partition(img_mask, ws).squeeze(-1)   # [nW, ws*ws]
        diff = windows.unsqueeze(1) - windows.unsqueeze(2)
        return diff.masked_fill(diff != 0, -100.0).masked_fill(diff == 0, 0.0)

    def _on_the_map(self, x: torch.Tensor) -> bool:
        """Whether the attention runs on the feature map as it lies
        (`ops.shifted_window_attention_qkv`, route "map"), for the dtype the
        qkv projection will produce."""
        if not (x.is_cuda and ops.extension_available()):
            return False
        h, w = self.input_resolution
        dtype = x.dtype
        if torch.is_autocast_enabled("cuda"):
            dtype = torch.get_autocast_dtype("cuda")
        drop_p = self.attn.attn_drop.p if self.training else 0.0
        return (h * w * 3 * self.dim * 2 < 2 ** 31
                and ops.shifted_window_attention_qkv_route(
                    self.window_size ** 2, self.dim // self.attn.num_heads,
                    dtype, drop_p, h, w, self.window_size,
                    self.shift) == "map")

    @staticmethod
    def _fused_norm(norm: nn.Module, x: torch.Tensor) -> bool:
        """Whether `norm` (and the residual add in front of it) goes through
        `ops.add_layer_norm`: a plain nn.LayerNorm on the GPU with the
        extension built, unless FLREID_SWIN_ADD_LN=0.  The norms FedWeIT
        swaps in compose their own weights and stay as they are."""
        return (type(norm) is nn.LayerNorm and x.is_cuda
                and ops.extension_available()
                and os.environ.get("FLREID_SWIN_ADD_LN", "1") != "0")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        h, w = self.input_resolution
        b, L, c = x.shape
        shortcut = x
        # the rows leave the fused norms in the dtype the next Linear reads
        out_dtype = (torch.get_autocast_dtype("cuda")
                     if x.is_cuda and torch.is_autocast_enabled("cuda")
                     else None)
        if self._fused_norm(self.norm1, x):
            x = ops.add_layer_norm(x, None, self.norm1.weight,
                                   self.norm1.bias, self.norm1.eps, out_dtype)
        else:
            x = self.norm1(x)
        x = x.view(b, h, w, c)
        if self._on_the_map(x):
            # qkv and proj are per-token: roll, partition and their inverses
            # are addressing inside the kernel
            x = self.attn(x, self.attn_mask, self.shift)
        else:
            if self.shift > 0:
                x = torch.roll(x, shifts=(-self.shift, -self.shift),
                               dims=(1, 2))
            win = window_partition(x, self.window_size)        # [b·nW, N, C]
            win = self.attn(win, self.attn_mask)
            x = window_reverse(win, self.window_size, h, w)
            if self.shift > 0:
                x = torch.roll(x, shifts=(self.shift, self.shift),
                               dims=(1, 2))
        x = self.drop_path(x.view(b, L, c))
        if self._fused_norm(self.norm2, x):
            x, xn = ops.add_layer_norm(shortcut, x, self.norm2.weight,
                                       self.norm2.bias, self.norm2.eps,
                                       out_dtype)
        else:
            x = shortcut + x
            xn = self.norm2(x)
        return x + self.drop_path(self.mlp(xn))


class PatchMerging(nn.Module):
    """2×2 concat + LN + Linear 4C→2C (ref:models/swin_transformer.py:398-444)."""

    def __init__(self, input_resolution: Tuple[int, int], dim: int):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.norm = nn.LayerNorm(4 * dim)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        h, w = self.input_resolution
        b, L, c = x.shape
        # fused K4 path (patch_merge.hip): gather + LN in one kernel, the
        # concat tensor never materialises; eager fallback elsewhere
        y = ops.patch_merge_ln(x, self.norm.weight, self.norm.bias, h, w,
                               self.norm.eps)
        if y is None:
            x = x.view(b, h, w, c)
            x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2],
                           x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1)
            y = self.norm(x.view(b, -1, 4 * c))
        return self.reduction(y)


class SwinStage(nn.Module):
    def __init__(self, dim, input_resolution, depth, num_heads, window_size,
                 mlp_ratio, qkv_bias, drop, attn_drop, drop_path,
                 downsample: bool, use_checkpoint: bool = False):
        super().__init__()
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            SwinBlock(dim, input_resolution, num_heads, window_size,
                      shift=0 if i % 2 == 0 else window_size // 2,
                      mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop,
                      attn_drop=attn_drop,
                      drop_path=drop_path[i] if isinstance(drop_path, (list, tuple)) else drop_path)
            for i in range(depth)])
        self.downsample = PatchMerging(input_resolution, dim) if downsample else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for blk in self.blocks:
            if self.use_checkpoint and self.training:
                x = torch.utils.checkpoint.checkpoint(blk, x, use_reentrant=False)
            else:
                x = blk(x)
        if self.downsample is not None:
            x = self.downsample(x)
        return x


class SwinTrunk(nn.Module):
    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7,
                 mlp_ratio=4.0, qkv_bias=True, drop_rate=0.0,
                 attn_drop_rate=0.0, drop_path_rate=0.1,
                 use_checkpoint=False):
        super().__init__()
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.patches_resolution = (img_size // patch_size, img_size // patch_size)

        self.patch_embed = nn.Conv2d(in_chans, embed_dim, patch_size, patch_size)
        self.patch_norm = nn.LayerNorm(embed_dim)
        self.pos_drop = nn.Dropout(drop_rate)

        dpr = torch.linspace(0, drop_path_rate, sum(depths)).tolist()
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            res = (self.patches_resolution[0] // 2 ** i,
                   self.patches_resolution[1] // 2 ** i)
            self.layers.append(SwinStage(
                dim=int(embed_dim * 2 ** i), input_resolution=res,
                depth=depths[i], num_heads=num_heads[i],
                window_size=window_size, mlp_ratio=mlp_ratio,
                qkv_bias=qkv_bias, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])],
                downsample=i < self.num_layers - 1,
                use_checkpoint=use_checkpoint))
        self.norm = nn.LayerNorm(self.num_features)
        self.apply(self._init)

    @staticmethod
    def _init(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.weight, 1.0)
            nn.init.constant_(m.bias, 0)

    def stem(self, x: torch.Tensor) -> torch.Tensor:
        x = self.patch_embed(x).flatten(2).transpose(1, 2)   # [B, L, C]
        return self.pos_drop(self.patch_norm(x))

    def head_pool(self, x: torch.Tensor) -> torch.Tensor:
        return self.norm(x).mean(dim=1)

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        x = self.stem(x)
        for layer in self.layers:
            x = layer(x)
        return self.head_pool(x)


_SWIN_ARCH = {
    "swin_tiny": dict(embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24)),
    "swin_small": dict(embed_dim=96, depths=(2, 2, 18, 2), num_heads=(3, 6, 12, 24)),
    "swin_base": dict(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32)),
    "swin_large": dict(embed_dim=192, depths=(2, 2, 18, 2), num_heads=(6, 12, 24, 48)),
}


class SwinReID(nn.Module):
    STAGES = ("stem", "layer0", "layer1", "layer2", "layer3", "head")

    def __init__(self, model_name: str, num_classes: int = 1000,
                 neck: str = "no", img_size: int = 224, window_size: int = 7,
                 use_checkpoint: bool = False, **kwargs):
        super().__init__()
        for n, p in kwargs.items():
            setattr(self, n, p)
        if model_name not in _SWIN_ARCH:
            raise ValueError(f"No model named {model_name}.")
        self.model_name = model_name
        self.num_classes = num_classes
        self.neck = neck
        self.img_size = img_size
        self.base = SwinTrunk(img_size=img_size, window_size=window_size,
                              use_checkpoint=use_checkpoint,
                              **_SWIN_ARCH[model_name])
        self.in_planes = self.base.num_features

        if neck == "no":
            self.classifier = nn.Linear(self.in_planes, num_classes)
        elif neck == "bnneck":
            from flreid_amd.models.resnet import EvalFusedBatchNorm1d
            self.bottleneck = EvalFusedBatchNorm1d(self.in_planes)
            self.bottleneck.bias.requires_grad_(False)
            self.classifier = nn.Linear(self.in_planes, num_classes, bias=False)
            self.bottleneck.apply(weights_init_kaiming)
            self.classifier.apply(weights_init_classifier)
        else:
            raise ValueError(f"Mismatched neck type {neck}.")

    # ---- staged execution (FedSTIL head-only training; see resnet.py) ------
    def stage_of(self, module_path: str) -> int:
        if module_path.startswith("base.layers."):
            return int(module_path.split(".")[2]) + 1
        if module_path.startswith("base."):
            return 0
        return len(self.STAGES) - 1

    def run_stages(self, x: torch.Tensor, start: int = 0, tap: int = None):
        tap_value = None
        if start == 0:
            if x.shape[-2:] != (self.img_size, self.img_size):
                x = F.interpolate(x, size=(self.img_size, self.img_size),
                                  mode="bilinear", align_corners=False)
            if tap == 0:
                tap_value = x
            x = self.base.stem(x)
        for idx in range(max(start - 1, 0), 4):
            stage = idx + 1
            if stage < start:
                continue
            if tap == stage:
                tap_value = x
            x = self.base.layers[idx](x)
        if tap == 5:
            tap_value = x
        global_feat = self.base.head_pool(x)
        feat = self.bottleneck(global_feat) if self.neck == "bnneck" else global_feat
        if self.training:
            return (self.classifier(feat), global_feat), tap_value
        return global_feat, tap_value

    def forward(self, x: torch.Tensor):
        out, _ = self.run_stages(x, 0)
        return out


def swin_reid(size: str, **kwargs):
    return SwinReID(f"swin_{size}", **kwargs)
