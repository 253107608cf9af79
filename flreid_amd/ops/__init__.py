"""Dispatch layer for flreid ops.

CPU tensors  -> pure-PyTorch reference implementations (ops/reference.py).
CUDA tensors -> hand-written HIP/CDNA4 kernels from the in-tree extension
                flreid_amd/ops/_flreid_hip.so (sources in ops/csrc, built by
                `python -m flreid_amd.ops.build` / __graft_entry__.build()).

On a GPU box the HIP path is mandatory: if the extension is missing the op
raises instead of silently falling back to eager PyTorch (set
FLREID_ALLOW_EAGER=1 to debug).  Numerics ground truth for every kernel is
the fp32 reference implementation (tests/test_ops_gpu.py).
"""

from __future__ import annotations

import os
from collections import OrderedDict
from typing import Dict, Optional, Sequence, Tuple

import torch

from flreid_amd.ops import reference as ref

_EXT = None
_EXT_ERR: Optional[str] = None

_F32, _BF16 = 0, 1


def _load_extension():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from flreid_amd.ops import _flreid_hip  # built in-tree

        _EXT = _flreid_hip
    except Exception as e:  # pragma: no cover - GPU boxes only
        _EXT_ERR = f"{type(e).__name__}: {e}"
        _EXT = None
    return _EXT


def extension_available() -> bool:
    return _load_extension() is not None


def require_extension(opname: str):
    """The built extension, or an error (None under FLREID_ALLOW_EAGER=1)."""
    ext = _load_extension()
    if ext is not None:
        return ext
    if os.environ.get("FLREID_ALLOW_EAGER", "0") == "1":
        return None
    raise RuntimeError(
        f"flreid HIP extension missing for GPU op '{opname}' ({_EXT_ERR}). "
        "Build it with `python -m flreid_amd.ops.build` "
        "or set FLREID_ALLOW_EAGER=1 to debug with eager PyTorch."
    )


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _F32
    if t.dtype == torch.bfloat16:
        return _BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


# ---------------------------------------------------------------------------
# layout helpers and the multi-tensor chunk table
# ---------------------------------------------------------------------------

def same_layout(t: torch.Tensor, like: torch.Tensor) -> bool:
    """Same shape and the same PHYSICAL layout: strides compared on every
    dim of extent > 1 (a size-1 dim's stride is arbitrary)."""
    return t.shape == like.shape and all(
        a == b for a, b, n in zip(t.stride(), like.stride(), like.shape)
        if n > 1)


def _dense(t: torch.Tensor) -> bool:
    """Non-overlapping and dense: the storage run [data_ptr, data_ptr + numel)
    holds every element exactly once (contiguous, channels-last, permuted)."""
    expect = 1
    for stride, size in sorted((s, n) for n, s in zip(t.shape, t.stride())
                               if n > 1):
        if stride != expect:
            return False
        expect *= size
    return True


def atten_geometry(w: torch.Tensor) -> Tuple[int, int]:
    """(L, inner): atten broadcasts over the LOGICAL last dim, whose
    physical index is (i / inner) % L — inner = C for channels-last
    [K][kh][kw][C] storage, 1 when the last dim is also physically last."""
    if w.dim() < 1 or w.numel() == 0:
        raise ValueError("atten_geometry: empty adaptive weight")
    if w.is_contiguous():
        return w.shape[-1], 1
    if w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last):
        return w.shape[-1], w.shape[1]
    raise ValueError("atten_geometry: adaptive weight is neither contiguous "
                     f"nor channels-last dense (strides {w.stride()})")


def _fusable(t, like: Optional[torch.Tensor] = None) -> bool:
    """What a multi-tensor kernel's float4 body needs: fp32 on a GPU, 16-byte
    aligned, and dense — or, given `like`, on its device in its very layout."""
    return (isinstance(t, torch.Tensor) and t.is_cuda
            and t.dtype == torch.float32 and t.data_ptr() % 16 == 0
            and (_dense(t) if like is None
                 else t.device == like.device and same_layout(t, like)))


def _chunk_table(numels: Sequence[int], chunk: int, pad_to: int = 1):
    """(chunk_rows, flat_offsets, total): one (tensor, elem_offset, len,
    flat_offset) row, i.e. one workgroup, per ≤ `chunk` elements; tensor i's
    slot of the flat buffer starts at flat_offsets[i], `pad_to`-aligned."""
    chunk_rows, offsets, flat_off = [], [], 0
    for i, n in enumerate(numels):
        offsets.append(flat_off)
        chunk_rows += [(i, off, min(chunk, n - off), flat_off + off)
                       for off in range(0, n, chunk)]
        flat_off += -(-n // pad_to) * pad_to
    return chunk_rows, offsets, flat_off


# the name require_extension had before it had callers outside ops/; test
# files written against it keep running
_ext_or_raise = require_extension


# ---------------------------------------------------------------------------
# distances / similarity (K8)
# ---------------------------------------------------------------------------

def _pairwise_gpu(ext, a: torch.Tensor, b: torch.Tensor, mode: int) -> torch.Tensor:
    a = a.contiguous().float()
    b = b.contiguous().float()
    m, n, d = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty(m, n, device=a.device, dtype=torch.float32)
    if mode == 2:
        aa = torch.empty(m, device=a.device, dtype=torch.float32)
        bb = torch.empty(n, device=a.device, dtype=torch.float32)
        ext.rowsq(a.data_ptr(), aa.data_ptr(), m, d, _stream())
        ext.rowsq(b.data_ptr(), bb.data_ptr(), n, d, _stream())
    else:
        aa = bb = out  # unused
    ext.pairwise(a.data_ptr(), b.data_ptr(), aa.data_ptr(), bb.data_ptr(),
                 out.data_ptr(), m, n, d, mode, _stream())
    return out


def similarity_matrix(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """A·Bᵀ — the eval GEMM."""
    if a.is_cuda and not a.requires_grad and not b.requires_grad:
        ext = require_extension("pairwise")
        if ext is not None:
            return _pairwise_gpu(ext, a, b, 0)
    return a.float() @ b.float().t()


def pairwise_sqeuclidean(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if a.is_cuda and not a.requires_grad and not b.requires_grad:
        ext = require_extension("pairwise")
        if ext is not None:
            return _pairwise_gpu(ext, a, b, 2)
    return ref.pairwise_sqeuclidean(a, b)


def pairwise_cosine_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if a.is_cuda and not a.requires_grad and not b.requires_grad:
        ext = require_extension("pairwise")
        if ext is not None:
            return _pairwise_gpu(ext, l2_normalize(a.float()),
                                 l2_normalize(b.float()), 1)
    return ref.pairwise_cosine_distance(a, b)


# ---------------------------------------------------------------------------
# rowwise L2 normalize (K11)
# ---------------------------------------------------------------------------

def l2_normalize(x: torch.Tensor, dim: int = 1) -> torch.Tensor:
    if (x.is_cuda and x.dim() == 2 and dim in (1, -1)
            and not x.requires_grad and x.dtype in (torch.float32, torch.bfloat16)):
        ext = require_extension("l2norm_rows")
        if ext is not None:
            x = x.contiguous()
            y = torch.empty_like(x)
            ext.l2norm_rows(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1],
                            _dt(x), 1e-12, _stream())
            return y
    return ref.l2_normalize(x, dim=dim)


# ---------------------------------------------------------------------------
# fused label-smooth CE (K6)
# ---------------------------------------------------------------------------

class _CeLabelSmoothFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, target, epsilon, ext):
        score_c = score.contiguous()
        B, C = score_c.shape
        row_loss = torch.empty(B, device=score.device, dtype=torch.float32)
        grad = torch.empty_like(score_c)
        ext.ce_smooth(score_c.data_ptr(), target.contiguous().data_ptr(),
                      row_loss.data_ptr(), grad.data_ptr(), B, C,
                      _dt(score_c), float(epsilon), _stream())
        ctx.save_for_backward(grad)
        return row_loss.sum() * (1.0 / B)

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None, None


def ce_label_smooth(score: torch.Tensor, target: torch.Tensor,
                    epsilon: float = 0.1) -> torch.Tensor:
    if score.is_cuda and score.dim() == 2:
        ext = require_extension("ce_smooth")
        if ext is not None:
            return _CeLabelSmoothFn.apply(score, target.long(), epsilon, ext)
    return ref.ce_label_smooth(score, target, epsilon)


# ---------------------------------------------------------------------------
# FedSTIL composition (K1/K2 prologue, standalone form)
# ---------------------------------------------------------------------------

class _ComposeFn(torch.autograd.Function):
    """theta = atten ⊙_lastdim gw + aw.  gw/atten frozen in FedSTIL; grad
    flows to aw (identity) and, when atten trains (fedstil-atten), reduces
    over all dims but the last."""

    @staticmethod
    def forward(ctx, gw, atten, aw, ext):
        gw_c, aw_c = gw.contiguous(), aw.contiguous()
        at = atten.detach().contiguous().float()
        out = torch.empty_like(gw_c)
        ext.compose2(gw_c.data_ptr(), at.data_ptr(), aw_c.data_ptr(),
                     out.data_ptr(), gw_c.numel(), gw_c.shape[-1], 1,
                     _dt(gw_c), _dt(gw_c), _stream())
        ctx.atten_requires = atten.requires_grad
        if ctx.atten_requires:
            ctx.save_for_backward(gw_c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        g_atten = None
        if ctx.atten_requires:
            (gw,) = ctx.saved_tensors
            g_atten = (grad_out * gw).reshape(-1, gw.shape[-1]).sum(dim=0)
        return None, g_atten, grad_out, None


def adaptive_compose(global_weight: torch.Tensor, atten: torch.Tensor,
                     adaptive_weight: torch.Tensor) -> torch.Tensor:
    if (global_weight.is_cuda and not global_weight.requires_grad
            and global_weight.dtype in (torch.float32, torch.bfloat16)
            and adaptive_weight.dtype == global_weight.dtype):
        ext = require_extension("compose2")
        if ext is not None:
            return _ComposeFn.apply(global_weight, atten, adaptive_weight, ext)
    return ref.adaptive_compose(global_weight, atten, adaptive_weight)


# ---------------------------------------------------------------------------
# FedWeIT decomposed-layer composition (decomposed.hip)
# ---------------------------------------------------------------------------

_TORCH_DT = {torch.float32: _F32, torch.bfloat16: _BF16}


def _decomposed_geometry(sw: torch.Tensor):
    """(rows, C, S, channels_last) of a dense weight, or None.  4-D weights
    whose two layouts coincide (S == 1 or C == 1) count as contiguous."""
    rows = sw.shape[0]
    if sw.dim() == 4:
        c, s = sw.shape[1], sw.shape[2] * sw.shape[3]
        if s > 1 and c > 1 and not sw.is_contiguous():
            if sw.is_contiguous(memory_format=torch.channels_last):
                return rows, c, s, True
            return None
        if sw.is_contiguous() or sw.is_contiguous(
                memory_format=torch.channels_last):
            return rows, c, s, False
        return None
    if not sw.is_contiguous():
        return None
    return rows, sw.numel() // max(rows, 1), 1, False


class _DecomposedComposeFn(torch.autograd.Function):
    """θ = thr(mask)⊙sw + thr(aw) + Σ_k atten_k·aw_kb[..., k] in one kernel
    per direction.  Only the inputs are saved; the backward re-reads them
    and emits d_aw, the d_mask partials and the d_atten partials in one
    pass (the partial sums are finished by torch — deterministic)."""

    @staticmethod
    def forward(ctx, sw, mask, aw, aw_kb, atten, lambda_l1, lambda_mask,
                training, out_dtype, geom, ext):
        rows, c, s, cl = geom
        kb = aw_kb.shape[-1]
        out = torch.empty_like(sw, dtype=out_dtype)
        ext.decomposed_fwd(sw.data_ptr(), mask.data_ptr(), aw.data_ptr(),
                           aw_kb.data_ptr(), atten.data_ptr(), out.data_ptr(),
                           rows, c, s, kb, int(cl), int(training),
                           float(lambda_l1), float(lambda_mask),
                           _TORCH_DT[out_dtype], _stream())
        ctx.save_for_backward(sw, mask, aw, aw_kb, atten)
        ctx.cfg = (geom, float(lambda_l1), float(lambda_mask), bool(training),
                   out_dtype, ext)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        sw, mask, aw, aw_kb, atten = ctx.saved_tensors
        (rows, c, s, cl), l1, lm, training, out_dtype, ext = ctx.cfg
        need_mask, need_aw, need_atten = (ctx.needs_input_grad[1],
                                          ctx.needs_input_grad[2],
                                          ctx.needs_input_grad[4])
        if not (need_mask or need_aw or need_atten):
            return (None,) * 11
        kb = aw_kb.shape[-1]
        # dθ in θ's dtype and layout
        g = grad_out.to(out_dtype)
        g = g.contiguous(memory_format=torch.channels_last) if cl \
            else g.contiguous()
        tpr, blocks = ext.decomposed_plan(rows, c, s, int(cl))
        dev = sw.device
        d_aw = torch.empty_like(aw) if need_aw else None
        dm_part = (torch.empty(rows, tpr, device=dev, dtype=torch.float32)
                   if need_mask else None)
        da_part = (torch.empty(blocks, kb, device=dev, dtype=torch.float32)
                   if need_atten else None)
        ext.decomposed_bwd(
            g.data_ptr(), _TORCH_DT[out_dtype], sw.data_ptr(),
            mask.data_ptr(), aw.data_ptr(), aw_kb.data_ptr(),
            d_aw.data_ptr() if need_aw else 0,
            dm_part.data_ptr() if need_mask else 0,
            da_part.data_ptr() if need_atten else 0,
            rows, c, s, kb, int(cl), int(training), l1, lm,
            int(need_aw), int(need_mask), int(need_atten), _stream())
        d_mask = dm_part.sum(dim=1).view(mask.shape) if need_mask else None
        d_atten = da_part.sum(dim=0).view(atten.shape) if need_atten else None
        return (None, d_mask, d_aw, None, d_atten) + (None,) * 6


def decomposed_compose(sw: torch.Tensor, mask: torch.Tensor, aw: torch.Tensor,
                       aw_kb: torch.Tensor, atten: torch.Tensor,
                       lambda_l1: float, lambda_mask: float, training: bool,
                       out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """FedWeIT composed weight.  Fused HIP forward+backward on GPU for fp32
    dense weights of dim ≥ 2 (contiguous, or channels-last for 4-D) with a
    frozen sw; the eager reference everywhere else (1-D BN/LN weights, CPU,
    mismatched layouts).  out_dtype (fp32 default, or bf16) is θ's dtype:
    bf16 is the round-to-nearest-even cast of the fp32 θ, emitted by the
    kernel directly.  FLREID_NO_FUSED_DECOMPOSE=1 forces the reference."""
    if (sw.is_cuda and os.environ.get("FLREID_NO_FUSED_DECOMPOSE", "0") != "1"
            and out_dtype in (None, torch.float32, torch.bfloat16)
            and all(t.is_cuda and t.dtype == torch.float32
                    for t in (sw, mask, aw, aw_kb, atten))
            and sw.dim() >= 2 and sw.numel() > 0 and not sw.requires_grad
            and not aw_kb.requires_grad and aw.shape == sw.shape
            and aw_kb.dim() == sw.dim() + 1 and aw_kb.shape[:-1] == sw.shape
            and aw_kb.shape[-1] >= 1 and aw_kb.is_contiguous()
            and atten.numel() == aw_kb.shape[-1] and atten.is_contiguous()
            and mask.numel() == sw.shape[0] and mask.is_contiguous()):
        geom = _decomposed_geometry(sw)
        if geom is not None and geom == _decomposed_geometry(aw):
            ext = require_extension("decomposed_fwd")
            if ext is not None:
                return _DecomposedComposeFn.apply(
                    sw, mask, aw, aw_kb, atten, lambda_l1, lambda_mask,
                    bool(training), out_dtype or torch.float32, geom, ext)
    out = ref.decomposed_compose(sw, mask, aw, aw_kb, atten, lambda_l1,
                                 lambda_mask, training)
    if out_dtype is not None and out.dtype != out_dtype:
        out = out.to(out_dtype)
    return out


# ---------------------------------------------------------------------------
# EWC/MAS importance accumulation (K9)
# ---------------------------------------------------------------------------

def importance_update(importance: Dict[str, torch.Tensor],
                      grads: Dict[str, torch.Tensor], mode: str = "sq",
                      scale: float = 1.0) -> None:
    first = next(iter(importance.values()), None)
    if first is not None and first.is_cuda:
        ext = require_extension("importance")
        if ext is not None:
            for n, g in grads.items():
                if g is None:
                    continue
                F = importance[n]
                ext.importance(F.data_ptr(), g.contiguous().data_ptr(),
                               g.numel(), _dt(g), mode == "sq", scale,
                               _stream())
            return
    for n, g in grads.items():
        if g is None:
            continue
        if mode == "sq":
            importance[n] += (g.detach().float() ** 2) * scale
        else:
            importance[n] += g.detach().float().abs() * scale


# ---------------------------------------------------------------------------
# pass-throughs (small tensors / composed autograd paths)
# ---------------------------------------------------------------------------

kl_distance = ref.kl_distance


class _KdLossFn(torch.autograd.Function):
    """Fused temperature-softmax KL distillation (K7, kd.hip): one kernel
    computes loss + dL/dz_student; the eager chain is 5 kernels plus the
    autograd graph."""

    @staticmethod
    def forward(ctx, zs, zt, temperature, ext):
        zs_c = zs.detach().float().contiguous()
        zt_c = zt.detach().float().contiguous()
        B, C = zs_c.shape
        row_loss = torch.empty(B, device=zs.device, dtype=torch.float32)
        grad = torch.empty_like(zs_c)
        ext.kd_fwd(zs_c.data_ptr(), zt_c.data_ptr(), row_loss.data_ptr(),
                   grad.data_ptr(), B, C, float(temperature), _stream())
        ctx.save_for_backward(grad)
        ctx.zs_dtype = zs.dtype
        return row_loss.sum()

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return (grad * grad_out).to(ctx.zs_dtype), None, None, None


def kd_loss(logits_student: torch.Tensor, logits_teacher: torch.Tensor,
            temperature: float = 4.0) -> torch.Tensor:
    if logits_student.is_cuda and logits_student.dim() == 2:
        ext = require_extension("kd_fwd")
        if ext is not None:
            return _KdLossFn.apply(logits_student, logits_teacher,
                                   temperature, ext)
    return ref.kd_loss(logits_student, logits_teacher, temperature)


class _IcarlDistillFn(torch.autograd.Function):
    """Fused iCaRL distillation step (K7, kd.hip): BOTH BCE-with-logits
    losses (one-hot classification + sigmoid-teacher distillation on the
    first P columns) and the combined gradient in ONE pass
    (ref:methods/icarl.py:216-236)."""

    @staticmethod
    def forward(ctx, score, target, prev, ext):
        score_c = score.detach().float().contiguous()
        prev_c = prev.detach().float().contiguous()
        B, C = score_c.shape
        P = prev_c.shape[1]
        row_loss = torch.empty(B, device=score.device, dtype=torch.float32)
        grad = torch.empty_like(score_c)
        ext.icarl_distill(score_c.data_ptr(),
                          target.long().contiguous().data_ptr(),
                          prev_c.data_ptr(), row_loss.data_ptr(),
                          grad.data_ptr(), B, C, P, _stream())
        ctx.save_for_backward(grad)
        ctx.score_dtype = score.dtype
        return row_loss.sum()

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return (grad * grad_out).to(ctx.score_dtype), None, None, None


def icarl_distill_loss(score: torch.Tensor, target: torch.Tensor,
                       prev_logits: torch.Tensor) -> torch.Tensor:
    """clf BCE(score, onehot(target)) + distill BCE(score[:, :P],
    sigmoid(prev_logits)) — fused on GPU, eager reference elsewhere."""
    if (score.is_cuda and score.dim() == 2
            and prev_logits.shape[1] <= score.shape[1]):
        ext = require_extension("icarl_distill")
        if ext is not None:
            return _IcarlDistillFn.apply(score, target, prev_logits, ext)
    return ref.icarl_distill_loss(score, target, prev_logits)


class _TripletHardFn(torch.autograd.Function):
    """Fused batch-hard euclidean triplet (margin mode) — K5."""

    @staticmethod
    def forward(ctx, feature, target, margin, ext):
        f = feature.detach().contiguous().float()
        n, d = f.shape
        norms = torch.empty(n, device=f.device, dtype=torch.float32)
        ext.rowsq(f.data_ptr(), norms.data_ptr(), n, d, _stream())
        row_loss = torch.empty(n, device=f.device, dtype=torch.float32)
        p_idx = torch.empty(n, device=f.device, dtype=torch.int32)
        n_idx = torch.empty(n, device=f.device, dtype=torch.int32)
        ext.triplet_fwd(f.data_ptr(), norms.data_ptr(),
                        target.contiguous().data_ptr(), row_loss.data_ptr(),
                        p_idx.data_ptr(), n_idx.data_ptr(), n, d,
                        float(margin), _stream())
        ctx.save_for_backward(f, row_loss, p_idx, n_idx)
        ctx.ext = ext
        return row_loss.mean()

    @staticmethod
    def backward(ctx, grad_out):
        f, row_loss, p_idx, n_idx = ctx.saved_tensors
        n, d = f.shape
        grad = torch.zeros_like(f)
        # coeff = go * (1/N) * 2  (hinge mean + d(dist)/d(f) factor)
        coeff = float(grad_out) * 2.0 / n
        ctx.ext.triplet_bwd(f.data_ptr(), row_loss.data_ptr(),
                            p_idx.data_ptr(), n_idx.data_ptr(),
                            grad.data_ptr(), n, d, coeff, _stream())
        return grad, None, None, None


def triplet_loss(feature: torch.Tensor, target: torch.Tensor,
                 margin: Optional[float] = 0.3, norm_feat: bool = False,
                 hard_mining: bool = True) -> torch.Tensor:
    if (feature.is_cuda and hard_mining and not norm_feat
            and margin is not None and margin > 0 and feature.dim() == 2):
        ext = require_extension("triplet_fwd")
        if ext is not None:
            return _TripletHardFn.apply(feature.float(), target.long(),
                                        margin, ext)
    return ref.triplet_loss(feature, target, margin, norm_feat, hard_mining)


def cmc_map(query_features, query_labels, gallery_features, gallery_labels,
            query_camera_labels=None, gallery_camera_labels=None,
            query_chunk: int = 2048):
    """On GPU the Q×G similarity runs on the MFMA pairwise kernel; the rank
    statistics stay in device-side torch ops.  Queries are processed in
    chunks so million-image galleries (iCaRL config — K8/288 GB HBM) never
    materialise more than [chunk, G] similarities at once."""
    if not query_features.is_cuda:
        return ref.cmc_map(query_features, query_labels, gallery_features,
                           gallery_labels, query_camera_labels,
                           gallery_camera_labels)
    q = query_features.shape[0]
    g = gallery_features.shape[0]
    if q <= query_chunk:
        sims = similarity_matrix(query_features, gallery_features)
        return ref.cmc_map_from_sims(sims, query_labels, gallery_labels,
                                     query_camera_labels, gallery_camera_labels)
    total_cmc = torch.zeros(g, dtype=torch.float64)
    total_ap = 0.0
    for s0 in range(0, q, query_chunk):
        s1 = min(q, s0 + query_chunk)
        sims = similarity_matrix(query_features[s0:s1], gallery_features)
        cmc, mAP = ref.cmc_map_from_sims(
            sims, query_labels[s0:s1], gallery_labels,
            query_camera_labels[s0:s1] if query_camera_labels is not None else None,
            gallery_camera_labels)
        n = s1 - s0
        total_cmc += cmc * n
        total_ap += mAP * n
    return total_cmc / q, total_ap / q


def _window_attn_fwd_raw(ext, q, k, v, bias, mask, scale):
    bw, h, n, d = q.shape
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    bias_c = bias.detach().contiguous().float()
    if mask is not None:
        mask_c = mask.detach().contiguous().float()
        nw = mask_c.shape[0]
        mask_ptr = mask_c.data_ptr()
    else:
        mask_c, nw, mask_ptr = None, 1, 0
    out = torch.empty_like(qc)
    ext.window_attn_fwd(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                        bias_c.data_ptr(), mask_ptr, out.data_ptr(),
                        bw, h, n, d, nw, float(scale), _dt(qc), _stream())
    return out, qc, kc, vc, bias_c, mask_c


class _WindowAttnFn(torch.autograd.Function):
    """Fused Swin window MHSA fwd+bwd (K3, window_attn.hip) — the TRAINING
    path: the backward recomputes S→P per (window, head) in LDS and emits
    dQ/dK/dV plus dS; the relative-position-bias gradient is the window
    reduction of dS (the bias-table gather backward stays in autograd)."""

    @staticmethod
    def forward(ctx, q, k, v, bias, mask, scale):
        ext = require_extension("window_attn_fwd")
        out, qc, kc, vc, bias_c, mask_c = _window_attn_fwd_raw(
            ext, q.detach(), k.detach(), v.detach(), bias, mask, scale)
        ctx.save_for_backward(qc, kc, vc, bias_c)
        ctx.mask_c = mask_c
        ctx.scale = float(scale)
        ctx.bias_requires = bias.requires_grad
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ext = require_extension("window_attn_bwd")
        qc, kc, vc, bias_c = ctx.saved_tensors
        mask_c = ctx.mask_c
        bw, h, n, d = qc.shape
        nw = mask_c.shape[0] if mask_c is not None else 1
        go = grad_out.contiguous().to(qc.dtype)
        dq = torch.empty_like(qc)
        dk = torch.empty_like(kc)
        dv = torch.empty_like(vc)
        ds = torch.empty(bw, h, n, n, device=qc.device, dtype=torch.float32)
        ext.window_attn_bwd(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                            bias_c.data_ptr(),
                            mask_c.data_ptr() if mask_c is not None else 0,
                            go.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                            dv.data_ptr(), ds.data_ptr(), bw, h, n, d, nw,
                            ctx.scale, _dt(qc), _stream())
        dbias = ds.sum(dim=0) if ctx.bias_requires else None
        return dq, dk, dv, dbias, None, None


def window_attention(q, k, v, bias, mask, scale, dropout=None):
    """Swin window MHSA (K3): fused HIP kernels on GPU — eval forward AND
    the training fwd+bwd (dropout-free, the Swin-ReID default); eager
    composition on CPU or when attention dropout is active."""
    drop_p = 0.0
    if dropout is not None:
        drop_p = float(getattr(dropout, "p", 0.0))
    if (q.is_cuda and q.shape[-2] <= 64 and q.shape[-1] <= 64
            and drop_p == 0.0 and extension_available()):
        if not torch.is_grad_enabled():
            ext = require_extension("window_attn_fwd")
            out, *_ = _window_attn_fwd_raw(ext, q, k, v, bias, mask, scale)
            return out
        return _WindowAttnFn.apply(q, k, v, bias, mask, scale)
    return ref.window_attention(q, k, v, bias, mask, scale, dropout)


class _PatchMergeLNFn(torch.autograd.Function):
    """Fused Swin PatchMerging gather + LayerNorm (K4, patch_merge.hip):
    the 2×2 strided concat tensor never materialises; forward emits the
    normalized [B, L/4, 4C] rows the reduction GEMM consumes, backward
    scatters dx and reduces per-block dgamma/dbeta partials."""

    @staticmethod
    def forward(ctx, x, gamma, beta, H, W, eps):
        ext = require_extension("patch_merge_ln_fwd")
        x_c = x.detach().contiguous()
        b, L, c = x_c.shape
        rows = b * (H // 2) * (W // 2)
        y = torch.empty(b, L // 4, 4 * c, device=x.device, dtype=x.dtype)
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
        gamma_c = gamma.detach().float().contiguous()
        beta_c = beta.detach().float().contiguous()
        ext.patch_merge_ln_fwd(x_c.data_ptr(), gamma_c.data_ptr(),
                               beta_c.data_ptr(), y.data_ptr(),
                               mean.data_ptr(), rstd.data_ptr(), rows, c, H,
                               W, float(eps), _dt(x_c), _stream())
        ctx.save_for_backward(x_c, gamma_c, mean, rstd)
        ctx.hw = (H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = require_extension("patch_merge_ln_bwd")
        x_c, gamma_c, mean, rstd = ctx.saved_tensors
        H, W = ctx.hw
        b, L, c = x_c.shape
        rows = b * (H // 2) * (W // 2)
        nblk = (rows + 3) // 4
        dy_c = dy.contiguous().to(x_c.dtype)
        dx = torch.empty_like(x_c)
        dg_part = torch.empty(nblk, 4 * c, device=x_c.device,
                              dtype=torch.float32)
        db_part = torch.empty(nblk, 4 * c, device=x_c.device,
                              dtype=torch.float32)
        ext.patch_merge_ln_bwd(x_c.data_ptr(), gamma_c.data_ptr(),
                               dy_c.data_ptr(), mean.data_ptr(),
                               rstd.data_ptr(), dx.data_ptr(),
                               dg_part.data_ptr(), db_part.data_ptr(), rows,
                               c, H, W, _dt(x_c), _stream())
        dgamma = dg_part.sum(0) if ctx.needs_input_grad[1] else None
        dbeta = db_part.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dgamma, dbeta, None, None, None


def patch_merge_ln(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                   H: int, W: int, eps: float = 1e-5) -> Optional[torch.Tensor]:
    """Fused PatchMerging gather+LN; None when out of regime (caller runs
    the eager concat + LayerNorm)."""
    if (not x.is_cuda or x.dim() != 3 or H % 2 or W % 2
            or 4 * x.shape[2] > 3072 or x.shape[1] != H * W
            or not extension_available()):
        return None
    if x.dtype not in (torch.float32, torch.bfloat16):
        return None
    return _PatchMergeLNFn.apply(x, gamma, beta, H, W, eps)


def adaptive_linear_fwd(x: torch.Tensor, gw: torch.Tensor,
                        atten: Optional[torch.Tensor],
                        aw: Optional[torch.Tensor],
                        bias: Optional[torch.Tensor],
                        split_layout: int = 1) -> torch.Tensor:
    """Fused y = x · (atten⊙gw + aw)ᵀ + bias (K2) — bf16 MFMA, no-grad path.

    x bf16 [M, K]; gw/aw fp32 [N, K]; atten fp32 [K]; bias fp32 [N].
    """
    ext = require_extension("adaptive_linear_fwd")
    if ext is None:
        theta = ref.adaptive_compose(gw, atten, aw) if atten is not None else gw
        return (torch.nn.functional.linear(x.float(), theta,
                                           bias).to(x.dtype))
    m, k = x.shape
    n = gw.shape[0]
    x_c = x.contiguous()
    out = torch.empty(m, n, device=x.device, dtype=torch.bfloat16)
    ext.adaptive_linear_fwd(
        x_c.data_ptr(), gw.contiguous().data_ptr(),
        aw.contiguous().data_ptr() if aw is not None else 0,
        atten.contiguous().float().data_ptr() if atten is not None else 0,
        bias.contiguous().float().data_ptr() if bias is not None else 0,
        out.data_ptr(), m, n, k, split_layout, _stream())
    return out


def bn_eval_2d(x: torch.Tensor, bn, relu: bool = False) -> Optional[torch.Tensor]:
    """Fused eval-mode BatchNorm2d (one coalesced pass; MIOpen's inference
    kernel measured ~0.3 TB/s on ReID shapes).  Returns None when the fused
    path does not apply (train mode, CPU, missing stats/extension)."""
    if (not x.is_cuda or x.requires_grad or bn.running_mean is None
            or x.dtype not in (torch.float32, torch.bfloat16)
            or x.dim() not in (2, 4)):
        return None
    ext = _load_extension()
    if ext is None:
        return None
    if x.dim() == 2:      # BatchNorm1d rows: NHWC layout with H·W == 1
        if not x.is_contiguous():
            x = x.contiguous()
        nhwc, hw = True, 1
    else:
        nhwc = x.is_contiguous(memory_format=torch.channels_last)
        if not nhwc and not x.is_contiguous():
            x = x.contiguous()
        hw = x.shape[2] * x.shape[3]
    out = torch.empty_like(x)
    c = x.shape[1]
    ext.bn_eval(x.data_ptr(), out.data_ptr(),
                bn.weight.detach().float().contiguous().data_ptr(),
                bn.bias.detach().float().contiguous().data_ptr(),
                bn.running_mean.float().contiguous().data_ptr(),
                bn.running_var.float().contiguous().data_ptr(),
                x.numel(), c, hw, float(bn.eps), int(nhwc), int(relu),
                _dt(x), _stream())
    return out


_DRIFT_CHUNK = 1 << 16
_DRIFT_META: Dict = {}


class _L1DriftHipFn(torch.autograd.Function):
    """Fused multi-tensor Σ|p − p₀| (ops/csrc/drift.hip): one read-only pass
    forward, one sign-write pass backward into a single flat buffer split
    into per-tensor grad views."""

    @staticmethod
    def forward(ctx, meta, *tensors):        # tensors: the params, the anchors
        ext = require_extension("drift")
        ptrs, chunks, sizes, total = meta
        partials = torch.empty(chunks.shape[0], device=tensors[0].device,
                               dtype=torch.float32)
        ext.drift_fwd(ptrs.data_ptr(), chunks.data_ptr(), partials.data_ptr(),
                      chunks.shape[0], _stream())
        # the tables and the tensors they point to must outlive the caller's
        ctx.meta = meta
        ctx.tensors = tensors
        return partials.sum()

    @staticmethod
    def backward(ctx, grad_out):
        ext = require_extension("drift")
        ptrs, chunks, sizes, total = ctx.meta
        flat = torch.empty(total, device=grad_out.device, dtype=torch.float32)
        g = grad_out.to(torch.float32).contiguous()
        ext.drift_bwd(ptrs.data_ptr(), chunks.data_ptr(), g.data_ptr(),
                      flat.data_ptr(), chunks.shape[0], _stream())
        views = [v.view_as(p) for v, p in zip(flat.split(sizes), ctx.tensors)]
        return (None, *views, *([None] * len(views)))


def _drift_meta(pairs):
    """(ptr_table, chunk_table, sizes, total) on device, cached on the
    parameter storages (in-place per-round updates keep pointers stable;
    a dispatch that rebinds storage changes the key and rebuilds)."""
    key = tuple((p.data_ptr(), a.data_ptr(), p.numel()) for p, a in pairs)
    meta = _DRIFT_META.get(key)
    if meta is not None:
        return meta
    dev = pairs[0][0].device
    sizes = [p.numel() for p, _ in pairs]
    chunk_rows, _, total = _chunk_table(sizes, _DRIFT_CHUNK)
    ptrs = torch.tensor([(p.data_ptr(), a.data_ptr()) for p, a in pairs],
                        dtype=torch.int64, device=dev)
    chunks = torch.tensor(chunk_rows, dtype=torch.int32, device=dev)
    # entries are never evicted: a captured hipGraph may hold the table
    # pointers for its lifetime, and each entry is only ~KBs
    meta = (ptrs, chunks, sizes, total)
    _DRIFT_META[key] = meta
    return meta


def l1_drift(pairs) -> torch.Tensor:
    """Σ |p − p₀| over drift pairs — fused HIP multi-tensor path on GPU when
    every p and anchor is fp32, 16-byte aligned (float4 reads) and contiguous
    (backward's grad views are) on one device; _foreach fallback elsewhere."""
    pairs = [(p, a.detach()) for p, a in pairs]
    if (pairs and pairs[0][0].is_cuda and extension_available()
            and all(p.is_contiguous() and p.device == pairs[0][0].device
                    and _fusable(p) and _fusable(a, p) for p, a in pairs)
            and sum(p.numel() for p, _ in pairs) < 2 ** 31):   # int32 table
        return _L1DriftHipFn.apply(_drift_meta(pairs), *(p for p, _ in pairs),
                                   *(a for _, a in pairs))
    return ref.l1_drift_fused(pairs)


# ---------------------------------------------------------------------------
# fused multi-tensor quadratic penalty — EWC/MAS/FedCurv/FedProx (penalty.hip)
# ---------------------------------------------------------------------------

_PENALTY_META_CAP = 8
_PENALTY_META: "OrderedDict" = OrderedDict()


def _penalty_plan(params, sets):
    """([(p, [a_0, F_0, a_1, F_1, …])], padded_total) when every tensor of
    the call fits the kernel, else None.  A set's absent name contributes
    (None, None); importance=None contributes (a, None).  Names no set knows
    are left out (no term, no gradient — as the reference)."""
    rows, total = [], 0
    for n, p in params.items():
        slots, present = [], False
        for anchors, importance in sets:
            if n not in anchors:
                slots += [None, None]
                continue
            present = True
            slots += [anchors[n],
                      importance[n] if importance is not None else None]
        if not present:
            continue
        if (not _fusable(p) or p.numel() == 0
                or (rows and p.device != rows[0][0].device)
                or not all(t is None or _fusable(t, p) for t in slots)):
            return None
        rows.append((p, slots))
        total += -(-p.numel() // 4) * 4     # float4 stores: quad-aligned slots
    if not rows or total >= 2 ** 31:
        return None
    return rows, total


def _penalty_meta(rows, n_sets: int, total: int, chunk: int):
    """(ptr_table, chunk_table, S, flat_offsets, padded_total) on device,
    cached on the storages.  Unlike _DRIFT_META the cache is a small LRU: the
    penalty methods re-clone their anchors every round, so the keys keep
    changing, and none of them replays a captured graph that could hold a
    table (an autograd node in flight keeps its own reference)."""
    ptr_rows = [(p.data_ptr(), *(0 if t is None else t.data_ptr()
                                 for t in slots)) for p, slots in rows]
    key = (n_sets, rows[0][0].device,
           tuple((p.numel(), *pr) for (p, _), pr in zip(rows, ptr_rows)))
    meta = _PENALTY_META.get(key)
    if meta is not None:
        _PENALTY_META.move_to_end(key)
        return meta
    chunk_rows, offsets, flat_off = _chunk_table(
        [p.numel() for p, _ in rows], chunk, pad_to=4)    # quad-aligned slots
    assert flat_off == total
    dev = rows[0][0].device
    meta = (torch.tensor(ptr_rows, dtype=torch.int64, device=dev),
            torch.tensor(chunk_rows, dtype=torch.int32, device=dev),
            n_sets, offsets, total)
    _PENALTY_META[key] = meta
    while len(_PENALTY_META) > _PENALTY_META_CAP:
        _PENALTY_META.popitem(last=False)
    return meta


class _QuadraticPenaltyHipFn(torch.autograd.Function):
    """Fused multi-tensor Σ_s Σ F_s·(p − a_s)² (ops/csrc/penalty.hip): the
    forward reads p once and every set and writes the per-chunk partials; the
    backward reads them again and writes the gradient — in the eager chain's
    own rounding, so the bits are the reference's — into one flat buffer,
    handed out as per-tensor views in each param's own shape and strides."""

    @staticmethod
    def forward(ctx, meta, consts, *params):
        ext = require_extension("penalty_fwd")
        ptrs, chunks, n_sets, offsets, total = meta
        partials = torch.empty(chunks.shape[0], device=params[0].device,
                               dtype=torch.float32)
        ext.penalty_fwd(ptrs.data_ptr(), chunks.data_ptr(), n_sets,
                        partials.data_ptr(), chunks.shape[0], _stream())
        # params are saved for autograd's in-place-modification check; the
        # tables and the constants they point to must outlive the cache entry
        ctx.save_for_backward(*params)
        ctx.meta = meta
        ctx.consts = consts
        return partials.sum()

    @staticmethod
    def backward(ctx, grad_out):
        ext = require_extension("penalty_bwd")
        params = ctx.saved_tensors
        ptrs, chunks, n_sets, offsets, total = ctx.meta
        g = grad_out.to(torch.float32).contiguous()
        flat = torch.empty(total, device=g.device, dtype=torch.float32)
        ext.penalty_bwd(ptrs.data_ptr(), chunks.data_ptr(), n_sets,
                        g.data_ptr(), flat.data_ptr(), chunks.shape[0],
                        _stream())
        views = [torch.as_strided(flat, p.shape, p.stride(), off)
                 for p, off in zip(params, offsets)]
        return (None, None, *views)


def quadratic_penalty_sets(
        params: Dict[str, torch.Tensor],
        sets: Sequence[Tuple[Dict[str, torch.Tensor],
                             Optional[Dict[str, torch.Tensor]]]],
) -> torch.Tensor:
    """Σ_s Σ_n F_s[n]·(p[n] − a_s[n])² over (anchors, importance) sets; p read once.

    importance=None in a set is unit importance (FedProx); a name a set's
    anchors lack is skipped for that set.  Gradients flow to params only
    (anchors and importance are constants) and carry the eager reference's
    bits; the value differs from it by summation order.  Fused HIP path on GPU when every
    tensor of the call is fp32, 16-byte aligned and p / a_s / F_s share one
    dense layout per name (contiguous, channels-last, …) and the extension is
    built; otherwise — CPU, any ineligible tensor, or
    FLREID_NO_FUSED_PENALTY=1 — the whole call runs the eager reference."""
    sets = list(sets)
    first = next(iter(params.values()), None)
    if (sets and first is not None and first.is_cuda
            and os.environ.get("FLREID_NO_FUSED_PENALTY", "0") != "1"):
        plan = _penalty_plan(params, sets)
        if plan is not None:
            ext = require_extension("penalty_fwd")
            if ext is not None:
                rows, total = plan
                meta = _penalty_meta(rows, len(sets), total,
                                     ext.penalty_chunk())
                consts = tuple(t for _, slots in rows for t in slots
                               if t is not None)
                return _QuadraticPenaltyHipFn.apply(
                    meta, consts, *(p for p, _ in rows))
    return ref.quadratic_penalty_sets(params, sets)


def quadratic_penalty(params: Dict[str, torch.Tensor],
                      anchors: Dict[str, torch.Tensor],
                      importance: Optional[Dict[str, torch.Tensor]] = None,
                      ) -> torch.Tensor:
    """Σ F·(p − p_anchor)² — EWC/MAS penalty; importance=None is the FedProx
    proximal term.  One-set form of quadratic_penalty_sets."""
    return quadratic_penalty_sets(params, [(anchors, importance)])


class _BnTrain2dFn(torch.autograd.Function):
    """Fused training BatchNorm2d over channels-last rows (bn_train.hip).

    One kernel per direction instead of MIOpen's 5-kernel chains +
    SubTensorOp casts + the autocast fp32 round-trip; running stats update
    inside the forward kernel (replay-safe for hipGraph capture)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps,
                nbt, relu):
        ext = require_extension("bn_train")
        c = x.shape[1]
        m = x.numel() // c
        y = torch.empty_like(x)
        smean = torch.empty(c, device=x.device, dtype=torch.float32)
        sinv = torch.empty(c, device=x.device, dtype=torch.float32)
        # split-row partial-sum workspace (overwritten densely every call —
        # no zeroing kernel needed)
        nslab = ext.bn_train_nslab(m, c)
        part = torch.empty(2, nslab, c, device=x.device, dtype=torch.float32)
        has_rs = running_mean is not None
        ext.bn_train_fwd(
            x.data_ptr(), y.data_ptr(),
            gamma.detach().contiguous().data_ptr(),
            beta.detach().contiguous().data_ptr(),
            running_mean.data_ptr() if has_rs else 0,
            running_var.data_ptr() if has_rs else 0,
            smean.data_ptr(), sinv.data_ptr(),
            part[0].data_ptr(), part[1].data_ptr(),
            nbt.data_ptr() if nbt is not None else 0, m, c,
            float(momentum), float(eps), float(m) / float(m - 1),
            int(relu), _dt(x), _stream())
        ctx.save_for_backward(x, gamma, beta, smean, sinv)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, smean, sinv = ctx.saved_tensors
        if x.dim() == 4:
            if not dy.is_contiguous(memory_format=torch.channels_last):
                dy = dy.contiguous(memory_format=torch.channels_last)
        elif not dy.is_contiguous():
            dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        ext = require_extension("bn_train")
        c = x.shape[1]
        m = x.numel() // c
        dx = torch.empty_like(x)
        dgamma = torch.empty(c, device=x.device, dtype=torch.float32)
        dbeta = torch.empty(c, device=x.device, dtype=torch.float32)
        nslab = ext.bn_train_nslab(m, c)
        part = torch.empty(2, nslab, c, device=x.device, dtype=torch.float32)
        ext.bn_train_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                         gamma.detach().contiguous().data_ptr(),
                         beta.detach().contiguous().data_ptr(),
                         smean.data_ptr(), sinv.data_ptr(),
                         dgamma.data_ptr(), dbeta.data_ptr(),
                         part[0].data_ptr(), part[1].data_ptr(),
                         m, c, int(ctx.relu), _dt(x), _stream())
        return dx, dgamma, dbeta, None, None, None, None, None, None


def bn_train_2d(x: torch.Tensor, bn,
                relu: bool = False) -> Optional[torch.Tensor]:
    """Fused TRAINING-mode BatchNorm for the head-epoch regime.  Applies to
    CUDA channels-last 4-D tensors (BatchNorm2d) and contiguous 2-D tensors
    (BatchNorm1d — the BNNeck bottleneck) with C % 64 == 0 and a small row
    count (M = N·H·W ≤ 16384 — covers the cached-prototype batches AND
    batch-64 layer-4 full-image fine-tuning at 16×8 spatial; very large M
    stays on MIOpen's multi-block reduction).  The
    num_batches_tracked increment is fused into the forward kernel.  Returns
    None when the fused path does not apply."""
    if os.environ.get("FLREID_NO_FUSED_BN", "0") == "1":
        return None
    if (not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16)
            or bn.weight is None or bn.bias is None):
        return None
    if x.dim() == 4:
        if not x.is_contiguous(memory_format=torch.channels_last):
            return None
    elif x.dim() == 2:
        if not x.is_contiguous():
            return None
    else:
        return None
    c = x.shape[1]
    m = x.numel() // c
    if c % 64 != 0 or m < 2 or m > 16384:
        return None
    if bn.momentum is None:  # cumulative-average mode: keep torch semantics
        return None
    if not extension_available():
        return None
    nbt = None
    if bn.track_running_stats and bn.running_mean is not None:
        nbt = bn.num_batches_tracked
        rm, rv = bn.running_mean, bn.running_var
    else:
        rm = rv = None
    return _BnTrain2dFn.apply(x, bn.weight, bn.bias, rm, rv,
                              bn.momentum, bn.eps, nbt, relu)


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=torch.channels_last) \
        else t.contiguous(memory_format=torch.channels_last)


def compose_theta_bf16(ext, gw: torch.Tensor, atten: Optional[torch.Tensor],
                       aw: Optional[torch.Tensor],
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """θ = atten⊙gw + aw composed DIRECTLY to bf16 in the weight's own
    physical layout (compose2 kernel) — one pass, no fp32 θ in HBM, no
    autocast cast kernel.  atten broadcasts over the LOGICAL last dim; for
    channels-last 4-D weights the physical index of that dim is
    (i / C) % kw.  `out`: a bf16 buffer in gw's layout to compose into."""
    gw_d = gw.detach()
    L, inner = atten_geometry(gw_d)
    if atten is not None and atten.numel() != L:
        # a non-4-D weight may be the flattened view of one whose last dim
        # atten spans (the 1×1 route's [K, C·1·1]): atten then tiles its rows
        if gw_d.dim() == 4 or not atten.numel() or L % atten.numel():
            raise ValueError(f"compose_theta_bf16: {atten.numel()} atten "
                             f"entries do not fit a last weight dim of {L}")
        L = atten.numel()
    if out is None:
        out = torch.empty_like(gw_d, dtype=torch.bfloat16)
    elif out.dtype != torch.bfloat16 or not same_layout(out, gw_d):
        raise ValueError("compose_theta_bf16: out must be bf16 in gw's layout")
    ext.compose2(gw_d.data_ptr(),
                 atten.detach().float().contiguous().data_ptr() if atten is not None else 0,
                 aw.detach().data_ptr() if aw is not None else 0,
                 out.data_ptr(), gw_d.numel(), L, inner, _dt(gw_d), _BF16,
                 _stream())
    return out


class _AdaptiveLinearFn(torch.autograd.Function):
    """y = x·θᵀ + bias for the adaptive linear / 1×1 layers, in
    _Conv3x3Fn's convention: θ = atten⊙weight + aw, or `weight` itself when
    it is a ready bf16 θ (the head epoch's live θ; atten and aw None).

    fwd:  k2  = the K2 tile loop: θ composed in its weight fetch and never
                materialised, or loaded as it is when ready — the two sum in
                the same order, so they agree bit for bit;
          lib = θ composed straight to bf16 (compose2 — no fp32 θ in HBM,
                no autocast cast pass) unless ready, then the bf16 library
                GEMM.
    bwd:  dx = g·θ (θ recomposed when the forward never materialised it),
          dθ = gᵀ·x_bf, d_bias = Σg.  dθ IS d(aw) (identity composition),
          cast once to fp32; a ready θ takes it in bf16 — no cast pass.
    Only frozen weight/atten are supported next to aw (FedSTIL)."""

    @staticmethod
    def forward(ctx, x, weight, atten, aw, bias, engine):
        ext = require_extension("adaptive_linear")
        x_bf = x.detach().to(torch.bfloat16).contiguous()
        ready = weight.dtype == torch.bfloat16 and atten is None and aw is None
        theta = weight.detach() if ready else None
        if engine == "k2" and not ready:
            y = adaptive_linear_fwd(x_bf, weight.detach(), atten, aw.detach(),
                                    bias.detach() if bias is not None else None)
        elif engine == "k2":
            m, k = x_bf.shape
            y = torch.empty(m, theta.shape[0], device=x.device,
                            dtype=torch.bfloat16)
            ext.theta_linear_fwd(
                x_bf.data_ptr(), theta.data_ptr(),
                bias.detach().contiguous().float().data_ptr()
                if bias is not None else 0,
                y.data_ptr(), m, theta.shape[0], k, _stream())
        else:
            if theta is None:
                theta = compose_theta_bf16(ext, weight, atten, aw)
            y = x_bf @ theta.t()
            if bias is not None:
                y = y + bias.detach().to(torch.bfloat16)
        ctx.save_for_backward(x_bf, weight, atten, aw, theta)
        ctx.x_dtype = x.dtype
        ctx.ready = ready
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x_bf, weight, atten, aw, theta = ctx.saved_tensors
        g = grad_out.to(torch.bfloat16)
        dx = None
        if ctx.needs_input_grad[0]:
            if theta is None:
                theta = compose_theta_bf16(require_extension("compose2"),
                                           weight.contiguous(), atten,
                                           aw.contiguous())
            dx = (g @ theta).to(ctx.x_dtype)
        d_theta = g.t() @ x_bf
        d_weight = d_aw = None
        if ctx.ready:
            d_weight = d_theta
        elif aw is not None:
            d_aw = d_theta.to(torch.float32)
        d_bias = grad_out.sum(0).to(torch.float32) if ctx.has_bias else None
        return dx, d_weight, None, d_aw, d_bias, None


def adaptive_linear(x2d: torch.Tensor, weight: torch.Tensor,
                    atten: Optional[torch.Tensor], aw: Optional[torch.Tensor],
                    bias: Optional[torch.Tensor],
                    engine: str = "k2") -> Optional[torch.Tensor]:
    """The one dispatch guard of the adaptive linear / 1×1 routes: bf16
    y = x2d·θᵀ + bias through _AdaptiveLinearFn, or None when out of regime
    (the caller runs the library on θ).  θ = atten⊙weight + aw with frozen
    fp32 weight/atten, or `weight` itself: a ready, contiguous bf16 [N, K] θ
    with atten and aw None.

    engine "k2" is the classifier's route, the K2 tile loop.  Composing, it
    needs K % 32 == 0 and one atten entry per column; a ready θ goes to the
    library GEMM instead when K % 32 != 0 or FLREID_CLASSIFIER_GEMM=lib
    (faster at 64×8000×2048, other summation order — profiles/README.md).
    engine "lib" is the pointwise conv's route over its [N·H·W, C] view,
    compose2 + the library GEMM; FLREID_NO_FUSED_1X1=1 switches it off.

    Every route needs a bf16 x2d or autocast — except the composing K2
    route, which runs in bf16 and returns bf16 whether or not autocast is on
    (its kernel reads fp32 weights and rounds them itself)."""
    if not x2d.is_cuda or x2d.dim() != 2 or not extension_available():
        return None
    if engine == "lib" and os.environ.get("FLREID_NO_FUSED_1X1", "0") == "1":
        return None
    k = weight.shape[-1]
    ready = weight.dtype == torch.bfloat16 and atten is None and aw is None
    if ready:
        if not weight.is_contiguous():
            return None
        if k % 32 or os.environ.get("FLREID_CLASSIFIER_GEMM", "k2") == "lib":
            engine = "lib"
    elif (weight.requires_grad or (atten is not None and atten.requires_grad)
          or weight.dtype != torch.float32
          or (aw is not None and aw.dtype != torch.float32)):
        return None
    elif engine == "k2" and (atten is None or aw is None or k % 32
                             or atten.numel() != k):
        return None
    if (x2d.dtype != torch.bfloat16 and not torch.is_autocast_enabled()
            and (ready or engine != "k2")):
        return None
    return _AdaptiveLinearFn.apply(x2d, weight, atten, aw, bias, engine)


def conv_theta_tile(ext, w: torch.Tensor, atten: Optional[torch.Tensor],
                    aw: Optional[torch.Tensor], mode: int) -> torch.Tensor:
    """θ = atten⊙w + aw emitted straight into the conv-tiled bf16 layout
    the hand-written conv consumes (mode 0: [C/32][9][K][32p]; mode 1: the
    flipped-transposed dgrad tile [K/32][9][C][32p]) — composition, cast
    and im2col-free weight re-layout in ONE pass.  mode 2: the same
    flipped-transposed θ as a plain [C][3][3][K] buffer, i.e. a
    channels-last [C, K, 3, 3] conv weight (see conv_theta_flipt)."""
    w_d = w.detach()
    assert w_d.is_contiguous(memory_format=torch.channels_last)
    k, c = w_d.shape[0], w_d.shape[1]
    out = torch.empty(c * 9 * k, device=w.device, dtype=torch.bfloat16)
    ext.conv3x3_tile(
        w_d.data_ptr(),
        atten.detach().float().contiguous().data_ptr() if atten is not None else 0,
        aw.detach().data_ptr() if aw is not None else 0,
        out.data_ptr(), c, k, _dt(w_d), mode, _stream())
    return out


def conv_theta_flipt(ext, theta: torch.Tensor) -> torch.Tensor:
    """wT[c, k, r, s] = θ[k, c, 2-r, 2-s] as a channels-last bf16 conv
    weight: dgrad of the 3×3 s1p1 conv is conv2d(dy, wT, padding=1)."""
    k, c = theta.shape[0], theta.shape[1]
    flat = conv_theta_tile(ext, theta, None, None, mode=2)
    return flat.view(c, 3, 3, k).permute(0, 3, 1, 2)


def _conv_impl() -> str:
    """Per-op conv engine policy.  'auto' (default) picks the MEASURED
    winner per op (profiles/README.md K1 table): the library conv
    currently beats the hand kernels on the ReID shapes (CK fwd 529 TF vs
    hand 428; wgrad 380 vs 103), so auto routes the conv math to the
    library while keeping the fused one-pass θ production (compose2 to
    bf16 — no fp32 θ, no autocast cast) and the fp32 weight-grad path.
    'hand' forces the hand-written kernels everywhere (the A/B switch the
    probe and profiles use); 'lib' forces the library.  auto's dgrad is the
    library's FORWARD conv on the flipped-transposed θ: the library's
    fastest bwd-data solver on these shapes sums its K-split with atomics,
    so dx — and every gradient upstream — differed in the last bits from
    run to run, while its forward solver is as fast and reproducible."""
    return os.environ.get("FLREID_CONV_IMPL", "auto")


class _Conv3x3Fn(torch.autograd.Function):
    """3×3 s1p1 conv with the FedSTIL composition fused into the weight
    production (K1).

    fwd:   θ_bf16 tile/tensor from ONE compose2/tile pass over
           (gw, atten, aw); conv = hand halo kernel (conv3x3_img*.hip) or
           the library on θ, by policy (_conv_impl).
    dgrad: hand = the same kernel on the flip-transposed θ tile;
           auto = conv2d on the flip-transposed θ; lib = conv2d_input on θ.
    wgrad: hand = transpose-first MFMA reduction (fp32 out);
           lib = conv2d_weight (bf16, cast once).  For the adaptive layer
           dθ IS d(adaptive_weight) (identity composition).
    Only frozen gw/atten are supported (FedSTIL trains aw alone;
    plain nn.Conv2d passes the weight in slot 1)."""

    @staticmethod
    def forward(ctx, x, weight, atten, aw):
        ext = require_extension("conv3x3_img_fwd")
        x_bf = _cl(x.detach().to(torch.bfloat16))
        n, c, h, w = x_bf.shape
        k = weight.shape[0]
        hand = _conv_impl() == "hand"
        if weight.dtype == torch.bfloat16 and atten is None and aw is None:
            # a ready bf16 θ (the head epoch's live θ): no copy-compose
            theta = weight.detach()
        else:
            theta = compose_theta_bf16(ext, weight, atten, aw)  # plain CL θ
        if hand:
            y = torch.empty(n, k, h, w, device=x.device, dtype=torch.bfloat16,
                            memory_format=torch.channels_last)
            ext.conv3x3_img_fwd_ldsw(x_bf.data_ptr(), theta.data_ptr(),
                                     y.data_ptr(), n, h, w, c, k, _stream())
        else:
            y = torch.nn.functional.conv2d(x_bf, theta, padding=1)
        # the lib dgrad reuses the forward's θ — composing twice per step
        # cost ~1.2 ms/round
        ctx.save_for_backward(x_bf, weight, atten, aw,
                              None if hand else theta)
        ctx.x_dtype = x.dtype
        ctx.w_dtype = weight.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = require_extension("conv3x3_img_fwd")
        x_bf, weight, atten, aw, theta = ctx.saved_tensors
        n, c, h, w = x_bf.shape
        k = weight.shape[0]
        hand = _conv_impl() == "hand"
        dy_bf = _cl(dy.to(torch.bfloat16))
        dx = None
        if ctx.needs_input_grad[0]:
            if hand:
                # dgrad = the same kernel on the flip-transposed θ tile
                wt_tile = conv_theta_tile(ext, weight, atten, aw, mode=1)
                dx = torch.empty(n, c, h, w, device=dy.device,
                                 dtype=torch.bfloat16,
                                 memory_format=torch.channels_last)
                ext.conv3x3_img_fwd(dy_bf.data_ptr(), wt_tile.data_ptr(),
                                    dx.data_ptr(), n, h, w, k, c, _stream())
            else:
                if theta is None:
                    theta = compose_theta_bf16(ext, weight, atten, aw)
                if _conv_impl() == "lib":
                    dx = torch.nn.grad.conv2d_input((n, c, h, w), theta,
                                                    dy_bf, padding=1)
                else:
                    dx = torch.nn.functional.conv2d(
                        dy_bf, conv_theta_flipt(ext, theta), padding=1)
            if ctx.x_dtype != torch.bfloat16:
                dx = dx.to(ctx.x_dtype)
        d_weight = d_aw = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[3]:
            if hand:
                # wgrad on pre-transposed operands (the in-kernel
                # transposed scatter measured 75 LDS-conflict cycles/MFMA);
                # two exclusive M-split partials summed here
                m_rows = n * h * w
                # 128-elem pads both ends: the wgrad kernel loads
                # shifted/tail chunks unclamped (OOR lanes zero-masked)
                dyt = torch.empty(k * m_rows + 256, device=dy.device,
                                  dtype=torch.bfloat16)
                xt = torch.empty(c * m_rows + 256, device=dy.device,
                                 dtype=torch.bfloat16)
                if m_rows % 64:
                    # xT is masked per element, dyT only per row: the last
                    # chunk of dyT's row K-1 multiplies its tail pad by the
                    # zeroed xT lanes, and 0·NaN = NaN — so the pad must be
                    # finite.  Aligned M never reads it.
                    dyt[-128:].zero_()
                ext.transpose_bf16(dy_bf.data_ptr(), dyt.data_ptr() + 256,
                                   m_rows, k, _stream())
                ext.transpose_bf16(x_bf.data_ptr(), xt.data_ptr() + 256,
                                   m_rows, c, _stream())
                part = torch.empty(2, k * 9 * c, device=dy.device,
                                   dtype=torch.float32)
                ext.conv3x3_wgrad(dyt.data_ptr() + 256, xt.data_ptr() + 256,
                                  part.data_ptr(), n, h, w, c, k, _stream())
                # [K][9][C] flat == channels-last [K,C,3,3] physical layout
                dw = (part[0] + part[1]).view(k, 3, 3, c).permute(0, 3, 1, 2)
            else:
                dw = torch.nn.grad.conv2d_weight(
                    x_bf, (k, c, 3, 3), dy_bf, padding=1)
            # fp32 for aw (identity composition) and fp32 weights; a bf16
            # weight (the live θ) takes the bf16 wgrad as it is — no cast pass
            want = torch.float32 if ctx.needs_input_grad[3] else ctx.w_dtype
            if dw.dtype != want:
                dw = dw.to(want)
            if ctx.needs_input_grad[3]:
                d_aw = dw
            else:
                d_weight = dw
        return dx, d_weight, None, d_aw


def conv3x3_try(x: torch.Tensor, weight: torch.Tensor,
                atten: Optional[torch.Tensor] = None,
                aw: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Dispatch guard for the hand-written 3×3 s1p1 conv: returns None when
    out of regime (caller falls back to the library conv).  Regime: the
    ReID layer-4 shapes — H·W ≤ 128 (one image per block), H·W % 16 == 0,
    C % 32, K % 32, channels-last weights, frozen gw/atten, bf16 compute
    (native or autocast)."""
    if not x.is_cuda or x.dim() != 4 or not extension_available():
        return None
    if os.environ.get("FLREID_NO_FUSED_CONV", "0") == "1":
        return None
    n, c, h, w = x.shape
    k = weight.shape[0]
    hw = h * w
    if hw > 128 or hw % 16 or h + 2 > 18 or w + 2 > 10:
        return None
    if c % 32 or k % 32:
        return None
    if x.dtype != torch.bfloat16 and not torch.is_autocast_enabled():
        return None
    if weight.requires_grad and (aw is not None or atten is not None):
        return None                      # composed path trains aw only
    if atten is not None and atten.requires_grad:
        return None
    if weight.dim() != 4 or not weight.is_contiguous(memory_format=torch.channels_last):
        return None
    if aw is not None and not aw.is_contiguous(memory_format=torch.channels_last):
        return None
    return _Conv3x3Fn.apply(x, weight, atten, aw)


def conv3x3_fwd_nhwc(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Hand-written 3×3 s1 p1 NHWC bf16 conv forward (K1; frozen-backbone
    eval path).  x: channels-last bf16 [N, C, H, W]; weight: fp32
    channels-last [K, C, 3, 3].  Returns channels-last bf16 [N, K, H, W].
    Falls back to the library conv outside the kernel constraints."""
    n, c, h, w = x.shape
    k = weight.shape[0]
    if c % 32 != 0 or k % 16 != 0:
        return torch.nn.functional.conv2d(x, weight.to(x.dtype), padding=1)
    ext = require_extension("conv3x3_fwd")
    assert x.is_contiguous(memory_format=torch.channels_last)
    wcl = weight.detach()
    if not wcl.is_contiguous(memory_format=torch.channels_last):
        wcl = wcl.contiguous(memory_format=torch.channels_last)
    out = torch.empty(n, k, h, w, device=x.device,
                      dtype=torch.bfloat16).to(memory_format=torch.channels_last)
    ext.conv3x3_fwd(x.data_ptr(), wcl.float().data_ptr(), out.data_ptr(),
                    n, h, w, c, k, _stream())
    return out


# ---------------------------------------------------------------------------
# one-pass FedSTIL head update (head_step.hip)
# ---------------------------------------------------------------------------

HEAD_STEP_CHUNK = 1 << 14
_HS_GRAD_BF16, _HS_VEC, _HS_THETA, _HS_ATTEN_VEC = 1, 2, 4, 8


def head_step_partials(rows) -> int:
    """Number of drift partials a head_step over `rows` writes."""
    return sum(-(-r["aw"].numel() // HEAD_STEP_CHUNK) for r in rows)


def _head_step_row(r: Dict, partial0: int):
    aw = r["aw"]
    if not aw.is_cuda or aw.dtype != torch.float32:
        raise TypeError("head_step: aw must be a CUDA fp32 tensor")
    L, inner = atten_geometry(aw)
    for k in ("aw0", "m", "v", "dw"):
        t = r.get(k)
        if t is None:
            raise ValueError(f"head_step: missing '{k}' (null pointer)")
        if not t.is_cuda or t.device != aw.device:
            raise TypeError(f"head_step: '{k}' is not on aw's device")
        if t.numel() != aw.numel() or not same_layout(t, aw):
            raise ValueError(
                f"head_step: '{k}' {tuple(t.shape)}/{t.stride()} does not "
                f"match aw's layout {tuple(aw.shape)}/{aw.stride()}")
        if k == "dw":
            if t.dtype not in (torch.float32, torch.bfloat16):
                raise TypeError("head_step: dw must be fp32 or bf16")
        elif t.dtype != torch.float32:
            raise TypeError(f"head_step: '{k}' must be fp32")
    step = r.get("step")
    if (step is None or not step.is_cuda or step.dtype != torch.float32
            or step.numel() != 1):
        raise TypeError("head_step: step must be a CUDA fp32 scalar tensor")
    dw = r["dw"]
    flags = _HS_GRAD_BF16 if dw.dtype == torch.bfloat16 else 0
    gw, atten, theta = r.get("gw"), r.get("atten"), r.get("theta")
    has_theta = theta is not None
    if has_theta:
        if gw is None or atten is None:
            raise ValueError("head_step: theta needs gw and atten "
                             "(null pointer)")
        if (gw.dtype != torch.float32 or gw.device != aw.device
                or not same_layout(gw, aw)):
            raise ValueError("head_step: gw does not match aw's layout")
        if (theta.dtype != torch.bfloat16 or theta.device != aw.device
                or not same_layout(theta, aw)):
            raise ValueError("head_step: theta must be bf16 in aw's layout")
        if (atten.dtype != torch.float32 or atten.device != aw.device
                or not atten.is_contiguous() or atten.numel() != L):
            raise ValueError("head_step: atten must be a contiguous fp32 "
                             f"vector of the last weight dim ({L})")
        flags |= _HS_THETA
    # float4 path only for 16-byte rows whose 4-runs stay inside one
    # atten-broadcast segment (as compose2_kernel); scalar path otherwise
    galign = 8 if dw.dtype == torch.bfloat16 else 16
    vec = (all(r[k].data_ptr() % 16 == 0 for k in ("aw", "aw0", "m", "v"))
           and dw.data_ptr() % galign == 0)
    if vec and has_theta:
        vec = gw.data_ptr() % 16 == 0 and theta.data_ptr() % 8 == 0
        if vec and inner == 1 and L > 1 and L % 4 == 0 \
                and atten.data_ptr() % 16 == 0:
            flags |= _HS_ATTEN_VEC
        elif not (L == 1 or inner % 4 == 0):
            vec = False
    if vec:
        flags |= _HS_VEC
    return [aw.data_ptr(), r["aw0"].data_ptr(), dw.data_ptr(),
            gw.data_ptr() if has_theta else 0,
            atten.data_ptr() if has_theta else 0,
            r["m"].data_ptr(), r["v"].data_ptr(),
            theta.data_ptr() if has_theta else 0, step.data_ptr(),
            aw.numel(), L, inner, flags, partial0]


def _head_step_cpu(rows, partials, lr, beta1, beta2, weight_decay, eps, lam):
    off = 0
    partials.zero_()
    for r in rows:
        aw = r["aw"]
        a, m1, v1, theta, drift = ref.head_step_reference(
            aw, r["aw0"], r["dw"], r["m"], r["v"], r["step"], lr, beta1,
            beta2, weight_decay, eps, lam, r.get("gw") if r.get("theta")
            is not None else None, r.get("atten"))
        aw.copy_(a)
        r["m"].copy_(m1)
        r["v"].copy_(v1)
        if theta is not None:
            r["theta"].copy_(theta)
        partials[off] = drift
        off += -(-aw.numel() // HEAD_STEP_CHUNK)


@torch.no_grad()
def head_step(rows, partials: torch.Tensor, lr: float, beta1: float,
              beta2: float, weight_decay: float, eps: float,
              lam: float) -> None:
    """One fused FedSTIL head step over a list of adaptive weights.

    rows: dicts with aw, aw0, dw (fp32 or bf16 gradient), m, v (Adam
    moments, torch's layout), step (device fp32 count) and optionally
    gw + atten + theta (bf16 output: the next step's composed weight).
    Advances every step count by one, then — in ONE kernel pass per element
    — adds the L1-drift subgradient λ·sign(aw − aw0) to dw, applies torch's
    original-mode Adam and emits θ; `partials` (fp64,
    head_step_partials(rows) entries) receives per-block Σ|aw − aw0| of the
    pre-update weights, so partials.sum() is the drift value.

    Every row is validated before anything is launched; a violated check
    raises.  CPU tensors run head_step_reference."""
    rows = list(rows)
    if not rows:
        raise ValueError("head_step: empty tensor table")
    need = head_step_partials(rows)
    if (partials.dtype != torch.float64 or partials.numel() < need
            or not partials.is_contiguous()
            or partials.device != rows[0]["aw"].device):
        raise ValueError(f"head_step: partials must be a contiguous fp64 "
                         f"tensor of ≥ {need} entries on aw's device")
    if not rows[0]["aw"].is_cuda:
        torch._foreach_add_([r["step"] for r in rows], 1)
        _head_step_cpu(rows, partials, lr, beta1, beta2, weight_decay, eps,
                       lam)
        return
    ext = require_extension("head_step")
    if ext is None:
        raise RuntimeError("head_step has no eager GPU path")
    table, off = [], 0
    for r in rows:
        table.append(_head_step_row(r, off))
        off += -(-r["aw"].numel() // HEAD_STEP_CHUNK)
    assert ext.head_step_chunk() == HEAD_STEP_CHUNK
    torch._foreach_add_([r["step"] for r in rows], 1)
    ext.head_step(table, partials.data_ptr(), partials.numel(), float(lr),
                  float(beta1), float(beta2), float(weight_decay), float(eps),
                  float(lam), _stream())
