#!/usr/bin/env python3
"""Kernel microbenchmarks: fused HIP ops vs eager PyTorch composition.

Run on an MI355X box:
    python benchmarks/kernels_bench.py
Profile (separate runs per rocprofv3 constraints):
    rocprofv3 --kernel-trace --stats -d out -- python benchmarks/kernels_bench.py
    rocprofv3 --pmc SQ_INSTS_MFMA,SQ_INSTS_VALU,SQ_LDS_BANK_CONFLICT \
        -d out -- python benchmarks/kernels_bench.py --once
"""

import argparse
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref


def bench(fn, n=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def bench_decomposed(results, n):
    """FedWeIT composition fwd+bwd (decomposed.hip) vs the eager chain:
    fp32 parameters, bf16 θ, KB=5, at the three layer classes of the
    benchmark model.  GBps uses the kernels' traffic model: (KB+3) floats
    per element forward + (KB+4) backward."""
    kb = 5
    for tag, shape, cl in (("conv3x3_cl", (512, 512, 3, 3), True),
                           ("conv1x1", (2048, 512, 1, 1), False),
                           ("linear", (8000, 2048), False)):
        sw = torch.randn(shape, device="cuda")
        aw = torch.randn(shape, device="cuda")
        go = torch.randn(shape, device="cuda").bfloat16()
        if cl:
            sw, aw, go = (t.contiguous(memory_format=torch.channels_last)
                          for t in (sw, aw, go))
        aw.requires_grad_(True)
        mask = torch.rand(shape[0], device="cuda", requires_grad=True)
        aw_kb = torch.randn(*shape, kb, device="cuda")
        atten = torch.randn(kb, device="cuda", requires_grad=True)

        def run(compose):
            theta = compose(sw, mask, aw, aw_kb, atten, 1e-3, 0.0, True)
            theta.backward(go)
            aw.grad = mask.grad = atten.grad = None

        def fused(*a):
            return ops.decomposed_compose(*a, out_dtype=torch.bfloat16)

        def eager(*a):
            return ref.decomposed_compose(*a).bfloat16()

        results[f"decomposed_{tag}_fused"] = bench(lambda: run(fused), n)
        results[f"decomposed_{tag}_eager"] = bench(lambda: run(eager), n)
        nbytes = sw.numel() * 4 * ((kb + 3) + (kb + 4))
        results[f"decomposed_{tag}_fused_GBps"] = round(
            nbytes / (results[f"decomposed_{tag}_fused"] / 1e3) / 1e9, 0)


def bench_head_step(results, n):
    """One-pass FedSTIL head update (head_step.hip) over the ResNet-50
    head's 11 adaptive weights (31.3 M fp32: layer4 channels-last convs +
    the 8000×2048 classifier) against the chain it replaces — drift
    fwd+bwd, gradient cast + add, torch's fused Adam, compose2 — and the
    classifier forward on a ready bf16 θ: K2 tile loop with the bf16-load
    prologue vs the composing K2 kernel vs a plain bf16 GEMM.  GBps uses the
    36 B/element model (read aw, aw0, bf16 dw, gw, m, v; write aw, m, v and
    bf16 θ)."""
    shapes = [(512, 1024, 1, 1), (512, 512, 3, 3), (2048, 512, 1, 1),
              (2048, 1024, 1, 1)]
    shapes += [(512, 2048, 1, 1), (512, 512, 3, 3), (2048, 512, 1, 1)] * 2
    shapes += [(8000, 2048)]

    def mk(shape, dtype=torch.float32, scale=0.05):
        t = torch.randn(shape, device="cuda") * scale
        if len(shape) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        return t.to(dtype)

    rows, params, anchors, gws, attens, dws = [], [], [], [], [], []
    for shp in shapes:
        aw0 = mk(shp)
        aw = aw0 + mk(shp, scale=1e-3)
        row = {"aw": aw.clone(), "aw0": aw0, "dw": mk(shp, torch.bfloat16, 1e-2),
               "gw": mk(shp), "atten": torch.full((shp[-1],), 0.9, device="cuda"),
               "m": torch.zeros_like(aw), "v": torch.zeros_like(aw),
               "step": torch.zeros((), device="cuda"),
               "theta": torch.empty_like(aw, dtype=torch.bfloat16)}
        rows.append(row)
        params.append(torch.nn.Parameter(aw.clone()))
        anchors.append(aw0)
        gws.append(row["gw"]); attens.append(row["atten"]); dws.append(row["dw"])
    numel = sum(r["aw"].numel() for r in rows)
    partials = torch.zeros(ops.head_step_partials(rows), dtype=torch.float64,
                           device="cuda")
    hyper = (1e-3, 0.9, 0.999, 1e-5, 1e-8, 1e-4)

    def fused():
        ops.head_step(rows, partials, *hyper)
        return partials.sum()

    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-5, fused=True,
                           capturable=True)
    ext = ops.require_extension("compose2")
    pairs = list(zip(params, anchors))

    def unfused():
        loss = ops.l1_drift(pairs) * 1e-4
        loss.backward()
        for p, dw in zip(params, dws):
            p.grad += dw.to(torch.float32)
        opt.step()
        for p, gw, at in zip(params, gws, attens):
            ops.compose_theta_bf16(ext, gw, at, p.detach())
            p.grad = None

    results["head_step_fused"] = bench(fused, n)
    results["head_step_unfused_chain"] = bench(unfused, n)
    results["head_step_fused_GBps"] = round(
        numel * 36 / (results["head_step_fused"] / 1e3) / 1e9, 0)

    x = (torch.randn(64, 2048, device="cuda") * 0.5).bfloat16()
    cls = rows[-1]
    with torch.no_grad():
        results["classifier_fwd_k2_theta"] = bench(
            lambda: ops.adaptive_linear(x, cls["theta"], None, None, None), n)
        results["classifier_fwd_k2_compose"] = bench(
            lambda: ops.adaptive_linear_fwd(x, cls["gw"], cls["atten"],
                                            cls["aw"], None), n)
        results["classifier_fwd_bf16_gemm"] = bench(
            lambda: x @ cls["theta"].t(), n)


DRIFT_SHAPES = [(512, 512, 3, 3), (2048, 512, 1, 1), (512, 2048, 1, 1),
                (8000, 2048)] * 3


def bench_penalty(results, n):
    """Multi-tensor quadratic penalty fwd+bwd (penalty.hip) vs the eager
    reference over the layer4+classifier shape list of the drift entry, at
    S = 1 (EWC/MAS) and S = 3 (FedCurv with two other clients).  GBps uses
    the fused form's traffic model: 2S + 1 weight-sized reads forward, the
    same reads and the gradient write backward — 4S + 3 passes."""
    params = {str(i): torch.randn(s, device="cuda", requires_grad=True)
              for i, s in enumerate(DRIFT_SHAPES)}
    numel = sum(p.numel() for p in params.values())
    all_sets = [({k: torch.randn_like(p) for k, p in params.items()},
                 {k: torch.rand_like(p) for k, p in params.items()})
                for _ in range(3)]

    def run(fn, sets):
        loss = fn(params, sets) * 100.0
        loss.backward()
        for p in params.values():
            p.grad = None

    for s in (1, 3):
        sets = all_sets[:s]
        results[f"penalty_fused_s{s}"] = bench(
            lambda: run(ops.quadratic_penalty_sets, sets), n)
        results[f"penalty_eager_s{s}"] = bench(
            lambda: run(ref.quadratic_penalty_sets, sets), n)
        results[f"penalty_fused_s{s}_GBps"] = round(
            numel * 4 * (4 * s + 3)
            / (results[f"penalty_fused_s{s}"] / 1e3) / 1e9, 0)


def bench_window_mfma(results, n):
    """K3 at the 384² / window-12 geometry: fwd+bwd of the MFMA route
    (window_attn_mfma.hip) against ref.window_attention on the same tensors
    — 1024 windows × 4 heads × 144 tokens × 32, bf16, shift mask of 64
    windows.  Seven rounds, fused and eager alternating; the median round
    and the min / max of the rounds are reported.  TFps counts the 14 N²·D
    matrix FLOPs per (window, head) the backward-with-recompute algorithm
    needs (S, PV; S again, dP, dV, dQ, dK), over the fused median."""
    bw, h, nt, d, nw = 1024, 4, 144, 32, 64
    q, k, v, do = (torch.randn(bw, h, nt, d, device="cuda").bfloat16()
                   for _ in range(4))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    bias = torch.randn(h, nt, nt, device="cuda", requires_grad=True)
    mask = torch.where(torch.rand(nw, nt, nt, device="cuda") < 0.3,
                       -100.0, 0.0)
    mask[:, torch.arange(nt), torch.arange(nt)] = 0.0
    assert ops.window_attention_route(nt, d, q.dtype, 0.0) == "mfma"

    def run(fn):
        fn(q, k, v, bias, mask, d ** -0.5).backward(do)
        q.grad = k.grad = v.grad = bias.grad = None

    rounds = {"fused": [], "eager": []}
    for _ in range(1 if n == 1 else 7):
        rounds["fused"].append(bench(lambda: run(ops.window_attention),
                                     min(n, 10), warmup=2))
        rounds["eager"].append(bench(lambda: run(ref.window_attention),
                                     min(n, 10), warmup=2))
    for tag, ts in rounds.items():
        ts.sort()
        results[f"window_attn_mfma_fwdbwd_{tag}"] = ts[len(ts) // 2]
        results[f"window_attn_mfma_fwdbwd_{tag}_min"] = ts[0]
        results[f"window_attn_mfma_fwdbwd_{tag}_max"] = ts[-1]
    flops = 14 * bw * h * nt * nt * d
    results["window_attn_mfma_fwdbwd_fused_TFps"] = round(
        flops / (results["window_attn_mfma_fwdbwd_fused"] / 1e3) / 1e12, 1)


def bench_window_qkv(results, n):
    """K3 at the 224² / window-7 geometry of swin-tiny stage 0, from the
    packed projection output: `ops.window_attention_qkv` on a [4096, 49, 288]
    bf16 qkv (3 heads, shift mask of 64 windows, bias with grad), "packed"
    route (window_attn_qkv.hip) against the "unpacked" route (split, three
    .contiguous() copies, the VALU kernel, transpose back, restack of the
    three gradients) on the same tensors.  fwd+bwd, and the forward alone
    under no_grad.  Seven rounds, alternating; median, min and max."""
    bw, h, nt, d, nw = 4096, 3, 49, 32, 64
    qkv = torch.randn(bw, nt, 3 * h * d, device="cuda").bfloat16()
    qkv.requires_grad_(True)
    do = torch.randn(bw, nt, h * d, device="cuda").bfloat16()
    bias = torch.randn(h, nt, nt, device="cuda", requires_grad=True)
    mask = torch.where(torch.rand(nw, nt, nt, device="cuda") < 0.3,
                       -100.0, 0.0)
    mask[:, torch.arange(nt), torch.arange(nt)] = 0.0
    assert ops.window_attention_qkv_route(nt, d, qkv.dtype, 0.0) == "packed"
    packed_route = ops.window_attention_qkv_route

    def fwdbwd():
        ops.window_attention_qkv(qkv, h, bias, mask, d ** -0.5).backward(do)
        qkv.grad = bias.grad = None

    def fwd():
        with torch.no_grad():
            ops.window_attention_qkv(qkv, h, bias, mask, d ** -0.5)

    rounds = {}
    try:
        for _ in range(1 if n == 1 else 7):
            for tag, route in (("packed", packed_route),
                               ("unpacked", lambda *a: "unpacked")):
                ops.window_attention_qkv_route = route
                for what, fn in (("fwdbwd", fwdbwd), ("fwd", fwd)):
                    rounds.setdefault(f"window_attn_qkv_{what}_{tag}",
                                      []).append(
                        bench(fn, min(n, 10), warmup=2))
    finally:
        ops.window_attention_qkv_route = packed_route
    for key, ts in rounds.items():
        ts.sort()
        results[key] = ts[len(ts) // 2]
        results[key + "_min"] = ts[0]
        results[key + "_max"] = ts[-1]


def bench_window_map(results, n):
    """One attention sub-block of swin-tiny stage 0 between the qkv and proj
    linears: `ops.shifted_window_attention_qkv` on a [64, 56, 56, 288] bf16
    qkv map (3 heads, window 7, shift 3, bias with grad), route "map"
    (window_attn_map.hip on the map as it lies) against route "windows"
    (roll, partition, the packed kernel with the shift mask, reverse, roll and
    autograd's mirror images) on the same tensors.  fwd+bwd, and the forward
    alone under no_grad.  Seven rounds, alternating; median, min and max."""
    from flreid_amd.models.swin import SwinBlock
    b, hi, ws, shift, h, d = 64, 56, 7, 3, 3, 32
    nt = ws * ws
    qkv = torch.randn(b, hi, hi, 3 * h * d, device="cuda").bfloat16()
    qkv.requires_grad_(True)
    do = torch.randn(b, hi, hi, h * d, device="cuda").bfloat16()
    bias = torch.randn(h, nt, nt, device="cuda", requires_grad=True)
    mask = SwinBlock(h * d, (hi, hi), h, ws, shift).attn_mask.cuda()
    map_route = ops.shifted_window_attention_qkv_route
    assert map_route(nt, d, qkv.dtype, 0.0, hi, hi, ws, shift) == "map"

    def op():
        return ops.shifted_window_attention_qkv(qkv, h, ws, shift, bias, mask,
                                                d ** -0.5)

    def fwdbwd():
        op().backward(do)
        qkv.grad = bias.grad = None

    def fwd():
        with torch.no_grad():
            op()

    rounds = {}
    try:
        for _ in range(1 if n == 1 else 7):
            for tag, route in (("map", map_route),
                               ("windows", lambda *a: "windows")):
                ops.shifted_window_attention_qkv_route = route
                for what, fn in (("fwdbwd", fwdbwd), ("fwd", fwd)):
                    rounds.setdefault(f"window_attn_map_{what}_{tag}",
                                      []).append(
                        bench(fn, min(n, 10), warmup=2))
    finally:
        ops.shifted_window_attention_qkv_route = map_route
    for key, ts in rounds.items():
        ts.sort()
        results[key] = ts[len(ts) // 2]
        results[key + "_min"] = ts[0]
        results[key + "_max"] = ts[-1]


# one-launch tiles per flagship shape: variant id -> channels per block
# (the instantiation table of ops/csrc/bn_onepass.hip); +256 = plain block
# order instead of the per-XCD channel ranges
BN_ONEPASS_TILES = {
    (2048, 512): {0: 4, 1: 8, 2: 8},
    (2048, 2048): {3: 8, 4: 16},
    (64, 2048): {5: 8, 6: 16, 7: 32},
}


def bench_bn(results, n):
    """Train BN fwd and bwd at the three flagship shapes (bf16): the
    two-launch pair against every one-launch tile.  Device events around n
    back-to-back launches, median of 5 such windows; where the figure stops
    falling with the kernel it is the host's launch rate.  *_GBps = bytes the
    direction must move (fwd: read x, write y; bwd: read x and dy, write dx)
    over that time — the tensors are 0.25–8 MB and cache-resident, so this is
    not a share of HBM bandwidth."""
    ext = ops.require_extension("bn bench")
    n = max(n, 1) * 4

    def timed(fn):
        for _ in range(10):
            fn()
        ts = []
        for _ in range(5):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / n)
        return sorted(ts)[2]

    for (m, c), tiles in BN_ONEPASS_TILES.items():
        x = torch.randn(m, c, device="cuda").bfloat16()
        dy = torch.randn(m, c, device="cuda").bfloat16()
        y, dx = torch.empty_like(x), torch.empty_like(x)
        f32 = dict(device="cuda", dtype=torch.float32)
        gamma, beta = torch.rand(c, **f32) + 0.5, torch.randn(c, **f32)
        rm, rv = torch.zeros(c, **f32), torch.ones(c, **f32)
        sm, si = torch.empty(c, **f32), torch.empty(c, **f32)
        dg, db = torch.empty(c, **f32), torch.empty(c, **f32)
        nbt = torch.zeros((), device="cuda", dtype=torch.long)
        part = torch.empty(2, ext.bn_train_nslab(m, c), c, **f32)
        unb = m / (m - 1)

        st = torch.cuda.current_stream().cuda_stream
        px, py, pdy, pdx = (t.data_ptr() for t in (x, y, dy, dx))
        pg, pb, prm, prv = (t.data_ptr() for t in (gamma, beta, rm, rv))
        psm, psi, pdg, pdb = (t.data_ptr() for t in (sm, si, dg, db))
        pa, pbb, pn = part[0].data_ptr(), part[1].data_ptr(), nbt.data_ptr()

        def fwd2():
            ext.bn_train_fwd(px, py, pg, pb, prm, prv, psm, psi, pa, pbb, pn,
                             m, c, 0.1, 1e-5, unb, 1, 1, st)

        def bwd2():
            ext.bn_train_bwd(px, pdy, pdx, pg, pb, psm, psi, pdg, pdb, pa,
                             pbb, m, c, 1, 1, st)

        def fwd1(v):
            ext.bn_onepass_fwd(px, py, pg, pb, prm, prv, psm, psi, pn, m, c,
                               0.1, 1e-5, unb, 1, v, st)

        def bwd1(v):
            ext.bn_onepass_bwd(px, pdy, pdx, pg, pb, psm, psi, pdg, pdb, m,
                               c, 1, v, st)

        tag = f"bn_m{m}_c{c}"
        nbytes = {"fwd": 2 * m * c * 2, "bwd": 3 * m * c * 2}
        runs = {"two_launch": (fwd2, bwd2)}
        for v, w in tiles.items():
            for order, vv in (("", v), ("_plain", v + 256)):
                runs[f"one_launch_t{v}_w{w}{order}"] = (
                    lambda vv=vv: fwd1(vv), lambda vv=vv: bwd1(vv))
        runs["one_launch_default"] = (lambda: fwd1(-1), lambda: bwd1(-1))
        for name, (f, b) in runs.items():
            for d, fn in (("fwd", f), ("bwd", b)):
                ms = timed(fn)
                results[f"{tag}_{d}_{name}"] = ms
                results[f"{tag}_{d}_{name}_GBps"] = round(
                    nbytes[d] / (ms / 1e3) / 1e9, 0)

    bench_bn_residual(results, timed)


def bench_bn_residual(results, timed):
    """relu(bn(x) + identity) from the BN kernel against the three-kernel
    chain (bn, add, ReLU / threshold_backward) it replaces: train forward and
    backward at 2048×2048 bf16, and the eval pass (16-byte kernel with the
    residual against the one-element kernel + add + ReLU) on a
    [512, 256, 32, 16] channels-last capture chunk.  *_GBps = the bytes the
    fused form must move over its time."""
    ext = ops.require_extension("bn bench")
    st = torch.cuda.current_stream().cuda_stream
    f32 = dict(device="cuda", dtype=torch.float32)

    m, c = 2048, 2048
    x, res, dz = (torch.randn(m, c, device="cuda").bfloat16()
                  for _ in range(3))
    y, z, dx, dres = (torch.empty_like(x) for _ in range(4))
    gamma, beta = torch.rand(c, **f32) + 0.5, torch.randn(c, **f32)
    rm, rv = torch.zeros(c, **f32), torch.ones(c, **f32)
    sm, si = torch.empty(c, **f32), torch.empty(c, **f32)
    dg, db = torch.empty(c, **f32), torch.empty(c, **f32)
    nbt = torch.zeros((), device="cuda", dtype=torch.long)
    unb = m / (m - 1)
    ptr = lambda *ts: [t.data_ptr() for t in ts]          # noqa: E731
    px, pres, pdz, py, pz, pdx, pdres = ptr(x, res, dz, y, z, dx, dres)
    pg, pb, prm, prv, psm, psi, pdg, pdb = ptr(gamma, beta, rm, rv, sm, si,
                                               dg, db)
    pn = nbt.data_ptr()

    def fwd_fused():
        ext.bn_onepass_res_fwd(px, pres, pz, pg, pb, prm, prv, psm, psi, pn,
                               m, c, 0.1, 1e-5, unb, -1, st)

    def fwd_chain():
        ext.bn_onepass_fwd(px, py, pg, pb, prm, prv, psm, psi, pn, m, c, 0.1,
                           1e-5, unb, 0, -1, st)
        torch.relu_(y + res)

    fwd_fused()                     # z for the two backward rows

    def bwd_fused():
        ext.bn_onepass_res_bwd(px, pdz, pz, pdres, pdx, pg, pb, psm, psi, pdg,
                               pdb, m, c, -1, st)

    def bwd_chain():
        d = torch.ops.aten.threshold_backward(dz, z, 0)
        ext.bn_onepass_bwd(px, d.data_ptr(), pdx, pg, pb, psm, psi, pdg, pdb,
                           m, c, 0, -1, st)

    el = m * c * 2
    for name, fn, nbytes in (("fwd_fused", fwd_fused, 3 * el),
                             ("fwd_chain", fwd_chain, 3 * el),
                             ("bwd_fused", bwd_fused, 5 * el),
                             ("bwd_chain", bwd_chain, 5 * el)):
        ms = timed(fn)
        results[f"bn_res_m{m}_c{c}_{name}"] = ms
        results[f"bn_res_m{m}_c{c}_{name}_GBps"] = round(
            nbytes / (ms / 1e3) / 1e9, 0)

    shape = (512, 256, 32, 16)
    xe, re_ = (torch.randn(shape, device="cuda").bfloat16().to(
        memory_format=torch.channels_last) for _ in range(2))
    ye = torch.empty_like(xe)
    ce = shape[1]
    ge, be = torch.rand(ce, **f32) + 0.5, torch.randn(ce, **f32)
    me, ve = torch.randn(ce, **f32), torch.rand(ce, **f32) + 0.5
    pxe, pre, pye, pge, pbe, pme, pve = ptr(xe, re_, ye, ge, be, me, ve)
    n_el, hw = xe.numel(), shape[2] * shape[3]

    def eval_fused():
        ext.bn_eval_res(pxe, pre, pye, pge, pbe, pme, pve, n_el, ce, hw, 1e-5,
                        1, 0, 1, 1, st)

    def eval_chain():
        ext.bn_eval_res(pxe, 0, pye, pge, pbe, pme, pve, n_el, ce, hw, 1e-5,
                        1, 0, 0, 1, st)
        torch.relu_(ye + re_)

    def eval_wide():
        ext.bn_eval_res(pxe, 0, pye, pge, pbe, pme, pve, n_el, ce, hw, 1e-5,
                        1, 1, 1, 1, st)

    def eval_scalar():
        ext.bn_eval_res(pxe, 0, pye, pge, pbe, pme, pve, n_el, ce, hw, 1e-5,
                        1, 1, 0, 1, st)

    for name, fn, nbytes in (("fused", eval_fused, 3 * n_el * 2),
                             ("chain", eval_chain, 3 * n_el * 2),
                             ("wide_noresidual", eval_wide, 2 * n_el * 2),
                             ("scalar_noresidual", eval_scalar, 2 * n_el * 2)):
        ms = timed(fn)
        results[f"bn_eval_res_{name}"] = ms
        results[f"bn_eval_res_{name}_GBps"] = round(
            nbytes / (ms / 1e3) / 1e9, 0)


def bench_herding(results, n):
    """K10 selection alone: ops.herding_select on the kernel route
    (herding.hip, Gram form) against the torch route (the batched
    expanded-form loop) on the same features, host tables and the final
    D2H copy included.  (P, n, D, m): the flagship round, a fuller identity,
    and identities large enough for the workspace path."""
    for P, rows, D, m in ((64, 8, 2048, 32), (64, 40, 2048, 32),
                          (16, 300, 2048, 32)):
        g = torch.Generator().manual_seed(P + rows)
        feats = torch.relu(torch.randn(P * rows, D, generator=g)).cuda()
        pids = torch.arange(P).repeat_interleave(rows)[
            torch.randperm(P * rows, generator=g)]
        assert ops.herding_route(rows, D, feats.dtype, True) == "kernel"
        tag = f"herding_p{P}_n{rows}"
        results[f"{tag}_kernel"] = bench(
            lambda: ops.herding_select(feats, pids, m), n)
        results[f"{tag}_torch"] = bench(
            lambda: ref.herding_select(feats, pids, m), n)


def bench_rank_stats(results, n):
    """K8 evaluation: ops.cmc_map end to end, and the statistics step alone on
    one [chunk, G] similarity tile, on the kernel route (rank_stats.hip)
    against the torch route (FLREID_CMC=torch, the argsort / cumsum chain) in
    one process, the two alternating call by call.  Every call is timed on its
    own around a synchronise; reported are the median and the min / max over
    the repetitions.  Shapes (Q, G, D, query_chunk, ids, cameras): the
    iCaRL-scale gallery, Market-1501's test split, the bench's own split.
    Features are a unit centre per identity plus noise (same-id cosine ≈ 0.67,
    others ≈ 0), as a trained model's are: the kernel drops what ranks behind
    a query's weakest good hit, so its time depends on where the good hits
    rank — the torch route's does not."""
    reps = 1 if n == 1 else 7

    def timed(fn, route):
        if route == "torch":
            os.environ["FLREID_CMC"] = "torch"
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        finally:
            os.environ.pop("FLREID_CMC", None)

    def both(tag, fn):
        ms = {"kernel": [], "torch": []}
        for rep in range(reps + 2):                    # two warm-up rounds
            for route in ms:
                t = timed(fn, route)
                if rep >= 2 or reps == 1:
                    ms[route].append(t)
        for route, v in ms.items():
            v.sort()
            results[f"{tag}_{route}"] = v[len(v) // 2]
            results[f"{tag}_{route}_min"] = v[0]
            results[f"{tag}_{route}_max"] = v[-1]

    for Q, G, D, chunk, ids, n_cam in ((2048, 1 << 20, 2048, 256, 50000, 0),
                                       (3368, 19732, 2048, 2048, 751, 6),
                                       (128, 256, 2048, 2048, 64, 0)):
        gen = torch.Generator().manual_seed(G)
        gl = torch.randint(0, ids, (G,), generator=gen)
        ql = gl[torch.randperm(G, generator=gen)[:Q]]
        qc = gc = None
        if n_cam:
            gl[torch.randperm(G, generator=gen)[:G // 5]] = -1
            qc = torch.randint(0, n_cam, (Q,), generator=gen)
            gc = torch.randint(0, n_cam, (G,), generator=gen)
        centres = ref.l2_normalize(torch.randn(ids + 1, D, device="cuda"))

        def feats(labels):
            noise = torch.randn(labels.numel(), D, device="cuda")
            return ref.l2_normalize(centres[labels.cuda()]
                                    + noise * (0.7 / D ** 0.5))

        qf, gf = feats(ql), feats(gl)
        del centres
        tag = f"cmc_q{Q}_g{G}"
        both(tag, lambda: ops.cmc_map(qf, ql, gf, gl, qc, gc,
                                      query_chunk=chunk))
        # the statistics step alone, on the first chunk's tile
        c = min(Q, chunk)
        sims = ops.similarity_matrix(qf[:c], gf)
        tables = ops.rank_stats_tables(ql, gl, qc, gc, "cuda").rows(0, c)
        assert ops.cmc_map_route(Q, G, tables.max_good, True) == "kernel"
        qlc, qcc = ql[:c], qc[:c] if qc is not None else None

        def stats():
            if os.environ.get("FLREID_CMC") == "torch":
                return ref.cmc_map_from_sims(sims, qlc, gl, qcc, gc)
            return ops.rank_stats_from_sims(sims, qlc, gl, qcc, gc,
                                            tables=tables)

        both(f"{tag}_stats{c}", stats)
        del qf, gf, sims


def bench_triplet(results, n):
    """K5b: triplet loss forward + backward in the seven modes that
    triplet_gram.hip serves, at 64×2048 and 128×2048 (P×4 labels, squared
    distances of about 4), the gram route against the eager chain
    (FLREID_TRIPLET=eager) in one process, the two alternating.  One sample
    is the mean time of `calls` back-to-back forward + backward calls around
    a synchronise; reported are the median and the min / max over the
    samples, in ms per call."""
    reps, calls = (1, 1) if n == 1 else (7, 100)
    modes = [(nf, hm, m) for nf in (False, True) for hm in (True, False)
             for m in (0.3, None) if (nf, hm, m) != (False, True, 0.3)]
    for N in (64, 128):
        gen = torch.Generator().manual_seed(N)
        feat = (torch.randn(N, 2048, generator=gen) * (2.0 / 2048) ** 0.5
                ).cuda().requires_grad_(True)
        labels = (torch.arange(N) // 4)[torch.randperm(N, generator=gen)].cuda()
        for nf, hm, m in modes:
            assert ops.triplet_loss_route(N, 2048, nf, hm, m, True) == "gram"

            def sample(route):
                if route == "eager":
                    os.environ["FLREID_TRIPLET"] = "eager"
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        ops.triplet_loss(feat, labels, m, nf, hm).backward()
                        feat.grad = None
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / calls * 1e3
                finally:
                    os.environ.pop("FLREID_TRIPLET", None)

            ms = {"gram": [], "eager": []}
            for rep in range(reps + 2):                # two warm-up rounds
                for route in ms:
                    t = sample(route)
                    if rep >= 2 or reps == 1:
                        ms[route].append(t)
            tag = (f"triplet_n{N}_{'cos' if nf else 'euc'}_"
                   f"{'hard' if hm else 'wtd'}_{'hinge' if m else 'soft'}")
            for route, v in ms.items():
                v.sort()
                results[f"{tag}_{route}"] = v[len(v) // 2]
                results[f"{tag}_{route}_min"] = v[0]
                results[f"{tag}_{route}_max"] = v[-1]


def bench_add_ln(results, n):
    """Residual add + LayerNorm (add_ln.hip) against the eager chain the Swin
    block ran before (add, fp32 LayerNorm, bf16 cast) at the four stage
    shapes of swin-tiny at batch 64: fp32 stream, bf16 branch, bf16 rows out,
    γ / β with gradients.  Forward under no_grad and forward + backward (both
    outputs receive a gradient), the two routes alternating in one process.
    One sample is the mean time of `calls` back-to-back calls around a
    synchronise; reported are the median and the min / max over the samples
    in ms per call, and for the fused route the GB/s of the traffic it needs:
    forward 4 + 2 + 4 + 2 B per element, backward 4 + 2 + 4 + 4 + 2 B."""
    reps, calls = (1, 1) if n == 1 else (7, 20)
    for rows, c in ((64 * 3136, 96), (64 * 784, 192), (64 * 196, 384),
                    (64 * 49, 768)):
        x = torch.randn(rows, c, device="cuda", requires_grad=True)
        br = torch.randn(rows, c, device="cuda").bfloat16().requires_grad_(True)
        w = torch.randn(c, device="cuda", requires_grad=True)
        b = torch.randn(c, device="cuda", requires_grad=True)
        ds = torch.randn(rows, c, device="cuda")
        dy = torch.randn(rows, c, device="cuda").bfloat16()
        assert ops.add_layer_norm_route(c, x.dtype, br.dtype,
                                        dy.dtype) == "kernel"
        fns = {"fused": ops.add_layer_norm, "eager": ref.add_layer_norm}

        def sample(route, grad):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                with torch.set_grad_enabled(grad):
                    s, y = fns[route](x, br, w, b, 1e-5, torch.bfloat16)
                if grad:
                    torch.autograd.backward([s, y], [ds, dy])
                    x.grad = br.grad = w.grad = b.grad = None
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / calls * 1e3

        for grad, kind, nbytes in ((False, "fwd", 12), (True, "fwdbwd", 28)):
            ms = {"fused": [], "eager": []}
            for rep in range(reps + 2):                # two warm-up rounds
                for route in ms:
                    t = sample(route, grad)
                    if rep >= 2 or reps == 1:
                        ms[route].append(t)
            tag = f"add_ln_{rows}x{c}_{kind}"
            for route, v in ms.items():
                v.sort()
                results[f"{tag}_{route}"] = v[len(v) // 2]
                results[f"{tag}_{route}_min"] = v[0]
                results[f"{tag}_{route}_max"] = v[-1]
            results[f"{tag}_fused_GBps"] = round(
                rows * c * nbytes / (results[f"{tag}_fused"] / 1e3) / 1e9, 0)


def report(results):
    for k in sorted(results):
        v = results[k]
        print(f"{k:28s} {v:10.4f}" + (" ms" if "_TF" not in k and "GBps" not in k else ""))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--once", action="store_true",
                   help="single invocation per op (for PMC counter runs)")
    p.add_argument("--decomposed-only", action="store_true",
                   help="run only the FedWeIT composition entry")
    p.add_argument("--head-step-only", action="store_true",
                   help="run only the FedSTIL one-pass head update entry")
    p.add_argument("--penalty-only", action="store_true",
                   help="run only the quadratic-penalty entry")
    p.add_argument("--window-mfma-only", action="store_true",
                   help="run only the 144-token window attention entry")
    p.add_argument("--window-qkv-only", action="store_true",
                   help="run only the packed-qkv 49-token window attention "
                        "entry")
    p.add_argument("--window-map-only", action="store_true",
                   help="run only the map-addressed shifted-window attention "
                        "entry")
    p.add_argument("--bn-only", action="store_true",
                   help="run only the train-BN entry: one-launch tiles "
                        "against the two-launch pair")
    p.add_argument("--herding-only", action="store_true",
                   help="run only the herding selection entry: kernel "
                        "against the torch route")
    p.add_argument("--rank-stats-only", action="store_true",
                   help="run only the CMC/mAP entry: rank-statistics kernel "
                        "against the torch sort chain")
    p.add_argument("--triplet-only", action="store_true",
                   help="run only the triplet entry: the Gram-form kernels "
                        "against the eager chain, seven modes")
    p.add_argument("--add-ln-only", action="store_true",
                   help="run only the residual add + LayerNorm entry: the "
                        "fused kernel against the eager chain, four Swin "
                        "stage shapes")
    args = p.parse_args()
    n = 1 if args.once else 50
    assert torch.cuda.is_available() and ops.extension_available()
    results = {}

    if args.add_ln_only:
        bench_add_ln(results, n)
        report(results)
        return

    if args.triplet_only:
        bench_triplet(results, n)
        report(results)
        return

    if args.rank_stats_only:
        bench_rank_stats(results, n)
        report(results)
        return
    if args.herding_only:
        bench_herding(results, n)
        report(results)
        return
    if args.bn_only:
        bench_bn(results, n)
        report(results)
        return
    if args.window_map_only:
        bench_window_map(results, n)
        report(results)
        return
    if args.window_mfma_only:
        bench_window_mfma(results, n)
        report(results)
        return
    if args.window_qkv_only:
        bench_window_qkv(results, n)
        report(results)
        return
    if args.penalty_only:
        bench_penalty(results, n)
        report(results)
        return
    if args.head_step_only:
        bench_head_step(results, n)
        report(results)
        return
    bench_head_step(results, n)
    bench_decomposed(results, n)
    if args.decomposed_only:
        report(results)
        return

    # K8: eval similarity GEMM (MFMA f32) — Q×G at validation scale
    qf = ref.l2_normalize(torch.randn(2048, 2048, device="cuda"))
    gf = ref.l2_normalize(torch.randn(16384, 2048, device="cuda"))
    with torch.no_grad():
        results["pairwise_sim_mfma"] = bench(
            lambda: ops.similarity_matrix(qf, gf), n)
        results["pairwise_sim_eager"] = bench(lambda: qf @ gf.t(), n)
        flops = 2 * qf.shape[0] * gf.shape[0] * qf.shape[1]
        results["pairwise_sim_mfma_TF"] = round(
            flops / (results["pairwise_sim_mfma"] / 1e3) / 1e12, 1)

    # K6: fused label-smooth CE fwd+bwd vs eager
    score = torch.randn(64, 8000, device="cuda", requires_grad=True)
    target = torch.randint(0, 8000, (64,), device="cuda")

    def fused_ce():
        loss = ops.ce_label_smooth(score, target, 0.1)
        loss.backward()
        score.grad = None

    def eager_ce():
        loss = ref.ce_label_smooth(score, target, 0.1)
        loss.backward()
        score.grad = None

    results["ce_smooth_fused"] = bench(fused_ce, n)
    results["ce_smooth_eager"] = bench(eager_ce, n)

    # K3: fused window attention (Swin stage-1 tiny shape) vs eager
    q = torch.randn(4096, 3, 49, 32, device="cuda").bfloat16()
    k, v = torch.randn_like(q), torch.randn_like(q)
    bias = torch.randn(3, 49, 49, device="cuda")
    with torch.no_grad():
        results["window_attn_fused"] = bench(
            lambda: ops.window_attention(q, k, v, bias, None, 0.18), n)
        results["window_attn_eager"] = bench(
            lambda: ref.window_attention(q, k, v, bias, None, 0.18), n)
    del q, k, v, bias
    bench_window_mfma(results, n)
    bench_window_qkv(results, n)
    bench_window_map(results, n)

    # K11: rowwise L2 normalize
    x = torch.randn(16384, 2048, device="cuda")
    with torch.no_grad():
        results["l2norm_fused"] = bench(lambda: ops.l2_normalize(x), n)
        results["l2norm_eager"] = bench(lambda: ref.l2_normalize(x), n)
        gbps = 2 * x.numel() * 4 / (results["l2norm_fused"] / 1e3) / 1e9
        results["l2norm_fused_GBps"] = round(gbps, 0)

    # compose (FedSTIL θ) standalone
    gw = torch.randn(2048, 8000, device="cuda")
    aw = torch.randn_like(gw)
    atten = torch.full((8000,), 0.9, device="cuda")
    with torch.no_grad():
        results["compose_fused"] = bench(
            lambda: ops.adaptive_compose(gw, atten, aw), n)
        results["compose_eager"] = bench(
            lambda: ref.adaptive_compose(gw, atten, aw), n)

    # fused train-mode BN fwd+bwd vs MIOpen (head-epoch shape: M=2048, C=512)
    import torch.nn as nn
    for c in (512, 2048):
        bn = nn.BatchNorm2d(c).cuda().train()
        xb = (torch.randn(64, c, 8, 4, device="cuda").bfloat16()
              .to(memory_format=torch.channels_last))

        def fused_bn():
            x1 = xb.detach().requires_grad_(True)
            y = ops.bn_train_2d(x1, bn)
            y.backward(y.detach())

        def miopen_bn():
            x1 = xb.detach().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = nn.functional.batch_norm(
                    x1, bn.running_mean, bn.running_var, bn.weight, bn.bias,
                    True, 0.1, bn.eps)
            y.backward(y.detach())

        results[f"bn_train_c{c}_fused"] = bench(fused_bn, n)
        results[f"bn_train_c{c}_miopen"] = bench(miopen_bn, n)

    # fused multi-tensor L1 drift (FedSTIL per-step regulariser) vs _foreach
    shapes = DRIFT_SHAPES
    params = [torch.randn(s, device="cuda", requires_grad=True)
              for s in shapes]
    anchors = [torch.randn(s, device="cuda") for s in shapes]
    pairs = list(zip(params, anchors))

    def fused_drift():
        loss = ops.l1_drift(pairs)
        loss.backward()
        for p in params:
            p.grad = None

    def foreach_drift():
        loss = ref.l1_drift_fused(pairs)
        loss.backward()
        for p in params:
            p.grad = None

    results["drift_fused"] = bench(fused_drift, n)
    results["drift_foreach"] = bench(foreach_drift, n)

    bench_penalty(results, n)

    report(results)


if __name__ == "__main__":
    main()
