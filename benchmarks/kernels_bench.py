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


def report(results):
    for k in sorted(results):
        v = results[k]
        print(f"{k:28s} {v:10.3f}" + (" ms" if "_TF" not in k and "GBps" not in k else ""))


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
    args = p.parse_args()
    n = 1 if args.once else 50
    assert torch.cuda.is_available() and ops.extension_available()
    results = {}

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
