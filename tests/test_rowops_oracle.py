"""The row-op oracle (tests/rowops_oracle.py) is sound and sharp — on the CPU.

For every case the GPU tests (test_rowops_exact_gpu.py) run:

* the grid preconditions hold (`exact=True` asserts them);
* an ideal kernel — the same operation in fp32 eager torch, float32
  throughout — passes the bound with worst ratio <= 1, so the bounds are not
  too tight;
* each of a fixed list of wrong results, made by mutating the float64
  reference, misses the bound by a factor of at least 10 wherever the
  mutation can be seen, so the bounds are not too loose;
* the hand-written float64 backward formulas agree with float64 autograd."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowops_oracle as ro
from flreid_amd.ops import reference as ref_ops

SHARP = 10.0


def _ids(c):
    return "x".join(str(v) for v in c)


def _ratios(got: dict, ref: ro.Ref) -> dict:
    return {k: ro.worst_ratio(got[k], *ref[k]) for k in got}


def _store(t32: torch.Tensor, dtype) -> torch.Tensor:
    return t32.to(dtype)


# ---------------------------------------------------------------------------
# pairwise and rowsq
# ---------------------------------------------------------------------------

def _pairwise_fp32(a, b, mode):
    if mode == 0:
        return a @ b.t()
    if mode == 1:
        return ref_ops.pairwise_cosine_distance(a, b)
    return ref_ops.pairwise_sqeuclidean(a, b)


@pytest.mark.parametrize("mode", ro.PAIRWISE_MODES)
@pytest.mark.parametrize("case", ro.PAIRWISE_CASES, ids=_ids)
def test_pairwise_cases(case, mode):
    m, n, d = case
    a, b = ro.pairwise_inputs("grid", case, mode)
    ref = ro.pairwise_reference(a, b, mode, exact=True)     # preconditions
    assert torch.equal(_pairwise_fp32(a, b, mode).double(), ref["out"][0])
    a, b = ro.pairwise_inputs("full", case, mode)
    ref = ro.pairwise_reference(a, b, mode)
    r = ro.worst_ratio(_pairwise_fp32(a, b, mode), *ref["out"])
    print("pairwise ideal", case, mode, round(r, 4))
    assert r <= 1.0, r
    # mutant: the K tail dropped (D rounded down to a multiple of 32)
    d32 = d // 32 * 32
    if d32 != d:
        bad = ro.pairwise_reference(a, b, mode, d_used=d32)["out"][0]
        assert ro.worst_ratio(bad, *ref["out"]) >= SHARP
        ga, gb = ro.pairwise_inputs("grid", case, mode)
        gref = ro.pairwise_reference(ga, gb, mode, exact=True)["out"][0]
        gbad = ro.pairwise_reference(ga, gb, mode, d_used=d32)["out"][0]
        assert not torch.equal(gbad, gref)


def test_pairwise_sliced_case_and_rowsq():
    a, b = ro.pairwise_inputs("grid", ro.PAIRWISE_SLICED_CASE, 0,
                              extra_row=True)
    assert a.shape[0] == ro.PAIRWISE_SLICED_CASE[0] + 1
    assert a[1:].is_contiguous() and a[1:].data_ptr() % 16 == 0
    ro.pairwise_reference(a[1:], b, 0, exact=True)
    for cols in ro.ROWSQ_COLS:
        x, z = ro.rowsq_inputs("grid", cols)
        ref = ro.pairwise_reference(x, z, 2, exact=True)["out"][0]
        assert torch.equal(ref[:, 0], (x.double() ** 2).sum(1))
        # the exact check sees one missing column out of 2048 (the bound,
        # at 2 (D + 3) u, cannot: that is what grid inputs are for)
        drop = (x[:, :-1].double() ** 2).sum(1)
        assert torch.equal(drop != ref[:, 0], x[:, -1] != 0)
        x, z = ro.rowsq_inputs("full", cols)
        ref = ro.pairwise_reference(x, z, 2)
        got = (x * x).sum(1, keepdim=True)
        assert ro.worst_ratio(got, *ref["out"]) <= 1.0


# ---------------------------------------------------------------------------
# triplet
# ---------------------------------------------------------------------------

def _triplet_fp32(f, labels, margin, upstream):
    """An ideal fp32 kernel: distances as sums of squared differences (so
    identical rows tie exactly, as they do in the kernel), numpy
    first-index selection, the analytic gradient — float32 throughout."""
    n, d = f.shape
    dist = ((f.view(n, 1, d) - f.view(1, n, d)) ** 2).sum(-1)
    is_pos = labels.view(n, 1).eq(labels.view(1, n))
    dp = (dist * is_pos).numpy()
    dn = (dist * ~is_pos + np.float32(1e9) * is_pos.float()).numpy()
    p, nn = dp.argmax(1), dn.argmin(1)
    ar = np.arange(n)
    row = np.maximum(np.float32(0), np.float32(margin) + dp[ar, p]
                     - dn[ar, nn])
    p = np.where(is_pos.numpy()[ar, p], p, ar)
    coeff = np.float32(2.0 * upstream / n)
    g = torch.zeros_like(f)
    for i in range(n):
        if row[i] > 0:
            for sign, j in ((1.0, int(p[i])), (-1.0, int(nn[i]))):
                t = float(sign * coeff) * (f[i] - f[j])
                g[i] += t
                g[j] -= t
    return torch.tensor(row.mean(dtype=np.float32)), g


@pytest.mark.parametrize("size,pattern", ro.TRIPLET_CASES,
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_triplet_cases(size, pattern):
    n, d = size
    # grid: preconditions, and autograd agrees with the analytic gradient
    f, labels = ro.triplet_inputs("grid", size, pattern)
    if n & (n - 1) == 0:
        for margin in ro.TRIPLET_MARGINS:
            for up in ro.TRIPLET_GRID_UPSTREAM:
                ref = ro.triplet_reference(f, labels, margin, up, exact=True)
                active = [i for i in range(n) if float(ref.row_loss[i]) > 0]
                analytic = ro._triplet_scatter(
                    f.double(), active, ref.p_idx, ref.n_idx, 2.0 * up / n)
                assert torch.equal(ref.grad[0], analytic)
                assert torch.equal(ref.grad[0].float().double(), ref.grad[0])
                loss32, g32 = _triplet_fp32(f, labels, margin, up)
                assert torch.equal(g32.double(), ref.grad[0])
                assert np.allclose(ro.triplet_row_loss_fp32(ref, margin),
                                   ref.row_loss.numpy(), rtol=1e-5, atol=0)
    # full: stable selection, ideal fp32 within the bound, mutants outside
    f, labels = ro.triplet_inputs("full", size, pattern)
    for margin in ro.TRIPLET_MARGINS:
        up = ro.TRIPLET_FULL_UPSTREAM
        ref = ro.triplet_reference(f, labels, margin, up)
        assert ref.stable, "selection within reach of the fp32 error"
        loss32, g32 = _triplet_fp32(f, labels, margin, up)
        r = {"loss": ro.worst_ratio(loss32, *ref.loss),
             "grad": ro.worst_ratio(g32, *ref.grad)}
        print("triplet ideal", size, pattern, margin, r)
        assert max(r.values()) <= 1.0, r
        if pattern == "one":
            assert float(ref.loss[0]) == 0 and not bool(ref.grad[0].any())
        if pattern.startswith("dup"):
            bad = ro.triplet_reference(f, labels, margin, up,
                                       last_index_ties=True)
            assert ro.worst_ratio(bad.grad[0], *ref.grad) >= SHARP
        # the suspected kernel behaviour shows wherever an ACTIVE anchor's
        # maximum sits on a negative's column: always for the singleton
        # patterns; never for "distinct", whose anchors are all inactive
        seen = any(float(ref.row_loss[i]) > 0 and ref.p_idx[i] != ref.p_first[i]
                   for i in range(n))
        assert seen == pattern.startswith("singleton"), seen
        if seen:
            bad = ro.triplet_reference(f, labels, margin, up,
                                       through_negative=True)
            assert ro.worst_ratio(bad.grad[0], *ref.grad) >= SHARP


@pytest.mark.parametrize("kind", ["grid", "full"])
@pytest.mark.parametrize("pattern", ["singleton_lo", "singleton_hi"])
@pytest.mark.parametrize("size", ro.TRIPLET_SIZES, ids=_ids)
def test_singleton_anchor_has_no_ap_gradient(size, pattern, kind):
    """The anchor alone in its class is active (its copy one grid step away
    is a negative, squared distance 1/64 < margin), its hardest positive is
    itself, and the reference sends nothing through ap: the whole gradient
    the anchor causes is the an part."""
    n, d = size
    f, labels = ro.triplet_inputs(kind, size, pattern)
    a = n // 2
    neg = a - 1 if pattern == "singleton_lo" else a + 1
    assert int((labels == labels[a]).sum()) == 1
    for margin in ro.TRIPLET_MARGINS:
        ref = ro.triplet_reference(f, labels, margin, 1.0)
        assert float(ref.row_loss[a]) > 0 and ref.n_idx[a] == neg
        assert abs(float(ref.an[a]) - 1 / 64) < 1e-6
        assert ref.p_idx[a] == a
        assert not bool(ro._triplet_scatter(
            f.double(), [a], ref.p_idx, ref.n_idx, 2.0 / n, part="ap").any())
        # float64 autograd agrees: the anchor's own row moves only along
        # f_a - f_neg, whatever else other anchors add to it
        others = [i for i in range(n)
                  if i != a and float(ref.row_loss[i]) > 0]
        rest = ro._triplet_scatter(f.double(), others, ref.p_idx, ref.n_idx,
                                   2.0 / n)
        own = ref.grad[0] - rest
        want = torch.zeros_like(own)
        want[a] = -(2.0 / n) * (f[a] - f[neg]).double()
        want[neg] = -want[a]
        assert torch.allclose(own, want, rtol=0, atol=1e-12)
        if ref.p_first[a] != a:       # the maximum sits on a negative
            bad = ro.triplet_reference(f, labels, margin, 1.0,
                                       through_negative=True)
            assert ro.worst_ratio(bad.grad[0], *ref.grad) >= SHARP


def test_triplet_patterns_do_what_they_say():
    for size in ro.TRIPLET_SIZES:
        assert sum(ro.triplet_admits(size, p)
                   for p in ro.TRIPLET_PATTERNS) >= 4
    for pattern, j2 in (("dup_stride", 5), ("dup_adjacent", 2)):
        for kind in ("grid", "full"):
            f, labels = ro.triplet_inputs(kind, (8, 64), pattern)
            ref = ro.triplet_reference(f, labels, 0.3, 1.0)
            assert torch.equal(f[1], f[j2]) and labels[1] == labels[j2]
            # anchor 0: the copies tie as hardest positive, first one wins
            assert ref.p_idx[0] == 1
            last = ro.triplet_reference(f, labels, 0.3, 1.0,
                                        last_index_ties=True)
            assert last.p_first[0] == j2
            # anchor 4: they tie as hardest negative
            assert ref.n_idx[4] == 1 and labels[4] != labels[1]
            assert float(ref.row_loss[0]) > 0 and float(ref.row_loss[4]) > 0


# ---------------------------------------------------------------------------
# window attention
# ---------------------------------------------------------------------------

def _window_autograd(inp, dt=torch.float64):
    """autograd, in `dt` throughout, of softmax(scale q k^T + bias[h] +
    mask[bw % nW]) v on the values the kernel reads -> dict of out, dq, dk,
    dv, dbias.  (reference.window_attention computes its softmax in fp32
    whatever it is given, and needs BW % nW == 0.)"""
    q, k, v = (t.to(dt).requires_grad_(True) for t in (inp.q, inp.k, inp.v))
    bias = inp.bias.to(dt).requires_grad_(True)
    attn = (q * float(np.float32(inp.scale))) @ k.transpose(-2, -1) + bias
    if inp.mask is not None:
        w = torch.arange(q.shape[0]) % inp.mask.shape[0]
        attn = attn + inp.mask.to(dt)[w].unsqueeze(1)
    out = torch.softmax(attn, -1) @ v
    out.backward(inp.do.to(dt))
    return {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad,
            "dbias": bias.grad}


@pytest.mark.parametrize("dtype", ro.WINDOW_DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ro.WINDOW_CASES, ids=_ids)
def test_window_cases(case, dtype):
    bw, h, n, d, nw = case
    inp = ro.window_inputs(case, dtype)
    ref = ro.window_reference(inp)
    if inp.mask is not None:
        assert inp.mask.shape[0] == nw
        assert set(inp.mask.unique().tolist()) <= {0.0, -100.0}
        assert int((inp.mask[0, 0] == 0).sum()) == 1
        if nw > 1:
            assert not torch.equal(inp.mask[0], inp.mask[1])
    if n > 1:
        assert not torch.equal(inp.bias, inp.bias.transpose(1, 2))
    # the hand-written float64 backward is autograd's
    auto = _window_autograd(inp)
    for name, got in auto.items():
        assert torch.allclose(got, ref[name][0], rtol=1e-10, atol=1e-12), name
    # ideal fp32 kernel
    ideal = _window_autograd(inp, torch.float32)
    for name in ("out", "dq", "dk", "dv"):
        ideal[name] = _store(ideal[name], dtype)
    r = _ratios(ideal, ref)
    print("window ideal", case, dtype, {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r
    # mutants
    mutants = {}
    if nw is not None and nw > 1:
        mutants["mask of window (w + 1) % nW"] = dict(mask_shift=1)
    if n > 1:
        mutants["bias transposed"] = dict(bias_transposed=True)
        mutants["softmax backward without the row sum"] = dict(rowsum=False)
    if d > 1:
        mutants["dK without scale"] = dict(dk_scale=False)
    for name, kw in mutants.items():
        bad = ro.window_reference(inp, **kw)
        worst = max(ro.worst_ratio(bad[k][0], *ref[k]) for k in ref)
        assert worst >= SHARP, (name, worst)
    assert len(mutants) == 4 or case in ((5, 2, 49, 32, None),
                                         (2, 1, 64, 64, 1), (1, 1, 1, 1, 1))


# ---------------------------------------------------------------------------
# patch-merge LayerNorm
# ---------------------------------------------------------------------------

def _patch_autograd(inp, dt, one_pass_variance=False):
    h, w = inp.hw
    x = inp.x.to(dt).requires_grad_(True)
    gamma = inp.gamma.to(dt).requires_grad_(True)
    beta = inp.beta.to(dt).requires_grad_(True)
    xc = ro.patch_gather(x, h, w)
    if one_pass_variance:
        mean = xc.mean(-1, keepdim=True)
        var = (xc * xc).mean(-1, keepdim=True) - mean * mean
        y = (xc - mean) * (var.clamp_min(0) + ro.PATCH_EPS).rsqrt() * gamma \
            + beta
    else:
        y = F.layer_norm(xc, (xc.shape[-1],), gamma, beta, ro.PATCH_EPS)
    y.backward(inp.dy.to(dt))
    return {"y": y.detach(), "dx": x.grad, "dgamma": gamma.grad,
            "dbeta": beta.grad}


def _patch_check(case, dtype, offset):
    inp = ro.patch_inputs(case, dtype, offset=offset)
    ref = ro.patch_merge_reference(inp)               # asserts the dy grid
    auto = _patch_autograd(inp, torch.float64)
    for name, got in auto.items():
        assert torch.allclose(got, ref[name][0], rtol=1e-9, atol=1e-11), name
    ideal = _patch_autograd(inp, torch.float32)
    for name in ("y", "dx"):
        ideal[name] = _store(ideal[name], dtype)
    r = _ratios(ideal, ref)
    print("patch ideal", case, dtype, offset,
          {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r
    bad = ro.patch_merge_reference(inp, order=(0, 2, 1, 3))
    worst = max(ro.worst_ratio(bad[k][0], *ref[k]) for k in ("y", "dx"))
    assert worst >= SHARP, worst
    return inp, ref


@pytest.mark.parametrize("dtype", ro.PATCH_DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ro.PATCH_CASES, ids=_ids)
def test_patch_merge_cases(case, dtype):
    _patch_check(case, dtype, offset=False)


@pytest.mark.parametrize("dtype", ro.PATCH_DTYPES, ids=["f32", "bf16"])
def test_patch_merge_offset_case(dtype):
    """Rows of mean 16 and spread 1/4: fp32 F.layer_norm meets the bound of
    a variance taken from centred values; E[x^2] - mean^2 in fp32 does not
    (in fp32 I/O, where no bf16 store hides it)."""
    inp, ref = _patch_check(ro.PATCH_OFFSET_CASE, dtype, offset=True)
    xc = ro.patch_gather(inp.x.double(), *inp.hw)
    assert float((xc.mean(-1).abs() / xc.std(-1)).min()) > 40
    if dtype == torch.float32:
        one_pass = _patch_autograd(inp, torch.float32, one_pass_variance=True)
        r = _ratios(one_pass, ref)
        print("patch one-pass variance", {k: round(v, 2)
                                          for k, v in r.items()})
        assert r["y"] > 1.0 and r["dx"] > 1.0, r


# ---------------------------------------------------------------------------
# row losses
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ro.CE_DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ro.CE_CASES, ids=_ids)
def test_ce_cases(case, dtype):
    b, c = case
    for scale in ro.CE_SCALES:
        score, target = ro.ce_inputs(case, scale, dtype)
        assert int(target[0]) == c - 1 and (b < 2 or int(target[1]) == 0)
        for eps in ro.CE_EPSILONS:
            ref = ro.ce_reference(score, target, eps)
            s32 = score.float().clone().requires_grad_(True)
            loss = ref_ops.ce_label_smooth(s32, target, eps)
            loss.backward()
            r = _ratios({"loss": loss.detach(),
                         "grad": _store(s32.grad, dtype)}, ref)
            print("ce ideal", case, dtype, scale, eps, r)
            assert max(r.values()) <= 1.0, r
            if c > 1:
                bad = ro.ce_reference(score, target, eps, target_shift=1)
                worst = max(ro.worst_ratio(bad[k][0], *ref[k]) for k in ref)
                assert worst >= SHARP, worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ro.KD_CASES, ids=_ids)
def test_kd_cases(case, dtype):
    b, c = case
    zs, zt = ro.kd_inputs(case, dtype)
    for temp in ro.KD_TEMPERATURES:
        ref = ro.kd_reference(zs, zt, temp)
        s32 = zs.float().clone().requires_grad_(True)
        loss = ref_ops.kd_loss(s32, zt.float(), temp)
        loss.backward()
        r = _ratios({"loss": loss.detach(), "grad": _store(s32.grad, dtype)},
                    ref)
        print("kd ideal", case, dtype, temp, r)
        assert max(r.values()) <= 1.0, r
        same = ro.kd_reference(zs, zs, temp)
        assert float(same["loss"][0]) == 0 and not bool(same["grad"][0].any())
        if temp != 1.0 and c > 1:
            bad = ro.kd_reference(zs, zt, temp, grad_factor_t=False)
            assert ro.worst_ratio(bad["grad"][0], *ref["grad"]) >= SHARP


@pytest.mark.parametrize("case", ro.ICARL_CASES, ids=_ids)
def test_icarl_cases(case):
    b, c, p = case
    score, target, prev = ro.icarl_inputs(case)
    assert bool((target == c - 1).all())
    assert float(score.abs().max()) <= ro.ICARL_LIMIT
    if c >= 96:
        assert float(score.abs().max()) > 0.9 * ro.ICARL_LIMIT
    ref = ro.icarl_reference(score, target, prev)
    # the float64 formulas are autograd's
    s64 = score.double().requires_grad_(True)
    l64 = F.binary_cross_entropy_with_logits(
        s64, F.one_hot(target, c).double()) \
        + F.binary_cross_entropy_with_logits(
            s64[:, :p], torch.sigmoid(prev.double()))
    l64.backward()
    assert torch.allclose(l64.detach(), ref["loss"][0], rtol=1e-12)
    assert torch.allclose(s64.grad, ref["grad"][0], rtol=1e-10, atol=1e-30)
    s32 = score.clone().requires_grad_(True)
    loss = ref_ops.icarl_distill_loss(s32, target, prev)
    loss.backward()
    r = _ratios({"loss": loss.detach(), "grad": s32.grad}, ref)
    print("icarl ideal", case, r)
    assert max(r.values()) <= 1.0, r
    # mutant: the target one column early
    if c > 1:
        bad = ro.icarl_reference(score, (target - 1) % c, prev)
        assert ro.worst_ratio(bad["grad"][0], *ref["grad"]) >= SHARP
