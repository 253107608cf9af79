"""One-pass FedSTIL head update (head_step.hip) on the GPU.

Kernel level: one launch over a table of linear / channels-last conv weights
against the unfused chain on the same GPU — bf16→fp32 cast, + λ·sign(aw−aw0),
torch's fused capturable Adam, compose2.  Step level: a tiny adaptive net
trained with FLREID_FUSED_HEAD_STEP / FLREID_LIVE_THETA on and off, eagerly
and through GraphedStep / EpochGraph.

aw, exp_avg, exp_avg_sq, θ and the step count are bit-equal to the unfused
chain (measured on MI355X: 0 unequal elements in every case).  The drift
VALUE is not comparable bit for bit — the kernel sums it in fp64, the
unfused paths in fp32 in their own orders — so both sides are measured
against head_step_reference (fp64) and the fused error must be ≤ 2× the
unfused one (measured: fused ≤ 0.5 fp32 ulp of the sum, i.e. the correctly
rounded value, in every case; unfused 0-2 ulps).
"""

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


# --------------------------------------------------------------------------
# kernel level
# --------------------------------------------------------------------------

# (shape, channels_last): L%4==0 float4-atten linear; odd-L scalar path;
# 1×1 and 3×3 (inner 4, L 3) channels-last convs; a scalar-path tensor over
# several 16 K chunks with a ragged tail; a float4 tensor over several chunks
TABLE = [((7, 12), False), ((3, 5), False), ((8, 4, 1, 1), True),
         ((8, 4, 3, 3), True), ((130, 1025), False), ((33, 1028), False)]


def _like(t, shape, cl):
    return t.contiguous(memory_format=torch.channels_last) if cl else t


def _make(shape, cl, gen, grad_dtype, nsteps=3):
    def rnd(scale):
        return _like(torch.randn(shape, generator=gen, device=DEV) * scale,
                     shape, cl)
    aw0 = rnd(0.05)
    delta = rnd(1e-3)
    # exact ties aw == aw0 on a third of the weights, both signs elsewhere
    delta[torch.rand(shape, generator=gen, device=DEV) < 1 / 3] = 0.0
    aw = aw0 + delta
    assert aw.stride() == aw0.stride()
    gw = rnd(0.05)
    atten = torch.rand(shape[-1], generator=gen, device=DEV)
    dws = [rnd(1e-2).to(grad_dtype) for _ in range(nsteps)]
    return {"aw": aw, "aw0": aw0, "gw": gw, "atten": atten, "dws": dws}


def _tensors(grad_dtype, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [_make(s, cl, gen, grad_dtype) for s, cl in TABLE]


def _err(got, want64):
    return float((got.double() - want64).abs().max())


def _check(name, fused, unfused, want64, report):
    """Bit-equal (reached on MI355X: no contraction difference between this
    kernel and torch's); the errors against fp64 are printed on a miss."""
    unequal = int((fused != unfused).sum())
    report.setdefault(name, [0, 0])
    report[name][0] += unequal
    report[name][1] += fused.numel()
    if unequal:
        print(f"{name}: {unequal}/{fused.numel()} unequal, fused err "
              f"{_err(fused, want64):.3e} unfused err "
              f"{_err(unfused, want64):.3e}")
    assert unequal == 0, name


@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16grad", "fp32grad"])
@pytest.mark.parametrize("lam,wd", [(0.0, 0.0), (1e-4, 1e-5), (1e-4, 0.0),
                                    (0.0, 1e-5)])
def test_kernel_matches_unfused_chain(grad_dtype, lam, wd):
    from flreid_amd import ops
    from flreid_amd.ops import reference as ref
    ext = ops.require_extension("head_step")
    data = _tensors(grad_dtype)
    lam32 = torch.tensor(lam, dtype=torch.float32, device=DEV)

    # unfused side: torch's fused capturable Adam on clones
    u_params = [nn.Parameter(d["aw"].clone()) for d in data]
    for p, d in zip(u_params, data):
        assert p.stride() == d["aw"].stride()
    opt = torch.optim.Adam(u_params, lr=LR, betas=(B1, B2), eps=EPS,
                           weight_decay=wd, fused=True, capturable=True)
    # fused side
    rows = []
    for d in data:
        aw = d["aw"].clone()
        rows.append({"aw": aw, "aw0": d["aw0"], "gw": d["gw"],
                     "atten": d["atten"],
                     "m": torch.zeros_like(aw), "v": torch.zeros_like(aw),
                     "step": torch.zeros((), device=DEV),
                     "theta": torch.empty_like(aw, dtype=torch.bfloat16)})
    partials = torch.zeros(ops.head_step_partials(rows), dtype=torch.float64,
                           device=DEV)
    # fp64 reference chain, fed the FUSED side's state each step
    report = {}
    for k in range(3):
        want = []
        for r, d in zip(rows, data):
            want.append(ref.head_step_reference(
                r["aw"], d["aw0"], d["dws"][k], r["m"], r["v"], k + 1, LR,
                B1, B2, wd, EPS, lam, d["gw"], d["atten"]))
        # unfused: cast -> add sign term -> Adam -> compose2, and the drift
        drift_u = ops.l1_drift([(p.detach(), d["aw0"])
                                for p, d in zip(u_params, data)])
        for p, d in zip(u_params, data):
            p.grad = d["dws"][k].to(torch.float32) \
                + torch.sign(p.detach() - d["aw0"]) * lam32
        opt.step()
        theta_u = [ops.compose_theta_bf16(ext, d["gw"], d["atten"],
                                          p.detach())
                   for p, d in zip(u_params, data)]
        # fused: one launch over the whole table
        for r, d in zip(rows, data):
            r["dw"] = d["dws"][k]
        ops.head_step(rows, partials, LR, B1, B2, wd, EPS, lam)
        torch.cuda.synchronize()

        for i, (r, p, w) in enumerate(zip(rows, u_params, want)):
            st = opt.state[p]
            a64, m64, v64, th64, _d64 = w
            assert float(r["step"]) == float(st["step"]) == k + 1
            _check(f"aw[{i}]", r["aw"], p.detach(), a64, report)
            _check(f"m[{i}]", r["m"], st["exp_avg"], m64, report)
            _check(f"v[{i}]", r["v"], st["exp_avg_sq"], v64, report)
            th_want = th64.to(torch.bfloat16)
            assert torch.equal(r["theta"], theta_u[i]), f"theta[{i}]"
            # within 1 bf16 ulp of the bf16 rounding of the reference
            ulp = th_want.float().abs().clamp_min(2.0 ** -126) * 2.0 ** -7
            assert bool(((r["theta"].float() - th_want.float()).abs()
                         <= ulp).all())
        drift64 = sum(float(w[4]) for w in want)
        drift_f = float(partials.sum().to(torch.float32))
        ef = abs(drift_f - drift64)
        eu = abs(float(drift_u) - drift64)
        print(f"step {k + 1}: drift fused {drift_f!r} unfused "
              f"{float(drift_u)!r} fp64 {drift64!r}")
        assert drift_f == float(drift_u) or ef <= 2 * eu, (ef, eu)
    print("compared elements:", sum(c[1] for c in report.values()),
          "unequal:", sum(c[0] for c in report.values()))


def _one_row(shape=(8, 4, 3, 3), cl=True):
    gen = torch.Generator(device=DEV).manual_seed(1)
    d = _make(shape, cl, gen, torch.float32, nsteps=1)
    aw = d["aw"].clone()
    row = {"aw": aw, "aw0": d["aw0"], "dw": d["dws"][0], "gw": d["gw"],
           "atten": d["atten"], "m": torch.zeros_like(aw),
           "v": torch.zeros_like(aw), "step": torch.zeros((), device=DEV),
           "theta": torch.empty_like(aw, dtype=torch.bfloat16)}
    return row, d


def _assert_untouched(row, d):
    torch.cuda.synchronize()
    assert torch.equal(row["aw"], d["aw"])
    assert float(row["step"]) == 0.0
    assert not row["m"].any() and not row["v"].any()


def test_validation_mismatched_strides_raises():
    from flreid_amd import ops
    row, d = _one_row()
    partials = torch.zeros(1, dtype=torch.float64, device=DEV)
    # a gradient in NCHW order for a channels-last weight (what a
    # conv2d_weight result may look like)
    row["dw"] = row["dw"].contiguous()
    assert row["dw"].stride() != row["aw"].stride()
    with pytest.raises(ValueError, match="layout"):
        ops.head_step([row], partials, LR, B1, B2, 0.0, EPS, 1e-4)
    _assert_untouched(row, d)


def test_validation_null_pointer_raises():
    from flreid_amd import ops
    ext = ops.require_extension("head_step")
    row, d = _one_row()
    partials = torch.zeros(1, dtype=torch.float64, device=DEV)
    row_missing = dict(row, m=None)
    with pytest.raises(ValueError, match="null"):
        ops.head_step([row_missing], partials, LR, B1, B2, 0.0, EPS, 1e-4)
    # the native entry refuses a null pointer as well, before any launch
    raw = ops._head_step_row(row, 0)
    raw[5] = 0
    with pytest.raises(RuntimeError, match="null pointer"):
        ext.head_step([raw], partials.data_ptr(), 1, LR, B1, B2, 0.0, EPS,
                      1e-4, torch.cuda.current_stream().cuda_stream)
    # ... and a float4 request for an unaligned row, and a partial range
    # outside the buffer
    raw = ops._head_step_row(row, 0)
    raw[0] += 4
    with pytest.raises(RuntimeError, match="unaligned"):
        ext.head_step([raw], partials.data_ptr(), 1, LR, B1, B2, 0.0, EPS,
                      1e-4, torch.cuda.current_stream().cuda_stream)
    raw = ops._head_step_row(row, 1)
    with pytest.raises(RuntimeError, match="out of bounds"):
        ext.head_step([raw], partials.data_ptr(), 1, LR, B1, B2, 0.0, EPS,
                      1e-4, torch.cuda.current_stream().cuda_stream)
    _assert_untouched(row, d)


def test_unaligned_row_takes_scalar_path():
    """A 4-byte-offset view: not float4-able, same results as the aligned
    launch (bit-equal — same per-element math on either path)."""
    from flreid_amd import ops
    shape = (9, 64)
    gen = torch.Generator(device=DEV).manual_seed(2)
    d = _make(shape, False, gen, torch.bfloat16, nsteps=1)
    n = d["aw"].numel()

    def rows_for(offset):
        def place(t):
            buf = torch.zeros(n + 8, dtype=t.dtype, device=DEV)
            view = buf[offset:offset + n].view(shape)
            view.copy_(t)
            return view
        aw = place(d["aw"])
        return {"aw": aw, "aw0": place(d["aw0"]), "dw": place(d["dws"][0]),
                "gw": place(d["gw"]), "atten": d["atten"],
                "m": place(torch.zeros(shape, device=DEV)),
                "v": place(torch.zeros(shape, device=DEV)),
                "step": torch.zeros((), device=DEV),
                "theta": place(torch.zeros(shape, dtype=torch.bfloat16,
                                           device=DEV))}
    aligned, shifted = rows_for(0), rows_for(1)
    assert ops._head_step_row(aligned, 0)[12] & ops._HS_VEC
    assert not ops._head_step_row(shifted, 0)[12] & ops._HS_VEC
    pa = torch.zeros(1, dtype=torch.float64, device=DEV)
    ps = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.head_step([aligned], pa, LR, B1, B2, 1e-5, EPS, 1e-4)
    ops.head_step([shifted], ps, LR, B1, B2, 1e-5, EPS, 1e-4)
    for k in ("aw", "m", "v", "theta"):
        assert torch.equal(aligned[k], shifted[k]), k
    assert abs(float(pa) - float(ps)) <= 1e-12 * abs(float(pa))


# --------------------------------------------------------------------------
# step level: a tiny adaptive net through the FedSTIL operator
# --------------------------------------------------------------------------

class _TinyNet(nn.Module):
    """1×1 conv → BN → 3×3 conv → BN → pool → linear, all one stage."""

    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(64, 64, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.c3 = nn.Conv2d(64, 64, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(64)
        self.fc = nn.Linear(64, 32, bias=False)

    def stage_of(self, name):
        return 0

    def run_stages(self, x, start=0, tap=None):
        h = torch.relu(self.bn1(self.c1(x)))
        h = torch.relu(self.bn3(self.c3(h)))
        feat = h.mean(dim=(2, 3))
        return (self.fc(feat), feat), None

    def forward(self, x):
        return self.run_stages(x)[0]


def _build(seed=5, channels_last=True):
    from flreid_amd import ops
    from flreid_amd.methods.fedstil import Model, Operator
    torch.manual_seed(seed)
    model = Model(_TinyNet(), lambda_l1=1e-4, lambda_k=8, atten_default=0.9)
    model.to(DEV)
    for p in model.net.parameters():
        if p.dim() == 4 and channels_last:
            p.data = p.data.to(memory_format=torch.channels_last)
    # start away from the anchor, with ties, so the sign term is live
    with torch.no_grad():
        for _n, leaf in model.adaptive_module_leaves():
            noise = torch.randn_like(leaf.adaptive_weight) * 1e-3
            noise[torch.rand_like(noise) < 1 / 3] = 0.0
            leaf.adaptive_weight.add_(noise)
    params = [p for p in model.net.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=LR, weight_decay=1e-5)
    crit = [lambda score, feature, target:
            ops.ce_label_smooth(score, target, 0.1)]
    op = Operator(optimizer=opt, criterion=crit)
    model.train()
    return model, op


def _batches(n, hw, seed=11):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn(8, 64, *hw, generator=gen, device=DEV) \
            .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        t = torch.randint(0, 32, (8,), generator=gen, device=DEV)
        out.append((x, t))
    return out


def _epoch(model, op):
    """The head-epoch scope of invoke_train around eager/graphed steps."""
    from flreid_amd.methods.fedstil import head_epoch
    return head_epoch(model, op)


def _snapshot(model, op):
    snap = {}
    for n, p in model.net.named_parameters():
        snap[f"p.{n}"] = p.detach().clone()
    for n, b in model.net.named_buffers():
        snap[f"b.{n}"] = b.detach().clone()
    for n, p in model.net.named_parameters():
        st = op.optimizer.state.get(p)
        if st:
            for k, v in st.items():
                snap[f"s.{n}.{k}"] = v.detach().clone()
    return snap


def _run_eager(model, op, batches, monkeypatch, switches):
    """switches: per-step (FUSED_HEAD_STEP, LIVE_THETA) env values; the
    epoch scope is re-entered whenever they change."""
    losses = []
    i = 0
    while i < len(batches):
        j = i
        while j < len(batches) and switches[j] == switches[i]:
            j += 1
        monkeypatch.setenv("FLREID_FUSED_HEAD_STEP", switches[i][0])
        monkeypatch.setenv("FLREID_LIVE_THETA", switches[i][1])
        with _epoch(model, op):
            for x, t in batches[i:j]:
                loss, _acc = op._train_step(model, x, t)
                losses.append(loss.clone())
        i = j
    torch.cuda.synchronize()
    return losses, _snapshot(model, op)


def _ulp(y: float) -> float:
    t = torch.tensor(abs(y), dtype=torch.float32)
    return float(torch.nextafter(t, t.new_tensor(float("inf"))) - t)


def _compare(a, b, what):
    """Weights, Adam state, BN parameters and buffers: bit-equal.  The
    step loss is fl32(task + fl32(λ·drift)) on both sides with a bit-equal
    task loss; the two drift values differ only by the fp32 summation error
    of the unfused path (the fused one sums in fp64), i.e. by < 1e-5
    relative on a term ~1e-3 of the loss — the two losses are fp32
    roundings of reals < 1e-8 apart, hence equal or adjacent: ≤ 1 ulp."""
    la, sa = a
    lb, sb = b
    assert sa.keys() == sb.keys(), (sa.keys() ^ sb.keys())
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, (what, bad[:6])
    unequal = sum(float(x) != float(y) for x, y in zip(la, lb))
    print(f"{what}: {unequal}/{len(la)} step losses not bit-equal")
    for x, y in zip(la, lb):
        assert abs(float(x) - float(y)) <= _ulp(float(y)), \
            (what, float(x), float(y))


MODES = {"off": ("0", "0"), "fused": ("1", "0"), "live": ("1", "1")}


@pytest.mark.parametrize("hw", [(4, 4), (4, 2)], ids=["4x4", "4x2"])
@pytest.mark.parametrize("mode", ["fused", "live"])
def test_three_steps_match_unfused(hw, mode, monkeypatch):
    batches = _batches(3, hw)
    m0, o0 = _build()
    m1, o1 = _build()
    off = _run_eager(m0, o0, batches, monkeypatch, [MODES["off"]] * 3)
    on = _run_eager(m1, o1, batches, monkeypatch, [MODES[mode]] * 3)
    _compare(on, off, mode)
    # torch's own state layout afterwards
    for _n, leaf in m1.adaptive_module_leaves():
        st = o1.optimizer.state[leaf.adaptive_weight]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == torch.float32 and st["step"].is_cuda
        assert float(st["step"]) == 3.0
        assert st["exp_avg"].stride() == leaf.adaptive_weight.stride()
        assert leaf.adaptive_weight.grad is None
        assert leaf._live is None          # nothing outlives the epoch


def test_three_steps_match_unfused_nchw_weights(monkeypatch):
    """NCHW-ordered conv weights (no channels-last conversion): the 3×3
    takes F.conv2d on θ, the 1×1 its GEMM route, atten indexes the
    physically-last dim."""
    batches = _batches(3, (4, 4))
    m0, o0 = _build(channels_last=False)
    m1, o1 = _build(channels_last=False)
    assert m1.net.c3.adaptive_weight.is_contiguous()
    off = _run_eager(m0, o0, batches, monkeypatch, [MODES["off"]] * 3)
    on = _run_eager(m1, o1, batches, monkeypatch, [MODES["live"]] * 3)
    _compare(on, off, "live-nchw")


@pytest.mark.parametrize("flip", [("live", "off"), ("off", "live"),
                                  ("fused", "off")])
def test_switch_flip_between_steps_continues(flip, monkeypatch):
    batches = _batches(3, (4, 4))
    m0, o0 = _build()
    m1, o1 = _build()
    off = _run_eager(m0, o0, batches, monkeypatch, [MODES["off"]] * 3)
    mixed = _run_eager(m1, o1, batches, monkeypatch,
                       [MODES[flip[0]]] * 2 + [MODES[flip[1]]])
    _compare(mixed, off, flip)


@pytest.mark.parametrize("mode", ["fused", "live"])
def test_graphed_step_equals_eager(mode, monkeypatch):
    from flreid_amd.runtime.hipgraph import GraphedStep
    monkeypatch.setenv("FLREID_FUSED_HEAD_STEP", MODES[mode][0])
    monkeypatch.setenv("FLREID_LIVE_THETA", MODES[mode][1])
    batches = _batches(5, (4, 4))
    m0, o0 = _build()
    eager = _run_eager(m0, o0, batches, monkeypatch, [MODES[mode]] * 5)

    m1, o1 = _build()
    losses = []
    with _epoch(m1, o1):
        assert o1._fused_head is not None
        gs = GraphedStep(lambda d, t: o1._train_step(m1, d, t))
        for i, (x, t) in enumerate(batches):
            if i < 2:
                out = gs.warmup(x, t)
            elif i == 2:
                out = gs.capture(x, t)
            else:
                out = gs(x, t)
            losses.append(out[0].clone())
    torch.cuda.synchronize()
    _compare((losses, _snapshot(m1, o1)), eager, f"graphed-{mode}")


@pytest.mark.parametrize("mode", ["fused", "live"])
def test_epoch_graph_equals_eager(mode, monkeypatch):
    from flreid_amd.runtime.hipgraph import EpochGraph
    monkeypatch.setenv("FLREID_FUSED_HEAD_STEP", MODES[mode][0])
    monkeypatch.setenv("FLREID_LIVE_THETA", MODES[mode][1])
    batches = _batches(3, (4, 4))
    store = torch.cat([x for x, _t in batches])
    pids = torch.cat([t for _x, t in batches])
    idx = torch.arange(24, device=DEV)
    m0, o0 = _build()
    # two epochs of the same three batches, eagerly
    eager = _run_eager(m0, o0, batches + batches, monkeypatch,
                       [MODES[mode]] * 6)

    m1, o1 = _build()
    eg = None
    sums = []
    for _epoch_no in range(2):         # warm-up epoch, then capture + replay
        with _epoch(m1, o1):
            if eg is None:
                eg = EpochGraph(lambda d, t: o1._train_step(m1, d, t), 3, 8,
                                store, pids, lambda rows: rows)
            loss, _acc = eg.run(store, pids, idx)
            sums.append(loss.clone())
    torch.cuda.synchronize()
    snap = _snapshot(m1, o1)
    assert eg.graph is not None
    bad = [k for k in snap if not torch.equal(snap[k], eager[1][k])]
    assert not bad, bad[:6]
    # Σ of three step losses, accumulated in fp32 in the same order on both
    # sides from bit-equal terms (same update path): bit-equal
    for e in range(2):
        want = None
        for x in eager[0][3 * e:3 * e + 3]:
            want = x.clone() if want is None else want + x
        assert float(sums[e]) == float(want), (float(sums[e]), float(want))


def test_live_theta_scope(monkeypatch):
    """θ lives for exactly one head epoch: after the scope exits, weights
    changed through update_model / init_training_weights are what an eval
    forward sees, and the next epoch starts from a freshly composed θ."""
    monkeypatch.setenv("FLREID_FUSED_HEAD_STEP", "1")
    monkeypatch.setenv("FLREID_LIVE_THETA", "1")
    from flreid_amd import ops
    ext = ops.require_extension("compose2")
    model, op = _build()
    (x, t), = _batches(1, (4, 4))
    with _epoch(model, op):
        leaves = [l for _n, l in model.adaptive_module_leaves()]
        assert all(l._live is not None for l in leaves)
        op._train_step(model, x, t)
        # the kernel kept θ current
        for l in leaves:
            want = ops.compose_theta_bf16(ext, l.global_weight,
                                          l.global_weight_atten,
                                          l.adaptive_weight)
            assert torch.equal(l._live.theta, want)
    assert all(l._live is None for l in leaves)

    # cleared on exceptions too
    with pytest.raises(RuntimeError, match="boom"):
        with _epoch(model, op):
            raise RuntimeError("boom")
    assert all(l._live is None for l in leaves)

    # change the weights behind the (dropped) θ, both ways
    state = model.model_state()
    new_aw = {k: v + 0.25 for k, v in state["adaptive_weights"].items()}
    model.update_model({"adaptive_weights": new_aw})
    leaves[0].init_training_weights()
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = model.net.c1(x)
    l = leaves[0]
    theta = ops.compose_theta_bf16(ext, l.global_weight,
                                   l.global_weight_atten, l.adaptive_weight)
    want = x.permute(0, 2, 3, 1).reshape(-1, 64) @ theta.view(64, 64).t()
    assert torch.equal(got.permute(0, 2, 3, 1).reshape(-1, 64), want)
    model.train()
    with _epoch(model, op):
        for l in leaves:
            want = ops.compose_theta_bf16(ext, l.global_weight,
                                          l.global_weight_atten,
                                          l.adaptive_weight)
            assert torch.equal(l._live.theta, want)


def test_ineligible_models_keep_the_old_path(monkeypatch):
    """Trainable atten (fedstil-atten style) or a switched-off flag: no
    plan, nothing attached."""
    from flreid_amd.methods.fedstil import head_epoch
    model, op = _build()
    monkeypatch.setenv("FLREID_FUSED_HEAD_STEP", "0")
    with head_epoch(model, op):
        assert op._fused_head is None
    monkeypatch.setenv("FLREID_FUSED_HEAD_STEP", "1")
    leaf = model.adaptive_module_leaves()[0][1]
    leaf.global_weight_atten.requires_grad = True
    with head_epoch(model, op):
        assert op._fused_head is None
        assert leaf._live is None
