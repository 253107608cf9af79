"""GPU numerics + dispatch for the fused multi-tensor quadratic penalty
(ops/csrc/penalty.hip) behind ops.quadratic_penalty_sets.

Truth is the float64 CPU evaluation of Σ_s Σ_n F_s·(p − a_s)² on the fp32
inputs.  Shapes are the smallest that reach every branch of the kernel and
of the wrapper's flat-buffer packing (see SHAPES)."""

import math

import pytest
import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
G = 0.37                # upstream gradient: (G * loss).backward()

# in table order
SHAPES = [
    ("t0", (7,), False),            # tail only; pads the next flat offset
    ("t1", (65536 + 5,), False),    # second chunk is a 5-element tail
    ("t2", (6, 4, 3, 3), True),     # channels-last p, a and F
    ("t3", (2048,), False),         # exact quads
    ("t4", (33, 65), False),        # odd 2-D
]
N_SETS = 5   # set 1 has importance=None, set 2 lacks "t4"; S = 5 takes the
             # kernel's runtime-S instantiation (S ≤ 4 are compile-time)


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension must be built in-tree"


def _mk(shape, cl, fn, gen):
    t = fn(shape, generator=gen, device="cuda")
    return t.contiguous(memory_format=torch.channels_last) if cl else t


@pytest.fixture(scope="module")
def data():
    gen = torch.Generator(device="cuda").manual_seed(1234)
    params = {n: _mk(s, cl, torch.randn, gen) for n, s, cl in SHAPES}
    sets = []
    for k in range(N_SETS):
        names = [(n, s, cl) for n, s, cl in SHAPES
                 if not (k == 2 and n == "t4")]
        anchors = {n: _mk(s, cl, torch.randn, gen) for n, s, cl in names}
        imp = (None if k == 1 else
               {n: _mk(s, cl, torch.rand, gen) for n, s, cl in names})
        sets.append((anchors, imp))
    return params, sets


def _leaves(params):
    # clone() keeps the channels-last strides
    return {n: p.detach().clone().requires_grad_(True)
            for n, p in params.items()}


def _truth(params, sets):
    """float64: loss, per-name gradient of G·loss, per-name Σ_s|2·G·F_s·d_s|."""
    loss = torch.zeros((), dtype=torch.float64)
    grads, mags = {}, {}
    for n, p in params.items():
        p64 = p.detach().double().cpu()
        gr, mg = torch.zeros_like(p64), torch.zeros_like(p64)
        for anchors, imp in sets:
            if n not in anchors:
                continue
            d = p64 - anchors[n].double().cpu()
            f = imp[n].double().cpu() if imp is not None \
                else torch.ones_like(d)
            loss = loss + (f * d * d).sum()
            t = 2.0 * G * f * d
            gr += t
            mg += t.abs()
        grads[n], mags[n] = gr, mg
    return loss, grads, mags


def _chain_length(params, sets):
    """Longest serial fp32 add chain of the fused value, from the kernel's
    constants: a thread's elements in one chunk × S, the block reduction's
    depth, and the final sum over the per-chunk partials."""
    ext = ops._load_extension()
    chunk, block = ext.penalty_chunk(), ext.penalty_block()
    n_chunks, per_thread = 0, 0
    for n, p in params.items():
        if not any(n in a for a, _ in sets):
            continue
        left = p.numel()
        while left > 0:
            ln = min(chunk, left)
            quads = ln // 4
            per_thread = max(per_thread,
                             4 * -(-quads // block) + (1 if ln % 4 else 0))
            n_chunks += 1
            left -= ln
    depth = int(math.log2(64)) + int(math.log2(block // 64))
    return per_thread * len(sets) + depth + n_chunks


def _case(data, kind):
    params, sets = data
    if kind == "prox":
        return params, [(sets[0][0], None)]
    return params, sets[:kind]


def _is_fused(loss):
    return type(loss.grad_fn).__name__.startswith("_QuadraticPenaltyHipFn")


@pytest.mark.parametrize("kind", [1, 3, 5, "prox"])
def test_loss_within_fp32_sum_bound(data, kind):
    params, sets = _case(data, kind)
    want, _, _ = _truth(params, sets)
    n = _chain_length(params, sets)
    fused = ops.quadratic_penalty_sets(_leaves(params), sets)
    eager = ref.quadratic_penalty_sets(params, sets)
    assert _is_fused(fused)
    err_f = abs(fused.double().item() - want.item())
    err_e = abs(eager.double().item() - want.item())
    bound = n * U * want.item()
    print(f"S={kind} n={n} f64={want.item():.9e} fused_err={err_f:.3e} "
          f"eager_err={err_e:.3e} bound={bound:.3e}")
    assert err_f <= bound
    assert err_e <= bound        # the bound is one the fp32 reference meets


@pytest.mark.parametrize("kind", [1, 3, 5, "prox"])
def test_gradient_elementwise_bound_and_layout(data, kind):
    params, sets = _case(data, kind)
    _, g64, mag = _truth(params, sets)
    S = len(sets)
    leaves = _leaves(params)
    loss = ops.quadratic_penalty_sets(leaves, sets)
    assert _is_fused(loss)
    (G * loss).backward()
    for n, p in leaves.items():
        assert p.grad is not None, n
        assert p.grad.shape == p.shape and p.grad.stride() == p.stride(), n
        err = (p.grad.double().cpu() - g64[n]).abs()
        bound = (S + 4) * U * mag[n]
        worst = (err - bound).max().item()
        print(f"S={kind} {n}: max err {err.max().item():.3e}, "
              f"max (err - bound) {worst:.3e}")
        assert bool((err <= bound).all()), n
    # the backward rounds as the eager chain does — fl(fl(g·F_s)·2d_s), sets
    # summed last to first as autograd's engine does — so the bits agree, for
    # unit importance (FedProx) and every S alike
    eager_leaves = _leaves(params)
    (G * ref.quadratic_penalty_sets(eager_leaves, sets)).backward()
    for n in leaves:
        assert torch.equal(leaves[n].grad, eager_leaves[n].grad), n


def test_deterministic_and_bounded_table_cache(data):
    params, sets = _case(data, 3)
    want, g64, mag = _truth(params, sets)
    n = _chain_length(params, sets)

    def run(sets_):
        leaves = _leaves(params)
        loss = ops.quadratic_penalty_sets(leaves, sets_)
        assert _is_fused(loss)
        (G * loss).backward()
        return loss.detach(), {k: p.grad for k, p in leaves.items()}

    l1, g1 = run(sets)
    l2, g2 = run(sets)
    assert torch.equal(l1, l2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k

    # fresh anchors (new pointers, same values), more often than the LRU holds
    keep = []
    for _ in range(ops._PENALTY_META_CAP + 3):
        fresh = [({k: a.clone() for k, a in anchors.items()}, imp)
                 for anchors, imp in sets]
        keep.append(fresh)
        lf, gf = run(fresh)
        assert torch.equal(lf, l1)
        for k in g1:
            assert torch.equal(gf[k], g1[k]), k
    assert len(ops._PENALTY_META) == ops._PENALTY_META_CAP
    assert abs(l1.double().item() - want.item()) <= n * U * want.item()
    for k in g1:
        assert bool(((g1[k].double().cpu() - g64[k]).abs()
                     <= (len(sets) + 4) * U * mag[k]).all()), k


def test_no_grad_returns_the_same_bits(data):
    params, sets = _case(data, 3)
    with_grad = ops.quadratic_penalty_sets(_leaves(params), sets)
    with torch.no_grad():
        without = ops.quadratic_penalty_sets(_leaves(params), sets)
    frozen = ops.quadratic_penalty_sets(params, sets)   # nothing requires grad
    assert without.grad_fn is None and not frozen.requires_grad
    assert torch.equal(with_grad.detach(), without)
    assert torch.equal(with_grad.detach(), frozen)


def _assert_reference_path(make, sets):
    """make() -> (params, leaves).  Value and gradient equal the eager
    reference's bits, and the fused Function is not what produced them."""
    params, leaves = make()
    got = ops.quadratic_penalty_sets(params, sets)
    assert not _is_fused(got)
    (G * got).backward()
    params_r, leaves_r = make()
    want = ref.quadratic_penalty_sets(params_r, sets)
    (G * want).backward()
    assert torch.equal(got.detach(), want.detach())
    for n in leaves:
        assert torch.equal(leaves[n].grad, leaves_r[n].grad), n


def _plain(params):
    def make():
        leaves = _leaves(params)
        return leaves, leaves
    return make


def test_fallback_bf16_importance(data):
    params, sets = _case(data, 1)
    anchors, imp = sets[0]
    imp = dict(imp, t3=imp["t3"].bfloat16())
    _assert_reference_path(_plain(params), [(anchors, imp)])


def test_fallback_misaligned_param_view(data):
    params, sets = _case(data, 1)
    anchors, imp = sets[0]
    base0 = torch.randn(2049, device="cuda")

    def make():
        base = base0.clone().requires_grad_(True)
        view = base[1:]
        assert view.data_ptr() % 16 != 0
        return {"t3": view}, {"t3": base}

    _assert_reference_path(make, [(anchors, imp)])


def test_fallback_mixed_layouts(data):
    params, sets = _case(data, 1)
    anchors, imp = sets[0]
    anchors = dict(anchors, t2=anchors["t2"].contiguous())
    assert anchors["t2"].stride() != params["t2"].stride()
    _assert_reference_path(_plain(params), [(anchors, imp)])


def test_fallback_env_switch(data, monkeypatch):
    params, sets = _case(data, 3)
    monkeypatch.setenv("FLREID_NO_FUSED_PENALTY", "1")
    _assert_reference_path(_plain(params), sets)


def test_dispatch_takes_the_fused_function(data):
    ext = ops._load_extension()
    assert hasattr(ext, "penalty_fwd") and hasattr(ext, "penalty_bwd")
    params, sets = _case(data, 1)
    leaves = _leaves(params)
    for loss in (ops.quadratic_penalty_sets(leaves, sets),
                 ops.quadratic_penalty(leaves, sets[0][0], sets[0][1]),
                 ops.quadratic_penalty(leaves, sets[0][0])):
        assert isinstance(loss.grad_fn,
                          ops._QuadraticPenaltyHipFn._backward_cls)
