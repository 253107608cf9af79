"""ops.quadratic_penalty_sets — the multi-set quadratic penalty of
EWC / MAS / FedCurv / FedProx — on the CPU dispatch (the eager reference):
it is Σ_s ref.quadratic_penalty, ops.quadratic_penalty is its one-set form,
and FedCurv's Model.penalty() goes through it with unchanged maths."""

import pytest
import torch
import torch.nn as nn

from flreid_amd import ops
from flreid_amd.ops import reference as ref

SHAPES = {"a": (7,), "b": (3, 5), "c": (2, 3, 2, 2)}


def _inputs(n_sets, seed=0):
    """params + n_sets (anchors, importance) sets; the LAST set lacks name
    'b', and set 0 has importance=None whenever there is more than one set
    (with one set, both forms are run by the test)."""
    g = torch.Generator().manual_seed(seed)
    params = {n: torch.randn(s, generator=g) for n, s in SHAPES.items()}
    sets = []
    for s in range(n_sets):
        names = [n for n in SHAPES if not (n == "b" and s == n_sets - 1
                                           and n_sets > 1)]
        anchors = {n: torch.randn(SHAPES[n], generator=g) for n in names}
        imp = {n: torch.rand(SHAPES[n], generator=g) for n in names}
        sets.append((anchors, None if (s == 0 and n_sets > 1) else imp))
    return params, sets


def _leaf(params):
    return {n: p.clone().requires_grad_(True) for n, p in params.items()}


@pytest.mark.parametrize("n_sets", [1, 2, 3])
def test_sets_equal_sum_of_single_penalties(n_sets):
    params, sets = _inputs(n_sets)
    p_new, p_old = _leaf(params), _leaf(params)

    got = ops.quadratic_penalty_sets(p_new, sets)
    want = None
    for anchors, imp in sets:
        s = ref.quadratic_penalty(p_old, anchors, imp)
        want = s if want is None else want + s
    assert torch.equal(got, want)
    assert torch.equal(ref.quadratic_penalty_sets(p_old, sets).detach(),
                       want.detach())

    (0.37 * got).backward()
    (0.37 * want).backward()
    for n in params:
        assert torch.equal(p_new[n].grad, p_old[n].grad), n


def test_single_set_without_importance_is_fedprox_term():
    params, sets = _inputs(1)
    anchors = sets[0][0]
    got = ops.quadratic_penalty_sets(params, [(anchors, None)])
    want = sum(((params[n] - anchors[n]) ** 2).sum() for n in params)
    assert torch.allclose(got, want, rtol=1e-6)


def test_quadratic_penalty_unchanged_on_test_ops_inputs():
    # the inputs of tests/test_ops.py::test_importance_update_and_penalty
    p = {"w": torch.tensor([1.0, 2.0])}
    anchors = {"w": torch.tensor([0.0, 0.0])}
    imp = {"w": torch.tensor([10.0, 5.0])}
    pen = ops.quadratic_penalty(p, anchors, imp)
    assert torch.equal(pen, ref.quadratic_penalty(p, anchors, imp))
    assert pen.item() == pytest.approx(10 * 1 + 5 * 4)
    prox = ops.quadratic_penalty(p, anchors)
    assert torch.equal(prox, ref.quadratic_penalty(p, anchors))
    assert prox.item() == pytest.approx(1 + 4)
    # keyword form of the signature
    assert torch.equal(
        ops.quadratic_penalty(params=p, anchors=anchors, importance=imp), pen)


def test_empty_sets_and_disjoint_names_give_zero_scalar():
    params, sets = _inputs(1)
    for out in (ops.quadratic_penalty_sets(params, []),
                ops.quadratic_penalty_sets(params, [({"zz": torch.ones(2)},
                                                     None)]),
                ops.quadratic_penalty(params, {})):
        assert out.shape == () and out.item() == 0.0
        assert out.device == params["a"].device


def test_fedcurv_penalty_equals_python_loop_formula():
    """Model.penalty() with two other clients == the per-set Python loop it
    replaced (ref:methods/fedcurv.py:79-86), value and gradient."""
    from flreid_amd.methods import methods
    torch.manual_seed(3)

    class Op:
        @staticmethod
        def _invoke_train(model, data, target):
            return {"loss": (model.net(data) ** 2).sum()}

    net = nn.Linear(5, 3)
    m = methods["fedcurv"].Model(net=net, operator=Op(), lambda_penalty=2.5)
    m.precision_matrices = {n: torch.rand_like(p) for n, p in m.params.items()}
    m.params_old = {n: p.detach() + 0.1 * torch.randn_like(p)
                    for n, p in m.params.items()}
    m.other_precision_matrices = [
        ({n: torch.rand_like(p) for n, p in m.params.items()},
         {n: p.detach() + torch.randn_like(p) for n, p in m.params.items()})
        for _ in range(2)]

    pen = m.penalty()
    pen.backward()
    got_grads = {n: p.grad.clone() for n, p in m.params.items()}
    net.zero_grad(set_to_none=True)

    own = ref.quadratic_penalty(m.params, m.params_old, m.precision_matrices)
    for importance, params in m.other_precision_matrices:
        own = own + ref.quadratic_penalty(m.params, params, importance)
    want = 2.5 * own
    want.backward()

    assert torch.equal(pen.detach(), want.detach())
    for n, p in m.params.items():
        assert torch.equal(got_grads[n], p.grad), n
