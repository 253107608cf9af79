"""The Gram-form triplet loss (triplet_gram.hip) against reference.triplet_loss
in float64 on the CPU: loss and feature.grad under a non-unit upstream factor,
the seven modes x shapes x label patterns, each run twice for equal bits.

Shapes, by the boundary of the design they cross (slices = K slices of the
Gram phase, kc = columns of D per slice):
  3 x 5       below one MFMA tile, one partial K panel, scalar loads (D % 4)
  33 x 65     one past a 32 edge; 3 slices of 32, the last holds one column
  65 x 1100   one past a 64 edge, 3 Gram tiles; 32 slices of 64: slice 17 is
              partial, slices 18..31 are empty (slabs of zeros)
  130 x 66    off-diagonal tiles and mirroring, 3 lanes' column groups, scalar
  512 x 8     the largest batch: 36 tiles, one slice, 8 columns per lane
  64 x 2048   the flagship: one tile, 32 full slices, 16-byte loads

Tolerance.  BASE[mode] = the largest error, over these same cases of the mode
on the CPU, of the fp32 eager reference.triplet_loss against the float64 one,
(loss, gradient), each normalised by the largest float64 magnitude of the
tensor.  The kernel gets 4 x base (loss 5.6e-7 .. 3.1e-6, gradient 1.6e-6 ..
3.6e-5): it sums in another order (MFMA tiles and K slices, not BLAS) but
rounds no more than fp32 does.  In the batch-hard modes each row's hardest
positive and negative lead their runner-up by 100 x that bound.
"""

import functools

import pytest
import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

# (norm_feat, hard_mining, margin) -> measured base (loss, gradient): all the
# modes but (False, True, 0.3), which is triplet.hip's
BASE = {
    (False, True, None): (4.29e-07, 4.16e-07),
    (False, False, 0.3): (7.85e-07, 1.71e-06),
    (False, False, None): (2.48e-07, 1.81e-06),
    (True, True, 0.3): (3.09e-07, 3.92e-07),
    (True, True, None): (1.40e-07, 4.07e-07),
    (True, False, 0.3): (4.71e-07, 1.30e-06),
    (True, False, None): (1.54e-07, 8.96e-06),
}
MODES = list(BASE)
UPSTREAM = 1.7
# A hinge argument this close to 0 (in units of the distances) could fall on
# either side of the kink in fp32: 100 x the rounding of a distance of O(10)
KINK = 1e-4

SHAPES = [(3, 5), (33, 65), (65, 1100), (130, 66), (512, 8), (64, 2048)]
PATTERNS = ["pk", "one_class", "distinct", "singleton"]
# seeds under which the input conditions below hold (0 where not listed)
SEEDS = {(33, 65, "pk"): 1, (33, 65, "distinct"): 1, (33, 65, "singleton"): 1,
         (65, 1100, "one_class"): 1, (65, 1100, "distinct"): 2,
         (130, 66, "pk"): 1, (130, 66, "singleton"): 1, (512, 8, "pk"): 36,
         (512, 8, "one_class"): 8, (512, 8, "distinct"): 28,
         (512, 8, "singleton"): 36, (64, 2048, "pk"): 11,
         (64, 2048, "one_class"): 8, (64, 2048, "distinct"): 3,
         (64, 2048, "singleton"): 11}


@functools.lru_cache(maxsize=None)
def _inputs(n, d, pattern, scale=1.0):
    """float64 features with squared distances of about 4·scale², labels."""
    gen = torch.Generator().manual_seed(SEEDS.get((n, d, pattern), 0))
    feat = torch.randn(n, d, generator=gen, dtype=torch.float64)
    feat = feat * (scale * (2.0 / d) ** 0.5)
    labels = torch.arange(n) // (4 if n >= 8 else 2)       # P x K groups
    if pattern == "one_class":
        labels = torch.zeros(n, dtype=torch.int64)
    elif pattern == "distinct":
        labels = torch.arange(n)
    elif pattern == "singleton":
        labels[-1] = n
    return feat, labels[torch.randperm(n, generator=gen)]


def _top2_gap(values, mask, largest):
    """The least lead of a row's best unmasked entry over its runner-up; rows
    with fewer than two candidates have nothing to confuse."""
    if values.shape[1] < 2:
        return float("inf")
    fill = float("-inf") if largest else float("inf")
    top = values.masked_fill(~mask, fill).topk(2, dim=1, largest=largest)[0]
    gap = (top[:, 0] - top[:, 1]).abs()
    gap = gap[~gap.isnan()]
    return float(gap.min()) if gap.numel() else float("inf")


def _check_inputs(feat, labels, norm_feat, hard_mining, margin, scale,
                  expect_overflow):
    """The conditions on the inputs, on float64 alone."""
    gap = 100 * 4 * max(BASE[norm_feat, hard_mining, margin])
    dist = (ref.pairwise_cosine_distance(feat, feat) if norm_feat
            else ref.pairwise_sqeuclidean(feat, feat))
    n = feat.shape[0]
    unit = 1.0 if norm_feat else scale * scale
    assert float(feat.norm(dim=1).min()) > 0.1 * scale      # no zero rows
    if n > 1:
        off = dist[~torch.eye(n, dtype=torch.bool)]
        assert 0.5 * unit < float(off.mean()) < 10 * unit
    is_pos = labels.view(n, 1).eq(labels.view(1, n)).to(dist.dtype)
    if hard_mining:
        ap_row, an_row = dist * is_pos, dist * (1 - is_pos) + 1e9 * is_pos
        assert _top2_gap(dist, is_pos > 0, True) >= gap * unit
        assert _top2_gap(dist, is_pos == 0, False) >= gap * unit
        ap, an = ap_row.max(1)[0], an_row.min(1)[0]
    else:
        w_ap = ref._softmax_weights(dist * is_pos, is_pos)
        w_an = ref._softmax_weights(-dist * (1 - is_pos), 1 - is_pos)
        ap = (dist * is_pos * w_ap).sum(1)
        an = (dist * (1 - is_pos) * w_an).sum(1)
    if margin is not None or expect_overflow:
        # no row sits on the hinge's kink
        hinge = (margin or 0.3) + ap - an
        assert float(hinge.abs().min()) >= KINK * unit
    if margin is None:
        if expect_overflow:
            assert float((an - ap).min()) < -800
        else:
            assert float((an - ap).min()) > -80


def _run_case(n, d, pattern, norm_feat, hard_mining, margin, scale=1.0,
              expect_overflow=False):
    assert ops.triplet_loss_route(n, d, norm_feat, hard_mining, margin,
                                  True) == "gram"
    feat, labels = _inputs(n, d, pattern, scale)
    _check_inputs(feat, labels, norm_feat, hard_mining, margin, scale,
                  expect_overflow)

    f64 = feat.clone().requires_grad_(True)
    want = ref.triplet_loss(f64, labels, margin, norm_feat, hard_mining)
    (want * UPSTREAM).backward()
    want = want.detach()
    if expect_overflow:   # the reference took its fallback, the 0.3 hinge
        hinge = ref.triplet_loss(feat, labels, 0.3, norm_feat, hard_mining)
        assert float(want) == float(hinge)

    runs = []
    for _ in range(2):
        f = feat.float().cuda().requires_grad_(True)
        loss = ops.triplet_loss(f, labels.cuda(), margin, norm_feat,
                                hard_mining)
        (loss * UPSTREAM).backward()
        runs.append((loss.detach().cpu(), f.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])

    loss, grad = runs[0]
    # a reference that is zero throughout is to be met to the bound itself
    err_loss = abs(float(loss) - float(want)) / (abs(float(want)) or 1.0)
    err_grad = (float((grad.double() - f64.grad).abs().max())
                / (float(f64.grad.abs().max()) or 1.0))
    base_loss, base_grad = BASE[norm_feat, hard_mining, margin]
    print(f"err_loss {err_loss:.3e} / {4 * base_loss:.3e} "
          f"err_grad {err_grad:.3e} / {4 * base_grad:.3e}")
    assert err_loss <= 4 * base_loss
    assert err_grad <= 4 * base_grad


# one added case, scaled so that a row has an - ap < -800: fp32 and float64
# both overflow, and the 0.3 hinge's loss and gradient must come back
CASES = [(*mode, *shape, pattern, 1.0) for mode in MODES for shape in SHAPES
         for pattern in PATTERNS] + [(False, True, None, 33, 65, "pk", 30.0)]


@pytest.mark.parametrize("norm_feat,hard_mining,margin,n,d,pattern,scale",
                         CASES)
def test_gram_route_matches_float64(norm_feat, hard_mining, margin, n, d,
                                    pattern, scale):
    _run_case(n, d, pattern, norm_feat, hard_mining, margin, scale,
              expect_overflow=scale > 1.0)
