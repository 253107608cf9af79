"""Herding kernel (herding.hip) against the float64 greedy-optimality
criterion of herding_oracle.py: mixed identity sizes in one call, shuffled
rows, both Gram paths, exact ties and the routes."""

import pytest
import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref

from herding_oracle import TOL, make_groups, worst_excess

pytestmark = pytest.mark.gpu

LDS_SIZES = [1, 2, 3, 8, 63, 64, 65, 128]     # every tile count, tile tails
WS_SIZES = [129, 300, 5, 1024]                # workspace Gram + one LDS one


def _kernel_picks(feats, pids, m):
    assert ops.extension_available()
    counts_max = int(torch.unique(pids, return_counts=True)[1].max())
    assert ops.herding_route(counts_max, feats.shape[1], feats.dtype,
                             True) == "kernel"
    persons, chosen = ops.herding_select(feats.cuda(), pids, m)
    assert chosen.shape == (len(persons), m) and chosen.dtype == torch.int64
    return persons, chosen


@pytest.mark.parametrize("sizes,d,m", [
    (LDS_SIZES, 36, 1), (LDS_SIZES, 36, 32),
    (LDS_SIZES, 2048, 1), (LDS_SIZES, 2048, 32),
    (WS_SIZES, 32, 32),
])
def test_picks_are_float64_optimal(sizes, d, m):
    feats, pids = make_groups(sizes, d, seed=d + m)
    persons, chosen = _kernel_picks(feats, pids, m)
    excess = worst_excess(feats, pids, persons, chosen)
    print(f"sizes={sizes} d={d} m={m}: worst excess {excess:.3e}")
    assert excess <= TOL


def test_duplicated_rows_tie_to_the_lowest_position():
    """Rows 3-5 copy rows 0-2: every step is an exact tie between a row and
    its copy, which the kernel resolves to the lower position."""
    base = torch.randn(3, 36, generator=torch.Generator().manual_seed(5))
    feats = torch.cat([base, base])
    pids = torch.full((6,), 4, dtype=torch.long)
    persons, chosen = _kernel_picks(feats, pids, 32)
    assert persons == [4] and int(chosen.max()) < 3
    assert worst_excess(feats, pids, persons, chosen) <= TOL


@pytest.mark.parametrize("sizes,d", [([5, 9], 34), ([1025, 3], 32)])
def test_out_of_range_calls_take_the_torch_route(sizes, d):
    feats, pids = make_groups(sizes, d, seed=1)
    assert ops.herding_route(max(sizes), d, feats.dtype, True) == "torch"
    feats = feats.cuda()
    persons, chosen = ops.herding_select(feats, pids, 4)
    ref_persons, ref_chosen = ref.herding_select(feats, pids, 4)
    assert persons == ref_persons and torch.equal(chosen, ref_chosen)
