"""CPU side of the sort-free CMC / mAP statistics: the route function and the
per-query torch version against the sort chain on exact ties."""

import pytest
import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref


def test_route_conditions(monkeypatch):
    cap = ops.rank_stats_max_good()
    assert ops.cmc_map_route(128, 256, 4, True) == "kernel"
    assert ops.cmc_map_route(128, 256, cap, True) == "kernel"
    assert ops.cmc_map_route(128, 256, 4, False) == "torch"
    assert ops.cmc_map_route(128, 256, cap + 1, True) == "torch"
    monkeypatch.setenv("FLREID_CMC", "torch")
    assert ops.cmc_map_route(128, 256, 4, True) == "torch"


@pytest.mark.parametrize("cams", [False, True])
def test_cpu_version_matches_the_sort_chain_on_ties(cams):
    gen = torch.Generator().manual_seed(11)
    q, g = 9, 61
    sims = torch.randint(-3, 4, (q, g), generator=gen).float()
    ql = torch.randint(-1, 4, (q,), generator=gen)
    ql[0] = 9                                   # no match in the gallery
    gl = torch.randint(-1, 4, (g,), generator=gen)
    qc = torch.randint(0, 2, (q,), generator=gen) if cams else None
    gc = torch.randint(0, 2, (g,), generator=gen) if cams else None
    first, n_good, ap = ops.rank_stats_from_sims(sims, ql, gl, qc, gc)
    for i in range(q):
        cam = (qc[i:i + 1], gc) if cams else (None, None)
        cmc, m = ref.cmc_map_from_sims(sims[i:i + 1], ql[i:i + 1], gl, *cam)
        step = cmc.nonzero()
        assert int(first[i]) == (int(step[0]) if step.numel() else -1)
        assert (int(n_good[i]) > 0) == bool(step.numel())
        assert abs(float(ap[i]) - m) <= 1e-12
