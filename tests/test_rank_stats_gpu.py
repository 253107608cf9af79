"""rank_stats.hip against the sort chain: reference.cmc_map_from_sims applied
one query at a time to the same similarities on the CPU.  For a single query
its CMC is a step whose position is first_rank, and its mAP is the AP."""

import pytest
import torch

from flreid_amd import ops
from flreid_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

QL = torch.tensor([7, 2, 7, -1, 7])         # 5 rows: every row misalignment
QC = torch.tensor([0, 1, 1, 0, 1])
AP_TOL = 1e-12      # ≤ 4096 float64 terms in (0, 1], reordered: 4096·2⁻⁵²


def _gallery(g, group, seed):
    """`group` entries of id 7, the rest from {-1, 0, 1, 2, 3}, shuffled."""
    gen = torch.Generator().manual_seed(seed)
    gl = torch.cat([torch.full((group,), 7),
                    torch.randint(-1, 4, (g - group,), generator=gen)])
    return (gl[torch.randperm(g, generator=gen)],
            torch.randint(0, 2, (g,), generator=gen), gen)


def _sims(regime, q, g, gen):
    if regime == "random":
        return ops.similarity_matrix(
            ref.l2_normalize(torch.randn(q, 16, generator=gen)).cuda(),
            ref.l2_normalize(torch.randn(g, 16, generator=gen)).cuda())
    # integers in [-3, 3], zeros of both signs: exact ties everywhere
    return (torch.randint(-3, 4, (q, g), generator=gen)
            * (torch.randint(0, 2, (q, g), generator=gen) * 2 - 1).float()).cuda()


def _sort_reference(sims, ql, gl, qc, gc):
    first, n_good, ap = [], [], []
    for i in range(sims.shape[0]):
        cam = (qc[i:i + 1], gc) if qc is not None else (None, None)
        cmc, m = ref.cmc_map_from_sims(sims[i:i + 1], ql[i:i + 1], gl, *cam)
        step = cmc.nonzero()
        first.append(int(step[0]) if step.numel() else -1)
        good = gl == ql[i]
        if qc is not None:
            good &= (gc != qc[i]) & (gl != -1)
        n_good.append(int(good.sum()))
        ap.append(m)
    return (torch.tensor(first), torch.tensor(n_good),
            torch.tensor(ap, dtype=torch.float64))


def _check(sims, ql, gl, qc, gc):
    first, n_good, ap = ops.rank_stats_from_sims(sims, ql, gl, qc, gc)
    r_first, r_n_good, r_ap = _sort_reference(sims.cpu(), ql, gl, qc, gc)
    assert torch.equal(first.cpu(), r_first)
    assert torch.equal(n_good.cpu(), r_n_good)
    err = float((ap.cpu() - r_ap).abs().max())
    print(f"max |ap - ap_ref| = {err:.3e}")
    assert err <= AP_TOL


G_SIZES = [1, 3, 4, 5, 255, 257, 1027]      # float4 head / tail, misaligned rows
GROUPS = [0, 1, 2, 3, 33, 64, 65, None]     # bitonic padding; None: all of G


@pytest.mark.parametrize("regime", ["random", "ties"])
@pytest.mark.parametrize("cams", [False, True])
@pytest.mark.parametrize("g,group", [(g, g if k is None else k)
                                     for g in G_SIZES for k in GROUPS
                                     if k is None or k < g])
def test_matches_the_sort_chain(g, group, cams, regime):
    gl, gc, gen = _gallery(g, group, seed=g * 100 + group)
    assert ops.cmc_map_route(len(QL), g, group, True) == "kernel"
    _check(_sims(regime, len(QL), g, gen), QL, gl,
           QC if cams else None, gc if cams else None)


def test_rows_of_a_larger_tensor():
    gl, gc, gen = _gallery(1027, 33, seed=1)
    _check(_sims("ties", len(QL) + 1, 1027, gen)[1:], QL, gl, QC, gc)


def _cmc_map_check(qf, ql, gf, gl, qc, gc, route, **kw):
    top = max(int((gl == label).sum()) for label in ql.unique())
    assert ops.cmc_map_route(len(ql), len(gl), top, True) == route
    cmc, m = ops.cmc_map(qf.cuda(), ql, gf.cuda(), gl, qc, gc, **kw)
    sims = ops.similarity_matrix(qf.cuda(), gf.cuda())
    r_cmc, r_m = ref.cmc_map_from_sims(sims.cpu(), ql, gl, qc, gc)
    assert torch.equal(cmc, r_cmc)
    assert abs(m - r_m) <= AP_TOL
    return sims


def test_cmc_map_chunks_not_dividing_q():
    """37 queries in chunks of 8; one-hot gallery features make the
    similarities small integers, so ties cross the chunked path too."""
    gl, gc, gen = _gallery(257, 33, seed=2)
    ql = torch.tensor([7, 2, -1, 0, 9])[torch.randint(0, 5, (37,), generator=gen)]
    qc = torch.randint(0, 2, (37,), generator=gen)
    qf = torch.randint(-3, 4, (37, 8), generator=gen).float()
    gf = torch.eye(8)[torch.randint(0, 8, (257,), generator=gen)]
    _cmc_map_check(qf, ql, gf, gl, qc, gc, "kernel", query_chunk=8)


@pytest.mark.parametrize("over", [0, 1])
def test_group_at_the_cap_and_above(over):
    """At the cap the kernel serves the group (a row of 3·8192 + 5 columns is
    also split over workgroups); one entry more takes the torch route."""
    group = ops.rank_stats_max_good() + over
    gl, _gc, gen = _gallery(3 * 8192 + 5, group, seed=3)
    ql = torch.tensor([7, 9])               # 9: a query without a match
    qf = ref.l2_normalize(torch.randn(2, 16, generator=gen))
    gf = ref.l2_normalize(torch.randn(len(gl), 16, generator=gen))
    sims = _cmc_map_check(qf, ql, gf, gl, None, None,
                          "torch" if over else "kernel")
    _check(sims, ql, gl, None, None)
