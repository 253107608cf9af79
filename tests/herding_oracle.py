"""Float64 greedy-optimality criterion for herding picks, shared by
test_herding.py and test_herding_gpu.py.

For identity p with rows F (float64) and picks j_0..j_{m-1}, step i has
acc_i = Σ_{t<i} F[j_t] and score_i(j) = ‖(i+1)μ − acc_i − F[j]‖².  A pick is
as good as the best one when

    score_i(j_i) − min_j score_i(j) ≤ tol · S_i,
    S_i = max_j‖F_j‖² + 2(i+1)·max_j|⟨F_j, μ⟩| + 2·max_j|⟨F_j, acc_i⟩|

which holds across exact ties (n = 2 ties at step 0; duplicated rows tie at
every step), so the criterion is optimality along the picks, not index
equality.  TOL = 1e-5: an fp32 numpy Gram form never picked differently from
float64 where the float64 gap between best and second best exceeded 1e-5·S
(normal and ReLU-shifted rows, n in 1..257, D in 32..2048, m = 32, 200 draws
per setting).
"""

import torch

TOL = 1e-5


def make_groups(sizes, d, seed):
    """(feats [N, d] fp32, pids [N] int64) on the CPU: one identity per entry
    of `sizes`, ids non-consecutive, rows shuffled.  Even identities are
    standard normal, odd ones ReLU-shifted (non-negative, many zeros)."""
    g = torch.Generator().manual_seed(seed)
    feats, pids = [], []
    for k, n in enumerate(sizes):
        f = torch.randn(n, d, generator=g)
        feats.append(f if k % 2 == 0 else torch.relu(f + 0.5))
        pids.append(torch.full((n,), 7 + 3 * k, dtype=torch.long))
    perm = torch.randperm(sum(sizes), generator=g)
    return torch.cat(feats)[perm].contiguous(), torch.cat(pids)[perm]


def worst_excess(feats, pids, persons, chosen):
    """max over identities and steps of (score_i(j_i) − min_j score_i(j)) / S_i
    in float64; asserts that every pick is a row of its identity."""
    f_all = feats.detach().double().cpu()
    assert persons == sorted(set(pids.tolist()))
    worst = 0.0
    for p, picks in zip(persons, chosen.tolist()):
        rows = (pids == p).nonzero().view(-1).tolist()
        assert set(picks) <= set(rows), f"identity {p}: foreign row picked"
        f = f_all[rows]
        mu = f.mean(dim=0)
        fixed = (f * f).sum(dim=1).max()
        fmu = (f @ mu).abs().max()
        acc = torch.zeros_like(mu)
        for i, j in enumerate(picks):
            score = (((i + 1) * mu - acc).unsqueeze(0) - f).pow(2).sum(dim=1)
            s_i = fixed + 2 * (i + 1) * fmu + 2 * (f @ acc).abs().max()
            excess = (score[rows.index(j)] - score.min()) / s_i
            worst = max(worst, float(excess))
            acc = acc + f_all[j]
    return worst
