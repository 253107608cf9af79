"""Which path serves which triplet mode: ops.triplet_loss_route."""

import itertools

import pytest

from flreid_amd import ops

MODES = list(itertools.product((False, True), (True, False), (0.3, None)))


@pytest.mark.parametrize("norm_feat,hard_mining,margin", MODES)
def test_route_over_the_mode_matrix(monkeypatch, norm_feat, hard_mining,
                                    margin):
    monkeypatch.delenv("FLREID_TRIPLET", raising=False)
    mode = (norm_feat, hard_mining, margin)
    served = "hard" if mode == (False, True, 0.3) else "gram"
    assert ops.triplet_loss_route(64, 2048, *mode, True) == served
    assert ops.triplet_loss_route(512, 8, *mode, True) == served
    # triplet.hip has no row limit; the Gram form stops at 512
    assert ops.triplet_loss_route(513, 8, *mode, True) == (
        "hard" if served == "hard" else "eager")
    assert ops.triplet_loss_route(64, 2048, *mode, False) == "eager"
    monkeypatch.setenv("FLREID_TRIPLET", "eager")
    assert ops.triplet_loss_route(64, 2048, *mode, True) == "eager"
