"""The hand-written 3x3 s1p1 conv suite (FLREID_CONV_IMPL=hand) against the
float64 oracle of tests/conv_oracle.py, through the public route.

On grid inputs every fp32 partial sum is exact, so forward, dx and dW must
equal the float64 reference BIT FOR BIT (after the one bf16 store for out
and dx).  On full-mantissa inputs they must stay within the forward error
bound.  The cases reach every MF instance of both forward kernels, widths
that are no power of two, the degenerate halos (W = 1, H = 2), odd batches,
partial 64-wide k-blocks, one / odd / >128 channel tiles, C != K both ways
and every wgrad M regime (single chunk with an empty split, odd chunk
count, M % 64 != 0 tails, aligned)."""

import math

import pytest
import torch

import conv_oracle as co

pytestmark = pytest.mark.gpu

from flreid_amd import ops

CASES = co.HAND_CASES
MODES = co.HAND_MODES


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


_case = co.hand_case


def _run_hand(inp, mode, before_backward=None):
    """conv3x3_try fwd + bwd on the GPU -> (out, dx, dW) as CPU tensors."""
    x = _cl(inp.x.cuda()).requires_grad_(True)
    gw = _cl(inp.gw.cuda())
    dy = _cl(inp.dy.cuda())
    if mode == "plain":
        wparam = gw.requires_grad_(True)
        out = ops.conv3x3_try(x, wparam)
    else:
        wparam = _cl(inp.aw.cuda()).requires_grad_(True)
        atten = inp.atten.cuda() if mode == "adaptive" else None
        out = ops.conv3x3_try(x, gw, atten, wparam)
    assert out is not None, "conv3x3_try declined an in-regime shape"
    if before_backward is not None:
        before_backward()
    out.backward(dy)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and x.grad.dtype == torch.bfloat16
    assert wparam.grad.dtype == torch.float32
    return out.detach().cpu(), x.grad.cpu(), wparam.grad.cpu()


def _mismatch(got, want):
    bad = got.double() != want.double()
    return "%d of %d differ, max |diff| %g" % (
        int(bad.sum()), bad.numel(),
        float((got.double() - want.double()).abs().max()))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_hand_conv_exact_on_grid_inputs(case, mode, monkeypatch):
    monkeypatch.setenv("FLREID_CONV_IMPL", "hand")
    inp, ref = _case("grid", case, mode)
    out, dx, dw = _run_hand(inp, mode)
    want_out, want_dx, want_dw = co.to_bf16(ref.out), co.to_bf16(ref.dx), \
        ref.dw.float()
    verdict = {"fwd": torch.equal(out, want_out),
               "dgrad": torch.equal(dx, want_dx),
               "wgrad": torch.equal(dw, want_dw)}
    print("grid", case, mode, verdict)
    assert verdict["fwd"], _mismatch(out, want_out)
    assert verdict["dgrad"], _mismatch(dx, want_dx)
    assert verdict["wgrad"], _mismatch(dw, want_dw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_hand_conv_within_bound_on_full_inputs(case, mode, monkeypatch):
    monkeypatch.setenv("FLREID_CONV_IMPL", "hand")
    inp, ref = _case("full", case, mode)
    out, dx, dw = _run_hand(inp, mode)
    ratios = {"fwd": co.worst_ratio(out, ref.out, ref.bound_out()),
              "dgrad": co.worst_ratio(dx, ref.dx, ref.bound_dx()),
              "wgrad": co.worst_ratio(dw, ref.dw, ref.bound_dw())}
    print("full", case, mode,
          {k: round(v, 4) for k, v in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("case", [(3, 32, 4, 4, 32), (3, 160, 14, 8, 96)],
                         ids=lambda c: "x".join(map(str, c)))
def test_hand_wgrad_ignores_its_operand_pads(case, monkeypatch):
    """With M % 64 != 0 the last wgrad chunk of dyT's row K-1 reaches into
    the buffer's tail pad; whatever lies there must not reach dW.  NaN-filled
    blocks of exactly the two operand buffers' sizes are freed just before
    backward, so the caching allocator most likely hands them back for those
    buffers (likely, not certain: the assertion is the same either way).
    Before the wrapper zeroed that pad, the (3, 32, 4, 4, 32) case gave a
    NaN dW[K-1] here: xT is zero-masked there, but 0 x NaN = NaN."""
    monkeypatch.setenv("FLREID_CONV_IMPL", "hand")
    n, c, h, w, k = case
    m_rows = n * h * w
    assert m_rows % 64
    inp, ref = _case("grid", case, "adaptive")

    def poison():
        blocks = [torch.full((rows * m_rows + 256,), math.nan, device="cuda",
                             dtype=torch.bfloat16) for rows in (k, c)]
        torch.cuda.synchronize()
        del blocks

    out, dx, dw = _run_hand(inp, "adaptive", before_backward=poison)
    assert bool(torch.isfinite(dw).all()), \
        "non-finite dW rows: %s" % sorted(set(
            (~torch.isfinite(dw)).nonzero()[:, 0].tolist()))
    assert torch.equal(dw, ref.dw.float()), _mismatch(dw, ref.dw.float())
    assert torch.equal(dx, co.to_bf16(ref.dx))


# ---------------------------------------------------------------------------
# weight re-layout kernels (conv3x3_tile modes 0 / 1, conv3x3_wt_plain mode 2)
# ---------------------------------------------------------------------------

def _invp(p):
    g, i = p >> 3, p & 7
    return 4 * g + i if i < 4 else 16 + 4 * g + i - 4


PERM = [_invp(p) for p in range(32)]


def _decode_expected(theta, mode):
    """The tile `mode` must hold for the bf16 conv weight theta [K, C, 3, 3],
    flat, derived from the documented layouts alone."""
    k, c = theta.shape[0], theta.shape[1]
    th = theta.permute(0, 2, 3, 1).reshape(k, 9, c)          # [K][tap][C]
    flipped = th.flip(1)                                     # tap -> 8 - tap
    perm = torch.tensor(PERM, device=theta.device)
    if mode == 0:        # [C/32][9][4][K][8], c = 32 ct + invp(8 kg + e)
        t = th.view(k, 9, c // 32, 32)[..., perm].view(k, 9, c // 32, 4, 8)
        return t.permute(2, 1, 3, 0, 4).reshape(-1)
    if mode == 1:        # [K/32][9][4][C][8], k = 32 kt + invp(8 kg + e)
        t = flipped.view(k // 32, 32, 9, c)[:, perm].view(k // 32, 4, 8, 9, c)
        return t.permute(0, 3, 1, 4, 2).reshape(-1)
    return flipped.permute(2, 1, 0).reshape(-1)              # [C][9][K]


def test_invp_is_the_inverse_of_the_lds_permutation():
    # p(c) = ((c % 16) >> 2) * 8 + (c >> 4) * 4 + (c & 3), conv3x3_img.hip
    assert sorted(PERM) == list(range(32))
    for cc in range(32):
        assert PERM[((cc % 16) >> 2) * 8 + (cc >> 4) * 4 + (cc & 3)] == cc


TILE_CASES = [(mode, ck) for mode in (0, 1, 2)
              for ck in ((32, 96), (96, 32), (64, 64))] + [(2, (24, 40))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("compose", ["atten_aw", "aw", "none"])
@pytest.mark.parametrize("mode,ck", TILE_CASES,
                         ids=["mode%d-C%dK%d" % (m, c, k)
                              for m, (c, k) in TILE_CASES])
def test_theta_tile_layouts(mode, ck, compose, dtype):
    ext = ops.require_extension("conv3x3_tile")
    c, k = ck
    for kind in ("grid", "full"):
        inp = (co.grid_inputs if kind == "grid" else co.full_inputs)(
            1, c, 4, 4, k, seed=co.HAND_SEED)
        gw = _cl(inp.gw.cuda().to(dtype))
        aw = None if compose == "none" else _cl(inp.aw.cuda().to(dtype))
        atten = inp.atten.cuda() if compose == "atten_aw" else None
        tile = ops.conv_theta_tile(ext, gw, atten, aw, mode)
        theta = ops.compose_theta_bf16(ext, gw, atten, aw)
        torch.cuda.synchronize()
        assert tile.dtype == torch.bfloat16 and tile.numel() == c * 9 * k
        want = _decode_expected(theta, mode)
        if kind == "grid":
            # theta itself is exact, however it is composed
            exact = co.to_bf16(co.compose_theta64(
                inp.gw, None if atten is None else inp.atten,
                None if aw is None else inp.aw))
            assert torch.equal(theta.cpu(), exact)
            assert torch.equal(tile, want), _mismatch(tile, want)
        else:
            dist = co.bf16_ulp_distance(tile, want)
            print("tile", mode, ck, compose, dtype, "ulp distance", dist)
            assert dist <= 1, dist
