"""add_ln.hip through `ops.add_layer_norm` against a float64 reference on the
values the kernel reads, and one Swin block with the fused route on and off.

s = a + b is one exactly rounded add and is compared BIT FOR BIT with the
CPU's.  dy sits on the grid i/8, |i| <= 8, so dbeta is exact in fp32 in any order
and is compared bit for bit too.  y, ds, the branch's copy of ds and dgamma
are held to the error model of `rowops_oracle.patch_merge_reference`, with
its row depth replaced by this kernel's: a lane of the G-lane group chains
its 8 K values (K = ceil(C / 8 / G) <= 3 chunks of 8 columns), log2 G
butterfly levels add the lanes, one division follows:
    h = 8 K + log2 G + 1        (31 at C = 1536, 20 at C = 96)
with G the narrowest of 8, 16, 32, 64 that keeps K <= 3.  On top of that
model: one rounding u |ds| for the ds_in add, and the bf16 store term where
an output is bf16.  dgamma keeps the model's (rows + 1) u term: a lane's
chain over its rows, the butterflies and the sum of the partials are no
deeper than a row-by-row sum.  Nothing here is tuned."""

import copy
import math

import pytest
import torch

import rowops_oracle as ro
from rowops_oracle import U, _final, _randgrid

from flreid_amd import ops
from flreid_amd.models.swin import SwinBlock

pytestmark = pytest.mark.gpu

F32, BF16, EPS = torch.float32, torch.bfloat16, 1e-5
DTYPES = [(F32, BF16, BF16), (F32, None, BF16), (F32, F32, F32),
          (BF16, BF16, BF16)]
WIDTHS = [8, 96, 104, 192, 384, 768, 1536]     # G = 8, 8, 8, 8, 16, 32, 64


def _geometry(c):                     # (G, K) as add_ln.hip picks them
    nc = c // 8
    g = next((g for g in (8, 16, 32) if -(-nc // g) <= 3), 64)
    return g, -(-nc // g)


def _name(v):
    return "-".join(str(d).replace("torch.", "") for d in v) \
        if isinstance(v, tuple) else str(v)


def _inputs(c, rows, dtypes, offset=False):
    a_dt, b_dt, y_dt = dtypes
    g = torch.Generator().manual_seed(1000 * c + rows)
    a = torch.randn(rows, c, generator=g)
    if offset:
        a = 0.25 * (2.0 ** 6 + a)
    b = None if b_dt is None else torch.randn(rows, c, generator=g).to(b_dt)
    return dict(a=a.to(a_dt), b=b,
                gamma=1.0 + 0.5 * torch.randn(c, generator=g),
                beta=torch.randn(c, generator=g),
                dy=_randgrid((rows, c), 8, 2.0 ** -3, g).to(y_dt),
                ds_in=torch.randn(rows, c, generator=g).to(a_dt))


def _reference(inp, dtypes, mode):
    """name -> (float64 reference, bound), as `patch_merge_reference`"""
    a_dt, b_dt, y_dt = dtypes
    s = inp["a"] if inp["b"] is None else inp["a"] + inp["b"]   # CPU add
    x, gamma, beta = s.double(), inp["gamma"].double(), inp["beta"].double()
    dy = inp["dy"].double() * (mode != "ds_in")
    rows, n = x.shape
    g_, k_ = _geometry(n)
    h = 8 * k_ + int(math.log2(g_)) + 1
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    xh = c * rstd
    y = xh * gamma + beta
    g = gamma * dy
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    dx = (g - m1 - xh * m2) * rstd
    e_mean = h * U * x.abs().mean(-1, keepdim=True)
    e_var = (h + 5) * U * var + e_mean ** 2
    e_rstd = rstd * (e_var / (2 * (var + EPS)) + 4 * U)
    e_xh = rstd * (e_mean + 2 * U * c.abs()) + c.abs() * e_rstd
    e_y = gamma.abs() * e_xh + 2 * U * ((xh * gamma).abs() + beta.abs())
    e_m1 = h * U * g.abs().mean(-1, keepdim=True)
    e_m2 = (g.abs() * e_xh).mean(-1, keepdim=True) \
        + (h + 2) * U * (g * xh).abs().mean(-1, keepdim=True)
    e_dx = rstd * (e_m1 + e_xh * m2.abs() + xh.abs() * e_m2
                   + 4 * U * (g.abs() + m1.abs() + (xh * m2).abs())) \
        + dx.abs() * e_rstd / rstd
    e_dg = (dy.abs() * e_xh).sum(0) + (rows + 1) * U * (dy * xh).abs().sum(0)
    ds, e_ds = dx, e_dx
    if mode in ("both", "ds_in", "no_affine") and inp["b"] is not None:
        ds = dx + inp["ds_in"].double()
        e_ds = e_dx + U * ds.abs()
    ref = {"s": (x, torch.zeros_like(x)),
           "y": (y, _final(e_y, y, y_dt == BF16)),
           "ds": (ds, _final(e_ds, ds, a_dt == BF16)),
           "dbranch": (ds, _final(e_ds, ds, b_dt == BF16)),
           "dgamma": ((dy * xh).sum(0), _final(e_dg)),
           "dbeta": (dy.sum(0), torch.zeros(n, dtype=torch.float64))}
    assert float(dy.abs().sum(0).max()) < 2.0 ** 20       # dbeta is exact
    return ref


def _gpu(inp, dtypes, mode):
    a_dt, b_dt, y_dt = dtypes
    affine = mode != "no_affine"
    a = inp["a"].cuda().requires_grad_(True)
    b = None if inp["b"] is None else inp["b"].cuda().requires_grad_(True)
    gamma = inp["gamma"].cuda().requires_grad_(affine)
    beta = inp["beta"].cuda().requires_grad_(affine)
    assert ops.add_layer_norm_route(a.shape[1], a_dt, b_dt, y_dt) == "kernel"
    out = ops.add_layer_norm(a, b, gamma, beta, EPS, y_dt)
    s, y = (a, out) if b is None else out
    outs, grads = [y], [inp["dy"].cuda()]
    if b is not None and mode != "dy":
        outs, grads = [s, y], [inp["ds_in"].cuda(), grads[0]]
        if mode == "ds_in":
            outs, grads = outs[:1], grads[:1]
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    assert y.dtype == y_dt and s.dtype == a_dt and a.grad.dtype == a_dt
    got = {"s": s.detach().cpu(), "y": y.detach().cpu(), "ds": a.grad.cpu()}
    if b is not None:
        assert b.grad.dtype == b_dt
        got["dbranch"] = b.grad.cpu()
    if affine and mode != "ds_in":
        got["dgamma"], got["dbeta"] = gamma.grad.cpu(), beta.grad.cpu()
    else:
        assert gamma.grad is None and beta.grad is None
    return got


def _check(c, rows, dtypes, mode="both", offset=False):
    inp = _inputs(c, rows, dtypes, offset)
    got, ref = _gpu(inp, dtypes, mode), _reference(inp, dtypes, mode)
    ratios = {k: ro.worst_ratio(got[k], *ref[k]) for k in got
              if k not in ("s", "dbeta")}
    print(c, rows, _name(dtypes), mode, ratios)
    assert torch.equal(got["s"].double(), ref["s"][0])
    if "dbeta" in got:
        assert torch.equal(got["dbeta"].double(), ref["dbeta"][0])
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("dtypes", DTYPES, ids=_name)
@pytest.mark.parametrize("c, rows", [
    (c, r) for c in WIDTHS for r in (1, 3, 256 // _geometry(c)[0] + 1)])
def test_add_ln_within_bound(c, rows, dtypes):
    """both gradients; rows: 1, 3 and one more than a block step covers"""
    _check(c, rows, dtypes)


@pytest.mark.parametrize("c, rows, dtypes, mode", [
    (c, r, d, m) for c, r in ((96, 33), (768, 9)) for d in DTYPES
    for m in ("ds_in", "dy", "no_affine") if d[1] is not None or m != "ds_in"],
    ids=_name)
def test_add_ln_backward_modes(c, rows, dtypes, mode):
    """either gradient absent (a null pointer); affine gradients off"""
    _check(c, rows, dtypes, mode)


def test_add_ln_every_block_loops_twice():
    """C = 8: 32 rows a block step and at most 1024 blocks, so every block
    goes round its row loop at least twice"""
    _check(8, 2 * 1024 * 32 + 5, DTYPES[0])


@pytest.mark.parametrize("dtypes", [DTYPES[0], DTYPES[2]], ids=_name)
def test_add_ln_rows_far_from_zero(dtypes):
    """x = 0.25 (2^6 + randn): E[x^2] - mean^2 misses the bound here"""
    _check(96, 33, dtypes, offset=True)


def _block_errors(flag, blk, x, dout, want, monkeypatch):
    monkeypatch.setenv("FLREID_SWIN_ADD_LN", flag)
    blk.zero_grad()
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        out = blk(xg)
    out.backward(dout.cuda().to(out.dtype))
    got = (out, xg.grad, blk.norm1.weight.grad, blk.norm2.weight.grad)
    return [float((g.detach().double().cpu() - w).abs().max())
            for g, w in zip(got, want)]


def test_swin_block_fused_route_no_worse_than_eager(monkeypatch):
    """One block under bf16 autocast against a float64 CPU run.  Both routes
    carry the same dominating bf16 roundings of the GEMMs: the fused route's
    largest error in out, dx and the two LN dgammas may be at most twice the
    eager route's on the same inputs."""
    torch.manual_seed(0)
    blk = SwinBlock(96, (14, 14), 3, window_size=7, shift=3)
    x, dout = torch.randn(2, 196, 96), torch.randn(2, 196, 96)
    ref_blk = copy.deepcopy(blk).double()
    x64 = x.double().requires_grad_(True)
    out64 = ref_blk(x64)
    out64.backward(dout.double())
    want = (out64.detach(), x64.grad, ref_blk.norm1.weight.grad,
            ref_blk.norm2.weight.grad)
    blk = blk.cuda()
    eager = _block_errors("0", blk, x, dout, want, monkeypatch)
    fused = _block_errors("1", blk, x, dout, want, monkeypatch)
    print("out, dx, dgamma1, dgamma2: eager", eager, "fused", fused)
    assert all(f <= 2.0 * e for f, e in zip(fused, eager)), (fused, eager)
