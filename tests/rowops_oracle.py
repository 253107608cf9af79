"""Float64 oracle for the row-wise HIP kernels: the pairwise MFMA GEMM and
rowsq (distance.hip), the batch-hard triplet (triplet.hip), Swin window
attention (window_attn.hip), the patch-merge LayerNorm (patch_merge.hip)
and the row losses (ce_smooth in elementwise.hip, kd_fwd and icarl_distill
in kd.hip).

For each family: the case list, input builders from a fixed seed, a float64
reference on exactly the values the kernel sees (bf16 inputs are rounded
first) and, per output, an elementwise bound.  A reference is a dict
`name -> (ref64, bound64)`.

Bounds are derived, not tuned.  The unit is u = 2^-24 (one fp32 rounding).
Every function below first adds up the FIRST-ORDER error e of the fp32
evaluation the kernel performs:

* an n-term sum of products: n u S, S the float64 sum of absolute values;
* one more rounding of a value x: u |x|;
* a stage that feeds another: its error times the absolute derivative;
* a fast intrinsic: __expf(x) has relative error (|x| + C_EXP) u — the
  argument is scaled by log2(e) (one rounding of a number of size |x|
  log2 e, which moves the result by |x| u relatively) and v_exp_f32 is
  good to 1 ulp = 2 u, the final rounding to another u, hence C_EXP = 4
  with one unit of slack; __logf(x) has ABSOLUTE error (|log x| + C_LOG) u:
  v_log_f32 is a 1-ulp log2 whose error near x = 1, where the result
  vanishes, is absolute (about 2^-22 = 4 u), times ln 2, plus the rounding
  of that product; C_LOG = 8;
* a subnormal intermediate (an exponential of a masked logit, say) may be
  flushed to zero and then scaled by what follows: TINY = 2^-100, thirty
  orders of magnitude below every quantity tested here.

and then returns `conv_oracle.bound`'s form  2 e (+ 2^-8 |ref| for a bf16
store) + TINY.  The factor 2 is the one `conv_oracle.bound` carries (an
accumulator that truncates instead of rounding).  Two families replace
"n = number of summed terms" by the depth of the kernel's reduction tree,
and say why: the patch-merge row statistics (`patch_merge_reference`) and
the triplet distances (`triplet_reference`).

Grid inputs: where the kernel's arithmetic is sums of products only, inputs
on a coarse grid make every partial sum exact in fp32 in any order, and the
result is compared bit for bit.  `exact=True` asserts the preconditions.

Everything here runs on the CPU; this module is imported by the CPU test of
the oracle itself (test_rowops_oracle.py) and by the GPU tests
(test_rowops_exact_gpu.py)."""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from conv_oracle import (U_BF16_STORE, U_FP32, bound, round_bf16,  # noqa: F401
                         to_bf16, worst_ratio)
from flreid_amd.ops import reference as ref_ops

U = U_FP32
TINY = 2.0 ** -100
C_EXP = 4.0
C_LOG = 8.0
SEED = 3

Ref = Dict[str, Tuple[torch.Tensor, torch.Tensor]]


def _gen(*key) -> torch.Generator:
    """One generator per (SEED, key): a case's inputs do not depend on
    which other cases ran."""
    g = torch.Generator()
    g.manual_seed(abs(hash((SEED,) + tuple(
        int(k) if isinstance(k, (int, bool)) else sum(map(ord, str(k)))
        for k in key))) % (2 ** 31))
    return g


def _final(e: torch.Tensor, ref: Optional[torch.Tensor] = None,
           bf16: bool = False) -> torch.Tensor:
    """first-order error e -> bound: conv_oracle.bound with n S = e."""
    b = bound(ref, e / U, 1, bf16_store=bf16) if bf16 else 2.0 * e
    return b + TINY


def _randgrid(shape, lim: int, scale: float, g) -> torch.Tensor:
    return torch.randint(-lim, lim + 1, shape, generator=g).float() * scale


# ---------------------------------------------------------------------------
# pairwise (distance.hip) through ops.similarity_matrix (mode 0),
# ops.pairwise_cosine_distance (mode 1: l2norm_rows, then 1 - A.B^T) and
# ops.pairwise_sqeuclidean (mode 2: rowsq twice, then aa + bb - 2 A.B^T)
# ---------------------------------------------------------------------------

PAIRWISE_CASES = [          # (M, N, D)
    (128, 128, 32),         # one interior tile, one K panel
    (256, 128, 64),         # two interior row tiles, two panels
    (257, 133, 36),         # interior tiles whose 2nd panel is the guarded
                            # tail, next to edge tiles
    (129, 127, 36),         # no interior tile
    (130, 130, 30),         # D % 4 != 0: guarded path on full tiles
    (3, 200, 7),            # small M, guarded path
    (1, 1, 1),              # degenerate
]
PAIRWISE_MODES = [0, 1, 2]
# the operand is a[1:] of an (M + 1)-row matrix: still contiguous, and the
# float4 loads start one row into the allocation (cmc_map's query chunks)
PAIRWISE_SLICED_CASE = (257, 133, 36)
ROWSQ_COLS = [1, 63, 256, 257, 2048]
ROWSQ_ROWS = 3
GRID_SUM_LIMIT = 2.0 ** 18   # multiples of 2^-6 below this are exact fp32


def _unit_grid_rows(m: int, d: int, g) -> torch.Tensor:
    """Rows that are unit-norm ON the grid: 16 entries of +-1/4 (d >= 16),
    4 of +-1/2 (d >= 4) or one of +-1, the rest zero.  Their sum of squares
    is exactly 1, so l2norm_rows returns them unchanged."""
    k = 16 if d >= 16 else (4 if d >= 4 else 1)
    x = torch.zeros(m, d)
    for r in range(m):
        cols = torch.randperm(d, generator=g)[:k]
        sign = torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
        x[r, cols] = sign / math.sqrt(k)
    return x


def pairwise_inputs(kind: str, case, mode: int, extra_row: bool = False):
    """(a, b) fp32.  grid: i/2^3, |i| <= 8 (mode 1: unit-norm grid rows)."""
    m, n, d = case
    m += int(extra_row)
    g = _gen("pairwise", kind, m, n, d, mode)
    if kind == "full":
        return (torch.randn(m, d, generator=g), torch.randn(n, d, generator=g))
    if mode == 1:
        return _unit_grid_rows(m, d, g), _unit_grid_rows(n, d, g)
    return (_randgrid((m, d), 8, 2.0 ** -3, g),
            _randgrid((n, d), 8, 2.0 ** -3, g))


def pairwise_reference(a, b, mode: int, exact: bool = False,
                       d_used: Optional[int] = None) -> Ref:
    """out = A.B^T (0), 1 - An.Bn^T on l2-normalised rows (1), aa + bb -
    2 A.B^T (2), in float64.  d_used < D drops the K tail (a mutant).

    Errors (n = D terms in the dot, S = |A|.|B|^T):
      mode 0: D u S.
      mode 2: aa and bb are D-term sums of rounded squares, (D + 1) u aa
        each; the dot enters doubled; the epilogue adds two roundings of
        partial results no larger than aa + bb + 2 S:
        (D + 3) u (aa + bb + 2 S).
      mode 1: each normalised element carries the row sum of squares
        ((D + 1) u, halved by the square root), the square root, the
        reciprocal and the product: ((D + 1)/2 + 3) u relative; two
        operands and the D-term dot give (2 D + 7) u S; 1 - v is one more
        rounding of a value <= 1 + S <= 2: 2 u.
    exact=True: products are multiples of 2^-6, so every sum is exact while
    the sum of absolute values stays below 2^18; mode 1 rows must have a
    sum of squares of exactly 1."""
    a64, b64 = a.double(), b.double()
    d = a64.shape[1]
    if mode == 1:
        if exact:
            for t in (a64, b64):
                assert torch.equal((t * t).sum(1), torch.ones(t.shape[0],
                                                              dtype=t.dtype))
        a64 = a64 / a64.norm(dim=1, keepdim=True).clamp_min(1e-12)
        b64 = b64 / b64.norm(dim=1, keepdim=True).clamp_min(1e-12)
    ak, bk = (a64, b64) if d_used is None else (a64[:, :d_used],
                                                b64[:, :d_used])
    dot = ak @ bk.t()
    s = a64.abs() @ b64.abs().t()
    if mode == 0:
        out, e = dot, d * U * s
    elif mode == 1:
        out, e = 1.0 - dot, (2 * d + 7) * U * s + 2 * U
    else:
        aa, bb = (a64 * a64).sum(1, keepdim=True), (b64 * b64).sum(1)
        out = aa + bb - 2.0 * dot
        s = aa + bb + 2.0 * s
        e = (d + 3) * U * s
    if exact:
        for t in (a, b):
            t8 = t.double() * 8
            assert torch.equal(t8, t8.round()) and float(t8.abs().max()) <= 8
        assert float(s.max()) < GRID_SUM_LIMIT
        assert torch.equal(out.float().double(), out)
    return {"out": (out, _final(e))}


def rowsq_inputs(kind: str, cols: int):
    """(x, zero row): ops.pairwise_sqeuclidean(x, 0) = rowsq(x) + 0 - 2.0,
    the row squares themselves, through the public wrapper."""
    g = _gen("rowsq", kind, cols)
    x = (torch.randn(ROWSQ_ROWS, cols, generator=g) if kind == "full"
         else _randgrid((ROWSQ_ROWS, cols), 8, 2.0 ** -3, g))
    return x, torch.zeros(1, cols)


# ---------------------------------------------------------------------------
# batch-hard triplet (triplet.hip) through ops.triplet_loss
# ---------------------------------------------------------------------------

TRIPLET_SIZES = [           # (N, D)
    (3, 5),                 # fewer anchors than waves, D < 64
    (8, 64),                # baseline
    (16, 65),               # D tail
    (64, 512),              # larger batch
    (32, 2048),             # production width
]
TRIPLET_PATTERNS = ["pk", "one", "distinct", "singleton_lo", "singleton_hi",
                    "dup_stride", "dup_adjacent"]
TRIPLET_MARGINS = [0.25, 0.3]
TRIPLET_GRID_UPSTREAM = [1.0, 2.0]
TRIPLET_FULL_UPSTREAM = 1.7


def triplet_admits(size, pattern: str) -> bool:
    n, d = size
    if pattern in ("one", "distinct", "singleton_lo", "singleton_hi"):
        return True
    return n % 4 == 0 and n >= 8 and d >= 8     # pk and the dup patterns


TRIPLET_CASES = [(size, p) for size in TRIPLET_SIZES
                 for p in TRIPLET_PATTERNS if triplet_admits(size, p)]


def triplet_inputs(kind: str, size, pattern: str):
    """`_triplet_build` at the first attempt (counting from 0) whose
    selection the fp32 error cannot reach (`TripletRef.stable`, both
    margins) — a property of the inputs alone, as conv_oracle's HAND_SEED;
    grid inputs need none and take attempt 0."""
    def make():
        for attempt in range(64):
            f, labels = _triplet_build(kind, size, pattern, attempt)
            if kind == "grid" or all(
                    triplet_reference(f, labels, m, TRIPLET_FULL_UPSTREAM
                                      ).stable for m in TRIPLET_MARGINS):
                return f, labels
        raise AssertionError("no stable inputs for %s %s" % (size, pattern))
    f, labels = cached(("triplet_inputs", kind, size, pattern), make)
    return f.clone(), labels.clone()


def _triplet_build(kind: str, size, pattern: str, attempt: int):
    """(feature fp32 [N, D], labels int64 [N]).

    grid features are i/2^3, |i| <= 8.  Perturbations are grid steps (1/8,
    squared distance 1/64) on a coordinate zeroed first.

    singleton_lo / singleton_hi: anchor a = N // 2 is alone in its class;
      row a - 1 (lo) or a + 1 (hi), of another class, is the anchor's copy
      one step away, so the anchor is ACTIVE for every margin > 1/64 while
      its only positive is itself.
    dup_stride / dup_adjacent: rows 1 and 5 (one wave's stride) or 1 and 2
      (neighbouring waves) are identical and both of class 0; the other
      class-0 rows 2 or 5, and 3, sit 1 and 3 steps from row 0, so for anchor 0
      the two copies TIE as hardest positive; row 4, of class 1, sits one
      step from row 1, so for anchor 4 they TIE as hardest negative."""
    n, d = size
    g = _gen("triplet", kind, n, d, pattern, attempt)
    f = (torch.randn(n, d, generator=g) if kind == "full"
         else _randgrid((n, d), 8, 2.0 ** -3, g))
    step = 0.125

    def near(src, coord, steps=1):
        row = f[src].clone()
        row[coord] = steps * step
        return row

    if pattern == "one":
        labels = torch.zeros(n, dtype=torch.int64)
    elif pattern == "distinct":
        labels = torch.arange(n, dtype=torch.int64)
    else:
        labels = torch.arange(n, dtype=torch.int64) // 4
    if pattern.startswith("singleton"):
        a = n // 2
        neg = a - 1 if pattern == "singleton_lo" else a + 1
        labels[a] = n + 7
        f[a, 0] = 0.0
        f[neg] = near(a, 0)
        assert labels[neg] != labels[a]
    if pattern.startswith("dup"):
        j2 = 5 if pattern == "dup_stride" else 2
        rest = [r for r in (2, 3, 5) if r != j2]       # two more class-0 rows
        labels[5] = 0
        f[0, :4] = 0.0
        f[1, :4] = 0.0
        f[j2] = f[1]
        for coord, r in enumerate(rest):       # 1 and 3 steps: no tie here
            f[r] = near(0, coord, 1 + 2 * coord)
        f[4] = near(1, 3)
        assert labels[4] != 0
    return f, labels


@dataclass
class TripletRef:
    loss: Tuple[torch.Tensor, torch.Tensor]
    grad: Tuple[torch.Tensor, torch.Tensor]
    row_loss: torch.Tensor       # float64 [N]
    ap: torch.Tensor
    an: torch.Tensor
    p_first: np.ndarray          # numpy first-index argmax of dist * is_pos
    p_idx: np.ndarray            # ... or i where that column is no positive
    n_idx: np.ndarray
    grad_ap: torch.Tensor        # the part of grad that flows through ap
    stable: bool                 # selection and hinge survive the fp32 error


def _triplet_scatter(f64, rows, p, nn, coeff, part="both", absolute=False):
    """Analytic gradient of mean_i hinge_i for the given (i, p_i, n_i)
    triples, or with absolute=True the sum of absolute values of its
    terms and the number of terms per row."""
    g = torch.zeros_like(f64)
    cnt = torch.zeros(f64.shape[0], dtype=torch.float64)
    for i in rows:
        fi = f64[i]
        for sign, j in ((1.0, int(p[i])), (-1.0, int(nn[i]))):
            if (sign > 0 and part == "an") or (sign < 0 and part == "ap"):
                continue
            fj = f64[j]
            if absolute:
                t = abs(coeff) * (fi.abs() + fj.abs())
                g[i] += t
                g[j] += t
                cnt[i] += 1
                cnt[j] += 1
            else:
                g[i] += sign * coeff * (fi - fj)
                g[j] += sign * coeff * (fj - fi)
    return (g, cnt) if absolute else g


def triplet_reference(feature, labels, margin: float, upstream: float = 1.0,
                      exact: bool = False, last_index_ties: bool = False,
                      through_negative: bool = False) -> TripletRef:
    """Float64 batch-hard triplet in the contract's form (ops/reference.py):
    ap = max_j d_ij [same class], an = min_j (d_ij [other class] + 1e9 [same
    class]), loss = mean max(0, margin + ap - an).

    The gradient is float64 autograd of `reference.triplet_loss`.  For an
    anchor all of whose positives are copies of itself (a class of one) the
    maximum is 0 and may sit on a negative's column, where the mask stops
    the gradient: nothing flows through ap.  p_idx records the anchor
    itself then.

    Mutants: last_index_ties takes the LAST index of tied maxima;
    through_negative pushes the ap gradient through whatever column the
    first-index maximum sits on, positive or not.

    Errors.  d_ij = aa_i + aa_j - 2 f_i.f_j with S2 = aa_i + aa_j + 2
    |f_i|.|f_j|.  As for the patch-merge statistics the term count is the
    DEPTH of the kernel's reductions, not D: a lane of the 64-lane wave
    chains ceil(D / 64) fmas and a 6-level butterfly adds the lanes (rowsq:
    ceil(D / 256) terms a thread, 6 + 2 levels, no deeper), then the
    doubling and two adds: e_d = (ceil(D / 64) + 9) u S2.  With n = D the
    allowance at D = 2048 would be wider than the gaps between random
    distances and no full-input case could be shown stable.  row: e_ap + e_an + 2 u (margin
    + ap + an); loss: the mean of those plus the N-term sum (N + 1) u
    mean(row).  grad: row r receives c_r terms coeff (f_a - f_b), each with
    the rounding of coeff = 2 g/N, the difference and the product, summed by
    atomics in any order: (c_r + 3) u sum |coeff| (|f_a| + |f_b|).  All of
    this holds only while the fp32 error can change neither a selected
    index nor an anchor's side of the hinge: `stable`, which
    test_rowops_oracle.py asserts for every full-input case.  Ties between
    IDENTICAL rows are exact ties in fp32 too and do not count.

    exact=True (grid inputs): every distance is an exact multiple of 2^-6
    below 2^18, N is a power of two and upstream is 1 or 2, so coeff is a
    power of two and the gradient is exact; no anchor may sit exactly ON
    the hinge, where kernel (inactive) and autograd (active) differ by
    convention."""
    f64 = feature.double()
    n, d = f64.shape
    # sum (f_i - f_j)^2, not the addmm form: identical rows then give
    # identical distances to the last bit and tie as they do in the kernel
    dist = ((f64.view(n, 1, d) - f64.view(1, n, d)) ** 2).sum(-1)
    lab = labels.view(n, 1)
    is_pos = lab.eq(lab.t())
    dp = (dist * is_pos).numpy()
    dn = (dist * ~is_pos + 1e9 * is_pos.double()).numpy()
    p_first = dp.argmax(1)                        # numpy: first index
    if last_index_ties:
        p_first = n - 1 - dp[:, ::-1].argmax(1)
    n_idx = dn.argmin(1)
    ap = torch.from_numpy(dp[np.arange(n), p_first].copy())
    an = torch.from_numpy(dn[np.arange(n), n_idx].copy())
    row = (margin + ap - an).clamp_min(0.0)
    loss = row.mean()
    real = is_pos.numpy()[np.arange(n), p_first]
    p_idx = np.where(real, p_first, np.arange(n))
    active = [i for i in range(n) if float(row[i]) > 0]
    coeff = 2.0 * upstream / n

    if last_index_ties or through_negative:
        grad = _triplet_scatter(f64, active, p_first, n_idx, coeff)
    else:
        leaf = f64.clone().requires_grad_(True)
        (ref_ops.triplet_loss(leaf, labels, margin) * upstream).backward()
        grad = leaf.grad
    grad_ap = _triplet_scatter(f64, active, p_idx, n_idx, coeff, part="ap")

    aa = (f64 * f64).sum(1)
    s2 = aa.view(n, 1) + aa.view(1, n) + 2.0 * (f64.abs() @ f64.abs().t())
    e_d = (-(-d // 64) + 9) * U * s2
    e_row = (e_d[torch.arange(n), torch.from_numpy(p_first)]
             + torch.where(an < 1e8, e_d[torch.arange(n),
                                         torch.from_numpy(n_idx)],
                           torch.zeros(n, dtype=torch.float64))
             + 2 * U * (margin + ap + torch.where(an < 1e8, an,
                                                  torch.zeros_like(an))))
    e_loss = e_row.mean() + (n + 1) * U * row.mean()
    s_g, cnt = _triplet_scatter(f64, active, p_idx, n_idx, coeff,
                                absolute=True)
    e_grad = (cnt.view(n, 1) + 3) * U * s_g

    # is the selection out of reach of the fp32 error?  Only ACTIVE anchors
    # matter: an inactive one contributes nothing whatever it selects.
    same_row = (f64.view(n, 1, d) == f64.view(1, n, d)).all(-1)
    stable = True
    for i in range(n):
        pos = is_pos[i]
        if bool(pos.all()):
            continue                               # no negative: loss 0
        hinge = margin + float(ap[i]) - float(an[i])
        stable &= abs(hinge) > 2.0 * float(e_row[i])
        if hinge < 0:
            continue
        emax = 2.0 * float(e_d[i].max())
        if float(dist[i][pos].max()) > 0:          # a positive that is no copy
            other = pos & ~same_row[p_first[i]]
            gap = float(ap[i]) - (float(dist[i][other].max())
                                  if bool(other.any()) else 0.0)
            stable &= gap > emax and float(ap[i]) > emax
        other = ~pos & ~same_row[n_idx[i]]
        if bool(other.any()):
            stable &= float(dist[i][other].min()) - float(an[i]) > emax
    if exact:
        t8 = f64 * 8
        assert torch.equal(t8, t8.round()) and float(t8.abs().max()) <= 8
        assert float(s2.max()) < GRID_SUM_LIMIT
        assert n & (n - 1) == 0 and upstream in (1.0, 2.0)
        on_hinge = (margin + ap - an == 0) & (an < 1e8)
        assert not bool(on_hinge.any()), "an anchor sits on the hinge"
    return TripletRef(
        loss=(loss, _final(e_loss)), grad=(grad, _final(e_grad)),
        row_loss=row, ap=ap, an=an, p_first=p_first, p_idx=p_idx,
        n_idx=n_idx, grad_ap=grad_ap, stable=bool(stable))


def triplet_row_loss_fp32(ref: TripletRef, margin: float) -> np.ndarray:
    """The kernel's own evaluation order on exact distances, in float32:
    max(0, (margin + ap) - an)."""
    m = np.float32(margin)
    ap, an = ref.ap.numpy().astype(np.float32), \
        ref.an.numpy().astype(np.float32)
    return np.maximum(np.float32(0), (m + ap) - an).astype(np.float32)


# ---------------------------------------------------------------------------
# Swin window attention (window_attn.hip) through ops.window_attention
# ---------------------------------------------------------------------------

WINDOW_CASES = [            # (BW, H, N, D, nW or None)
    (4, 2, 49, 32, 2),      # production shape
    (2, 1, 64, 64, 1),      # both limits at once
    (3, 2, 16, 24, 3),      # D % 8 != 0, BW == nW
    (5, 2, 49, 32, None),   # odd BW, no mask
    (5, 1, 63, 8, 2),       # BW % nW != 0, N N % 256 != 0
    (1, 1, 1, 1, 1),        # degenerate
]
WINDOW_EAGER_CASE = (2, 1, 65, 8, None)      # N = 65: the eager route
WINDOW_DTYPES = [torch.float32, torch.bfloat16]


@dataclass
class WindowInputs:
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    do: torch.Tensor
    bias: torch.Tensor                 # [H, N, N] fp32, untied
    mask: Optional[torch.Tensor]       # [nW, N, N] fp32, 0 / -100
    scale: float


def window_inputs(case, dtype) -> WindowInputs:
    """Masks differ per window, hold 0 and -100 with an open diagonal, and
    row 0 of window 0 keeps the single key N // 2.  bias[h, i, j] and
    bias[h, j, i] are independent."""
    bw, h, n, d, nw = case
    g = _gen("window", bw, h, n, d, nw or 0, dtype == torch.bfloat16)
    q, k, v, do = (torch.randn(bw, h, n, d, generator=g).to(dtype)
                   for _ in range(4))
    bias = torch.randn(h, n, n, generator=g)
    mask = None
    if nw is not None:
        mask = torch.where(torch.rand(nw, n, n, generator=g) < 0.3,
                           -100.0, 0.0)
        mask[:, torch.arange(n), torch.arange(n)] = 0.0
        mask[0, 0, :] = -100.0
        mask[0, 0, n // 2] = 0.0
    return WindowInputs(q, k, v, do, bias, mask, float(d) ** -0.5)


def window_reference(inp: WindowInputs, mask_shift: int = 0,
                     bias_transposed: bool = False, dk_scale: bool = True,
                     rowsum: bool = True) -> Ref:
    """Float64 forward and hand-written backward (test_rowops_oracle.py
    checks it against float64 autograd) of
      S = scale Q K^T + bias[h] + mask[bw % nW], P = softmax(S), O = P V,
      dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dP P)),
      dQ = scale dS K, dK = scale dS^T Q, dbias = sum_bw dS.
    The keyword arguments are the mutants.

    Errors, each stage feeding the next (e_x is the absolute error of x):
      e_S  = (D + 3) u (scale |Q||K|^T + |bias| + |mask|): D-term dot,
             scale, two adds.
      t    = e_S + e_S at the row maximum + (2 |x| + C_EXP) u with x = S -
             max: the subtraction's rounding joins __expf's |x| u.
      e_P  = P (t + P.t + (N + 3) u): d softmax_j = P_j (dS_j - sum_k P_k
             dS_k), then the N-term sum, the reciprocal and the product.
      e_O  = e_P |V| + N u P |V|                          (+ bf16 store)
      e_dV = e_P^T |dO| + N u P^T |dO|                    (+ bf16 store)
      e_dP = D u |dO| |V|^T
      e_rd = sum_j (e_dP P + |dP| e_P) + (N + 1) u sum_j |dP| P
      e_dS = e_P |dP - rd| + P (e_dP + e_rd) + 2 u P (|dP| + |rd|)
      e_dQ = scale (e_dS |K| + (N + 1) u |dS| |K|)        (+ bf16 store)
      e_dK = scale (e_dS^T |Q| + (N + 1) u |dS|^T |Q|)    (+ bf16 store)
      e_db = sum_bw e_dS + BW u sum_bw |dS|."""
    q, k, v, do = (t.double() for t in (inp.q, inp.k, inp.v, inp.do))
    bw, h, n, d = q.shape
    bf16 = inp.q.dtype == torch.bfloat16
    scale = float(np.float32(inp.scale))
    bias = inp.bias.double()
    if bias_transposed:
        bias = bias.transpose(1, 2)
    s = scale * (q @ k.transpose(-1, -2)) + bias
    s_abs = scale * (q.abs() @ k.abs().transpose(-1, -2)) + bias.abs()
    if inp.mask is not None:
        nw = inp.mask.shape[0]
        w = (torch.arange(bw) + mask_shift) % nw
        m = inp.mask.double()[w].unsqueeze(1)
        s, s_abs = s + m, s_abs + m.abs()
    smax, imax = s.max(-1, keepdim=True)
    x = s - smax
    p = torch.softmax(s, -1)
    o = p @ v
    dv = p.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    rd = (dp * p).sum(-1, keepdim=True) if rowsum else torch.zeros_like(smax)
    ds = p * (dp - rd)
    dq = scale * (ds @ k)
    dk = (scale if dk_scale else 1.0) * (ds.transpose(-1, -2) @ q)
    db = ds.sum(0)

    e_s = (d + 3) * U * s_abs
    t = e_s + e_s.gather(-1, imax) + (2 * x.abs() + C_EXP) * U
    e_p = p * (t + (p * t).sum(-1, keepdim=True) + (n + 3) * U)
    va, doa, ka, qa = v.abs(), do.abs(), k.abs(), q.abs()
    e_o = e_p @ va + n * U * (p @ va)
    e_dv = e_p.transpose(-1, -2) @ doa + n * U * (p.transpose(-1, -2) @ doa)
    e_dp = d * U * (doa @ va.transpose(-1, -2))
    e_rd = (e_dp * p + dp.abs() * e_p).sum(-1, keepdim=True) \
        + (n + 1) * U * (dp.abs() * p).sum(-1, keepdim=True)
    e_ds = e_p * (dp - rd).abs() + p * (e_dp + e_rd) \
        + 2 * U * p * (dp.abs() + rd.abs())
    dsa = ds.abs()
    e_dq = scale * (e_ds @ ka + (n + 1) * U * (dsa @ ka))
    e_dk = scale * (e_ds.transpose(-1, -2) @ qa
                    + (n + 1) * U * (dsa.transpose(-1, -2) @ qa))
    e_db = e_ds.sum(0) + bw * U * dsa.sum(0)
    return {"out": (o, _final(e_o, o, bf16)),
            "dq": (dq, _final(e_dq, dq, bf16)),
            "dk": (dk, _final(e_dk, dk, bf16)),
            "dv": (dv, _final(e_dv, dv, bf16)),
            "dbias": (db, _final(e_db))}


# ---------------------------------------------------------------------------
# patch-merge gather + LayerNorm (patch_merge.hip) through ops.patch_merge_ln
# ---------------------------------------------------------------------------

PATCH_CASES = [             # (B, H, W, C)
    (1, 2, 2, 1),           # 4C = 4: fewer channels than lanes
    (3, 2, 2, 48),          # small
    (2, 4, 6, 24),          # non-square
    (5, 4, 2, 40),          # 10 rows: three blocks, the last half full
    (1, 2, 2, 768),         # 4C = 3072, the limit
]
PATCH_OFFSET_CASE = (2, 4, 4, 96)      # x = 2^6 sigma + sigma randn
PATCH_OFFSET_SIGMA = 0.25
PATCH_DECLINED_C = 769                 # 4C > 3072: the wrapper returns None
PATCH_DTYPES = [torch.float32, torch.bfloat16]
PATCH_EPS = 1e-5


@dataclass
class PatchInputs:
    x: torch.Tensor         # [B, H W, C]
    gamma: torch.Tensor     # [4C] fp32
    beta: torch.Tensor
    dy: torch.Tensor        # [B, H W / 4, 4C]; on the grid i/2^3, |i| <= 8
    hw: Tuple[int, int]


def patch_inputs(case, dtype, offset: bool = False) -> PatchInputs:
    """dy is ALWAYS on the grid i/2^3 (|i| <= 8, exact in bf16), so that
    dbeta = sum_rows dy is exact in fp32 in any order and is compared bit
    for bit; nothing else in this kernel is sums of products only."""
    b, h, w, c = case
    g = _gen("patch", b, h, w, c, dtype == torch.bfloat16, offset)
    x = torch.randn(b, h * w, c, generator=g)
    if offset:
        x = PATCH_OFFSET_SIGMA * (2.0 ** 6 + x)
    return PatchInputs(
        x=x.to(dtype),
        gamma=1.0 + 0.5 * torch.randn(4 * c, generator=g),
        beta=torch.randn(4 * c, generator=g),
        dy=_randgrid((b, h * w // 4, 4 * c), 8, 2.0 ** -3, g).to(dtype),
        hw=(h, w))


def patch_gather(x: torch.Tensor, h: int, w: int,
                 order=(0, 1, 2, 3)) -> torch.Tensor:
    """[B, H W, C] -> [B, H W / 4, 4C] in the model's concat order
    [x(0::2, 0::2), x(1::2, 0::2), x(0::2, 1::2), x(1::2, 1::2)]."""
    b, _, c = x.shape
    xv = x.view(b, h, w, c)
    blocks = [xv[:, 0::2, 0::2], xv[:, 1::2, 0::2], xv[:, 0::2, 1::2],
              xv[:, 1::2, 1::2]]
    return torch.cat([blocks[i] for i in order], -1).reshape(
        b, h * w // 4, 4 * c)


def patch_scatter(dxc: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """the inverse of patch_gather for a gradient"""
    b, _, c4 = dxc.shape
    c = c4 // 4
    dx = torch.zeros(b, h, w, c, dtype=dxc.dtype)
    parts = dxc.view(b, h // 2, w // 2, 4, c)
    dx[:, 0::2, 0::2], dx[:, 1::2, 0::2] = parts[..., 0, :], parts[..., 1, :]
    dx[:, 0::2, 1::2], dx[:, 1::2, 1::2] = parts[..., 2, :], parts[..., 3, :]
    return dx.view(b, h * w, c)


def patch_merge_reference(inp: PatchInputs, order=(0, 1, 2, 3),
                          exact_dbeta: bool = True) -> Ref:
    """Float64 gather + LayerNorm over 4C and its backward (hand-written;
    test_rowops_oracle.py checks it against float64 autograd of
    F.layer_norm).  order != (0, 1, 2, 3) is the concat-order mutant.

    Row statistics.  The kernel gives one 64-lane wave to a row: a lane
    adds ceil(4C / 64) values, a 6-level butterfly adds the lanes, one
    division follows.  Each value passes through h = ceil(4C / 64) + 7
    roundings, so a row sum errs by at most h u sum |x|, for this kernel
    and for any other summation no deeper than that (torch's cascade sum
    and Welford are not).  This h replaces the term count n = 4C here and
    ONLY here: with n = 4C the mean's allowance, which grows with the
    row's offset as |mean|, would be as large as the error of a variance
    taken as E[x^2] - mean^2, and excuse it.
      e_mean = h u mean|x|
      e_var  = (h + 5) u var + e_mean^2 — the variance of CENTRED values:
               sum (x - m')^2 = sum (x - m)^2 + n (m' - m)^2 exactly, so a
               wrong centre enters squared; each centred value is rounded
               once and squared (3 u), then the sum and the division.
               No term carries sum x^2.
      e_rstd = rstd (e_var / (2 (var + eps)) + 4 u): rsqrtf to 1 ulp.
      e_xh   = rstd (e_mean + 2 u |x - mean|) + |x - mean| e_rstd
      e_y    = |gamma| e_xh + 2 u (|xh gamma| + |beta|)   (+ bf16 store)
    Backward, g = gamma dy, m1 = mean g, m2 = mean g xh:
      e_m1 = h u mean|g|,  e_m2 = mean(|g| e_xh) + (h + 2) u mean|g xh|
      e_dx = rstd (e_m1 + e_xh |m2| + |xh| e_m2 + 4 u (|g| + |m1| +
             |xh m2|)) + |dx| e_rstd / rstd                (+ bf16 store)
      e_dg = sum_rows |dy| e_xh + (R + 1) u sum_rows |dy xh|, R rows
      e_db = 0: dy is on a grid, the sum is exact (asserted)."""
    h_, w_ = inp.hw
    bf16 = inp.x.dtype == torch.bfloat16
    x = patch_gather(inp.x.double(), h_, w_, order)
    gamma, beta, dy = inp.gamma.double(), inp.beta.double(), inp.dy.double()
    n = x.shape[-1]
    rows = x.shape[0] * x.shape[1]
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = (var + PATCH_EPS).rsqrt()
    xh = c * rstd
    y = xh * gamma + beta
    g = gamma * dy
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    dxc = (g - m1 - xh * m2) * rstd
    dg = (dy * xh).sum((0, 1))
    db = dy.sum((0, 1))

    h = -(-n // 64) + 7
    e_mean = h * U * x.abs().mean(-1, keepdim=True)
    e_var = (h + 5) * U * var + e_mean ** 2
    e_rstd = rstd * (e_var / (2 * (var + PATCH_EPS)) + 4 * U)
    e_xh = rstd * (e_mean + 2 * U * c.abs()) + c.abs() * e_rstd
    e_y = gamma.abs() * e_xh + 2 * U * ((xh * gamma).abs() + beta.abs())
    e_m1 = h * U * g.abs().mean(-1, keepdim=True)
    e_m2 = (g.abs() * e_xh).mean(-1, keepdim=True) \
        + (h + 2) * U * (g * xh).abs().mean(-1, keepdim=True)
    e_dx = rstd * (e_m1 + e_xh * m2.abs() + xh.abs() * e_m2
                   + 4 * U * (g.abs() + m1.abs() + (xh * m2).abs())) \
        + dxc.abs() * e_rstd / rstd
    e_dg = (dy.abs() * e_xh).sum((0, 1)) \
        + (rows + 1) * U * (dy * xh).abs().sum((0, 1))
    if exact_dbeta:
        d8 = dy * 8
        assert torch.equal(d8, d8.round()) and float(d8.abs().max()) <= 8
        assert float(dy.abs().sum((0, 1)).max()) < 2.0 ** 20
    dx = patch_scatter(dxc, h_, w_)
    return {"y": (y, _final(e_y, y, bf16)),
            "dx": (dx, _final(patch_scatter(e_dx, h_, w_), dx, bf16)),
            "dgamma": (dg, _final(e_dg)),
            "dbeta": (db, torch.zeros_like(db))}


# ---------------------------------------------------------------------------
# row losses: ce_smooth (elementwise.hip), kd_fwd and icarl_distill (kd.hip)
# ---------------------------------------------------------------------------

ROWLOSS_B = [1, 3]
ROWLOSS_C = [1, 7, 255, 256, 257, 1000]
CE_CASES = [(b, c) for b in ROWLOSS_B for c in ROWLOSS_C]
CE_EPSILONS = [0.0, 0.1]
CE_SCALES = [1.0, 30.0]
CE_DTYPES = [torch.float32, torch.bfloat16]
KD_CASES = CE_CASES
KD_TEMPERATURES = [1.0, 4.0]
KD_SCALE = 30.0
ICARL_CASES = [(1, 1, 1), (3, 96, 1), (3, 96, 96), (2, 300, 40)]  # (B, C, P)
ICARL_LIMIT = 50.0


def row_targets(b: int, c: int) -> torch.Tensor:
    """the LAST column first, then column 0, then the middle"""
    return torch.tensor([c - 1, 0, c // 2][:b], dtype=torch.int64)


def ce_inputs(case, scale: float, dtype):
    b, c = case
    g = _gen("ce", b, c, int(scale), dtype == torch.bfloat16)
    return (scale * torch.randn(b, c, generator=g)).to(dtype), \
        row_targets(b, c)


def _softmax_errors(a: torch.Tensor, e_a: torch.Tensor):
    """For a row of scaled logits a (absolute error e_a) the kernels form
    m = max a, x = a - m, se = sum __expf(x), log se = __logf(se), p =
    __expf(x) / se.  Returns (x, p, log se, r, e_logse, e_p) with
      r       = e_a + e_a at the maximum + (2 |x| + C_EXP) u, the relative
                error of each exponential (subtraction rounding included);
      e_se    = sum_j p_j r_j + (C + 1) u relative: a weighted mean of the
                terms' errors, then the C-term sum;
      e_logse = e_se + (|log se| + C_LOG) u absolute;
      e_p     = p (r + e_se + 2 u): reciprocal and product."""
    c = a.shape[-1]
    m, im = a.max(-1, keepdim=True)
    x = a - m
    ex = x.exp()
    se = ex.sum(-1, keepdim=True)
    p = ex / se
    logse = se.log()
    r = e_a + e_a.gather(-1, im) + (2 * x.abs() + C_EXP) * U
    e_se = (p * r).sum(-1, keepdim=True) + (c + 1) * U
    e_logse = e_se + (logse.abs() + C_LOG) * U
    e_p = p * (r + e_se + 2 * U)
    return x, p, logse, r, e_logse, e_p


def ce_reference(score, target, epsilon: float, target_shift: int = 0) -> Ref:
    """Label-smoothed CE, mean over the batch, and its gradient (upstream
    1) in float64 on the values the kernel reads.  target_shift is the
    mutant.  With `_softmax_errors` on a = score (e_a = 0):
      log_z = log se + m: e_lz = e_logse + u |log_z|
      logp  = s - log_z:  e_lp = e_lz + u |logp|
      row   = sum_j t_j (-logp_j): sum t e_lp + (C + 3) u sum t |logp|
              (t = eps/C + (1 - eps)[j = y] is rounded twice)
      loss  = mean of B rows: mean e_row + (B + 1) u mean |row|
      grad  = (p - t) / B: (e_p + 3 u (p + t)) / B     (+ bf16 store)."""
    s = score.double()
    b, c = s.shape
    bf16 = score.dtype == torch.bfloat16
    eps = float(np.float32(epsilon))
    y = (target + target_shift) % c
    t = torch.full_like(s, eps / c)
    t[torch.arange(b), y] += 1.0 - eps
    x, p, logse, r, e_logse, e_p = _softmax_errors(s, torch.zeros_like(s))
    log_z = logse + s.max(-1, keepdim=True)[0]
    logp = s - log_z
    row = (t * -logp).sum(-1)
    loss = row.mean()
    grad = (p - t) / b
    e_lp = e_logse + U * log_z.abs() + U * logp.abs()
    e_row = (t * e_lp).sum(-1) + (c + 3) * U * (t * logp.abs()).sum(-1)
    e_loss = e_row.mean() + (b + 1) * U * row.abs().mean()
    e_grad = (e_p + 3 * U * (p + t)) / b
    return {"loss": (loss, _final(e_loss)),
            "grad": (grad, _final(e_grad, grad, bf16))}


def kd_inputs(case, dtype=torch.float32):
    b, c = case
    g = _gen("kd", b, c, dtype == torch.bfloat16)
    return ((KD_SCALE * torch.randn(b, c, generator=g)).to(dtype),
            (KD_SCALE * torch.randn(b, c, generator=g)).to(dtype))


def kd_reference(zs, zt, temperature: float, grad_factor_t: bool = True
                 ) -> Ref:
    """Temperature-softmax KL distillation (reference.kd_loss) and its
    student gradient in float64.  grad_factor_t=False is the mutant whose
    gradient lacks the factor T.

    a = z (1/T): 2 u |a| (the reciprocal and the product).  With
    `_softmax_errors` on both rows, lt = x_t, ls = x_s:
      delta = (lt - log se_t) - (ls - log se_s):
              e_delta = sum over both of (e_x + e_logse + u |x| + u |x -
              log se|) + u |delta|, e_x = r - (2 |x| + C_EXP) u + u |x|
      row   = sum_j p_t delta: sum (e_pt |delta| + p_t e_delta)
              + (C + 1) u sum p_t |delta|
      loss  = (T^2 / B) sum rows: + (B + 3) u |loss|
      grad  = (T / B)(p_s - p_t): (T / B)(e_ps + e_pt + 3 u (p_s + p_t))
              (+ bf16 store when the logits are bf16)."""
    s, t = zs.double(), zt.double()
    b, c = s.shape
    bf16 = zs.dtype == torch.bfloat16
    inv_t = float(np.float32(1.0 / temperature))
    temp = float(np.float32(temperature))
    a_s, a_t = s * inv_t, t * inv_t
    xs, ps, lse_s, r_s, el_s, e_ps = _softmax_errors(a_s, 2 * U * a_s.abs())
    xt, pt, lse_t, r_t, el_t, e_pt = _softmax_errors(a_t, 2 * U * a_t.abs())
    delta = (xt - lse_t) - (xs - lse_s)
    row = (pt * delta).sum(-1)
    loss = row.sum() * (temp * temp / b)
    grad = (temp if grad_factor_t else 1.0) / b * (ps - pt)
    e_delta = U * delta.abs()
    for x, r, lse, el in ((xs, r_s, lse_s, el_s), (xt, r_t, lse_t, el_t)):
        e_x = r - (2 * x.abs() + C_EXP) * U + U * x.abs()
        e_delta = e_delta + e_x + el + U * x.abs() + U * (x - lse).abs()
    e_row = (e_pt * delta.abs() + pt * e_delta).sum(-1) \
        + (c + 1) * U * (pt * delta.abs()).sum(-1)
    e_loss = e_row.sum() * (temp * temp / b) + (b + 3) * U * loss.abs()
    e_grad = temp / b * (e_ps + e_pt + 3 * U * (ps + pt))
    return {"loss": (loss, _final(e_loss)),
            "grad": (grad, _final(e_grad, grad, bf16))}


def icarl_inputs(case):
    """score and prev uniform in [-50, 50]; every target is the LAST
    column."""
    b, c, p = case
    g = _gen("icarl", b, c, p)
    score = (torch.rand(b, c, generator=g) * 2 - 1) * ICARL_LIMIT
    prev = (torch.rand(b, p, generator=g) * 2 - 1) * ICARL_LIMIT
    return score, torch.full((b,), c - 1, dtype=torch.int64), prev


def icarl_reference(score, target, prev) -> Ref:
    """mean_{b,c} bce(x, onehot) + mean_{b,c<P} bce(x, sigmoid(prev)) and
    its gradient in float64; bce(x, y) = max(x, 0) - x y + log1p(e^-|x|).

      sigmoid(z) = 1 / (1 + __expf(-z)): (|z| + C_EXP + 2) u relative.
      bce: e = |x| y (e_y + u) + l (|x| + C_EXP + 4) u + 3 u (max(x, 0) +
           |x y| + l), l = log1p(e^-|x|) (log1pf to 2 ulp; d log1p <= 1);
      a row sums C (or P) of them: + (C + 1) u sum |bce|; the two means
      and their sum: 4 u more; the B rows: + (B + 1) u |loss|.
      grad = (sig x - y) / (B C) + [c < P] (sig x - yt) / (B P):
           each part sig x e_sig + yt e_yt + 3 u (sig x + y)."""
    x, pv = score.double(), prev.double()
    b, c = x.shape
    npv = pv.shape[1]
    onehot = F.one_hot(target, c).double()
    yt = torch.sigmoid(pv)
    sig = torch.sigmoid(x)
    e_sig = sig * (x.abs() + C_EXP + 2) * U
    e_yt = yt * (pv.abs() + C_EXP + 2) * U

    def bce(xx, y, e_y):
        lg = torch.log1p(torch.exp(-xx.abs()))
        val = xx.clamp_min(0) - xx * y + lg
        e = xx.abs() * (y * U + e_y) + lg * (xx.abs() + C_EXP + 4) * U \
            + 3 * U * (xx.clamp_min(0) + (xx * y).abs() + lg)
        n = xx.shape[1]
        return val.sum(-1), e.sum(-1) + (n + 1) * U * val.abs().sum(-1)

    clf, e_clf = bce(x, onehot, torch.zeros_like(x))
    dis, e_dis = bce(x[:, :npv], yt, e_yt)
    row = clf / (b * c) + dis / (b * npv)
    loss = row.sum()
    e_loss = (e_clf / (b * c) + e_dis / (b * npv)).sum() \
        + 4 * U * row.abs().sum() + (b + 1) * U * loss.abs()
    grad = (sig - onehot) / (b * c)
    e_grad = (e_sig + 3 * U * (sig + onehot)) / (b * c)
    grad[:, :npv] += (sig[:, :npv] - yt) / (b * npv)
    e_grad[:, :npv] += (e_sig[:, :npv] + e_yt
                        + 3 * U * (sig[:, :npv] + yt)) / (b * npv)
    e_grad = e_grad + U * grad.abs()
    return {"loss": (loss, _final(e_loss)), "grad": (grad, _final(e_grad))}


# ---------------------------------------------------------------------------
# references computed once and shared; callers must not modify them
# ---------------------------------------------------------------------------

_CACHE: dict = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]
