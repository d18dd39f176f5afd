"""Cases for the forward sweep over feature magnitude and dynamic range, and their CPU references.

Every convolution of the forward sweep is a split-fp16 MFMA whose operands are staged as fp16
hi + lo at a power-of-two scale taken from a bound, not from the data ("Staging
scales"): cell 0's cost slice x and the omega conv's sq from one number per sweep, 8 max|f|^2 over
every view; cells 3 and 4's GroupNorm+ReLU part from |gamma| sqrt(n - 1) + |beta|; the weights from
a per-tensor exponent.  Every other forward test feeds N(0,1) features (two go to x100 features and
x1e5 GroupNorm affines).  The cases here move what that leaves fixed, on one small frame
(synthetic.scene(1, 3, 32, 48, 3, seed=5): several omega tiles) with the real weights:

* the features' scale, x 2^k for k = -60 .. +20 (at -56 and -60 the bound is below the 2^-100
  clamp of the exponent), x 2^-80 (8 max|f|^2 is 0 in fp32) and exact zeros in every view, in one
  source view, in the reference view;
* the dynamic range inside a frame: one element set to R = 30, 300, 3000 in a source view, 300 in
  the reference view, a whole source view x 10.  The scale is global, so the outlier raises it
  for every pixel and the lo parts of ordinary pixels drop into fp16's subnormals;
* both deconvs' GroupNorm affine x 2^-40 and exactly 0 (a non-positive bound: exponent 0);
* every cell and deconv conv weight x 2^-8 and x 2^+2 (non-default per-tensor exponents; the
  biases stay).

A case belongs here only while the float32 oracle itself agrees with float64 at the parity
tolerance; that is what removed a whole view x 300 / x 100 and the weights x 2^+8 / 2^+4 (see the
comments in CASES).

``references(case)`` holds three CPU runs of the oracle, computed once per process and never
modified: ``ref64`` (float64), ``ref32`` (float32, the reference's arithmetic) and ``stage64``:
float64 with the documented staging applied at the two points that take the feature bound, v ->
(fp16(s) + fp16(s - fp16(s))) 2^e with s = v 2^-e.  It models the design and uses no output of the
library.  tests/test_fwd_range_cases.py asserts on the CPU what keeps the GPU test honest;
tests/test_gpu_fwd_range.py runs the library against the references.
"""
from __future__ import annotations

import functools
import math
import os
from typing import Callable, NamedTuple

import numpy as np
import torch

from aarmvs import synthetic as syn

SHAPE = (1, 3, 32, 48, 3)   # B, N, H, W, D
SEED = 5
TOL = 1e-4                  # the parity tolerance on cost: atol = rtol
OUTLIER = (0, 3, 5, 7)      # (batch, channel, y, x) of the one-element outliers
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CELL_W = tuple(f"cost_regularization.cell_list.{i}.conv.weight" for i in range(5))
DECONV_W = tuple(f"cost_regularization.deconv_{j}.conv.weight" for j in range(2))
DECONV_GN = tuple(f"cost_regularization.deconv_{j}.gn.{t}" for j in range(2) for t in ("weight", "bias"))


def _same(t):
    return t


def _scaled(k):
    return lambda f: f * 2.0 ** k   # a power of two: exact (or flushed, at -80 in the products)


def _zero_views(*views):
    def fn(f):
        f = f.clone()
        for v in views:
            f[v] = 0.0
        return f
    return fn


def _element(view, R):
    def fn(f):
        f = f.clone()
        f[(view,) + OUTLIER] = R
        return f
    return fn


def _view_times(view, s):
    def fn(f):
        f = f.clone()
        f[view] *= s
        return f
    return fn


def _params_times(keys, s):
    return lambda P: {k: (v * s if k in keys else v) for k, v in P.items()}


class Case(NamedTuple):
    name: str
    kind: str                  # "scale" | "zero" | "outlier" | "gn" | "weight"
    feat: Callable = _same     # features [N,B,32,H,W] -> features
    par: Callable = _same      # {param: tensor} -> {param: tensor}
    k: int | None = None       # scale cases: the features are the base frame's x 2^k
    factor: float | None = None   # outlier cases: the outlier's stated size
    beyond: bool = False       # beyond the cliff: the documented staging itself loses the tolerance


SCALE_KS = (-60, -56, -40, -20, -8, 8, 20)
BASE = Case("scale+0", "scale", k=0)   # the unmodified frame: a reference, not in CASES

CASES = tuple(Case(f"scale{k:+d}", "scale", _scaled(k), k=k) for k in SCALE_KS) + (
    Case("zero_all", "zero", _zero_views(0, 1, 2)),
    Case("zero_src", "zero", _zero_views(1)),
    Case("zero_ref", "zero", _zero_views(0)),
    Case("flush", "zero", _scaled(-80), k=-80),
    Case("outlier_src30", "outlier", _element(1, 30.0), factor=30.0),
    Case("outlier_src300", "outlier", _element(1, 300.0), factor=300.0),
    Case("outlier_src3000", "outlier", _element(1, 3000.0), factor=3000.0, beyond=True),
    Case("outlier_ref300", "outlier", _element(0, 300.0), factor=300.0),
    # source view 2 x 10, not x 300: at x 300 the staging model loses 3.3e-5 on cost (over a quarter
    # of TOL) and at x 100 the float32 oracle itself is 4.7e-3 off float64 (the regulariser
    # amplifies its rounding); x 10 is the largest power of ten at which both hold (3.7e-6)
    Case("view_x10", "outlier", _view_times(2, 10.0), factor=10.0),
    Case("gn_tiny", "gn", par=_params_times(DECONV_GN, 2.0 ** -40)),
    Case("gn_zero", "gn", par=_params_times(DECONV_GN, 0.0)),
    # x 2^-8: the cells' exponents reach the +20 clamp (max|w| 1.0 .. 3.9 -> e = 20, 20, 20, 20, 20
    # from 12, 13, 13, 13, 13), the deconvs' unclamped pack goes from 15 to 23
    Case("weights-8", "weight", par=_params_times(CELL_W + DECONV_W, 2.0 ** -8)),
    # x 2^+2, not x 2^+8: at x 2^8 (and 2^4) the float32 oracle is 1.8 (4.0e-2) off float64 on
    # cost, out of the reference's own range; x 2^2 is within it (4.6e-4 where |cost| ~ 40)
    Case("weights+2", "weight", par=_params_times(CELL_W + DECONV_W, 2.0 ** 2)),
)

BY_NAME = {c.name: c for c in CASES + (BASE,)}
NAMES = tuple(c.name for c in CASES)


@functools.lru_cache(maxsize=None)
def _frame():
    sc = syn.scene(*SHAPE, seed=SEED)
    g = np.load(os.path.join(GOLDEN, "real_weights_sweep.npz"), allow_pickle=False)
    P = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    return (torch.from_numpy(sc["features"]), torch.from_numpy(sc["proj_matrices"]),
            torch.from_numpy(sc["depth_values"]), P)


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """(features [N,B,32,H,W], proj [B,N,4,4], depth_values [B,D], {param: tensor}) of a case,
    float32.  Shared, never modified."""
    feats, proj, dv, P = _frame()
    return case.feat(feats), proj, dv, case.par(P)


def views(feats, proj):
    N = feats.shape[0]
    return feats[0], [feats[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)]


# ----------------------------------------------------------------------------------
# the documented staging ("Staging scales")
# ----------------------------------------------------------------------------------
def feature_bound(feats: torch.Tensor) -> float:
    """8 max|f|^2 over every view in fp32 arithmetic (the sweep's one number)."""
    m = feats.float().abs().max()
    return float(torch.tensor(8.0) * m * m)


def guard_exp(bound: float) -> int:
    """e with bound 2^-e in [2^14, 2^15); held at -114 for bound < 2^-100 and at 120 for bound >=
    2^134 (so that 2^-e and the rescale 2^(e+12) stay finite fp32 numbers); 0 for no bound."""
    if not bound > 0.0:
        return 0
    k = math.frexp(bound)[1] - 1   # 2^k <= bound < 2^(k+1)
    return 120 if k >= 134 else (-114 if k < -100 else k - 14)


def omega_exp(bound: float) -> int:
    """The omega conv's sq: bound 2^-e in [2^13, 2^15), e even."""
    e = guard_exp(bound)
    return e + (e & 1)


def split_fp16(v: torch.Tensor, e: int) -> torch.Tensor:
    """(fp16(s) + fp16(s - fp16(s))) 2^e with s = v 2^-e, in float64 around the two fp16
    roundings (gradual underflow, as the hardware's conversions)."""
    s = v.double() * 2.0 ** -e
    hi = s.to(torch.float16).double()
    lo = (s - hi).to(torch.float16).double()
    return (hi + lo) * 2.0 ** e


def staging(bound: float) -> dict:
    """oracle.sweep's ``stage`` for a sweep whose feature bound is ``bound``."""
    ex, eo = guard_exp(bound), omega_exp(bound)
    return {"x": lambda x: split_fp16(x, ex), "sq": lambda sq: split_fp16(sq, eo)}


# ----------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------
class References(NamedTuple):
    ref64: dict      # oracle.sweep's cost [B,D,H,W], depth, conf [B,H,W] in float64
    ref32: dict      # ... in float32
    stage64: dict    # ... in float64 with the documented staging of x and sq
    x0: torch.Tensor  # ref64's cost slice of plane 0 [B,32,H,W] (float64)


@functools.lru_cache(maxsize=None)
def references(case: Case) -> References:
    from oracle import sweep_oracle as orc
    feats, proj, dv, P = inputs(case)
    args = views(feats, proj)
    xs = []

    def keep(x):
        xs.append(x)
        return x

    pick = lambda out: {k: out[k] for k in ("cost", "depth", "conf")}   # noqa: E731
    r64 = orc.sweep(*args, dv, P, fast=True, dtype=torch.float64, stage={"x": keep})
    r32 = orc.sweep(*args, dv, P, fast=True)
    st = orc.sweep(*args, dv, P, fast=True, dtype=torch.float64, stage=staging(feature_bound(feats)))
    return References(pick(r64), pick(r32), pick(st), xs[0])


class SliceReference(NamedTuple):
    x: torch.Tensor        # float64 cost slice [B,32,H,W] of the plane
    omega: torch.Tensor    # float64 omega weights [nsrc,B,H,W]
    x_loss: float          # max |x with sq staged for the omega conv - x|
    omega_loss: float      # max |omega of the staged sq - omega|
    x32_rl2: float         # the float32 oracle's slice: relative L2 error against x


@functools.lru_cache(maxsize=None)
def slice_reference(case: Case, plane: int) -> SliceReference:
    """float64 orc.cost_slice / omega_weight of one plane, and the documented sq staging's loss."""
    from oracle import sweep_oracle as orc
    feats, proj, dv, P = inputs(case)
    ref, srcs, rp, sps = views(feats.double(), proj)
    P64 = {k: v.double() for k, v in P.items()}
    rels = [orc.relative_projection(sp, rp) for sp in sps]
    dep = dv[:, plane]
    eo = omega_exp(feature_bound(feats))
    with torch.no_grad():
        x = orc.cost_slice(ref, srcs, rels, dep, P64, fast=True)
        xs = orc.cost_slice(ref, srcs, rels, dep, P64, fast=True, stage_sq=lambda sq: split_fp16(sq, eo))
        sqs = [(orc.homo_warp(s, r, dep, fast=True) - ref).pow(2) for s, r in zip(srcs, rels)]
        om = torch.stack([orc.omega_weight(sq, P64, fast=True) for sq in sqs]).squeeze(2)
        oms = torch.stack([orc.omega_weight(split_fp16(sq, eo), P64, fast=True) for sq in sqs]).squeeze(2)
        x32 = orc.cost_slice(*views(feats, proj)[:2], rels, dep, P, fast=True)
    return SliceReference(x, om, float((xs - x).abs().max()), float((oms - om).abs().max()), rel_l2(x32, x))


PIXEL = (0, slice(None), 5, 7)   # the pixel (every channel) of the standalone step's x that is scaled
PIXEL_FACTORS = (1e3, 1e5, 1e7)


@functools.lru_cache(maxsize=None)
def step_reference(factor: float):
    """(x float32 [B,32,H,W], float64 orc.unet_step cost [B,1,H,W], max |cost with x staged at the
    scale of max|x| - cost|): the base frame's plane-0 slice with one pixel x ``factor``, through
    one step from the zero state.  The standalone step takes max|x| itself as the bound."""
    from oracle import sweep_oracle as orc
    _, _, _, P = inputs(BASE)
    P64 = {k: v.double() for k, v in P.items()}
    x = references(BASE).x0.float().clone()
    x[PIXEL] *= factor
    B, _, H, W = x.shape
    state = [(h.double(), c.double()) for h, c in orc.init_state(B, H, W)]
    with torch.no_grad():
        c64, _ = orc.unet_step(x.double(), state, P64, fast=True)
        cst, _ = orc.unet_step(split_fp16(x, guard_exp(float(x.abs().max()))), state, P64, fast=True)
    return x, c64, float((cst - c64).abs().max())


class GradReference(NamedTuple):
    g64: tuple     # test_gpu_bptt._oracle_grads' (prob, dL/dfeatures, {param: grad}, [dL/dx_d]), float64
    e32: dict      # float32 autograd's relative L2 error per tensor (test_gpu_bptt._f32_spread)


@functools.lru_cache(maxsize=None)
def grad_reference(case: Case) -> GradReference:
    """float64 autograd of the oracle under L = sum(cost) (dL/dcost = 1 everywhere) and float32
    autograd's own error against it, as tests/bptt_range_cases.py builds them."""
    from test_gpu_bptt import _f32_spread, _oracle_grads
    feats, proj, dv, P = inputs(case)
    B, N, H, W, D = SHAPE
    R = torch.ones(B, D, H, W)
    g64 = _oracle_grads(feats, proj, dv, P, R, torch.float64, "linear")
    return GradReference(g64, _f32_spread(feats, proj, dv, P, R, g64, "linear"))


def max_abs(a, ref) -> float:
    return float((torch.as_tensor(a).double() - torch.as_tensor(ref).double()).abs().max())


def rel_l2(a, ref) -> float:
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def within(a, ref, atol=TOL, rtol=TOL) -> bool:
    """numpy.testing.assert_allclose's criterion |a - ref| <= atol + rtol |ref| everywhere."""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return bool(((a - ref).abs() <= atol + rtol * ref.abs()).all())
