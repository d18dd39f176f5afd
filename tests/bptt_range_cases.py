"""Cases for the training backward over gradient range and argument limits, and their CPU
references (float64 autograd of the oracle, float32 autograd's own error against it).

Every backward test elsewhere feeds the cotangent of a loss on softmax(cost): it sums to zero over
D at every pixel, is dense and has about one size on every plane.  The cases here move what that
leaves fixed:

* the argument limits (softmax loss): one and sixteen source views, the 4x4 minimum frame, a
  4x132 strip, a frame that is no multiple of any backward tile, a batch of three;
* the plane count (linear loss L = sum(R * cost), dL/dcost = R exactly): D = 1 and D = 17 (one
  whole 16-plane group plus one plane);
* the cotangent's shape (linear loss, D = 34: groups of 16 + 16 + 2 planes): a vanishing
  gradient on the last or the first groups, a single plane, two pixels, all zero;
* the cotangent's scale (softmax loss): R * 2^k, k = -96 .. +96, against the k = 0 reference
  scaled by 2^k (float64 and float32 autograd are exactly scale-invariant there).

``reference(case)`` and ``f32_spread(case)`` are computed once per process and never modified.
tests/test_bptt_range_cases.py asserts on the CPU what keeps the GPU test honest; tests/
test_gpu_bptt_range.py runs the library against them.
"""
from __future__ import annotations

import functools
from typing import Callable, NamedTuple

import numpy as np
import torch

from aarmvs import synthetic as syn

PLANES = 16          # bptt.hip kPlaneGroup: groups start at multiples of 16 planes
TINY = 2.0 ** -112   # on R; the unscaled max |dL/dz| is 2^-2 .. 2^-11 per cell (measured)
GZ_TINY = 2.0 ** -113   # below it an unclamped 2^(14 - ilogb(max)) overflows float32
R_SEED = 5
W_SEED = 6


def _same(R):
    return R


def _tail_tiny(R):
    R = R.clone()
    R[:, PLANES:] *= TINY
    return R


def _head_tiny(R):
    R = R.clone()
    R[:, :PLANES] *= TINY
    return R


def _one_plane(R):
    out = torch.zeros_like(R)
    out[:, 20] = R[:, 20]
    return out


def _sparse(R):
    out = torch.zeros_like(R)
    for y, x in ((0, 0), (5, 7)):
        out[:, :, y, x] = R[:, :, y, x]
    return out


def _zero(R):
    return torch.zeros_like(R)


class Case(NamedTuple):
    name: str
    shape: tuple            # (B, N, H, W, D)
    loss: str               # "softmax" | "linear"
    cot: Callable = _same   # R -> R'
    seed: int | None = None  # scene seed; None: H * 1000 + W + N
    k: int = 0              # the cotangent is cot(R) * 2^k; the reference is the k = 0 one * 2^k
    tiny_groups: tuple = ()  # plane groups whose max |dL/dz| must be below GZ_TINY in every cell
    zero_groups: tuple = ()  # plane groups whose dL/dz must be exactly 0 in every cell


SCALE_SHAPE = (1, 3, 16, 24, 3)
SCALE_BASE = Case("scale_k0", SCALE_SHAPE, "softmax", seed=11)   # reference only, not in CASES
SCALE_KS = (-96, -48, 48, 96)

CASES = (
    # argument limits
    Case("nsrc1", (1, 2, 16, 24, 3), "softmax"),
    Case("nsrc16", (1, 17, 16, 24, 3), "softmax"),
    Case("min", (1, 3, 4, 4, 2), "softmax"),
    Case("strip", (1, 3, 4, 132, 3), "softmax"),
    Case("ragged", (1, 3, 52, 84, 3), "softmax"),
    Case("batch3", (3, 3, 8, 12, 2), "softmax"),
    # plane counts
    Case("d1", (1, 3, 8, 12, 1), "linear"),
    Case("d17", (1, 3, 8, 12, 17), "linear"),
    # cotangent shape: three groups of 16 + 16 + 2 planes
    Case("tail_tiny", (1, 3, 8, 12, 34), "linear", _tail_tiny, tiny_groups=(1, 2)),
    Case("head_tiny", (1, 3, 8, 12, 34), "linear", _head_tiny),
    Case("one_plane", (1, 3, 8, 12, 34), "linear", _one_plane, zero_groups=(2,)),
    Case("sparse", (1, 3, 8, 12, 34), "linear", _sparse),
    Case("zero", (1, 3, 8, 12, 34), "linear", _zero),
) + tuple(Case(f"scale{k:+d}", SCALE_SHAPE, "softmax", seed=11, k=k) for k in SCALE_KS)

BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """(features [N,B,32,H,W], proj [B,N,4,4], depth_values [B,D], {param: tensor}, R' [B,D,H,W])
    of a case, R' = cot(randn) * 2^k in float32 (a power of two: exact).  Shared, never modified."""
    B, N, H, W, D = case.shape
    sc = syn.scene(B, N, H, W, D, seed=H * 1000 + W + N if case.seed is None else case.seed)
    P = {k: torch.from_numpy(v) for k, v in syn.sweep_weights(W_SEED).items()}
    R = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(R_SEED))
    Rp = case.cot(R) * 2.0 ** case.k
    return (torch.from_numpy(sc["features"]), torch.from_numpy(sc["proj_matrices"]),
            torch.from_numpy(sc["depth_values"]), P, Rp)


class Reference(NamedTuple):
    g64: tuple          # _oracle_grads' (prob, dL/dfeatures, {param: grad}, [dL/dx_d]) in float64
    cost: torch.Tensor  # float64 raw cost volume [B,D,H,W]
    tsum: float         # sum |dL/d omega logit|: the terms of omega.reweight_network.2.bias
    gzmax: np.ndarray   # [5 cells][D] max |dL/dz| (gate pre-activation gradients)


def _scaled(ref: Reference, s: float) -> Reference:
    prob, gf, gp, gx = ref.g64
    return Reference((prob, gf * s, {k: v * s for k, v in gp.items()}, [g * s for g in gx]),
                     ref.cost, ref.tsum * s, ref.gzmax * s)


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> Reference:
    """float64 autograd of the oracle on the case's inputs, one run per process.  A scale case
    (k != 0) takes the k = 0 run's gradients times 2^k (exact in float64)."""
    from oracle import sweep_oracle as orc
    from test_gpu_bptt import _oracle_grads
    if case.k != 0:
        assert case._replace(name=SCALE_BASE.name, k=0) == SCALE_BASE
        return _scaled(reference(SCALE_BASE), 2.0 ** case.k)
    feats, proj, dv, P, Rp = inputs(case)
    D = case.shape[4]
    tsum = [0.0]
    gz = np.zeros((5, D))
    calls = [0]

    def gate_hook(z):   # call n: cell n % 5 of plane n // 5 (oracle.unet_step's order)
        n = calls[0]
        calls[0] += 1
        z.register_hook(lambda g: gz.__setitem__((n % 5, n // 5), float(g.abs().max())))

    orc.LOGIT_HOOK = lambda z: z.register_hook(lambda g: tsum.__setitem__(0, tsum[0] + float(g.abs().sum())))
    orc.GATE_HOOK = gate_hook
    keep = {}
    try:
        g64 = _oracle_grads(feats, proj, dv, P, Rp, torch.float64, case.loss, keep)
    finally:
        orc.LOGIT_HOOK = None
        orc.GATE_HOOK = None
    assert calls[0] == 5 * D
    return Reference(g64, keep["cost"], tsum[0], gz)


@functools.lru_cache(maxsize=None)
def f32_spread(case: Case) -> dict:
    """{tensor: float32 CPU autograd's relative L2 error against float64 for the case's own
    cotangent, max over test_gpu_bptt.F32_THREADS}."""
    from test_gpu_bptt import _f32_spread
    feats, proj, dv, P, Rp = inputs(case)
    return _f32_spread(feats, proj, dv, P, Rp, reference(case).g64, case.loss)


def group_planes(group: int, D: int) -> slice:
    return slice(group * PLANES, min((group + 1) * PLANES, D))
