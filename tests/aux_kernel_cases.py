"""Cases for the three small training-side kernel families -- GroupNorm (csrc/group_norm.hip),
the ConvLSTM gate math (csrc/lstm_train.hip) and the deformable sampling backward (csrc/
deform.hip) -- with their float64 CPU references and float32 CPU torch's own error against them.

The references are plain float64 on the CPU: F.group_norm, the module.py:83-90 gate formula
(test_gpu_lstm_gates._torch_gates) and test_deform_conv.planar_val, each under float64 autograd.

Error measure of one compared tensor t of a case:

    m(t) = max over elements |got - ref64| / (|ref64| + s_t)

s_t is the RMS, in float64, of the *uncancelled* magnitude of that output (``scales``): |x a| +
|mean a| + |beta| for the group-norm y, |gamma dy rstd| for dx, the per-channel sum |dy xhat| /
sum |dy| for dgamma / dbeta, |f c_prev| + |i g| for the gates' h and c, (|dc| + |dh o (1 - tc^2)|)
max(1, |c_prev|) for the gate gradients, the sum of absolute corner terms for the deform outputs.
Where that magnitude is zero over the whole tensor s_t = 1 and the result must be exactly 0.

Bound: max(FLOOR * kappa, 3 * m_f32).  FLOOR = 16 * 2^-24 (the longest chain of float32 roundings
on these paths is 11 operations, rounded up), m_f32 is the same measure for float32 CPU torch on
the case (the factor 3 is test_gpu_deform.py's), kappa = 1 + max_g |mean_g| rstd_g for group norm
(the kernels keep the mean in float32: one rounding of it moves every xhat by 2^-24 |mean| rstd,
which is conditioning) and 1 elsewhere.  The collision case's gx has its own bound, N 2^-24 sum
|terms|: the worst case of a float32 sum of N terms in any order.  Elsewhere gx (an atomic sum
too) keeps the common bound: the offset patterns leave a pixel a few dozen terms at the most, and
``df_gx_order_spread`` sums them in random orders on the CPU to show that the order is not what
decides the GPU test.

``*_inputs``, ``*_reference`` and ``*_f32`` are computed once per process and never modified.
tests/test_aux_kernel_cases.py asserts on the CPU what keeps the GPU test honest; tests/
test_gpu_aux_kernels.py runs the library against the references.
"""
from __future__ import annotations

import functools
import itertools
import math
import zlib
from typing import NamedTuple

import torch
import torch.nn.functional as F

FLOOR = 16 * 2.0 ** -24
F32_FACTOR = 3.0
EPS = 1e-5


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def rms(t: torch.Tensor) -> float:
    """RMS over the finite elements; 0.0 for none."""
    t = t.double().reshape(-1)
    t = t[torch.isfinite(t)]
    return float(t.square().mean().sqrt()) if t.numel() else 0.0


def scale_of(mag: torch.Tensor) -> float:
    """s_t of a tensor's uncancelled magnitude: its RMS, or 1 where it is zero."""
    s = rms(mag)
    return s if s > 0.0 else 1.0


def measure(got: torch.Tensor, ref: torch.Tensor, s: float) -> float:
    """m(t) over the elements where the float64 reference is finite."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    ok = torch.isfinite(ref)
    if not bool(ok.any()):
        return 0.0
    e = (got[ok] - ref[ok]).abs() / (ref[ok].abs() + s)
    return float(e.nan_to_num(nan=math.inf).max())   # a non-finite result against a finite reference


def bound(m_f32: float, kappa: float = 1.0) -> float:
    return max(FLOOR * kappa, F32_FACTOR * m_f32)


# ---------------------------------------------------------------------------------------------
# group norm
# ---------------------------------------------------------------------------------------------
GN_SPAN = 4096      # group_norm.hip kGnSpan: elements of a channel plane per partial block
GN_THREADS = 256    # group_norm.hip kGnThreads: the stats kernels stride their partials by it
GN_DATA_SHAPE = (2, 8, 13, 17)


class GnCase(NamedTuple):
    name: str
    shape: tuple           # (B, C, *spatial)
    G: int
    affine: str = "wb"     # "wb" | "none" | "w" | "b"
    data: str = "randn"    # the distribution of x
    gy: str = "randn"      # the cotangent
    layout: str = ""       # "" | "x": x is a permuted view | "gy": gy is a permuted view
    repeat: bool = False   # also assert run-to-run bit identity


GN_CASES = tuple(
    GnCase(f"hw{hw}", (2, 4, 1, hw), 2, repeat=hw == 4097) for hw in (1, 255, 4095, 4096, 4097, 8193)
) + (
    GnCase("cg1", (2, 6, 5, 7), 6),
    GnCase("g1_c130", (1, 130, 1, 4097), 1),
    GnCase("plane1024x1025", (1, 1, 1024, 1025), 1, repeat=True),
    GnCase("affine_wb", GN_DATA_SHAPE, 2, "wb"),
    GnCase("affine_none", GN_DATA_SHAPE, 2, "none"),
    GnCase("affine_w", GN_DATA_SHAPE, 2, "w"),
    GnCase("affine_b", GN_DATA_SHAPE, 2, "b"),
    GnCase("nd5", (1, 4, 3, 5, 7), 2),
    GnCase("noncontig_x", GN_DATA_SHAPE, 2, layout="x"),
    GnCase("noncontig_gy", GN_DATA_SHAPE, 2, layout="gy"),
    GnCase("mean100", GN_DATA_SHAPE, 2, data="mean100"),
    GnCase("mean1000", GN_DATA_SHAPE, 2, data="mean1000"),
    GnCase("std1e-4", GN_DATA_SHAPE, 2, data="std1e-4"),
    GnCase("std1e18", GN_DATA_SHAPE, 2, data="std1e18"),
    GnCase("std1e-20", GN_DATA_SHAPE, 2, data="std1e-20"),
    GnCase("const_groups", GN_DATA_SHAPE, 2, data="const_groups"),
    GnCase("const_one_group", GN_DATA_SHAPE, 2, data="const_one_group"),
    GnCase("gy_zero", GN_DATA_SHAPE, 2, gy="zero"),
    GnCase("gy_const", GN_DATA_SHAPE, 2, gy="const"),
)
GN_BY_NAME = {c.name: c for c in GN_CASES}
GN_MEAN_STD = {"randn": (0.3, 2.0), "mean100": (100.0, 1.0), "mean1000": (1000.0, 1.0),
               "std1e-4": (0.0, 1e-4), "std1e18": (0.0, 1e18), "std1e-20": (0.0, 1e-20)}
GN_TENSORS = ("y", "dx", "dgamma", "dbeta")


def gn_hw(case: GnCase) -> int:
    return math.prod(case.shape[2:])


def gn_nb(case: GnCase) -> int:
    """Partial blocks per channel plane (group_norm.hip gn_nb)."""
    return -(-gn_hw(case) // GN_SPAN)


def _permuted(t: torch.Tensor) -> torch.Tensor:
    """The same values as a channels-last (non-contiguous) view."""
    v = t.permute(0, *range(2, t.dim()), 1).contiguous().permute(0, t.dim() - 1, *range(1, t.dim() - 1))
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


@functools.lru_cache(maxsize=None)
def gn_inputs(case: GnCase):
    """(x, weight | None, bias | None, gy) in float32."""
    g = _gen("gn:" + case.name)
    B, C = case.shape[:2]
    cg = C // case.G
    if case.data in GN_MEAN_STD:
        mean, std = GN_MEAN_STD[case.data]
        x = torch.randn(case.shape, generator=g, dtype=torch.float64) * std + mean
    else:
        x = torch.randn(case.shape, generator=g, dtype=torch.float64) * 2.0 + 0.3
        xg = x.view(B, case.G, -1)
        # a group's constant is a multiple of 1/4: its sum over the group is exact in float64
        const = torch.randint(-16, 17, (B, case.G, 1), generator=g).double() / 4 + 0.25
        if case.data == "const_groups":
            xg.copy_(const.expand_as(xg))
        else:
            assert case.data == "const_one_group"
            xg[:, 0] = const[:, 0]
    x = x.float()
    w = (torch.randn(C, generator=g) * 0.5 + 1.0) if "w" in case.affine else None
    b = (torch.randn(C, generator=g) * 0.3) if "b" in case.affine else None
    if case.gy == "zero":
        gy = torch.zeros(case.shape)
    elif case.gy == "const":
        # gamma_c dy constant over a group (to float32 rounding): the true dx is what is left of
        # gamma dy - mean(gamma dy) - xhat mean(gamma dy xhat), almost entirely cancellation
        k = torch.randn(B, case.G, 1, generator=g).expand(B, case.G, cg).reshape(B, C) + 2.0
        per_c = k / (w if w is not None else 1.0)
        gy = per_c.view(B, C, *([1] * (len(case.shape) - 2))).expand(case.shape).contiguous()
    else:
        gy = torch.randn(case.shape, generator=g)
    if case.layout == "x":
        x = _permuted(x)
    if case.layout == "gy":
        gy = _permuted(gy)
    return x, w, b, gy


def _gn_run(case: GnCase, dtype):
    x, w, b, gy = gn_inputs(case)
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) if t is not None else None for t in (x, w, b)]
    wt = leaves[1]
    if wt is None and leaves[2] is not None:   # torch's CPU backward wants a weight beside a bias
        wt = torch.ones(case.shape[1], dtype=dtype)
    y = F.group_norm(leaves[0], case.G, wt, leaves[2], EPS)
    y.backward(gy.to(dtype))
    return {"y": y.detach(), "dx": leaves[0].grad,
            "dgamma": leaves[1].grad if leaves[1] is not None else None,
            "dbeta": leaves[2].grad if leaves[2] is not None else None}


class Reference(NamedTuple):
    out: dict       # {tensor: float64 reference | None}
    scales: dict    # {tensor: s_t}
    kappa: float
    zero: tuple     # the tensors whose uncancelled magnitude is zero: the result is exactly 0


def _scales(mags: dict):
    """({tensor: s_t}, the tensors of zero magnitude)."""
    return {k: scale_of(v) for k, v in mags.items()}, tuple(k for k, v in mags.items() if rms(v) == 0.0)


@functools.lru_cache(maxsize=None)
def gn_reference(case: GnCase) -> Reference:
    x, w, b, gy = gn_inputs(case)
    out = _gn_run(case, torch.float64)
    B, C = case.shape[:2]
    xg = x.double().reshape(B, case.G, -1)
    mean = xg.mean(-1, keepdim=True)
    var = (xg - mean).square().mean(-1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    kappa = 1.0 + float((mean.abs() * rstd).max())
    per_c = lambda t: t.expand(B, case.G, C // case.G).reshape(B, C, 1)   # noqa: E731
    mean_c, rstd_c = per_c(mean), per_c(rstd)
    gam = w.double().view(1, C, 1) if w is not None else torch.ones(1, C, 1, dtype=torch.float64)
    bet = b.double().view(1, C, 1) if b is not None else torch.zeros(1, C, 1, dtype=torch.float64)
    x3, gy3 = x.double().reshape(B, C, -1), gy.double().reshape(B, C, -1)
    a = rstd_c * gam
    xhat = (x3 - mean_c) * rstd_c
    scales, zero = _scales({"y": (x3 * a).abs() + (mean_c * a).abs() + bet.abs(),
                            "dx": gam * gy3 * rstd_c,
                            "dgamma": (gy3 * xhat).abs().sum((0, 2)),
                            "dbeta": gy3.abs().sum((0, 2))})
    return Reference(out, scales, kappa, zero)


@functools.lru_cache(maxsize=None)
def gn_f32(case: GnCase) -> dict:
    """{tensor: m of float32 CPU torch}."""
    ref = gn_reference(case)
    f32 = _gn_run(case, torch.float32)
    return {k: measure(f32[k], ref.out[k], ref.scales[k]) for k in GN_TENSORS if ref.out[k] is not None}


# ---------------------------------------------------------------------------------------------
# LSTM gates
# ---------------------------------------------------------------------------------------------
GATE_Z = (0.0, 0.5, -0.5, 8.0, -8.0, 17.0, -17.0, 30.0, -30.0, 89.0, -89.0, 200.0, -200.0)
GATE_C = (0.0, 1e-3, -1e-3, 1.0, -1.0, 9.5, -9.5, 50.0, -50.0, 1e4, -1e4)
GATE_COTS = ("both", "dh", "dc")
GATE_TENSORS = ("h", "c", "dz", "dc_prev")
GATE_MEANS = (-1.5, 0.5, 2.0, -0.25)   # of the i, f, o, g channel blocks in the index cases


class GateCase(NamedTuple):
    name: str
    shape: tuple          # (B, hid, HW)
    kind: str             # "grid" | "index" | "nonfinite"
    repeat: bool = False


GATE_CASES = (
    GateCase("grid", (1, 1, len(GATE_Z) ** 4 * len(GATE_C)), "grid", repeat=True),
    GateCase("idx_3_5_63", (3, 5, 63), "index"),
    GateCase("idx_2_1_1", (2, 1, 1), "index"),
    GateCase("idx_1_16_1", (1, 16, 1), "index"),
    GateCase("idx_4_3_257", (4, 3, 257), "index"),
    GateCase("nonfinite", (2, 3, 67), "nonfinite"),
)
GATE_BY_NAME = {c.name: c for c in GATE_CASES}
INF = math.inf
# (b, channel of z or of c_prev, position, value): z at isolated elements, c_prev at others, and
# one element where f = sigmoid(-inf) = 0 meets c_prev = inf (0 * inf: NaN in c, h and the gradients)
NONFINITE_Z = ((0, 0, 3, INF), (0, 1, 9, -INF), (0, 3, 15, INF), (0, 4, 21, -INF), (0, 6, 27, INF),
               (1, 7, 33, -INF), (1, 9, 39, INF), (1, 11, 45, -INF), (1, 3, 60, -INF))
NONFINITE_C = ((0, 0, 50, INF), (0, 2, 55, -INF), (1, 0, 60, INF), (1, 1, 5, -INF))


def torch_gates(z, c, hid):
    from test_gpu_lstm_gates import _torch_gates
    return _torch_gates(z, c, hid)


@functools.lru_cache(maxsize=None)
def gate_inputs(case: GateCase):
    """(z [B,4 hid,1,HW], c_prev [B,hid,1,HW], dh, dc) in float32."""
    g = _gen("gate:" + case.name)
    B, hid, HW = case.shape
    if case.kind == "grid":
        prod = torch.tensor(list(itertools.product(GATE_Z, GATE_Z, GATE_Z, GATE_Z, GATE_C)))
        assert tuple(prod.shape) == (HW, 5)
        z = prod[:, :4].t().reshape(1, 4, 1, HW).contiguous()
        c = prod[:, 4].reshape(1, 1, 1, HW).contiguous()
    else:
        z = torch.randn(B, 4, hid, 1, HW, generator=g) * 2
        z = (z + torch.tensor(GATE_MEANS).view(1, 4, 1, 1, 1)).reshape(B, 4 * hid, 1, HW)
        c = torch.randn(B, hid, 1, HW, generator=g)
        if case.kind == "nonfinite":
            for b, ch, p, v in NONFINITE_Z:
                z[b, ch, 0, p] = v
            for b, ch, p, v in NONFINITE_C:
                c[b, ch, 0, p] = v
    dh = torch.randn(B, hid, 1, HW, generator=g)
    dc = torch.randn(B, hid, 1, HW, generator=g)
    return z, c, dh, dc


def gate_cotangents(case: GateCase, cot: str):
    """(dh, dc) of a cotangent pattern; the missing one is an explicit zero tensor, which is what
    autograd hands the library's Function for an output without a gradient."""
    _, _, dh, dc = gate_inputs(case)
    return (dh if cot in ("both", "dh") else torch.zeros_like(dh),
            dc if cot in ("both", "dc") else torch.zeros_like(dc))


def gates_run(z, c, dh, dc, dtype, hid):
    zz, cc = z.to(dtype).clone().requires_grad_(True), c.to(dtype).clone().requires_grad_(True)
    h, cn = torch_gates(zz, cc, hid)
    torch.autograd.backward([h, cn], [dh.to(dtype), dc.to(dtype)])
    return {"h": h.detach(), "c": cn.detach(), "dz": zz.grad, "dc_prev": cc.grad}


@functools.lru_cache(maxsize=None)
def gate_reference(case: GateCase, cot: str) -> Reference:
    z, c, _, _ = gate_inputs(case)
    dh, dc = gate_cotangents(case, cot)
    hid = case.shape[1]
    out = gates_run(z, c, dh, dc, torch.float64, hid)
    zi, zf, zo, zg = torch.split(z.double(), hid, dim=1)
    i, f, o, gg = torch.sigmoid(zi), torch.sigmoid(zf), torch.sigmoid(zo), torch.tanh(zg)
    cp = c.double()
    tc = torch.tanh(out["c"])
    fwd = (f * cp).abs() + (i * gg).abs()
    gc = dc.double().abs() + (dh.double() * o * (1 - tc * tc)).abs()
    bwd = gc * cp.abs().clamp_min(1.0)
    scales, zero = _scales({"h": fwd, "c": fwd, "dz": bwd, "dc_prev": bwd})
    return Reference(out, scales, 1.0, zero)


@functools.lru_cache(maxsize=None)
def gate_f32_out(case: GateCase, cot: str) -> dict:
    z, c, _, _ = gate_inputs(case)
    dh, dc = gate_cotangents(case, cot)
    return gates_run(z, c, dh, dc, torch.float32, case.shape[1])


@functools.lru_cache(maxsize=None)
def gate_f32(case: GateCase, cot: str) -> dict:
    ref = gate_reference(case, cot)
    f32 = gate_f32_out(case, cot)
    return {k: measure(f32[k], ref.out[k], ref.scales[k]) for k in GATE_TENSORS}


def nonfinite_pattern(t: torch.Tensor) -> torch.Tensor:
    """0 finite, 1 +inf, 2 -inf, 3 NaN, per element."""
    t = t.detach().cpu()
    return (torch.isposinf(t) * 1 + torch.isneginf(t) * 2 + torch.isnan(t) * 3).to(torch.int8)


# ---------------------------------------------------------------------------------------------
# deformable sampling
# ---------------------------------------------------------------------------------------------
DF_C = 32            # deform.hip kDfC
DF_TAPS = 9
DF_STEP = 2.0 ** -6  # every offset is a multiple of it, |offset| < 2^10
DF_SHAPES = ((1, 5, 7, 1), (2, 9, 11, 1), (1, 13, 9, 2), (1, 1, 1, 1))   # (B, H, W, stride)
DF_PATTERNS = ("integer", "edge", "ring", "far", "random")
DF_MASKS = ("rand", "zero", "one", "none")
DF_COTS = ("dense", "lane0", "lane15", "lane16", "lane31", "tap4")
DF_COT_SHAPE = (1, 5, 7, 1)   # 315 items: the last block is partly filled
DF_COLLISION_SHAPE = (1, 9, 11, 1)
DF_TENSORS = ("val", "gx", "goff", "gm")


class DfCase(NamedTuple):
    name: str
    shape: tuple      # (B, H, W, stride)
    pattern: str      # DF_PATTERNS | "collision"
    mask: str
    cot: str


def _df_name(shape, pattern, mask, cot):
    B, H, W, s = shape
    return f"{pattern}-{B}x{H}x{W}s{s}-m{mask}-{cot}"


DF_COLLISION = DfCase(_df_name(DF_COLLISION_SHAPE, "collision", "pos", "pos"), DF_COLLISION_SHAPE,
                      "collision", "pos", "pos")
DF_CASES = tuple(
    DfCase(_df_name(s, p, m, "dense"), s, p, m, "dense")
    for s in DF_SHAPES for p in DF_PATTERNS for m in DF_MASKS
) + tuple(
    DfCase(_df_name(DF_COT_SHAPE, p, "rand", c), DF_COT_SHAPE, p, "rand", c)
    for p in DF_PATTERNS for c in DF_COTS[1:]
) + (DF_COLLISION,)
DF_BY_NAME = {c.name: c for c in DF_CASES}
COLLISION_TARGET = (4, 5)   # the padded-image position (4.5, 5.5): input pixels (3..4, 4..5)


def df_out_hw(case: DfCase):
    _, H, W, s = case.shape
    return (H - 1) // s + 1, (W - 1) // s + 1


def df_base(case: DfCase):
    """p0 + pn of every (tap, pixel) as integers: rows [9,h,1], columns [9,1,w]."""
    _, _, _, s = case.shape
    h, w = df_out_hw(case)
    n = torch.arange(DF_TAPS)
    rows = (torch.arange(h) * s + 1).view(1, h, 1) + (n // 3 - 1).view(DF_TAPS, 1, 1)
    cols = (torch.arange(w) * s + 1).view(1, 1, w) + (n % 3 - 1).view(DF_TAPS, 1, 1)
    return rows, cols


def df_positions(case: DfCase, offset: torch.Tensor, dtype):
    """(pr, pc) [B,9,h,w] = (p0 + pn) + offset, computed in dtype."""
    rows, cols = df_base(case)
    off = offset.to(dtype)
    return rows.to(dtype) + off[:, :DF_TAPS], cols.to(dtype) + off[:, DF_TAPS:]


def _dyadic(t: torch.Tensor) -> torch.Tensor:
    return (t / DF_STEP).round() * DF_STEP


def _choose(g, shape, options):
    """Per element one of the option tensors, uniformly."""
    pick = torch.randint(0, len(options), shape, generator=g)
    out = torch.zeros(shape, dtype=torch.float64)
    for k, o in enumerate(options):
        out = torch.where(pick == k, o.double().expand(shape), out)
    return out


def _df_offset(case: DfCase, g) -> torch.Tensor:
    B, H, W, _ = case.shape
    h, w = df_out_hw(case)
    shp = (B, DF_TAPS, h, w)
    rows, cols = df_base(case)
    rows, cols = rows.double().expand(shp), cols.double().expand(shp)
    rnd = lambda scale: _dyadic(torch.randn(shp, generator=g, dtype=torch.float64) * scale)   # noqa: E731
    uni = lambda: _dyadic(torch.rand(shp, generator=g, dtype=torch.float64))                   # noqa: E731
    if case.pattern == "integer":
        ir = lambda: torch.randint(-2, 3, shp, generator=g).double()   # noqa: E731
        return torch.cat([ir(), ir()], 1)
    if case.pattern == "random":
        return torch.cat([rnd(3.0), rnd(3.0)], 1)
    if case.pattern == "far":
        far = float(H + W)
        fr = lambda: _choose(g, shp, [torch.tensor(far), torch.tensor(-far), rnd(1.0), rnd(1.0)])   # noqa: E731
        return torch.cat([fr(), fr()], 1)
    if case.pattern == "collision":
        tr, tc = COLLISION_TARGET
        return torch.cat([tr + 0.5 - rows, tc + 0.5 - cols], 1)
    target = []
    for base, last in ((rows, float(H + 1)), (cols, float(W + 1))):   # last = Hp - 1 / Wp - 1
        inside = (base + rnd(1.0)).clamp(1.0, last - 1.0)
        if case.pattern == "edge":
            opts = [torch.tensor(0.0), torch.tensor(last), torch.tensor(-DF_STEP),
                    torch.tensor(last + DF_STEP), inside]
        else:
            assert case.pattern == "ring"
            # [0, 1) and (Hp - 2, Hp - 1]
            # a third of the rows and of the columns: a ninth of the samples meets in the four image
            # corners, which keeps the terms of any one pixel of gx to a few dozen
            opts = [uni().clamp_max(1.0 - DF_STEP), last - uni().clamp_max(1.0 - DF_STEP)] + [inside] * 4
        target.append(_choose(g, shp, opts))
    return torch.cat([target[0] - rows, target[1] - cols], 1)


@functools.lru_cache(maxsize=None)
def df_inputs(case: DfCase):
    """(x [B,32,H,W], offset [B,18,h,w], mask [B,9,h,w] | None, gval [B,32,h,w,9]) in float32."""
    B, H, W, _ = case.shape
    h, w = df_out_hw(case)
    g = _gen(f"df:{case.shape}:{case.pattern}")   # the mask and cotangent variants share x and offsets
    x = torch.randn(B, DF_C, H, W, generator=g)
    off64 = _df_offset(case, g)
    offset = off64.float()
    assert torch.equal(offset.double(), off64) and float(offset.abs().max()) < 2.0 ** 10
    assert torch.equal(_dyadic(off64), off64)
    rand_m = torch.rand(B, DF_TAPS, h, w, generator=g).clamp(0.01, 0.99)
    mask = {"rand": rand_m, "pos": rand_m, "zero": torch.zeros_like(rand_m), "one": torch.ones_like(rand_m),
            "none": None}[case.mask]
    dense = torch.randn(B, DF_C, h, w, DF_TAPS, generator=g)
    gval = torch.zeros_like(dense)
    if case.cot == "dense":
        gval = dense
    elif case.cot == "pos":
        gval = dense.abs() + 0.1
    elif case.cot.startswith("lane"):
        lane = int(case.cot[4:])
        gval[:, lane] = dense[:, lane]
    else:
        tap = int(case.cot[3:])
        gval[..., tap] = dense[..., tap]
    if case.pattern == "collision":
        x = x.abs() + 0.1
    return x, offset, mask, gval


def _df_autograd(case: DfCase, dtype):
    from test_deform_conv import planar_val
    x, offset, mask, gval = df_inputs(case)
    xx = x.to(dtype).clone().requires_grad_(True)
    oo = offset.to(dtype).clone().requires_grad_(True)
    mm = mask.to(dtype).clone().requires_grad_(True) if mask is not None else None
    val = planar_val(xx, oo, mm, case.shape[3], 1)
    val.backward(gval.to(dtype))
    return {"val": val.detach(), "gx": xx.grad, "goff": oo.grad, "gm": mm.grad if mm is not None else None}


class DfTerms(NamedTuple):
    out: dict      # {tensor: value} of the explicit formula, in planar_val's layouts
    mag: dict      # {tensor: sum of absolute corner terms}, same shapes
    count: dict    # what the offsets contain
    terms: int     # atomic terms into COLLISION_TARGET's left-top input pixel (x >= 0, gval >= 0)


def _df_geometry(case: DfCase, dtype):
    """Positions, clamp gates, the four one-dimensional factors, the corner factors g_lt, g_rb,
    g_lb, g_rt and the corners' rows / columns in the padded image, all [B,9,h,w], in dtype."""
    _, H, W, _ = case.shape
    Hp, Wp = H + 2, W + 2
    pr, pc = df_positions(case, df_inputs(case)[1], dtype)
    r0, c0 = pr.floor(), pc.floor()
    r0c, r1c = r0.clamp(0, Hp - 1), (r0 + 1).clamp(0, Hp - 1)
    c0c, c1c = c0.clamp(0, Wp - 1), (c0 + 1).clamp(0, Wp - 1)
    rin, cin = (pr >= 0) & (pr <= Hp - 1), (pc >= 0) & (pc <= Wp - 1)
    prc, pcc = pr.clamp(0, Hp - 1), pc.clamp(0, Wp - 1)
    ar0, ar1 = 1 + (r0c - prc), 1 - (r1c - prc)
    ac0, ac1 = 1 + (c0c - pcc), 1 - (c1c - pcc)
    gk = [ar0 * ac0, ar1 * ac1, ar0 * ac1, ar1 * ac0]        # lt, rb, lb, rt
    return pr, pc, r0, c0, rin, cin, (ar0, ar1, ac0, ac1), gk, [r0c, r1c, r0c, r1c], [c0c, c1c, c1c, c0c]


def df_gx_order_spread(case: DfCase, orders: int, seed: int = 0) -> float:
    """The largest m of gx over float32 sums of its terms (gval * mask) * g_k, rounded as the kernel
    and float32 torch round them, taken in `orders` random orders: what an atomic float32 sum may
    give whatever the kernel's schedule."""
    import numpy as np
    _, _, mask, gval = df_inputs(case)
    B, H, W, _ = case.shape
    Hp, Wp = H + 2, W + 2
    *_, gk, rk, ck = _df_geometry(case, torch.float32)
    gu = gval.permute(0, 1, 4, 2, 3) * (mask.unsqueeze(1) if mask is not None else 1.0)
    plane = (torch.arange(B).view(B, 1, 1, 1, 1) * DF_C + torch.arange(DF_C).view(1, DF_C, 1, 1, 1)) * (Hp * Wp)
    idx = torch.cat([(plane + (r.long() * Wp + c.long()).unsqueeze(1)).reshape(-1) for r, c in zip(rk, ck)]).numpy()
    term = torch.cat([(gu * g.unsqueeze(1)).reshape(-1) for g in gk]).numpy()
    ref = df_reference(case)
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(orders):
        p = rng.permutation(len(idx))
        acc = np.zeros(B * DF_C * Hp * Wp, np.float32)
        np.add.at(acc, idx[p], term[p])
        got = torch.from_numpy(acc).view(B, DF_C, Hp, Wp)[:, :, 1:-1, 1:-1]
        worst = max(worst, measure(got, ref.out["gx"], ref.scales["gx"]))
    return worst


def df_explicit(case: DfCase, neg_dpr_term: int | None = None, drop_lane: int | None = None) -> DfTerms:
    """deform.hip's formulas in float64: val, gx, goff, gm and the sums of their absolute terms.
    neg_dpr_term flips the sign of one of the four dL/dpr terms, drop_lane leaves one channel
    out of the channel sums of goff and gm: the perturbed copies the CPU test uses."""
    x, offset, mask, gval = df_inputs(case)
    B, H, W, _ = case.shape
    h, w = df_out_hw(case)
    Hp, Wp = H + 2, W + 2
    xp = F.pad(x.double(), (1, 1, 1, 1))
    pr, pc, r0, c0, rin, cin, (ar0, ar1, ac0, ac1), gk, rk, ck = _df_geometry(case, torch.float64)
    r0c, r1c, c0c, c1c = rk[0], rk[1], ck[0], ck[1]
    flat = xp.reshape(B, DF_C, Hp * Wp)
    idx = [(r.long() * Wp + c.long()).reshape(B, 1, -1).expand(-1, DF_C, -1) for r, c in zip(rk, ck)]
    tk = [flat.gather(2, i).view(B, DF_C, DF_TAPS, h, w) for i in idx]
    gk = [g.unsqueeze(1) for g in gk]
    m = mask.double().unsqueeze(1) if mask is not None else torch.ones(1, 1, 1, 1, 1, dtype=torch.float64)
    gv = gval.double().permute(0, 1, 4, 2, 3)                 # [B,C,9,h,w]
    vu = sum(g * t for g, t in zip(gk, tk))
    vu_abs = sum((g * t).abs() for g, t in zip(gk, tk))
    gu = gv * m
    gxp, gxp_abs = torch.zeros_like(flat), torch.zeros_like(flat)
    for g, i in zip(gk, idx):
        gxp.scatter_add_(2, i, (gu * g).reshape(B, DF_C, -1))
        gxp_abs.scatter_add_(2, i, (gu * g).abs().reshape(B, DF_C, -1))
    crop = lambda t: t.view(B, DF_C, Hp, Wp)[:, :, 1:-1, 1:-1]   # noqa: E731
    a_r0, a_r1, a_c0, a_c1 = (t.unsqueeze(1) for t in (ar0, ar1, ac0, ac1))
    dpr = [-(a_c0 * tk[0]), a_c1 * tk[1], -(a_c1 * tk[2]), a_c0 * tk[3]]
    dpc = [-(a_r0 * tk[0]), a_r1 * tk[1], a_r0 * tk[2], -(a_r1 * tk[3])]
    if neg_dpr_term is not None:
        dpr[neg_dpr_term] = -dpr[neg_dpr_term]
    lanes = [c for c in range(DF_C) if c != drop_lane]
    csum = lambda t: t[:, lanes].sum(1)   # noqa: E731
    goff = torch.cat([csum(gu * sum(dpr)) * rin, csum(gu * sum(dpc)) * cin], 1)
    goff_abs = torch.cat([csum(sum((gu * t).abs() for t in dpr)) * rin,
                          csum(sum((gu * t).abs() for t in dpc)) * cin], 1)
    planar = lambda t: t.permute(0, 1, 3, 4, 2)   # noqa: E731   [B,C,9,h,w] -> [B,C,h,w,9]
    out = {"val": planar(m * vu), "gx": crop(gxp), "goff": goff,
           "gm": csum(gv * vu) if mask is not None else None}
    mag = {"val": planar(m.abs() * vu_abs), "gx": crop(gxp_abs), "goff": goff_abs,
           "gm": csum(gv.abs() * vu_abs) if mask is not None else None}
    ring = lambda r, c: (r == 0) | (r == Hp - 1) | (c == 0) | (c == Wp - 1)   # noqa: E731
    count = {
        "on_first": int((pr == 0).sum() + (pc == 0).sum()),
        "on_last": int((pr == Hp - 1).sum() + (pc == Wp - 1).sum()),
        "outside": int((~rin).sum() + (~cin).sum()),
        "far": int(((pr < -1) | (pr > Hp)).sum() + ((pc < -1) | (pc > Wp)).sum()),
        "ring_corner": int(functools.reduce(torch.logical_or, [ring(r, c) for r, c in zip(rk, ck)]).sum()),
        "in_ring": int((rin & ((pr < 1) | (pr > Hp - 2))).sum() + (cin & ((pc < 1) | (pc > Wp - 2))).sum()),
        "coinciding": int(((r0c == r1c) | (c0c == c1c)).sum()),
        "integer": int(((pr == r0) & (pc == c0)).sum()),
        "samples": pr.numel(),
    }
    tr, tc = COLLISION_TARGET
    terms = int(sum(int((i[:, 0] == tr * Wp + tc).sum()) for i in idx))
    return DfTerms(out, mag, count, terms)


@functools.lru_cache(maxsize=None)
def df_reference(case: DfCase) -> Reference:
    """float64 autograd of planar_val; the scales from the explicit formula's absolute terms."""
    out = _df_autograd(case, torch.float64)
    ex = df_explicit(case)
    scales, zero = _scales({k: ex.mag[k] for k in DF_TENSORS if out[k] is not None})
    return Reference(out, scales, 1.0, zero)


@functools.lru_cache(maxsize=None)
def df_magnitude(case: DfCase) -> dict:
    """{tensor: per-element sum of absolute terms}: where it is 0 the kernel's result is exactly 0."""
    return df_explicit(case).mag


@functools.lru_cache(maxsize=None)
def df_f32(case: DfCase) -> dict:
    ref = df_reference(case)
    f32 = _df_autograd(case, torch.float32)
    return {k: measure(f32[k], ref.out[k], ref.scales[k]) for k in DF_TENSORS if ref.out[k] is not None}


def collision_terms() -> int:
    _, H, W, _ = DF_COLLISION_SHAPE
    return DF_TAPS * H * W


def collision_gx_bound() -> torch.Tensor:
    """Per element of gx: N 2^-24 sum |terms|, N = 9 h w."""
    return collision_terms() * 2.0 ** -24 * df_magnitude(DF_COLLISION)["gx"]


# ---------------------------------------------------------------------------------------------
# cases whose float32 CPU torch error is above FLOOR * kappa: the 3 m_f32 arm of the bound
# carries them (tests/test_aux_kernel_cases.py asserts that this is the whole list)
# ---------------------------------------------------------------------------------------------
# std1e18: float32 torch's sum of squares of the group overflows (1768 elements of ~1e36) and its y is 0
F32_ABOVE_FLOOR: dict = {"gn std1e18": ("y", "dx", "dgamma")}
