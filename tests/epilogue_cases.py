"""Cases for the kernels that turn a cost volume into what the user sees -- ops.softmax_depth,
the standalone ops.wta_update and ops.evidential_epilogue (csrc/depth_head.hip softmax_depth_kernel
and wta_update_kernel, csrc/evidential.hip) -- with their references, and the one frame that
reaches the second stride of the launchers that cap their grid at 4096 blocks of 256 threads.

softmax_depth.  Hand-made columns repeated over SM_P = 257 pixels of a [2, D, 1, 257] volume.
The reference is float64 torch.softmax at test_softmax_depth_matches_torch's rtol 1e-5 / atol
1e-7; on the non-finite columns the result is NaN exactly where float32 torch.softmax is.
``sm_online`` restates the kernel's online recurrence in float32 numpy, as it was (the running
max starts at -inf) and as it is.

wta_update.  ``wta_restatement`` is drmvsnet.py:324-334 in float32 numpy, op for op (what
oracle.sweep_oracle.sweep does per plane inside its loop).  Costs of different planes differ by
at least WTA_GAP unless they tie exactly, so an ulp between the device's expf and numpy's cannot
flip a selection: depth is compared bit for bit, max_prob within 4 * 2^-24 relative (one expf on
each side at <= 1 ulp each, doubled), exp_sum within (4 + D) * 2^-24.

evidential_epilogue.  One [1, 4, 32, H, W] triple per case, never concatenated.  The reference
is ``epilogue64`` (evidential/models.py:421-459) under float64 autograd.  Measure and bound are
aux_kernel_cases': m(t) = max |got - ref64| / (|ref64| + s_t) <= max(FLOOR, 3 m_f32), m_f32 the
same measure of ``epilogue64`` run in float32 on the CPU.  s_t is the RMS of the uncancelled
magnitude of the tensor, from ``ev_explicit``: evidential.hip's closed-form backward in float64
with a second track that takes absolute values at gu = g.u - gd1 - gd2, at g.la - gu n / la^2
(and the gn a.u added back) and at the softmax backward's gp[d] - dot.  A tensor whose magnitude
is zero everywhere must be exactly 0.

FLOOR = (32 + 41) * 2^-24.  32 is the term sum; 41 is the longest chain of scalar operations in
evidential.hip, the one that ends in a cost gradient of head 0: softmax (v - m, expf, 1 / s,
* inv: 4), the logit's product and sum (2), softplus (expf, log1pf: 2), e01's la and u (+; *, +,
/: 4), the outer moe_nig_bwd (n's *, +; /; d1; 2 d1; a.la *; gq *; the two subtractions of gu;
gn; gn a.la; +=: 12 to g01.u), the inner one (gu's two subtractions; gn; gn u; g.la -;
+ gn a.u; +=: 7 to g0.la), gl0 = ge.la * softplus' (1), q's product and four sums (5), dot's
product and sum (2), gp - dot and pr * (2).

Where float32 CPU torch is not finite on a finite float64 reference (EV_NONFINITE_F32) there is
no m_f32 on those elements: the kernel's NaN pattern must equal float32 torch's, and measure and
bound are taken over the elements where float32 torch is finite.

The large frame.  BIG_H x BIG_W = 1028 x 1024 = 4096 * 256 + 4096 pixels, B = 2: 16 blocks take a
second stride and the rest do not.  Each cost input repeats a base of BIG_BASE = 4099 (a prime)
pixels, pixel p of batch element b holding base[b][p % 4099], so a float64 reference on the base
is the large frame's after tiling.

Everything here is computed once per process and never modified.  tests/test_epilogue_cases.py
asserts on the CPU what keeps the GPU test honest; tests/test_gpu_epilogue.py runs the library.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from aux_kernel_cases import F32_FACTOR, Reference, _gen, _scales, measure

INF, NAN = math.inf, math.nan
F32 = np.float32

# ---------------------------------------------------------------------------------------------
# softmax_depth
# ---------------------------------------------------------------------------------------------
SM_B, SM_P = 2, 257
SM_RTOL, SM_ATOL = 1e-5, 1e-7            # test_softmax_depth_matches_torch's
SM_UNROLL_D = (1, 2, 3, 4, 5, 7, 8, 37)  # the 4-plane unroll and its tail
SM_FINITE = {
    "ascending": (-6.5, -4.0, -1.5, 0.25, 1.0, 2.5, 7.0),      # every element raises the running max
    "descending": (7.0, 2.5, 1.0, 0.25, -1.5, -4.0, -6.5),     # none does
    "equal": (1.5,) * 7,
    "tie_first_last": (5.0, 1.0, 2.0, 3.0, 0.0, -1.0, 5.0),
    "gap_underflow": (60.0, -44.0, -50.0, -60.0, -45.0, -70.0, -80.0),   # gaps >= 104: exactly 0
    "gap_subnormal": (10.0, -78.0, -80.0, -85.0, -90.0, -92.0, -93.0),   # gaps 88 .. 103
    "overflow": (3e38, -3e38, 0.0, 0.0, 0.0, 0.0, 0.0),        # v - m overflows to -inf
}
_SM_BASE = (0.5, -1.0, 2.0, 1.0, -0.5, 1.5, 0.0)


def _with(values: dict) -> tuple:
    return tuple(values.get(i, v) for i, v in enumerate(_SM_BASE))


SM_NONFINITE = {
    "ninf_first": _with({0: -INF}),
    "ninf_middle": _with({3: -INF}),
    "ninf_last": _with({6: -INF}),
    "ninf_all_but_one": _with({i: -INF for i in (0, 1, 2, 4, 5, 6)}),
    "ninf_all": (-INF,) * 7,
    "pinf_first": _with({0: INF}),
    "pinf_last": _with({6: INF}),
    "pinf_twice": _with({1: INF, 4: INF}),
    "nan_first": _with({0: NAN}),
    "nan_middle": _with({3: NAN}),
    "nan_last": _with({6: NAN}),
    "pinf_and_ninf": _with({2: INF, 5: -INF}),
}
SM_COLUMNS = {**SM_FINITE, **SM_NONFINITE}
# the columns on which the recurrence that started its running max at -inf left torch.softmax
SM_PARENT_DIFFERS = ("ninf_first", "ninf_all_but_one", "pinf_first", "pinf_last", "pinf_and_ninf")


def sm_volume(column) -> torch.Tensor:
    """[2, D, 1, 257] float32: the column at every pixel of both batch elements."""
    col = torch.tensor(column, dtype=torch.float32)
    return col.view(1, -1, 1, 1).expand(SM_B, col.numel(), 1, SM_P).contiguous()


@functools.lru_cache(maxsize=None)
def sm_random(D: int) -> torch.Tensor:
    """[2, D, 1, 257] float32 costs, uniform in +-80 (the range of the existing test)."""
    return torch.rand(SM_B, D, 1, SM_P, generator=_gen(f"sm:{D}")) * 160.0 - 80.0


def sm_reference(cost: torch.Tensor) -> torch.Tensor:
    return torch.softmax(cost.double(), dim=1)


def sm_online(column, fixed: bool = True) -> np.ndarray:
    """softmax_depth_kernel's two passes over one column in float32 numpy.  ``fixed=False``: the
    recurrence as it was, the running max starting at -inf and the sum taken as it stands."""
    with np.errstate(all="ignore"):
        v = np.asarray(column, F32)
        m = F32(-np.finfo(F32).max) if fixed else F32(-INF)
        s = F32(0)
        for x in v:
            dv = F32(x - m)
            e = np.exp(-np.abs(dv)).astype(F32)
            if dv > 0:
                s, m = F32(F32(s * e) + F32(1)), x
            else:
                s = F32(s + e)
        if fixed:
            s = F32(s + F32(m - m))
        return (np.exp((v - m).astype(F32)).astype(F32) * F32(F32(1) / s)).astype(F32)


def sm_check(got: torch.Tensor, cost: torch.Tensor, label: str) -> None:
    """NaN exactly where float32 torch.softmax has it; elsewhere the finite tolerance against
    float64 torch.softmax."""
    got = got.detach().cpu()
    nan32 = torch.isnan(torch.softmax(cost, dim=1))
    assert torch.equal(torch.isnan(got), nan32), (
        f"{label}: NaN at {torch.isnan(got)[0, :, 0, 0].tolist()}, torch at {nan32[0, :, 0, 0].tolist()}")
    ref = sm_reference(cost)
    ok = ~nan32
    np.testing.assert_allclose(got[ok].double().numpy(), ref[ok].numpy(), rtol=SM_RTOL, atol=SM_ATOL, err_msg=label)


# ---------------------------------------------------------------------------------------------
# standalone WTA
# ---------------------------------------------------------------------------------------------
WTA_P = 257
WTA_GAP = 1e-3
U = 2.0 ** -24


class WtaCase(NamedTuple):
    name: str
    costs: tuple
    descending: bool = False   # the depth values fall from plane to plane


WTA_CASES = (
    WtaCase("tie2", (0.5, 0.5, -1.0)),
    WtaCase("tie3", (-1.0, 2.0, 2.0, 0.0, 2.0)),
    WtaCase("all_underflow", (-104.5, -110.0, -200.0, -150.0)),   # every exp is 0: depth stays 0
    WtaCase("inf_once", (1.0, 89.0, 2.0, -1.0)),
    WtaCase("inf_twice", (1.0, 89.0, 2.0, 89.0, 0.0)),            # the second select: 0 * inf
    WtaCase("nan_first", (NAN, 1.0, 2.0, 0.0)),
    WtaCase("nan_middle", (1.0, NAN, 2.0, 0.0)),
    WtaCase("nan_last", (1.0, 2.0, 0.0, NAN)),
    WtaCase("depth_ascending", (0.3, 1.2, -0.7, 2.1, 0.9)),
    WtaCase("depth_descending", (0.3, 1.2, -0.7, 2.1, 0.9), descending=True),
    WtaCase("one_plane", (0.7,)),
)
WTA_BY_NAME = {c.name: c for c in WTA_CASES}


def wta_depths(case: WtaCase) -> np.ndarray:
    d = np.linspace(425.0, 935.0, max(len(case.costs), 2)).astype(F32)[:len(case.costs)]
    return d[::-1].copy() if case.descending else d


def wta_volume(case: WtaCase) -> torch.Tensor:
    """[1, D, 1, 257] float32: the column at every pixel."""
    col = torch.tensor(case.costs, dtype=torch.float32)
    return col.view(1, -1, 1, 1).expand(1, col.numel(), 1, WTA_P).contiguous()


def wta_restatement(cost, depth_values, dtype=F32) -> dict:
    """drmvsnet.py:324-334 plane by plane, each operation rounded on its own: cost [B, D, P],
    depth_values [B, D] -> {'depth', 'max_prob', 'exp_sum'} [B, P]."""
    c = np.asarray(cost, dtype)
    dv = np.asarray(depth_values, dtype)
    B, D, P = c.shape
    mp, dp, es = (np.zeros((B, P), dtype) for _ in range(3))
    one = dtype(1)
    with np.errstate(all="ignore"):
        for d in range(D):
            p = np.exp(c[:, d]).astype(dtype)                 # :324, no max-subtraction
            f = (mp < p).astype(dtype)                        # :327, strict
            mp = (f * p + (one - f) * mp).astype(dtype)       # :328, arithmetic select
            dp = (f * dv[:, d:d + 1] + (one - f) * dp).astype(dtype)
            es = (es + p).astype(dtype)                       # :334
    return {"depth": dp, "max_prob": mp, "exp_sum": es}


def bits_equal(a, b) -> bool:
    """Bit for bit, with every NaN counted as one value."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.array_equal(np.isnan(a), np.isnan(b))
                and np.array_equal(np.where(np.isnan(a), F32(0), a).view(np.int32),
                                   np.where(np.isnan(b), F32(0), b).view(np.int32)))


def wta_check(got: dict, ref: dict, D: int, label: str) -> None:
    """depth bit for bit; max_prob and exp_sum within their ulp budgets; equal NaN / inf patterns."""
    g = {k: np.asarray(v, F32).reshape(ref[k].shape) for k, v in got.items()}
    assert bits_equal(g["depth"], ref["depth"]), f"{label}: depth differs from the restatement"
    for k, tol in (("max_prob", 4 * U), ("exp_sum", (4 + D) * U)):
        for test in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(test(g[k]), test(ref[k])), f"{label}: {k} {test.__name__} pattern"
        ok = np.isfinite(ref[k])
        err = np.abs(g[k][ok].astype(np.float64) - ref[k][ok]) / np.maximum(np.abs(ref[k][ok].astype(np.float64)), 1e-300)
        err = np.where(g[k][ok] == ref[k][ok], 0.0, err)
        assert err.size == 0 or float(err.max()) <= tol, f"{label}: {k} off by {float(err.max()) / U:.2f} x 2^-24"


# ---------------------------------------------------------------------------------------------
# the frame with one stride past 4096 x 256 pixels
# ---------------------------------------------------------------------------------------------
GRID_CAP, BLOCK = 4096, 256
BIG_B, BIG_H, BIG_W, BIG_BASE = 2, 1028, 1024, 4099
BIG_HW = BIG_H * BIG_W


@functools.lru_cache(maxsize=None)
def big_base(D: int, scale: float = 3.0) -> torch.Tensor:
    """[2, D, 4099] float32 costs, randn * scale; plane pairs closer than WTA_GAP are moved apart."""
    c = torch.randn(BIG_B, D, BIG_BASE, generator=_gen(f"big:{D}"), dtype=torch.float64) * scale
    for d in range(1, D):
        for e in range(d):
            near = (c[:, d] - c[:, e]).abs() < 2 * WTA_GAP
            c[:, d] = torch.where(near, c[:, d] + 4 * WTA_GAP * (d + 1), c[:, d])
    return c.float()


def big_tile(base) -> torch.Tensor:
    """[..., 4099] -> [..., 1028 * 1024]: element p is base[..., p % 4099]."""
    base = torch.as_tensor(base)
    reps = -(-BIG_HW // BIG_BASE)
    return base.repeat(*([1] * (base.dim() - 1)), reps)[..., :BIG_HW].contiguous()


def big_depths(D: int) -> torch.Tensor:
    """[2, D]: ascending for element 0, descending for element 1."""
    d = torch.linspace(425.0, 935.0, max(D, 2))[:D]
    return torch.stack([d, d.flip(0)]).contiguous()


# ---------------------------------------------------------------------------------------------
# evidential epilogue
# ---------------------------------------------------------------------------------------------
EV_D = 32
FLOOR = (32 + 41) * 2.0 ** -24
EV_COSTS = ("random", "flat", "near_flat", "onehot_apart", "onehot_agree", "onehot_head0")
EV_LOGITS = ("rand4", "eq19.999", "eq20", "eq20.001", "eq60", "eq-30", "eq-80", "eq-120", "one_head-120")
EV_COTS = ("both", "ev", "pc", "zero", "ch_u", "ch_la", "ch_alpha", "ch_beta")
EV_COT_COSTS = ("random", "flat", "onehot_apart")
EV_SHAPES = ((1, 1), (1, 255), (1, 256), (1, 257), (257, 1))
EV_CHANNELS = ("cost", "la", "alpha", "beta")
EV_FWD = ("u", "la", "alpha", "beta", "pc")
EV_GRADS = tuple(f"g{i}.{c}" for i in range(3) for c in EV_CHANNELS)
EV_TENSORS = EV_FWD + EV_GRADS
ONEHOT_GAP = 200.0
ONEHOT_PLANES = {"onehot_apart": (0, 31, 15), "onehot_agree": (7, 7, 7)}
AGREE_LA = (32.0, 32.0, 64.0)


class EvCase(NamedTuple):
    name: str
    cost: str
    logit: str
    cot: str
    hw: tuple = (1, 64)


EV_CASES = tuple(
    EvCase(f"cost_{c}", c, "rand4", "both") for c in EV_COSTS
) + tuple(
    EvCase(f"logit_{lg}", "random", lg, "both") for lg in EV_LOGITS[1:]
) + tuple(
    EvCase(f"cot_{ct}-{c}", c, "rand4", ct) for c in EV_COT_COSTS for ct in EV_COTS[1:]
) + tuple(
    EvCase(f"hw{h}x{w}", "random", "rand4", "both", (h, w)) for h, w in EV_SHAPES
)
EV_BY_NAME = {c.name: c for c in EV_CASES}


def ev_depths() -> torch.Tensor:
    from aarmvs import synthetic as syn
    return torch.from_numpy(syn.depth_hypotheses(EV_D))


@functools.lru_cache(maxsize=None)
def ev_inputs(case: EvCase):
    """(heads: three [1, 4, 32, H, W] float32, g_ev [4, H, W] | None, g_pc [1, 32, H, W] | None);
    None is an output that takes no part in the backward."""
    H, W = case.hw
    P = H * W
    g = _gen(f"ev:{case.cost}:{case.logit}:{case.hw}")   # the cotangent variants share the heads
    cost = torch.randn(3, EV_D, P, generator=g, dtype=torch.float64) * 10.0
    logit = torch.randn(3, 3, EV_D, P, generator=g, dtype=torch.float64) * 4.0
    if case.cost == "flat":
        cost = torch.full_like(cost, 0.75)
    elif case.cost == "near_flat":
        cost = cost * 1e-4
    elif case.cost in ONEHOT_PLANES:
        cost = torch.zeros_like(cost)
        for i, pl in enumerate(ONEHOT_PLANES[case.cost]):
            cost[i, pl] = ONEHOT_GAP
    elif case.cost == "onehot_head0":
        cost[0] = 0.0
        cost[0, 11] = ONEHOT_GAP
    else:
        assert case.cost == "random"
    if case.logit.startswith("eq"):
        logit = torch.full_like(logit, float(case.logit[2:]))
    elif case.logit == "one_head-120":
        logit[1] = -120.0
    else:
        assert case.logit == "rand4"
    if case.cost == "onehot_agree":
        # la = 32, 32 and 64 (past softplus's threshold, so la is the logit): powers of two, with
        # which (la1 u + u la2) / la is u exactly at both levels and d1 = d2 = 0 in any precision
        for i, v in enumerate(AGREE_LA):
            logit[i, 0] = v
    heads =tuple(torch.cat([cost[i:i + 1], logit[i]]).float().view(1, 4, EV_D, H, W) for i in range(3))
    g_ev = torch.randn(4, H, W, generator=g)
    g_pc = torch.randn(1, EV_D, H, W, generator=g)
    if case.cot.startswith("ch_"):
        keep = ("u", "la", "alpha", "beta").index(case.cot[3:])
        g_ev = torch.stack([g_ev[k] if k == keep else torch.zeros(H, W) for k in range(4)])
    cots = {"both": (g_ev, g_pc), "ev": (g_ev, None), "pc": (None, g_pc),
            "zero": (torch.zeros_like(g_ev), torch.zeros_like(g_pc))}
    g_ev, g_pc = cots.get(case.cot, (g_ev, None))
    return heads, g_ev, g_pc


def epilogue64(heads, dv):
    """Restatement of evidential/models.py:421-459 on [1,4,D,H,W] classifier outputs, in the
    inputs' dtype: (evidential [4,H,W], prob_combine [1,D,H,W])."""
    ests, probs = [], []
    sp = lambda x: F.softplus(x)   # noqa: E731
    for o in heads:
        cost, la, al, be = (o[:, i] for i in range(4))
        p = F.softmax(cost, dim=1)
        pred = (p * dv.view(1, -1, 1, 1)).sum(1)
        ests.append((pred, sp((la * p).sum(1)), sp((al * p).sum(1)) + 1, sp((be * p).sum(1))))
        probs.append(p)

    def moe(a, b):
        u1, la1, al1, be1 = a
        u2, la2, al2, be2 = b
        la = la1 + la2
        u = (la1 * u1 + u2 * la2) / la
        return u, la, al1 + al2 + 0.5, be1 + be2 + 0.5 * (la1 * (u1 - u) ** 2 + la2 * (u2 - u) ** 2)
    r = moe(moe(ests[0], ests[1]), ests[2])
    return torch.cat(r), torch.stack(probs).mean(0)


def ev_named(ev, pc, grads) -> dict:
    """{tensor name: value} from the epilogue's two outputs and the three heads' gradients."""
    out = {"u": ev[0], "la": ev[1], "alpha": ev[2], "beta": ev[3], "pc": pc}
    for i, g in enumerate(grads):
        for c, ch in enumerate(EV_CHANNELS):
            out[f"g{i}.{ch}"] = g[0, c]
    return {k: v.detach() for k, v in out.items()}


def ev_autograd(case: EvCase, dtype) -> dict:
    heads, g_ev, g_pc = ev_inputs(case)
    hs = [h.to(dtype).clone().requires_grad_(True) for h in heads]
    ev, pc = epilogue64(hs, ev_depths().to(dtype))
    outs = [(o, g.to(dtype)) for o, g in ((ev, g_ev), (pc, g_pc)) if g is not None]
    torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
    return ev_named(ev, pc, [h.grad for h in hs])


EV_DEFECTS = ("alpha_half", "beta_swap", "no_gpc", "no_gn_au", "no_gd", "nesting")
EV_NEUTRAL_DEFECTS = ("no_gd", "nesting")   # no defects: see tests/test_epilogue_cases.py


def ev_explicit(case: EvCase, defect: str | None = None):
    """evidential.hip's forward and closed-form backward in float64: ({tensor: value}, {tensor:
    uncancelled magnitude}), in ``ev_named``'s layout.  ``defect`` is one of EV_DEFECTS: alpha's
    + 0.5 left out, a.la and b.la swapped in beta's term, g_pc / 3 left out, the gn a.u (gn b.u)
    added back to dL/dla left out, the - gd1 - gd2 of gu left out, the mixture nested as
    (e0, (e1, e2))."""
    heads, g_ev, g_pc = ev_inputs(case)
    H, W = case.hw
    hs = [h.double().view(4, EV_D, -1) for h in heads]
    dv = ev_depths().double().view(EV_D, 1)
    sg = lambda x: torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x))   # noqa: E731
    prs, lgs, est = [], [], []
    for h in hs:
        pr = torch.softmax(h[0], 0)
        lg = [(h[k] * pr).sum(0) for k in (1, 2, 3)]
        prs.append(pr)
        lgs.append(lg)
        est.append(((pr * dv).sum(0), F.softplus(lg[0]), F.softplus(lg[1]) + 1.0, F.softplus(lg[2])))

    def moe(a, b):
        la = a[1] + b[1]
        u = (a[1] * a[0] + b[0] * b[1]) / la
        d1, d2 = a[0] - u, b[0] - u
        wa, wb = (b[1], a[1]) if defect == "beta_swap" else (a[1], b[1])
        half = 0.0 if defect == "alpha_half" else 0.5
        return u, la, a[2] + b[2] + half, a[3] + b[3] + 0.5 * (wa * d1 * d1 + wb * d2 * d2)

    def moe_bwd(a, b, g, gm):
        """(ga, gb, their magnitudes) of moe_nig_bwd; g, gm = dL/d the result and its magnitude."""
        la = a[1] + b[1]
        n = a[1] * a[0] + b[0] * b[1]
        u = n / la
        d1, d2 = a[0] - u, b[0] - u
        outs = []
        for t, mag in ((g, False), (gm, True)):
            ab = (lambda x: x.abs()) if mag else (lambda x: x)
            sub = (lambda x, y: x + y) if mag else (lambda x, y: x - y)
            gq = 0.5 * t[3]
            gd1, gd2 = gq * ab(a[1] * (2.0 * d1)), gq * ab(b[1] * (2.0 * d2))
            gu = t[0] if defect == "no_gd" and not mag else sub(sub(t[0], gd1), gd2)
            gn = gu / la
            gla = sub(t[1], gu * ab(n) / (la * la))
            back = 0.0 if defect == "no_gn_au" and not mag else 1.0
            outs.append(((gd1 + gn * a[1], gq * (d1 * d1) + (gla + back * gn * ab(a[0])), t[2], t[3]),
                         (gd2 + gn * b[1], gq * (d2 * d2) + (gla + back * gn * ab(b[0])), t[2], t[3])))
        return outs[0][0], outs[0][1], outs[1][0], outs[1][1]

    P = H * W
    zero = torch.zeros(P, dtype=torch.float64)
    g = tuple(g_ev.double().view(4, P)) if g_ev is not None else (zero,) * 4
    gm = tuple(t.abs() for t in g)
    if defect == "nesting":
        r = moe(est[0], moe(est[1], est[2]))
        g0, g12, m0, m12 = moe_bwd(est[0], moe(est[1], est[2]), g, gm)
        g1, g2, m1, m2 = moe_bwd(est[1], est[2], g12, m12)
    else:
        e01 = moe(est[0], est[1])
        r = moe(e01, est[2])
        g01, g2, m01, m2 = moe_bwd(e01, est[2], g, gm)
        g0, g1, m0, m1 = moe_bwd(est[0], est[1], g01, m01)
    pc = torch.stack(prs).mean(0)
    out = {"u": r[0], "la": r[1], "alpha": r[2], "beta": r[3], "pc": pc}
    mag = {k: v.abs() for k, v in out.items()}
    gpc = g_pc.double().view(EV_D, P) / 3.0 if g_pc is not None and defect != "no_gpc" else torch.zeros(EV_D, P, dtype=torch.float64)
    for i, (h, pr, lg, ge, gem) in enumerate(zip(hs, prs, lgs, (g0, g1, g2), (m0, m1, m2))):
        gl = [ge[k + 1] * sg(lg[k]) for k in range(3)]
        glm = [gem[k + 1] * sg(lg[k]) for k in range(3)]
        q = ge[0] * dv + gl[0] * h[1] + gl[1] * h[2] + gl[2] * h[3] + gpc
        qm = gem[0] * dv + glm[0] * h[1].abs() + glm[1] * h[2].abs() + glm[2] * h[3].abs() + gpc.abs()
        out[f"g{i}.cost"] = pr * (q - (pr * q).sum(0))
        mag[f"g{i}.cost"] = pr * (qm + (pr * qm).sum(0))
        for k, ch in enumerate(EV_CHANNELS[1:]):
            out[f"g{i}.{ch}"] = gl[k] * pr
            mag[f"g{i}.{ch}"] = glm[k] * pr
    shape = lambda k, v: v.view(1, EV_D, H, W) if k == "pc" else v.view(*v.shape[:-1], H, W)   # noqa: E731
    return {k: shape(k, v) for k, v in out.items()}, {k: shape(k, v) for k, v in mag.items()}


@functools.lru_cache(maxsize=None)
def ev_reference(case: EvCase) -> Reference:
    """float64 autograd of ``epilogue64``; the scales from ``ev_explicit``'s magnitudes."""
    scales, zero = _scales(ev_explicit(case)[1])
    return Reference(ev_autograd(case, torch.float64), scales, 1.0, zero)


@functools.lru_cache(maxsize=None)
def ev_f32_out(case: EvCase) -> dict:
    return ev_autograd(case, torch.float32)


def ev_masked(case: EvCase, name: str) -> torch.Tensor:
    """The float64 reference of a tensor, NaN where float32 CPU torch is not finite (``measure``
    passes over those elements)."""
    ref, f32 = ev_reference(case).out[name], ev_f32_out(case)[name]
    return torch.where(torch.isfinite(f32), ref, torch.full_like(ref, NAN))


@functools.lru_cache(maxsize=None)
def ev_f32(case: EvCase) -> dict:
    """{tensor: m of float32 CPU torch} over the elements where it is finite."""
    ref, f32 = ev_reference(case), ev_f32_out(case)
    return {k: measure(f32[k], ev_masked(case, k), ref.scales[k]) for k in EV_TENSORS}


def ev_bound(m_f32: float) -> float:
    return max(FLOOR, F32_FACTOR * m_f32)


# The cases and tensors on which float32 CPU torch is not finite while float64 is
# (tests/test_epilogue_cases.py asserts that this is the whole list): with every evidence logit at
# -120 softplus is exactly 0 in float32, la = 0 and u = 0 / 0.
_G = lambda *chs: tuple(f"g{i}.{c}" for i in range(3) for c in chs)   # noqa: E731
EV_NONFINITE_F32: dict = {"logit_eq-120": ("u", "beta") + _G("cost", "la")}

# The cases and tensors whose float32 CPU torch error is above FLOOR: the 3 m_f32 arm of the bound
# carries them and no other (tests/test_epilogue_cases.py asserts that this is the whole list).
#  * flat and nearly flat costs: the cost gradient is what gp[d] - dot leaves of terms at depths of
#    425 to 935, and the magnitude track does not count the subtraction d1 = a.u - u, which with
#    equal predictions leaves only float32's rounding of u (cot_ch_beta-flat: the beta cotangent
#    reaches the cost and la channels through d1 and d2 alone);
#  * evidence logits of -30 and -80: softplus and its derivative are exp(l), and the 32-term sum
#    that gives l carries an absolute error of some 2^-24 |l|, which exp turns into a relative one;
#  * -120: exp(l) is below float32's smallest subnormal, 0 is its correctly rounded value and the
#    float64 reference (1e-52) is its own scale, so m = 1/2.
EV_F32_ABOVE_FLOOR: dict = {
    "cost_flat": ("g2.cost",),
    "cot_ev-flat": ("g2.cost",),
    "cost_near_flat": _G("cost"),
    "cot_ch_beta-flat": _G("cost", "la"),
    "logit_eq-30": _G("alpha", "beta"),
    "logit_eq-80": ("la", "beta") + _G("alpha", "beta"),
    "logit_eq-120": ("la",) + _G("alpha", "beta"),
    "logit_one_head-120": ("g1.la", "g1.alpha", "g1.beta"),
}
