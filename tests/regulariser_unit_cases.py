"""Cases and float64 references for the unit-level tests of the ConvLSTM U-Net regulariser.

One U-Net step is six units, each a pure function of tensors that can be read back from the GPU:

    U0   x, h0-, c0-         -> h0, c0
    U1   h0, h1-, c1-        -> h1, c1      (max-pool 2x2 of h0)
    U2   h1, h2-, c2-        -> h2, c2
    U3   h2, h1, h3-, c3-    -> h3, c3      (deconv_0 + GroupNorm(2) + ReLU, cat h1)
    U4   h3, h0, h4-, c4-    -> h4, c4      (deconv_1 ..., cat h0)
    head h4                  -> cost

(``-`` marks the state before the step.)  "Teacher-forced": every unit is recomputed in float64
from the inputs the GPU itself used, so an error neither hides downstream nor accumulates over
planes, and a failure names the unit, the level and the pixel.  ``infer_units`` is that
decomposition.  The training record exposes more per plane; ``train_units`` splits further, each
tensor from the record's own: the gate pre-activations z_k of the five cells, (h_k, c_k) from the
record's z_k, the two deconv outputs u_j, their GroupNorm statistics, and the head.

The true references use oracle.sweep_oracle's ``lstm_cell``, ``deconv_gn_relu`` (``fast=False``)
and the head conv; the primitives below restate them with switches, one per planted fault
(FAULTS): a wrong float64 reference that models one way a kernel could plausibly be wrong.
tests/test_regulariser_unit_cases.py asserts on the CPU that the restatement without a switch
equals the oracle's functions, that every fault moves its unit by >= 10x the GPU test's bound and
that the float32 evaluation of every unit stays inside it; tests/test_gpu_regulariser_units.py runs
the library against the references.  Nothing here loads the library.

Frames (B, H, W): the smallest at which each tiling can go wrong (cells: 8 rows x 32 pixels per
block, the inference cells 0 and 1 2-row x 16-column patches per wave; deconvs: 8 x 32 input
tiles; cells 3 and 4 and the GroupNorm statistics per batch element):

* (1, 4, 4): the minimum; levels 4x4, 2x2, 1x1: every tile partial, every pixel border;
* (2, 8, 36): W crosses the 32-pixel tile by 4, level 1 (4x18) the 16-column patch by 2, level 2 is
  2x9 (odd width, deconv_0's input); B = 2;
* (1, 36, 68): 4 block rows + 4, two tiles + 4; level 1 18x34, level 2 9x17 (odd x odd);
  deconv_1's input 18x34 ragged against 8x32 both ways;
* (2, 12, 132): level 2 is 3x33, a deconv input one column past a 32-wide tile; level 1 6x66; B = 2.
"""
from __future__ import annotations

import functools
import os
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from aarmvs import synthetic as syn
from oracle import sweep_oracle as orc

import fp16_mode_ref as fref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FRAMES = ((1, 4, 4), (2, 8, 36), (1, 36, 68), (2, 12, 132))
STATE_SETS = ("plain", "edge")
HID = (16, 16, 16, 16, 8)
SCALE = (1, 2, 4, 2, 1)
SYN_SEED = 7
GN_EPS = 1e-5

REL = 2e-5         # |got - ref64| <= REL max(1, max|ref64|): the project's per-tensor figure
REL_STATS = 1e-6   # the statistics (fp64 sums of fp32 values): |got - ref64| <= REL_STATS max|ref64|
FAULT_FACTOR = 10.0

INFER_UNITS = {"U0": ("h0", "c0"), "U1": ("h1", "c1"), "U2": ("h2", "c2"), "U3": ("h3", "c3"),
               "U4": ("h4", "c4"), "head": ("cost",)}
TRAIN_TENSORS = (tuple(f"z{k}" for k in range(5)) + tuple(n for k in range(5) for n in (f"h{k}", f"c{k}"))
                 + ("u0", "u1", "stats0", "stats1", "cost"))


class Case(NamedTuple):
    frame: tuple    # (B, H, W)
    sset: str       # "plain" | "edge"
    wkind: str      # "real" | "syn"
    k: int          # the step index of the inference test: rings of 6/4/3/3/2 slots

    @property
    def id(self):
        return f"{'x'.join(map(str, self.frame))}-{self.sset}-{self.wkind}-k{self.k}"


# k = 1, 2, 5, 6 over the cases: step k reads slot k % r and writes slot (k + 1) % r, so these wrap
# the rings of cell 4 (k = 1), cells 2 and 3 (2), cells 0, 2, 3, 4 (5) and start a second lap (6).
# The synthetic-weight edge case takes k = 3, the one step at which cell 1's ring of 4 wraps.
_KS = (1, 2, 5, 6)
CASES = tuple(Case(f, s, "real", _KS[(i + j) % 4]) for i, f in enumerate(FRAMES) for j, s in enumerate(STATE_SETS)) + (
    Case((2, 8, 36), "plain", "syn", 5), Case((2, 8, 36), "edge", "syn", 3))
BY_ID = {c.id: c for c in CASES}


def level_shape(frame, k):
    B, H, W = frame
    return B, HID[k], H // SCALE[k], W // SCALE[k]


# ----------------------------------------------------------------------------------
# weights and inputs
# ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(kind: str, dtype=torch.float32) -> dict:
    if kind == "real":
        g = np.load(os.path.join(GOLDEN, "real_weights_sweep.npz"), allow_pickle=False)
        P = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    else:
        P = {k: torch.from_numpy(v) for k, v in syn.sweep_weights(SYN_SEED).items()}
    return {k: v.to(dtype) for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def x_scale() -> float:
    """The rms of a real cost slice: plane 0 of fwd_range_cases' base frame under the real weights."""
    import fwd_range_cases as frc
    x0 = frc.references(frc.BASE).x0
    return float(torch.sqrt((x0 * x0).mean()))


def _checkerboard(h0: np.ndarray, rng) -> None:
    """h0-'s last two columns: signs alternate like a checkerboard whose phase moves every two
    window rows, and one of each 2x2 window's two positive entries is the larger, so the window
    maxima at the right edge fall on each of the four positions in turn."""
    B, C, H, W = h0.shape
    for y in range(H):
        wy = y // 2
        for j in range(2):
            sign = 1.0 if (y + j + wy // 2) % 2 == 0 else -1.0
            big = (y % 2) == (wy % 2)
            mag = (0.9 if big else 0.45) * rng.uniform(0.6, 1.0, size=(B, C)).astype(np.float32)
            h0[:, :, y, W - 2 + j] = sign * mag


def zero_row(Hk: int) -> int:
    """The row of h- that the edge set zeroes: the first (a border row; the checkerboard keeps
    every window below it)."""
    return 0


ZERO_CHANNEL = 3


@functools.lru_cache(maxsize=None)
def inputs(frame: tuple, sset: str) -> dict:
    """{'x' [B,32,H,W], 'hp' / 'cp' / 'stale': five float32 tensors each}: the injected cost slice,
    the state before the step and what the ring slot of the step before holds.  Seeded; shared,
    never modified."""
    B, H, W = frame
    rng = np.random.default_rng(1000 * H + W + (0 if sset == "plain" else 500000))
    f32 = np.float32
    out = {"x": (rng.standard_normal((B, 32, H, W)) * x_scale()).astype(f32), "hp": [], "cp": [], "stale": []}
    for k in range(5):
        shp = level_shape(frame, k)
        h = rng.uniform(-0.999, 0.999, size=shp).astype(f32)
        c = rng.uniform(-4.0, 4.0, size=shp).astype(f32)
        stale = rng.uniform(-0.999, 0.999, size=shp).astype(f32)
        if sset == "edge":
            # |c-| up to 30 on a tenth of the pixels (tanh(c) saturates, the forget gate carries)
            _, C, Hk, Wk = shp
            mask = rng.random((B, 1, Hk, Wk)) < 0.1
            mask[:, 0, Hk - 1, Wk - 1] = True
            big = rng.uniform(-30.0, 30.0, size=shp).astype(f32)
            c = np.where(mask, big, c)
            c[:, 0, Hk - 1, Wk - 1] = [25.0 if b % 2 == 0 else -27.0 for b in range(B)]
            if k == 0:
                _checkerboard(h, rng)
            h[:, ZERO_CHANNEL] = 0.0
            h[:, :, zero_row(Hk)] = 0.0
        out["hp"].append(h)
        out["cp"].append(c)
        out["stale"].append(stale)
    return {k: (torch.from_numpy(v) if k == "x" else [torch.from_numpy(t) for t in v]) for k, v in out.items()}


# ----------------------------------------------------------------------------------
# planted faults
# ----------------------------------------------------------------------------------
# (name, what the kernel would have done wrong); a fault is applied as (name, k): to cell k / its unit
FAULTS = {
    "seam": "the conv drops the taps that cross the tile seam column (x = 32; x = 16 for cell 1's "
            "2x16 patches) or the last partial 8-row block",
    "pool": "the max-pool window at the last column and the last row is shifted by one pixel",
    "stale": "cell k's h- is taken from the ring slot of the step before",
    "c_elem0": "element 1 of a per-element launch uses element 0's c-",
    "gn_elem0": "element 1's GroupNorm uses element 0's statistics",
    "deconv_col": "the deconv's input columns past its last full 32-wide tile contribute nothing",
    "swap_if": "the i and f gate blocks are exchanged for the last hidden-channel quad",
}


def seams(frame, k):
    """(columns, rows) at which cell k's tiling has a seam inside its image."""
    _, _, Hk, Wk = level_shape(frame, k)
    col = 16 if k == 1 else 32
    r0 = (Hk // 8) * 8
    return ([col] if col < Wk else []), ([r0] if 0 < r0 < Hk else [])


def applicable(frame) -> tuple:
    """Every (fault, cell) that exists on the frame."""
    B, H, W = frame
    out = []
    for k in range(5):
        if any(seams(frame, k)):
            out.append(("seam", k))
        out += [("stale", k), ("swap_if", k)]
    out += [("pool", 1), ("pool", 2)]
    if B > 1:
        out += [("c_elem0", 3), ("c_elem0", 4), ("gn_elem0", 3), ("gn_elem0", 4)]
    for k, Wi in ((3, W // 4), (4, W // 2)):
        if Wi > 32 and Wi % 32:
            out.append(("deconv_col", k))
    return tuple(out)


# ----------------------------------------------------------------------------------
# primitives (dtype-generic; rnd: the fp16 mode's operand rounding; fault: (name, k) or None)
# ----------------------------------------------------------------------------------
def _cw(P, k):
    return (P[f"cost_regularization.cell_list.{k}.conv.weight"], P[f"cost_regularization.cell_list.{k}.conv.bias"])


def round_operand(t):
    """fp16_mode_ref's operand rounding (11 significant bits), kept in t's dtype."""
    return fref.round11(t).to(t.dtype)


def cell_z(P, k, inp, hp, frame, rnd=None, fault=None):
    """conv3x3(cat[inp, h-]) + b of cell k."""
    w, b = _cw(P, k)
    a = torch.cat([inp, hp], 1)
    if rnd is not None:
        a, w = rnd(a), rnd(w)
    if fault != ("seam", k):
        return F.conv2d(a, w, b, padding=1)
    cols, rows = seams(frame, k)
    Hk, Wk = a.shape[2:]
    out = a.new_empty(a.shape[0], w.shape[0], Hk, Wk)
    xs, ys = [0] + cols + [Wk], [0] + rows + [Hk]
    for y0, y1 in zip(ys[:-1], ys[1:]):      # each strip on its own: zero padding at the seams
        for x0, x1 in zip(xs[:-1], xs[1:]):
            out[:, :, y0:y1, x0:x1] = F.conv2d(a[:, :, y0:y1, x0:x1], w, b, padding=1)
    return out


def gates(z, cp, k, fault=None):
    """ConvLSTMCell's gate math (module.py:83-90): (h, c) from z [B, 4 hid, h, w] and c-."""
    hid = HID[k]
    i, f, o, g = torch.split(z, hid, dim=1)
    if fault == ("swap_if", k):
        i, f = i.clone(), f.clone()
        i[:, hid - 4:], f[:, hid - 4:] = z[:, 2 * hid - 4: 2 * hid], z[:, hid - 4: hid]
    if fault == ("c_elem0", k):
        cp = cp.clone()
        cp[1] = cp[0]
    c = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def pool(h, k, fault=None):
    """max_pool2d(h, 2, 2), the input of cell k."""
    p = F.max_pool2d(h, 2, 2)
    if fault == ("pool", k):
        H, W = h.shape[2:]
        ninf = float("-inf")
        pc = F.max_pool2d(F.pad(h, (1, 0, 0, 0), value=ninf)[..., :W], 2, 2)      # windows one column left
        pr = F.max_pool2d(F.pad(h, (0, 0, 1, 0), value=ninf)[..., :H, :], 2, 2)   # windows one row up
        p = p.clone()
        p[:, :, -1, :] = pr[:, :, -1, :]
        p[:, :, :, -1] = pc[:, :, :, -1]
    return p


def deconv(P, j, x, rnd=None, fault=None):
    """u_j: the transposed conv of deconv_j plus bias (module.py:269-285)."""
    k = f"cost_regularization.deconv_{j}."
    w = P[k + "conv.weight"]
    if fault == ("deconv_col", 3 + j):
        x = x.clone()
        x[..., (x.shape[3] // 32) * 32:] = 0.0
    if rnd is not None:
        x, w = rnd(x), rnd(w)
    return F.conv_transpose2d(x, w, P[k + "conv.bias"], stride=2, padding=1, output_padding=1)


def gn_stats(u):
    """[B, 2 groups, (sum, sum of squares)] of u [B, 16, h, w]: the record's statistics."""
    B = u.shape[0]
    g = u.reshape(B, 2, -1)
    return torch.stack([g.sum(2), (g * g).sum(2)], 2)


def gn_relu(P, j, u, stats, fault=None):
    """deConvGnReLU's GroupNorm(2) + ReLU of u from given statistics (mean = s / n,
    var = ss / n - mean^2 as the cells form them)."""
    k = f"cost_regularization.deconv_{j}."
    B, C, h, w = u.shape
    if fault == ("gn_elem0", 3 + j):
        stats = stats.clone()
        stats[1] = stats[0]
    n = 8.0 * h * w
    mean = stats[:, :, 0] / n
    var = (stats[:, :, 1] / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    xh = (u.reshape(B, 2, -1) - mean.unsqueeze(2)) * rstd.unsqueeze(2)
    y = xh.reshape(B, C, h, w) * P[k + "gn.weight"].view(1, C, 1, 1) + P[k + "gn.bias"].view(1, C, 1, 1)
    return F.relu(y)


def head(P, h4):
    return F.conv2d(h4, P["cost_regularization.conv_0.weight"], P["cost_regularization.conv_0.bias"], padding=1)


# ----------------------------------------------------------------------------------
# the units
# ----------------------------------------------------------------------------------
def to_dtype(t: dict, dtype) -> dict:
    return {k: ([v.to(dtype) for v in val] if isinstance(val, (list, tuple)) else val.to(dtype))
            for k, val in t.items()}


def infer_units(P, t, frame, rnd=None, fault=None, oracle=False):
    """The six units of one step -> {'h0', 'c0', ..., 'h4', 'c4', 'cost'} in the dtype of P and t.
    t: 'x', 'hp', 'cp' (the state before), 'stale', and 'h' = [h0, h1, h2, h3, h4], the unit
    outputs that feed later units (the GPU's own in the GPU test).  ``oracle``: through
    oracle.sweep_oracle's functions (no rnd, no fault): what the true references use."""
    hp, cp, h = t["hp"], t["cp"], t["h"]
    if fault is not None and fault[0] == "stale":
        hp = list(hp)
        hp[fault[1]] = t["stale"][fault[1]]
    out = {}

    def cell(k, inp):
        if oracle:
            out[f"h{k}"], out[f"c{k}"] = orc.lstm_cell(inp, hp[k], cp[k], *_cw(P, k))
        else:
            out[f"h{k}"], out[f"c{k}"] = gates(cell_z(P, k, inp, hp[k], frame, rnd, fault), cp[k], k, fault)

    def up(j, src):
        if oracle:
            return orc.deconv_gn_relu(src, P, f"deconv_{j}", fast=False)
        u = deconv(P, j, src, rnd, fault)
        return gn_relu(P, j, u, gn_stats(u), fault)

    cell(0, t["x"])
    cell(1, pool(h[0], 1, fault))
    cell(2, pool(h[1], 2, fault))
    cell(3, torch.cat([up(0, h[2]), h[1]], 1))
    cell(4, torch.cat([up(1, h[3]), h[0]], 1))
    out["cost"] = head(P, h[4])
    return out


def train_units(P, r, frame, fault=None):
    """The training record's tensors of one plane, each from the record's own -> {'z0'..'z4', 'h0',
    'c0', ..., 'u0', 'u1', 'stats0', 'stats1', 'cost'}.  r: 'x', 'hp', 'cp', 'stale', 'h' [5], 'z'
    [5] (NCHW, gates i, f, o, g), 'u' [2], 'stats' [2] ([B, 2, 2])."""
    hp, cp, h, z, u, st = r["hp"], r["cp"], r["h"], r["z"], r["u"], r["stats"]
    if fault is not None and fault[0] == "stale":
        hp = list(hp)
        hp[fault[1]] = r["stale"][fault[1]]
    ins = [r["x"], pool(h[0], 1, fault), pool(h[1], 2, fault),
           torch.cat([gn_relu(P, 0, u[0], st[0], fault), h[1]], 1),
           torch.cat([gn_relu(P, 1, u[1], st[1], fault), h[0]], 1)]
    out = {}
    for k in range(5):
        out[f"z{k}"] = cell_z(P, k, ins[k], hp[k], frame, None, fault)
        out[f"h{k}"], out[f"c{k}"] = gates(z[k], cp[k], k, fault)
    for j, src in ((0, h[2]), (1, h[3])):
        out[f"u{j}"] = deconv(P, j, src, None, fault)
        out[f"stats{j}"] = gn_stats(u[j])
    out["cost"] = head(P, h[4])
    return out


def chain(P, t, frame, rnd=None):
    """One whole step evolved from t's 'x', 'hp', 'cp' in P's dtype: every tensor a GPU run would
    leave (the CPU tests' stand-in for what is read back): 'h', 'c', 'z', 'u', 'stats', 'cost'."""
    hp, cp = t["hp"], t["cp"]
    h, c, z, u, st = [], [], [], [], []

    def cell(k, inp):
        z.append(cell_z(P, k, inp, hp[k], frame, rnd))
        hk, ck = gates(z[k], cp[k], k)
        h.append(hk)
        c.append(ck)

    def up(j, src):
        u.append(deconv(P, j, src, rnd))
        st.append(gn_stats(u[j]))
        return gn_relu(P, j, u[j], st[j])

    cell(0, t["x"])
    cell(1, pool(h[0], 1))
    cell(2, pool(h[1], 2))
    cell(3, torch.cat([up(0, h[2]), h[1]], 1))
    cell(4, torch.cat([up(1, h[3]), h[0]], 1))
    return {"h": h, "c": c, "z": z, "u": u, "stats": st, "cost": head(P, h[4])}


def fault_target(fault, training=False) -> tuple:
    """The tensors in which a fault must show: its unit's outputs."""
    name, k = fault
    if not training:
        return INFER_UNITS[f"U{k}"]
    if name in ("seam", "pool", "stale", "gn_elem0"):
        return (f"z{k}",)
    if name == "deconv_col":
        return (f"u{k - 3}",)
    return (f"h{k}", f"c{k}")    # c_elem0, swap_if: the gate update


# ----------------------------------------------------------------------------------
# bounds and comparisons
# ----------------------------------------------------------------------------------
def bound(name: str, ref64: torch.Tensor):
    """The GPU test's bound on |got - ref64| for the tensor ``name``: a float, or for the
    statistics a [1, 1, 2] tensor (the sums and the sums of squares each against their own
    largest)."""
    if name.startswith("stats"):
        return REL_STATS * ref64.abs().amax(dim=(0, 1), keepdim=True)
    return REL * max(1.0, float(ref64.abs().max()))


def worst(name: str, got: torch.Tensor, ref64: torch.Tensor):
    """(max over elements of |got - ref64| / bound, its index, the absolute error there)."""
    err = (got.double() - ref64).abs()
    ratio = err / bound(name, ref64)
    i = int(torch.argmax(ratio))
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    return float(ratio.reshape(-1)[i]), idx, float(err.reshape(-1)[i])


# ----------------------------------------------------------------------------------
# CPU-side references of a case (the GPU test builds its own from what it reads back)
# ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_reference(case: Case) -> dict:
    """The case's step evolved in float64, rounded to float32 as a GPU run's tensors are, and the
    float64 / float32 unit references from those: {'t' (float32 inputs incl. 'h', 'z', 'u',
    'stats'), 'inf64', 'inf32', 'trn64', 'trn32'}.  Computed once per process, never modified."""
    P64, P32 = weights(case.wkind, torch.float64), weights(case.wkind, torch.float32)
    t = dict(inputs(case.frame, case.sset))
    with torch.no_grad():
        ev = chain(P64, to_dtype(t, torch.float64), case.frame)
        for key in ("h", "z", "u"):
            t[key] = [v.float() for v in ev[key]]
        t["stats"] = [gn_stats(v.double()) for v in t["u"]]    # fp64 sums of the fp32 values
        t64, t32 = to_dtype(t, torch.float64), to_dtype(t, torch.float32)
        return {"t": t,
                "inf64": infer_units(P64, t64, case.frame, oracle=True),
                "inf32": infer_units(P32, t32, case.frame, oracle=True),
                "trn64": train_units(P64, t64, case.frame),
                "trn32": train_units(P32, t32, case.frame)}


# ----------------------------------------------------------------------------------
# the training record's layout (csrc/aarmvs_internal.h TrainLayout, convlstm.hip train_layout)
# ----------------------------------------------------------------------------------
def _al(n):
    return (n + 63) // 64 * 64


def record_layout(frame) -> dict:
    """Offsets in elements (floats; the statistics in doubles) within one plane's slab of each
    record buffer.  Every tensor is NHWC; z is planar, [B][hid/4][4 gates][H W][4]; the
    statistics are [B][2 deconvs][2 groups][32 slots][2] with the sums in slot 0
    (reg_stat_index)."""
    B, H, W = frame
    px = [B * (H // s) * (W // s) for s in SCALE]
    L = {"x_plane": B * H * W * 32, "h_off": [], "c_off": [], "z_off": [], "px": px}
    o = 0
    for k in range(5):
        L["h_off"].append(o)
        o += _al(px[k] * HID[k])
        L["c_off"].append(o)
        o += _al(px[k] * HID[k])
    L["state_slab"] = o
    o = 0
    for k in range(5):
        L["z_off"].append(o)
        o += _al(px[k] * 4 * HID[k])
    L["z_slab"] = o
    L["u_off"] = [0, _al(B * (H // 2) * (W // 2) * 16)]
    L["u_slab"] = L["u_off"][1] + _al(B * H * W * 16)
    L["stats_slab"] = B * 4 * 32 * 2
    return L


def state_views(state_f32: torch.Tensor, frame, slab: int):
    """([h_k], [c_k]) NCHW views of state slab ``slab`` of a record's float32 state buffer."""
    L = record_layout(frame)
    base = slab * L["state_slab"]
    hs, cs = [], []
    for k in range(5):
        B, C, Hk, Wk = level_shape(frame, k)
        n = B * C * Hk * Wk
        for off, dst in ((L["h_off"][k], hs), (L["c_off"][k], cs)):
            dst.append(state_f32[base + off: base + off + n].view(B, Hk, Wk, C).permute(0, 3, 1, 2))
    return hs, cs


def parse_record(rec: dict, frame, i: int) -> dict:
    """Plane ``i`` (record-relative) of a record's buffers (uint8 tensors, any device) as float32 /
    float64 CPU tensors in train_units' form, plus 'h' and 'c', the state the plane left."""
    B, H, W = frame
    L = record_layout(frame)
    f = {k: rec[k].view(torch.float32) for k in ("x", "state", "z", "u")}
    r = {"x": f["x"][i * L["x_plane"]: (i + 1) * L["x_plane"]].view(B, H, W, 32).permute(0, 3, 1, 2)}
    r["hp"], r["cp"] = state_views(f["state"], frame, i)
    r["h"], r["c"] = state_views(f["state"], frame, i + 1)
    r["z"], r["u"], r["stats"] = [], [], []
    for k in range(5):
        _, C, Hk, Wk = level_shape(frame, k)
        o = i * L["z_slab"] + L["z_off"][k]
        z = f["z"][o: o + B * 4 * C * Hk * Wk].view(B, C // 4, 4, Hk * Wk, 4)
        # [B][quad][gate][HW][4] -> [B, (gate, channel = 4 quad + lane), H, W]
        r["z"].append(z.permute(0, 2, 1, 4, 3).reshape(B, 4 * C, Hk, Wk))
    for j, s in ((0, 2), (1, 1)):
        o = i * L["u_slab"] + L["u_off"][j]
        n = B * 16 * (H // s) * (W // s)
        r["u"].append(f["u"][o: o + n].view(B, H // s, W // s, 16).permute(0, 3, 1, 2))
    st = rec["stats"].view(torch.float64)[i * L["stats_slab"]: (i + 1) * L["stats_slab"]].view(B, 2, 2, 32, 2)
    for j in range(2):
        r["stats"].append(st[:, j, :, 0, :])
    return {k: ([v.cpu().contiguous() for v in val] if isinstance(val, list) else val.cpu().contiguous())
            for k, val in r.items()}
