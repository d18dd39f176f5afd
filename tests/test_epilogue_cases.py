"""The cases of tests/epilogue_cases.py say what tests/test_gpu_epilogue.py believes they say (CPU
only: torch and numpy in float64 and float32, no library):

* the tables are the agreed ones; the softmax columns contain what they are named for, float32
  and float64 torch.softmax have the same NaN pattern on every column and the same zero pattern on
  the non-finite ones, the online recurrence as the kernel has it agrees with torch on every
  column and keeps the bits of the earlier one on the finite columns, and the earlier one (running
  max from -inf) leaves torch on exactly SM_PARENT_DIFFERS;
* the WTA columns tie exactly or differ by WTA_GAP, and the restatement gives on them what they
  are named for (0 * inf = NaN on the second 89, depth 0 where every exp is 0, ...);
* the evidential cases: one-hot softmax exactly 1 and 0 in float32, agreeing heads d1 = d2 = 0
  exactly, logits of -120 NaN in float32 and finite in float64, 19.999 / 20.001 below / above
  softplus's threshold and 20.0 within a few ulp of it, where both branches give the same float32;
  the float64 reference is finite everywhere; ev_explicit equals float64 autograd; float32 CPU
  torch is finite except on EV_NONFINITE_F32 and at most FLOOR except on EV_F32_ABOVE_FLOOR;
* a reference with one defect (alpha's + 0.5 left out, a.la and b.la swapped in beta's term,
  g_pc / 3 left out, the gn a.u added back to dL/dla left out) lies more than 100 bounds from the
  true one on some case and tensor.  Two further candidates turn out to be no defects and are
  asserted as such, not counted.  gu's - gd1 - gd2: gd1 + gd2 = g.be (a.la d1 + b.la d2), and the
  la-weighted deviations from the la-weighted mean sum to zero, so the term is rounding only (a
  sign error in it would be equally invisible: it is dead weight in the formula, kept because
  autograd has it).  The mixture nested as (e0, (e1, e2)): moe_nig is associative (la and alpha
  are sums, u a weighted mean, and beta's term the weighted scatter about the mean, which splits
  into within and between parts), so it differs from the true reference by float64 rounding
  only, beta included;
* the large frame has exactly one partial second stride, and its base is a prime.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import epilogue_cases as ec


# ---------------------------------------------------------------------------------------------
# softmax_depth
# ---------------------------------------------------------------------------------------------
def test_softmax_tables_are_the_agreed_ones():
    assert ec.SM_UNROLL_D == (1, 2, 3, 4, 5, 7, 8, 37) and (ec.SM_B, ec.SM_P) == (2, 257)
    assert set(ec.SM_FINITE) == {"ascending", "descending", "equal", "tie_first_last", "gap_underflow",
                                 "gap_subnormal", "overflow"}
    assert set(ec.SM_NONFINITE) == {"ninf_first", "ninf_middle", "ninf_last", "ninf_all_but_one", "ninf_all",
                                    "pinf_first", "pinf_last", "pinf_twice", "nan_first", "nan_middle", "nan_last",
                                    "pinf_and_ninf"}
    assert all(len(c) == 7 for c in ec.SM_COLUMNS.values())
    v = ec.sm_volume(ec.SM_FINITE["ascending"])
    assert tuple(v.shape) == (2, 7, 1, 257) and bool((v == v[:1, :, :, :1]).all())
    for D in ec.SM_UNROLL_D:
        c = ec.sm_random(D)
        assert tuple(c.shape) == (2, D, 1, 257) and float(c.abs().max()) <= 80.0 and float(c.abs().max()) > 40.0


def test_softmax_columns_are_what_they_are_named_for():
    col = {k: np.asarray(v, np.float32) for k, v in ec.SM_COLUMNS.items()}
    assert (np.diff(col["ascending"]) > 0).all() and (np.diff(col["descending"]) < 0).all()
    assert (col["equal"] == col["equal"][0]).all()
    t = col["tie_first_last"]
    assert t[0] == t[-1] == t.max() and (t[1:-1] < t.max()).all()
    soft32 = lambda c: torch.softmax(torch.tensor(c), 0).numpy()   # noqa: E731
    g = col["gap_underflow"]
    assert (g.max() - np.sort(g)[:-1] >= 104).all()
    assert (soft32(g)[1:] == 0).all() and soft32(g)[0] == 1
    g = col["gap_subnormal"]
    gaps = g.max() - np.sort(g)[:-1]
    assert (gaps >= 88).all() and (gaps <= 103).all()
    tiny = float(np.finfo(np.float32).tiny)
    assert ((soft32(g)[1:] > 0) & (soft32(g)[1:] < tiny)).all()
    o = col["overflow"]
    with np.errstate(over="ignore"):
        assert np.isneginf(np.float32(o[1]) - np.float32(o[0])) and np.isfinite(o).all()
    assert np.isneginf(col["ninf_first"][0]) and np.isneginf(col["ninf_middle"][3]) and np.isneginf(col["ninf_last"][6])
    assert np.isneginf(col["ninf_all_but_one"]).sum() == 6 and np.isneginf(col["ninf_all"]).all()
    assert np.isposinf(col["pinf_first"][0]) and np.isposinf(col["pinf_last"][6]) and np.isposinf(col["pinf_twice"]).sum() == 2
    assert np.isnan(col["nan_first"][0]) and np.isnan(col["nan_middle"][3]) and np.isnan(col["nan_last"][6])
    assert np.isposinf(col["pinf_and_ninf"]).sum() == 1 and np.isneginf(col["pinf_and_ninf"]).sum() == 1
    for name in ec.SM_FINITE:
        assert np.isfinite(col[name]).all(), name


def test_float32_and_float64_torch_softmax_agree_on_the_patterns():
    """So the choice between them as the reference of a pattern cannot matter."""
    for name, c in ec.SM_COLUMNS.items():
        t = torch.tensor(c, dtype=torch.float32)
        s32, s64 = torch.softmax(t, 0), torch.softmax(t.double(), 0)
        assert torch.equal(torch.isnan(s32), torch.isnan(s64)), name
        if name in ec.SM_NONFINITE:
            assert torch.equal(s32 == 0, s64 == 0), name
    # what torch gives: -inf is a term of 0 unless nothing else is there; +inf or NaN poison the column
    soft = lambda n: torch.softmax(torch.tensor(ec.SM_NONFINITE[n]), 0)   # noqa: E731
    for n in ("ninf_first", "ninf_middle", "ninf_last", "ninf_all_but_one"):
        s = soft(n)
        assert torch.equal(s == 0, torch.isneginf(torch.tensor(ec.SM_NONFINITE[n]))) and abs(float(s.sum()) - 1) < 1e-6
    for n in ("ninf_all", "pinf_first", "pinf_last", "pinf_twice", "nan_first", "nan_middle", "nan_last", "pinf_and_ninf"):
        assert bool(torch.isnan(soft(n)).all()), n


def _agrees(got, col):
    t32 = torch.softmax(torch.tensor(col, dtype=torch.float32), 0).numpy()
    t64 = torch.softmax(torch.tensor(col, dtype=torch.float32).double(), 0).numpy()
    ok = ~np.isnan(t32)
    return np.array_equal(np.isnan(got), np.isnan(t32)) and np.allclose(got[ok], t64[ok], rtol=ec.SM_RTOL, atol=ec.SM_ATOL)


def test_online_recurrence_with_and_without_the_fix():
    differs = []
    for name, c in ec.SM_COLUMNS.items():
        new, old = ec.sm_online(c, fixed=True), ec.sm_online(c, fixed=False)
        assert _agrees(new, c), name
        if not _agrees(old, c):
            differs.append(name)
        if name in ec.SM_FINITE:
            assert ec.bits_equal(new, old), name
    assert tuple(differs) == ec.SM_PARENT_DIFFERS
    # the earlier recurrence on the issue's three columns
    assert np.isnan(ec.sm_online((-math.inf, 1.0, 2.0), fixed=False)).all()
    old = ec.sm_online((math.inf, 1.0, 2.0), fixed=False)
    assert np.isnan(old[0]) and (old[1:] == 0).all()
    old = ec.sm_online((1.0, math.inf), fixed=False)
    assert old[0] == 0 and np.isnan(old[1])
    rng = np.random.default_rng(5)
    for D in ec.SM_UNROLL_D:
        c = (rng.random(D) * 160 - 80).astype(np.float32)
        assert ec.bits_equal(ec.sm_online(c, True), ec.sm_online(c, False)) and _agrees(ec.sm_online(c, True), c)


# ---------------------------------------------------------------------------------------------
# standalone WTA
# ---------------------------------------------------------------------------------------------
def _wta(name):
    case = ec.WTA_BY_NAME[name]
    out = ec.wta_restatement(ec.wta_volume(case).view(1, len(case.costs), -1).numpy(), ec.wta_depths(case)[None])
    assert all(bool((v == v[:, :1]).all() or np.isnan(v).all()) for v in out.values())
    return {k: float(v[0, 0]) for k, v in out.items()}, ec.wta_depths(case)


def test_wta_columns_are_what_they_are_named_for():
    assert [c.name for c in ec.WTA_CASES] == ["tie2", "tie3", "all_underflow", "inf_once", "inf_twice", "nan_first",
                                              "nan_middle", "nan_last", "depth_ascending", "depth_descending", "one_plane"]
    for case in ec.WTA_CASES:
        c = np.asarray(case.costs, np.float64)
        c = c[np.isfinite(c)]
        gaps = np.abs(c[:, None] - c[None, :])[np.triu_indices(len(c), 1)]
        assert ((gaps == 0) | (gaps >= ec.WTA_GAP)).all(), case.name
        assert tuple(ec.wta_volume(case).shape) == (1, len(case.costs), 1, 257)
        d = ec.wta_depths(case)
        assert len(d) == len(case.costs) and ((np.diff(d) < 0).all() if case.descending else (np.diff(d) > 0).all())
    r, d = _wta("tie2")
    assert r["depth"] == d[0]                                  # the first of two
    r, d = _wta("tie3")
    assert r["depth"] == d[1]                                  # the first of three
    r, d = _wta("all_underflow")
    assert max(ec.WTA_BY_NAME["all_underflow"].costs) <= -104 and r == {"depth": 0.0, "max_prob": 0.0, "exp_sum": 0.0}
    r, d = _wta("inf_once")
    assert r["depth"] == d[1] and math.isinf(r["max_prob"]) and math.isinf(r["exp_sum"])
    r, d = _wta("inf_twice")
    assert r["depth"] == d[1] and math.isnan(r["max_prob"]) and math.isinf(r["exp_sum"])   # 0 * inf
    r, d = _wta("nan_first")
    assert r["depth"] == 0.0 and math.isnan(r["max_prob"]) and math.isnan(r["exp_sum"])
    r, d = _wta("nan_middle")
    assert r["depth"] == d[0] and math.isnan(r["max_prob"])
    r, d = _wta("nan_last")
    assert r["depth"] == d[1] and math.isnan(r["max_prob"])
    r, d = _wta("depth_ascending")
    r2, d2 = _wta("depth_descending")
    assert r["depth"] == d[3] and r2["depth"] == d2[3] and d[3] != d2[3] and r["exp_sum"] == r2["exp_sum"]
    r, d = _wta("one_plane")
    assert r["depth"] == d[0] and r["max_prob"] == r["exp_sum"] == float(np.exp(np.float32(0.7)))


def test_wta_restatement_is_the_oracle_sweep_rule():
    """The same three lines as oracle.sweep_oracle.sweep's loop body, in torch float32."""
    rng = np.random.default_rng(3)
    cost = rng.standard_normal((2, 6, 19)).astype(np.float32) * 3
    dv = np.stack([np.linspace(425, 935, 6), np.linspace(935, 425, 6)]).astype(np.float32)
    mp, dp, es = (torch.zeros(2, 19) for _ in range(3))
    for d in range(6):
        prob = torch.exp(torch.from_numpy(cost[:, d]))
        flag = (mp < prob).float()
        mp = flag * prob + (1 - flag) * mp
        dp = flag * torch.from_numpy(dv[:, d]).view(2, 1) + (1 - flag) * dp
        es = es + prob
    got = ec.wta_restatement(cost, dv)
    assert ec.bits_equal(got["depth"], dp.numpy())
    np.testing.assert_allclose(got["max_prob"], mp.numpy(), rtol=4 * ec.U)
    np.testing.assert_allclose(got["exp_sum"], es.numpy(), rtol=10 * ec.U)


# ---------------------------------------------------------------------------------------------
# evidential epilogue
# ---------------------------------------------------------------------------------------------
def test_evidential_tables_are_the_agreed_ones():
    names = [c.name for c in ec.EV_CASES]
    assert len(names) == len(set(names)) == 6 + 8 + 3 * 7 + 5
    assert ec.EV_COSTS == ("random", "flat", "near_flat", "onehot_apart", "onehot_agree", "onehot_head0")
    assert ec.EV_LOGITS == ("rand4", "eq19.999", "eq20", "eq20.001", "eq60", "eq-30", "eq-80", "eq-120", "one_head-120")
    assert ec.EV_COTS == ("both", "ev", "pc", "zero", "ch_u", "ch_la", "ch_alpha", "ch_beta")
    assert {(c.cost, c.cot) for c in ec.EV_CASES if c.logit == "rand4" and c.hw == (1, 64)} >= {
        (c, t) for c in ec.EV_COT_COSTS for t in ec.EV_COTS}
    assert {c.hw for c in ec.EV_CASES} == {(1, 64), (1, 1), (1, 255), (1, 256), (1, 257), (257, 1)}
    assert ec.ONEHOT_PLANES == {"onehot_apart": (0, 31, 15), "onehot_agree": (7, 7, 7)} and ec.ONEHOT_GAP == 200.0
    assert ec.FLOOR == 73 * 2.0 ** -24 and ec.F32_FACTOR == 3.0
    for c in ec.EV_CASES:
        heads, g_ev, g_pc = ec.ev_inputs(c)
        H, W = c.hw
        assert all(tuple(h.shape) == (1, 4, 32, H, W) and h.dtype == torch.float32 for h in heads)
        assert g_ev is None or tuple(g_ev.shape) == (4, H, W)
        assert g_pc is None or tuple(g_pc.shape) == (1, 32, H, W)
        assert (g_ev is None) == (c.cot == "pc") and (g_pc is None) == (c.cot not in ("both", "pc", "zero"))
        if c.cot.startswith("ch_"):
            nz = [k for k in range(4) if bool((g_ev[k] != 0).any())]
            assert nz == [("u", "la", "alpha", "beta").index(c.cot[3:])]
    dv = ec.ev_depths()
    assert tuple(dv.shape) == (32,) and float(dv[0]) == 425.0 and float(dv[-1]) == 935.0


def _parts(case, dtype):
    """Per head: softmax, pred, the three logits, in dtype, as epilogue64 forms them."""
    heads, _, _ = ec.ev_inputs(case)
    dv = ec.ev_depths().to(dtype)
    out = []
    for h in heads:
        h = h.to(dtype)
        p = F.softmax(h[:, 0], dim=1)
        out.append((p, (p * dv.view(1, -1, 1, 1)).sum(1), [(h[:, k] * p).sum(1) for k in (1, 2, 3)]))
    return out


def test_evidential_cases_are_what_they_are_named_for():
    by = ec.EV_BY_NAME
    dv = ec.ev_depths()
    # one-hot: exactly 1 and 0 in float32, the predictions 510 apart
    parts = _parts(by["cost_onehot_apart"], torch.float32)
    for (p, pred, _), pl in zip(parts, (0, 31, 15)):
        assert bool((p[:, pl] == 1).all()) and float(p.sum()) == p[:, 0].numel() and bool((pred == dv[pl]).all())
    assert float(parts[1][1][0, 0, 0] - parts[0][1][0, 0, 0]) == 510.0
    # agreeing heads: d1 = d2 = 0 exactly, in both moe levels and both precisions
    for dtype in (torch.float32, torch.float64):
        parts = _parts(by["cost_onehot_agree"], dtype)
        u = [pred for _, pred, _ in parts]
        la = [F.softplus(lg[0]) for _, _, lg in parts]
        u01 = (la[0] * u[0] + u[1] * la[1]) / (la[0] + la[1])
        u012 = ((la[0] + la[1]) * u01 + u[2] * la[2]) / (la[0] + la[1] + la[2])
        for a in (u[0] - u01, u[1] - u01, u01 - u012, u[2] - u012):
            assert bool((a == 0).all())
    parts = _parts(by["cost_onehot_head0"], torch.float32)
    assert bool((parts[0][0][:, 11] == 1).all()) and float(parts[1][0].max()) < 1
    heads = ec.ev_inputs(by["cost_flat"])[0]
    assert all(bool((h[:, 0] == h[0, 0, 0, 0, 0]).all()) for h in heads)
    heads = ec.ev_inputs(by["cost_near_flat"])[0]
    assert all(3e-4 < float(h[:, 0].std()) < 3e-3 for h in heads)
    # the threshold of softplus (20): which side the logits of each case fall on, in float32
    for name, side in (("logit_eq19.999", -1), ("logit_eq20.001", 1), ("logit_eq60", 1)):
        for _, _, lg in _parts(by[name], torch.float32):
            for l in lg:
                assert bool((l > 20).all()) if side > 0 else bool((l < 20).all()), name
    for _, _, lg in _parts(by["logit_eq20"], torch.float32):
        for l in lg:   # on either side by the rounding of the 32-term sum; the branches agree there
            assert float((l - 20).abs().max()) <= 16 * 2.0 ** -19
            assert torch.equal(torch.log1p(torch.exp(l)), l)
    # -30 and -80: la tiny but normal; -120: exactly 0 in float32
    tiny = float(np.finfo(np.float32).tiny)
    for name in ("logit_eq-30", "logit_eq-80"):
        la = ec.ev_f32_out(by[name])["la"]
        assert tiny < float(la.min()) and float(la.max()) < 1e-12, name
    f32, ref = ec.ev_f32_out(by["logit_eq-120"]), ec.ev_reference(by["logit_eq-120"])
    assert bool((f32["la"] == 0).all()) and bool((f32["alpha"] == 4.0).all())
    assert bool(torch.isnan(f32["u"]).all()) and bool(torch.isnan(f32["beta"]).all())
    assert 0 < float(ref.out["la"].max()) < 1e-45
    f32 = ec.ev_f32_out(by["logit_one_head-120"])
    assert float(f32["la"].min()) > 0 and all(bool(torch.isfinite(t).all()) for t in f32.values())


def test_float64_reference_is_finite_and_explicit_formula_equals_autograd():
    for c in ec.EV_CASES:
        ref = ec.ev_reference(c)
        ex, mag = ec.ev_explicit(c)
        for k in ec.EV_TENSORS:
            assert bool(torch.isfinite(ref.out[k]).all()), (c.name, k)
            assert tuple(ex[k].shape) == tuple(ref.out[k].shape) == tuple(mag[k].shape)
            assert bool((mag[k] >= ex[k].abs() * (1 - 1e-12)).all()), (c.name, k)
            assert ec.measure(ex[k], ref.out[k], ref.scales[k]) <= 1e-13, (c.name, k)
        grads = set(ec.EV_GRADS)
        if c.cot == "zero":
            assert set(ref.zero) == grads
        elif c.cot == "pc":
            assert set(ref.zero) == {g for g in grads if not g.endswith(".cost")}
        elif c.cot in ("both", "ev"):
            assert not ref.zero
        for k in ref.zero:
            assert float(ref.out[k].abs().max()) == 0.0, (c.name, k)


def test_float32_cpu_torch_is_below_the_floor_except_on_the_listed_tensors():
    nonfinite, above = {}, {}
    for c in ec.EV_CASES:
        f32o, f32 = ec.ev_f32_out(c), ec.ev_f32(c)
        nf = tuple(k for k in ec.EV_TENSORS if not bool(torch.isfinite(f32o[k]).all()))
        ab = tuple(k for k in ec.EV_TENSORS if f32[k] > ec.FLOOR)
        if nf:
            nonfinite[c.name] = nf
        if ab:
            above[c.name] = ab
    assert nonfinite == ec.EV_NONFINITE_F32
    assert above == ec.EV_F32_ABOVE_FLOOR, above
    # the cancelling cost gradients are where the issue found them: several floors, not orders
    assert ec.ev_f32(ec.EV_BY_NAME["cost_near_flat"])["g2.cost"] < 10 * ec.FLOOR


@pytest.mark.parametrize("defect", ec.EV_DEFECTS)
def test_a_reference_with_one_defect_is_far_from_the_true_one(defect):
    worst = (0.0, "", "")
    for c in ec.EV_CASES:
        if c.name in ec.EV_NONFINITE_F32:
            continue
        ref, f32 = ec.ev_reference(c), ec.ev_f32(c)
        bad, _ = ec.ev_explicit(c, defect)
        for k in ec.EV_TENSORS:
            r = ec.measure(bad[k], ref.out[k], ref.scales[k]) / ec.ev_bound(f32[k])
            worst = max(worst, (r, c.name, k))
    print(f"\ndefect {defect}: {worst[0]:.3g} bounds at {worst[1]} {worst[2]}")
    if defect in ec.EV_NEUTRAL_DEFECTS:   # the same function, up to float64 rounding
        assert worst[0] < 1e-6
    else:
        assert worst[0] > 100.0
        assert worst[2] == {"alpha_half": "alpha", "beta_swap": "beta"}.get(defect, worst[2])


# ---------------------------------------------------------------------------------------------
# the large frame
# ---------------------------------------------------------------------------------------------
def test_large_frame_reaches_one_partial_second_stride():
    stride = ec.GRID_CAP * ec.BLOCK
    assert ec.BIG_HW == 1028 * 1024 == stride + 4096 and ec.BIG_H % 4 == 0 and ec.BIG_W % 4 == 0
    assert (ec.BIG_HW - stride) // ec.BLOCK == 16 < ec.GRID_CAP          # 16 blocks loop, the rest do not
    assert (1024 * 1024) <= stride                                       # the next smaller frame does not loop
    assert ec.BIG_BASE == 4099 and all(ec.BIG_BASE % q for q in range(2, 65)) and stride % ec.BIG_BASE != 0
    t = ec.big_tile(torch.arange(2 * ec.BIG_BASE).view(2, ec.BIG_BASE))
    assert tuple(t.shape) == (2, ec.BIG_HW)
    p = torch.tensor([0, 4098, 4099, stride - 1, stride, ec.BIG_HW - 1])
    assert torch.equal(t[1, p], ec.BIG_BASE + p % ec.BIG_BASE)
    for D in (2, 3, 5):
        c = ec.big_base(D).double()
        assert tuple(c.shape) == (2, D, ec.BIG_BASE)
        gaps = torch.stack([(c[:, d] - c[:, e]).abs() for d in range(D) for e in range(d)])
        assert float(gaps.min()) >= ec.WTA_GAP
    dv = ec.big_depths(3)
    assert tuple(dv.shape) == (2, 3) and bool((dv[0] == dv[1].flip(0)).all()) and float(dv[0, 0]) < float(dv[0, 1])
