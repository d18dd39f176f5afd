"""The cases of tests/aux_kernel_cases.py say what tests/test_gpu_aux_kernels.py believes they
say (CPU only: torch in float64 and float32, no library):

* the group-norm shapes reach nb = ceil(HW / 4096) = 1, 2, 3 and 257, one forward case has
  cg * nb > 256, the non-contiguous inputs are non-contiguous, the constant groups have var == 0
  and a dgamma of exactly 0, the cancelling cotangent's dx is almost entirely cancellation;
* the gate grid holds, in float32, sigmoid == 1, sigmoid == 0, tanh(c) == +-1 and exp(-z) == inf,
  and its float64 reference is finite everywhere; the non-finite case's inf / NaN pattern is the
  same in float32 and float64 torch; every gate block of the index cases has its own mean;
* every deform position p0 + pn + offset is the same number in float32 and float64, every offset
  pattern contains what it is named for, the explicit float64 formula that supplies the sums of
  absolute terms equals float64 autograd of planar_val, and the collision case's target pixels
  receive exactly 9 h w terms of one sign, the largest of them more than ten bounds large; the
  terms of gx summed in float32 in random orders stay within 3/4 of the bound;
* float32 CPU torch's own m is at most floor * kappa on every case and tensor but the listed
  ones, so that the 3 * m_f32 arm of the bound carries nothing else;
* a reference with two gate blocks swapped, with one dL/dpr term negated, or with lane 31 left
  out of a channel sum is more than 100 bounds away from the true one on at least one case.
"""
import math

import pytest
import torch

import aux_kernel_cases as ac


# ---------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------
def test_case_tables_are_the_agreed_ones():
    gn = {c.name: (c.shape, c.G) for c in ac.GN_CASES}
    for hw in (1, 255, 4095, 4096, 4097, 8193):
        assert gn[f"hw{hw}"] == ((2, 4, 1, hw), 2)
    assert gn["cg1"] == ((2, 6, 5, 7), 6) and gn["g1_c130"] == ((1, 130, 1, 4097), 1)
    assert gn["plane1024x1025"] == ((1, 1, 1024, 1025), 1) and gn["nd5"] == ((1, 4, 3, 5, 7), 2)
    data = ("affine_wb", "affine_none", "affine_w", "affine_b", "noncontig_x", "noncontig_gy", "mean100",
            "mean1000", "std1e-4", "std1e18", "std1e-20", "const_groups", "const_one_group", "gy_zero", "gy_const")
    assert all(gn[n] == ((2, 8, 13, 17), 2) for n in data) and len(gn) == 10 + len(data)
    assert {c.affine for c in ac.GN_CASES} == {"wb", "none", "w", "b"}
    assert {c.name for c in ac.GN_CASES if c.repeat} == {"hw4097", "plane1024x1025"}
    # the only large case is the one 4 MB plane
    assert max(math.prod(c.shape) for c in ac.GN_CASES if c.name != "plane1024x1025") <= 130 * 4097

    assert ac.GATE_Z == (0.0, 0.5, -0.5, 8.0, -8.0, 17.0, -17.0, 30.0, -30.0, 89.0, -89.0, 200.0, -200.0)
    assert ac.GATE_C == (0.0, 1e-3, -1e-3, 1.0, -1.0, 9.5, -9.5, 50.0, -50.0, 1e4, -1e4)
    gates = {c.name: c.shape for c in ac.GATE_CASES}
    assert gates["grid"] == (1, 1, 13 ** 4 * 11) and gates["grid"][2] % 256 != 0
    assert {gates[n] for n in gates if n.startswith("idx")} == {(3, 5, 63), (2, 1, 1), (1, 16, 1), (4, 3, 257)}
    assert ac.GATE_COTS == ("both", "dh", "dc") and ac.GATE_BY_NAME["grid"].repeat

    assert ac.DF_SHAPES == ((1, 5, 7, 1), (2, 9, 11, 1), (1, 13, 9, 2), (1, 1, 1, 1))
    assert (ac.df_out_hw(ac.DF_CASES[0])[0] * ac.df_out_hw(ac.DF_CASES[0])[1] * 9) % 8 != 0   # 315 items
    dense = {(c.shape, c.pattern, c.mask) for c in ac.DF_CASES if c.cot == "dense"}
    assert dense == {(s, p, m) for s in ac.DF_SHAPES for p in ac.DF_PATTERNS for m in ac.DF_MASKS}
    cots = {(c.pattern, c.cot) for c in ac.DF_CASES if c.cot not in ("dense", "pos")}
    assert cots == {(p, c) for p in ac.DF_PATTERNS for c in ("lane0", "lane15", "lane16", "lane31", "tap4")}
    assert ac.DF_COLLISION.shape == (1, 9, 11, 1) and ac.DF_COLLISION in ac.DF_CASES
    assert len(ac.DF_CASES) == len(ac.DF_BY_NAME) == 4 * 5 * 4 + 5 * 5 + 1


# ---------------------------------------------------------------------------------------------
# group norm
# ---------------------------------------------------------------------------------------------
def test_group_norm_shapes_reach_every_path():
    nbs = {ac.gn_nb(c) for c in ac.GN_CASES}
    assert nbs >= {1, 2, 3, 257}
    assert ac.gn_nb(ac.GN_BY_NAME["hw4096"]) == 1 and ac.gn_nb(ac.GN_BY_NAME["hw4097"]) == 2
    # forward stats loop: cg * nb partials per group, strided by the block's 256 threads
    over = [c.name for c in ac.GN_CASES if (c.shape[1] // c.G) * ac.gn_nb(c) > ac.GN_THREADS]
    assert "g1_c130" in over and (130 // 1) * ac.gn_nb(ac.GN_BY_NAME["g1_c130"]) == 260
    # backward stats loop: nb partials per channel, strided likewise
    assert [c.name for c in ac.GN_CASES if ac.gn_nb(c) > ac.GN_THREADS] == ["plane1024x1025"]
    assert any(c.shape[1] == c.G and c.G > 1 for c in ac.GN_CASES)


def test_group_norm_inputs_are_what_they_are_named_for():
    for name in ("noncontig_x", "noncontig_gy"):
        x, _, _, gy = ac.gn_inputs(ac.GN_BY_NAME[name])
        assert x.is_contiguous() == (name != "noncontig_x") and gy.is_contiguous() == (name != "noncontig_gy")
    for c in ac.GN_CASES:
        x, w, b, gy = ac.gn_inputs(c)
        assert (w is not None) == ("w" in c.affine) and (b is not None) == ("b" in c.affine)
        assert x.dtype == gy.dtype == torch.float32 and tuple(x.shape) == tuple(gy.shape) == c.shape
        assert bool(torch.isfinite(x).all())
        for t in ac.gn_reference(c).out.values():
            assert t is None or bool(torch.isfinite(t).all()), c.name
    for name, (mean, std) in ac.GN_MEAN_STD.items():
        if name == "randn":
            continue
        x = ac.gn_inputs(ac.GN_BY_NAME[name])[0].double()
        assert abs(float(x.mean()) - mean) <= 0.1 * std and 0.9 * std <= float(x.std()) <= 1.1 * std, name
    assert 90 < ac.gn_reference(ac.GN_BY_NAME["mean100"]).kappa < 120
    assert 900 < ac.gn_reference(ac.GN_BY_NAME["mean1000"]).kappa < 1200
    # constant groups: var == 0 exactly, xhat == 0, dgamma exactly 0 in the float64 reference
    case = ac.GN_BY_NAME["const_groups"]
    xg = ac.gn_inputs(case)[0].view(2, 2, -1)
    assert bool((xg == xg[:, :, :1]).all()) and bool((xg[:, :, 0] != 0).all())
    ref = ac.gn_reference(case)
    assert float(ref.out["dgamma"].abs().max()) == 0.0 and ref.zero == ("dgamma",)
    assert float((ref.out["y"] - ac.gn_inputs(case)[2].double().view(1, 8, 1, 1)).abs().max()) <= 1e-12   # y = beta
    xg = ac.gn_inputs(ac.GN_BY_NAME["const_one_group"])[0].view(2, 2, -1)
    assert bool((xg[:, 0] == xg[:, 0, :1]).all()) and float(xg[:, 1].std()) > 1.0
    # zero cotangent: every gradient exactly 0
    ref = ac.gn_reference(ac.GN_BY_NAME["gy_zero"])
    assert set(ref.zero) == {"dx", "dgamma", "dbeta"}
    assert all(float(ref.out[k].abs().max()) == 0.0 for k in ref.zero)
    # the cancelling cotangent: |dx| is a 1e-5-th of its uncancelled magnitude
    ref = ac.gn_reference(ac.GN_BY_NAME["gy_const"])
    assert float(ref.out["dx"].abs().max()) <= 1e-5 * ref.scales["dx"]
    assert all(not ac.gn_reference(c).zero for c in ac.GN_CASES if c.name not in ("const_groups", "gy_zero"))


# ---------------------------------------------------------------------------------------------
# LSTM gates
# ---------------------------------------------------------------------------------------------
def test_gate_grid_saturates_in_float32_and_not_in_float64():
    case = ac.GATE_BY_NAME["grid"]
    z, c, dh, dc = ac.gate_inputs(case)
    assert tuple(z.shape) == (1, 4, 1, 13 ** 4 * 11) and tuple(c.shape) == (1, 1, 1, 13 ** 4 * 11)
    rows = torch.cat([z[0, :, 0], c[0, :, 0]]).t()
    assert len({tuple(r) for r in rows[:: 997].tolist()}) == len(rows[:: 997])   # a product, not a repeat
    for k in range(4):
        assert set(z[0, k, 0].tolist()) == set(ac.GATE_Z)
    assert set(c.flatten().tolist()) == {float(torch.tensor(v)) for v in ac.GATE_C}
    s = torch.sigmoid(z)
    assert bool((s == 1).any()) and bool((s == 0).any())
    assert bool((torch.sigmoid(torch.tensor(17.0)) == 1)) and bool((1 - torch.sigmoid(torch.tensor(17.0)) == 0))
    assert bool(torch.isinf(torch.exp(-z)).any()) and bool(torch.isinf(torch.exp(torch.tensor(89.0))))
    f32 = ac.gate_f32_out(case, "both")
    tc = torch.tanh(f32["c"])
    assert bool((tc == 1).any()) and bool((tc == -1).any())
    assert float(torch.tanh(torch.tensor(9.5))) == 1.0 and float(torch.tanh(torch.tensor(9.5, dtype=torch.float64))) < 1.0
    for cot in ac.GATE_COTS:
        ref = ac.gate_reference(case, cot)
        assert all(bool(torch.isfinite(t).all()) for t in ref.out.values()) and not ref.zero
        # in float64 nothing saturates at 17 or 30: the gradient there is small, not 0
        assert all(bool(torch.isfinite(t).all()) for t in ac.gate_f32_out(case, cot).values())
    both = ac.gate_reference(case, "both").out
    assert float((both["dz"] != 0).double().mean()) > 0.5
    assert float(dh.std()) > 0.9 and float(dc.std()) > 0.9


def test_gate_index_cases_tell_the_blocks_apart():
    for case in ac.GATE_CASES:
        if case.kind != "index":
            continue
        B, hid, HW = case.shape
        z, c, dh, dc = ac.gate_inputs(case)
        assert tuple(z.shape) == (B, 4 * hid, 1, HW) and tuple(c.shape) == (B, hid, 1, HW)
        if B * hid * HW >= 256:
            means = z.view(B, 4, -1).mean((0, 2))
            assert float((means - torch.tensor(ac.GATE_MEANS)).abs().max()) < 0.25, (case.name, means)
    assert len(set(ac.GATE_MEANS)) == 4


def test_gate_nonfinite_case_has_one_pattern_in_float32_and_float64():
    case = ac.GATE_BY_NAME["nonfinite"]
    z, c, _, _ = ac.gate_inputs(case)
    assert int(torch.isinf(z).sum()) == len(ac.NONFINITE_Z) and int(torch.isinf(c).sum()) == len(ac.NONFINITE_C)
    seen = set()
    for cot in ac.GATE_COTS:
        ref, f32 = ac.gate_reference(case, cot).out, ac.gate_f32_out(case, cot)
        for k in ac.GATE_TENSORS:
            p64, p32 = ac.nonfinite_pattern(ref[k]), ac.nonfinite_pattern(f32[k])
            assert torch.equal(p64, p32), (cot, k)
            seen |= set(p64.flatten().tolist())
            assert int((p64 != 0).sum()) <= 4 * (len(ac.NONFINITE_Z) + len(ac.NONFINITE_C))   # isolated
        assert bool(torch.isnan(ref["c"]).any()) and bool(torch.isinf(ref["c"]).any())
        assert bool(torch.isnan(ref["dz"]).any())
    assert seen == {0, 1, 2, 3}   # finite, +inf, -inf and NaN all occur


# ---------------------------------------------------------------------------------------------
# deformable sampling
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ac.DF_CASES if c.mask in ("rand", "pos") and c.cot in ("dense", "pos")])
def test_deform_positions_and_patterns(name):
    case = ac.DF_BY_NAME[name]
    _, offset, _, _ = ac.df_inputs(case)
    # exact positions: the float32 and the float64 floor cannot disagree
    p32, p64 = ac.df_positions(case, offset, torch.float32), ac.df_positions(case, offset, torch.float64)
    for a, b in zip(p32, p64):
        assert a.dtype == torch.float32 and torch.equal(a.double(), b)
    assert torch.equal((offset.double() / ac.DF_STEP).round() * ac.DF_STEP, offset.double())
    assert float(offset.abs().max()) < 2.0 ** 10
    n = ac.df_explicit(case).count
    S = n["samples"]
    print(f"\n{name}: {n}")
    if case.pattern == "integer":
        assert n["integer"] == S and set(offset.flatten().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    elif case.pattern == "edge":
        # exactly on 0 and on Hp - 1 / Wp - 1 (the gradient passes), and 2^-6 outside (it does not)
        assert n["on_first"] >= S // 8 and n["on_last"] >= S // 8 and n["outside"] >= S // 4 and n["far"] == 0
        assert n["coinciding"] >= S // 4 and n["ring_corner"] >= S // 2
    elif case.pattern == "ring":
        assert n["in_ring"] >= S // 2 and n["outside"] == 0 and n["ring_corner"] >= S // 2
    elif case.pattern == "far":
        assert n["far"] >= S // 4
    elif case.pattern == "random":
        assert n["integer"] <= S // 8
    else:
        assert case.pattern == "collision"
        assert n["outside"] == n["ring_corner"] == n["coinciding"] == n["integer"] == n["in_ring"] == 0


def test_deform_cases_share_inputs_across_mask_and_cotangent_variants():
    base = ac.df_inputs(ac.DF_BY_NAME["edge-1x5x7s1-mrand-dense"])
    for name in ("edge-1x5x7s1-mzero-dense", "edge-1x5x7s1-mnone-dense", "edge-1x5x7s1-mrand-lane31"):
        other = ac.df_inputs(ac.DF_BY_NAME[name])
        assert torch.equal(other[0], base[0]) and torch.equal(other[1], base[1])
    x, off, mask, gval = ac.df_inputs(ac.DF_BY_NAME["edge-1x5x7s1-mrand-lane31"])
    assert bool((gval[:, 31] != 0).all()) and float(gval[:, :31].abs().max()) == 0.0
    gval = ac.df_inputs(ac.DF_BY_NAME["edge-1x5x7s1-mrand-tap4"])[3]
    assert bool((gval[..., 4] != 0).all()) and float(gval[..., :4].abs().max()) == float(gval[..., 5:].abs().max()) == 0.0
    assert float(ac.df_inputs(ac.DF_BY_NAME["edge-2x9x11s1-mzero-dense"])[2].abs().max()) == 0.0
    assert float(ac.df_inputs(ac.DF_BY_NAME["edge-2x9x11s1-mone-dense"])[2].min()) == 1.0
    m = base[2]
    assert 0.0 < float(m.min()) and float(m.max()) < 1.0


@pytest.mark.parametrize("name", [c.name for c in ac.DF_CASES])
def test_deform_explicit_formula_is_float64_autograd(name):
    """The formula that supplies the scales (and the perturbed references below) is the reference."""
    case = ac.DF_BY_NAME[name]
    ref, ex = ac.df_reference(case), ac.df_explicit(case)
    for k in ac.DF_TENSORS:
        if ref.out[k] is None:
            assert ex.out[k] is None and case.mask == "none"
            continue
        assert bool(torch.isfinite(ref.out[k]).all())
        assert tuple(ex.out[k].shape) == tuple(ref.out[k].shape)
        assert ac.measure(ex.out[k], ref.out[k], ref.scales[k]) <= 1e-12, k
        assert bool((ex.mag[k] >= ex.out[k].abs() * (1 - 1e-12)).all()), k
    if case.pattern == "far":   # far outside: val, goff and that tap's share of gx exactly 0
        pr, pc = ac.df_positions(case, ac.df_inputs(case)[1], torch.float64)
        gone = ((pr < -1) | (pr > case.shape[1] + 2) | (pc < -1) | (pc > case.shape[2] + 2))
        assert float(ref.out["val"].permute(0, 1, 4, 2, 3)[gone.unsqueeze(1).expand(-1, 32, -1, -1, -1)].abs().max()) == 0.0
        assert float(ref.out["goff"][:, :9][gone].abs().max()) == 0.0 and float(ref.out["goff"][:, 9:][gone].abs().max()) == 0.0
        assert float(ex.mag["val"].permute(0, 1, 4, 2, 3)[gone.unsqueeze(1).expand(-1, 32, -1, -1, -1)].max()) == 0.0
    if case.mask == "zero":
        assert set(ref.zero) >= {"val", "gx", "goff"}


@pytest.mark.parametrize("name", [c.name for c in ac.DF_CASES if c.mask == "rand" and c.shape[1] > 1])
def test_deform_gx_bound_holds_in_any_summation_order(name):
    """gx is an atomic float32 sum: its terms taken in 8 random orders on the CPU stay within 3/4
    of the bound, so the GPU test does not hang on the kernel's schedule.  (The collision case has
    its own bound; a 1 x 1 frame has no two terms in one pixel that are not zero.)"""
    case = ac.DF_BY_NAME[name]
    spread = ac.df_gx_order_spread(case, 8)
    print(f"\n{name}: m(gx) up to {spread:.3e} over 8 orders, bound {ac.bound(ac.df_f32(case)['gx']):.3e}")
    assert spread <= 0.75 * ac.bound(ac.df_f32(case)["gx"])


def test_collision_case_sums_9hw_same_signed_terms_into_one_pixel():
    case = ac.DF_COLLISION
    ex = ac.df_explicit(case)
    N = ac.collision_terms()
    assert N == 9 * 9 * 11 and ex.terms == N
    x, offset, mask, gval = ac.df_inputs(case)
    assert float(gval.min()) > 0 and float(mask.min()) > 0
    pr, pc = ac.df_positions(case, offset, torch.float64)
    tr, tc = ac.COLLISION_TARGET
    assert bool((pr == tr + 0.5).all()) and bool((pc == tc + 0.5).all())
    ref = ac.df_reference(case).out["gx"]
    hit = torch.zeros(9, 11, dtype=torch.bool)
    hit[tr - 1:tr + 1, tc - 1:tc + 1] = True     # padded (tr, tc) is input pixel (tr - 1, tc - 1)
    assert bool((ref[0][:, hit] > 0).all()) and float(ref[0][:, ~hit].abs().max()) == 0.0
    assert torch.equal(ex.mag["gx"] > 0, hit.expand(1, 32, 9, 11))
    # one sign: the sum of the absolute terms is the sum
    assert float(((ex.mag["gx"] - ref).abs() / ex.mag["gx"].clamp_min(1e-300))[0][:, hit].max()) <= 1e-12
    # each of the four pixels gets gval * mask / 4 from every (tap, pixel): the largest such term
    terms = (gval.double().permute(0, 1, 4, 2, 3) * mask.double().unsqueeze(1) * 0.25).reshape(32, -1)
    assert terms.shape[1] == N
    assert float(((terms.sum(1) - ref[0, :, tr - 1, tc - 1]).abs() / terms.sum(1)).max()) <= 1e-12
    lim = ac.collision_gx_bound()[0, :, tr - 1, tc - 1]
    assert bool((terms.max(1).values > 10 * lim).all()), float((terms.max(1).values / lim).min())
    print(f"\ncollision: largest term / bound {float((terms.max(1).values / lim).min()):.1f} .. "
          f"{float((terms.max(1).values / lim).max()):.1f}, mean term / bound {float((terms.mean(1) / lim).mean()):.1f}")


# ---------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------
def _all_f32():
    for c in ac.GN_CASES:
        yield "gn " + c.name, ac.gn_f32(c), ac.gn_reference(c)
    for c in ac.GATE_CASES:
        for cot in ac.GATE_COTS:
            yield f"gates {c.name} {cot}", ac.gate_f32(c, cot), ac.gate_reference(c, cot)
    for c in ac.DF_CASES:
        yield "deform " + c.name, ac.df_f32(c), ac.df_reference(c)


def test_float32_torch_stays_below_the_floor():
    """m_f32 <= floor * kappa: the reference alone is within the bound, the 3 * m_f32 arm carries
    no case by itself -- but for the listed (case, tensor) pairs, which the record names."""
    assert ac.FLOOR == 16 * 2.0 ** -24 and ac.F32_FACTOR == 3.0
    above = {}
    for label, f32, ref in _all_f32():
        assert ref.kappa >= 1.0 and (ref.kappa == 1.0 or label.startswith("gn "))
        for k, m in f32.items():
            assert m == m, (label, k)
            if m > ac.FLOOR * ref.kappa and k not in ref.zero:
                above.setdefault(label, []).append(k)
                print(f"\n{label} {k}: m_f32 {m:.3e} > floor * kappa {ac.FLOOR * ref.kappa:.3e}")
    assert {k: tuple(v) for k, v in above.items()} == ac.F32_ABOVE_FLOOR


# ---------------------------------------------------------------------------------------------
# the cases can see the errors they are there for
# ---------------------------------------------------------------------------------------------
def test_swapped_gate_blocks_are_seen():
    worst = 0.0
    for case in ac.GATE_CASES:
        if case.kind != "index":
            continue
        hid = case.shape[1]
        z, c, _, _ = ac.gate_inputs(case)
        dh, dc = ac.gate_cotangents(case, "both")
        zs = z.clone()
        zs[:, :hid], zs[:, hid:2 * hid] = z[:, hid:2 * hid], z[:, :hid]       # i <-> f
        bad = ac.gates_run(zs, c, dh, dc, torch.float64, hid)
        bad["dz"] = torch.cat([bad["dz"][:, hid:2 * hid], bad["dz"][:, :hid], bad["dz"][:, 2 * hid:]], 1)
        ref, f32 = ac.gate_reference(case, "both"), ac.gate_f32(case, "both")
        ratio = max(ac.measure(bad[k], ref.out[k], ref.scales[k]) / ac.bound(f32[k]) for k in ac.GATE_TENSORS)
        print(f"\n{case.name}: swapped i / f blocks are {ratio:.3g} bounds away")
        assert ratio > 100, case.name
        worst = max(worst, ratio)
    assert worst > 1e4


@pytest.mark.parametrize("term", range(4))
def test_a_negated_dpr_term_is_seen(term):
    seen = 0
    for case in ac.DF_CASES:
        if case.mask == "zero":
            continue
        ref, f32 = ac.df_reference(case), ac.df_f32(case)
        bad = ac.df_explicit(case, neg_dpr_term=term).out["goff"]
        ratio = ac.measure(bad, ref.out["goff"], ref.scales["goff"]) / ac.bound(f32["goff"])
        seen += ratio > 100
    print(f"\ndL/dpr term {term} negated: more than 100 bounds away on {seen} cases")
    assert seen >= 40


def test_a_dropped_lane_is_seen():
    for lane, others in ((31, ("lane0", "lane15", "lane16")), (0, ("lane15", "lane16", "lane31"))):
        for pattern in ac.DF_PATTERNS:
            case = ac.DF_BY_NAME[f"{pattern}-1x5x7s1-mrand-lane{lane}"]
            ref, f32 = ac.df_reference(case), ac.df_f32(case)
            bad = ac.df_explicit(case, drop_lane=lane).out
            for k in ("goff", "gm"):
                ratio = ac.measure(bad[k], ref.out[k], ref.scales[k]) / ac.bound(f32[k])
                assert ratio > 100, (case.name, k, ratio)
                assert float(bad[k].abs().max()) == 0.0       # that lane carried the whole cotangent
            for o in others:   # and no other single-lane case notices
                oc = ac.DF_BY_NAME[f"{pattern}-1x5x7s1-mrand-{o}"]
                same = ac.df_explicit(oc, drop_lane=lane).out
                assert torch.equal(same["goff"], ac.df_explicit(oc).out["goff"])
    case = ac.DF_BY_NAME["random-2x9x11s1-mrand-dense"]
    ref, f32 = ac.df_reference(case), ac.df_f32(case)
    bad = ac.df_explicit(case, drop_lane=31).out
    assert ac.measure(bad["goff"], ref.out["goff"], ref.scales["goff"]) > 100 * ac.bound(f32["goff"])
