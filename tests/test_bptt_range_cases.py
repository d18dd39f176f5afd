"""The cases of tests/bptt_range_cases.py say what tests/test_gpu_bptt_range.py believes they
say (CPU only: the oracle's float64 and float32 autograd, no library):

* every float64 gradient is finite;
* float32 CPU autograd's own relative L2 error, which sets the GPU test's bound max(2e-5, 2 x
  it), is at most 1e-3 for every tensor: above that the bound says nothing about the GPU;
* tail_tiny's last two plane groups really carry a gate gradient below 2^-113 in all five cells
  (where an unclamped 2^(14 - ilogb(max)) staging scale overflows float32), and one_plane's last
  group one that is exactly zero;
* under the linear loss conv_0.bias's gradient is sum(R'), not ~0.
"""
import numpy as np
import pytest
import torch

import bptt_range_cases as rc

CAP = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _threads():
    prev = torch.get_num_threads()
    yield
    torch.set_num_threads(prev)


def test_case_table_is_the_agreed_one():
    shapes = {c.name: c.shape for c in rc.CASES}
    assert shapes == {
        "nsrc1": (1, 2, 16, 24, 3), "nsrc16": (1, 17, 16, 24, 3), "min": (1, 3, 4, 4, 2),
        "strip": (1, 3, 4, 132, 3), "ragged": (1, 3, 52, 84, 3), "batch3": (3, 3, 8, 12, 2),
        "d1": (1, 3, 8, 12, 1), "d17": (1, 3, 8, 12, 17),
        "tail_tiny": (1, 3, 8, 12, 34), "head_tiny": (1, 3, 8, 12, 34), "one_plane": (1, 3, 8, 12, 34),
        "sparse": (1, 3, 8, 12, 34), "zero": (1, 3, 8, 12, 34),
        "scale-96": (1, 3, 16, 24, 3), "scale-48": (1, 3, 16, 24, 3),
        "scale+48": (1, 3, 16, 24, 3), "scale+96": (1, 3, 16, 24, 3)}
    linear = {c.name for c in rc.CASES if c.loss == "linear"}
    assert linear == {"d1", "d17", "tail_tiny", "head_tiny", "one_plane", "sparse", "zero"}
    assert {c.loss for c in rc.CASES} == {"softmax", "linear"}


def test_cotangents_have_their_shape():
    R = torch.randn(1, 34, 8, 12, generator=torch.Generator().manual_seed(rc.R_SEED))
    for name in ("tail_tiny", "head_tiny", "one_plane", "sparse", "zero"):
        assert torch.equal(rc.inputs(rc.BY_NAME[name])[4], rc.BY_NAME[name].cot(R)), name
    t = rc.inputs(rc.BY_NAME["tail_tiny"])[4]
    assert torch.equal(t[:, :16], R[:, :16]) and torch.equal(t[:, 16:], R[:, 16:] * 2.0 ** -112)
    h = rc.inputs(rc.BY_NAME["head_tiny"])[4]
    assert torch.equal(h[:, 16:], R[:, 16:]) and torch.equal(h[:, :16], R[:, :16] * 2.0 ** -112)
    o = rc.inputs(rc.BY_NAME["one_plane"])[4]
    assert torch.equal(o[:, 20], R[:, 20]) and int((o != 0).sum()) == int((R[:, 20] != 0).sum())
    s = rc.inputs(rc.BY_NAME["sparse"])[4]
    assert int((s != 0).sum()) == 2 * 34 and bool((s[0, :, 0, 0] != 0).all()) and bool((s[0, :, 5, 7] != 0).all())
    assert float(rc.inputs(rc.BY_NAME["zero"])[4].abs().max()) == 0.0
    base = rc.inputs(rc.SCALE_BASE)[4]
    for k in rc.SCALE_KS:   # a power of two in float32's range: exact
        assert torch.equal(rc.inputs(rc.BY_NAME[f"scale{k:+d}"])[4], base * 2.0 ** k)
        assert bool(torch.isfinite(base * 2.0 ** k).all())


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_keeps_the_gpu_test_honest(name):
    case = rc.BY_NAME[name]
    B, N, H, W, D = case.shape
    ref = rc.reference(case)
    prob, gf, gp, gx = ref.g64
    assert bool(torch.isfinite(gf).all()) and all(bool(torch.isfinite(g).all()) for g in gx)
    assert all(bool(torch.isfinite(g).all()) for g in gp.values())
    assert bool(torch.isfinite(ref.cost).all()) and tuple(ref.cost.shape) == (B, D, H, W)
    # the cap on float32 autograd's own error
    e32 = dict(rc.f32_spread(case))
    if case.loss == "softmax":   # true gradient 0 (softmax over D): held to an absolute bound
        del e32["cost_regularization.conv_0.bias"]
    worst = max(e32, key=e32.get)
    print(f"\n{name:10s} {case.shape} {case.loss}: worst float32 error {e32[worst]:.3e} ({worst}); "
          f"max |dL/dz| per cell 2^{np.round(np.log2(np.maximum(ref.gzmax.max(1), 1e-300)), 1).tolist()}")
    assert max(e32.values()) <= CAP, {k: v for k, v in e32.items() if v > CAP}
    assert set(rc.f32_spread(case)) >= {"features", "x"} | set(gp) | {f"features[{v},{b}]" for v in range(N) for b in range(B)}
    # the case reaches the code it is meant for
    for g in case.tiny_groups:
        m = ref.gzmax[:, rc.group_planes(g, D)].max(axis=1)
        print(f"  group {g}: max |dL/dz| per cell 2^{np.round(np.log2(m), 1).tolist()}")
        assert m.shape == (5,) and (m > 0).all() and (m < rc.GZ_TINY).all(), (g, m)
    for g in case.zero_groups:
        assert (ref.gzmax[:, rc.group_planes(g, D)] == 0.0).all(), g
    if case.tiny_groups or case.zero_groups:   # ... and the other groups carry a plain gradient
        rest = [g for g in range(-(-D // rc.PLANES)) if g not in case.tiny_groups + case.zero_groups]
        for g in rest:
            assert (ref.gzmax[:, rc.group_planes(g, D)].max(axis=1) > 2.0 ** -40).all(), g
    Rp = rc.inputs(case)[4]
    kb = "cost_regularization.conv_0.bias"
    if case.loss == "linear":
        want = float(Rp.double().sum())
        assert abs(float(gp[kb]) - want) <= 1e-9 * abs(want), (float(gp[kb]), want)
        if name != "zero":
            assert abs(want) > 1e-2 * float(Rp.double().abs().sum()) / np.sqrt(Rp.numel()), want
    if name == "zero":
        assert float(gf.abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in gp.values())


def test_scale_reference_is_the_k0_reference_scaled():
    """float64 autograd at R * 2^k against the k = 0 gradients times 2^k (what reference() hands
    out): equal to rounding, so that the GPU test's deviation at k != 0 is the kernels' own."""
    from test_gpu_bptt import _oracle_grads, rel_l2
    case = rc.BY_NAME["scale-96"]
    feats, proj, dv, P, Rp = rc.inputs(case)
    _, gf, gp, gx = _oracle_grads(feats, proj, dv, P, Rp, torch.float64, case.loss)
    _, gf0, gp0, gx0 = rc.reference(case).g64
    assert rel_l2(gf.numpy(), gf0.numpy()) <= 1e-12
    for k in gp:
        assert rel_l2(gp[k].numpy(), gp0[k].numpy()) <= 1e-12, k
