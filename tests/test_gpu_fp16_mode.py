"""GPU tests of the opt-in fp16 mode of the inference sweep (DepthSweep(precision="fp16"),
AARMVS_PREC_FP16: one fp16 matrix product per fp32 product in the five ConvLSTM convs and the
two deconvs).

Every bound is computed here from the CPU oracle and the CPU emulation of the mode
(tests/fp16_mode_ref.py), never from a GPU result.  E_rms / E_max: rms / max of
(emulated - fp32 oracle) on the tensor under test, i.e. the mode's own error.  Two emulation runs
whose cell inputs differ by one fp32 ulp end up 0.02 E_rms apart after one cell and 0.26-0.37
E_rms apart after 8-32 planes (a difference below an fp16 step vanishes or becomes a whole step
when it is re-rounded), so the GPU matches the emulation tightly per cell and statistically over a
sweep.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from aarmvs import synthetic as syn

import fp16_mode_ref as fref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def rel_l1(a, b):
    return float((a - b).abs().sum() / max(float(b.abs().sum()), 1e-30))


@functools.lru_cache(maxsize=None)
def weights(kind):
    if kind == "real":
        g = np.load(os.path.join(GOLDEN, "real_weights_sweep.npz"), allow_pickle=False)
        return {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    return {k: torch.from_numpy(v) for k, v in syn.sweep_weights(7).items()}


def _views(feats, proj):
    N = feats.shape[0]
    return feats[0], [feats[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)]


@functools.lru_cache(maxsize=None)
def case(shape, kind, scale=1.0):
    """The scene, the fp32 oracle's sweep and the emulated mode's, computed once per case and
    shared (read-only) by the tests."""
    from oracle import sweep_oracle as orc
    B, N, H, W, D = shape
    sc = syn.scene(B, N, H, W, D, seed=N * 100 + D)
    feats = torch.from_numpy(sc["features"]) * scale
    proj = torch.from_numpy(sc["proj_matrices"])
    dv = torch.from_numpy(sc["depth_values"])
    P = weights(kind)
    ref = orc.sweep(*_views(feats, proj), dv, P)
    with fref.fp16_operands():
        emu = orc.sweep(*_views(feats, proj), dv, P)
    return dict(feats=feats, proj=proj, dv=dv, P=P, ref=ref, emu=emu)


@functools.lru_cache(maxsize=None)
def sweeper(kind):
    from aarmvs import ops
    return ops.DepthSweep({n: v.to(DEV) for n, v in weights(kind).items()}, DEV)


def run(c, kind, precision, sw=None, **kw):
    sw = sw or sweeper(kind)
    sw.precision = precision
    try:
        out = sw(*_views(c["feats"].to(DEV), c["proj"]), c["dv"], want_cost=True, **kw)
        torch.cuda.synchronize()
    finally:
        sw.precision = "split"
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items() if k != "_keepalive"}


def check_against_oracle(c, out, tag):
    """Items 2 and 3 of the mode's acceptance on one sweep's outputs."""
    ref, emu = c["ref"], c["emu"]
    E = emu["cost"] - ref["cost"]
    E_rms, E_max = fref.rms(E), float(E.abs().max())
    assert E_rms > 0
    cost = out["cost"]
    assert torch.isfinite(cost).all() and torch.isfinite(out["depth"]).all() and torch.isfinite(out["conf"]).all()
    r_orc, r_emu = fref.rms(cost - ref["cost"]), fref.rms(cost - emu["cost"])
    bound = 2 * E_max + 1e-4 + 1e-4 * ref["cost"].abs()          # per element
    over = float(((cost - ref["cost"]).abs() - bound).max())
    conf_E = float((emu["conf"] - ref["conf"]).abs().max())
    conf_d = float((out["conf"] - ref["conf"]).abs().max())
    print(f"[{tag}] E_rms {E_rms:.3e} E_max {E_max:.3e} | gpu-oracle rms {r_orc:.3e} ({r_orc / E_rms:.2f} E_rms) "
          f"max {float((cost - ref['cost']).abs().max()):.3e} | gpu-emulation rms {r_emu:.3e} "
          f"({r_emu / E_rms:.2f} E_rms) | conf {conf_d:.3e} (emulation {conf_E:.3e})")
    assert 0.5 * E_rms <= r_orc <= 1.5 * E_rms      # the mode is on, and nothing else is lost
    assert over <= 0.0
    assert r_emu <= 0.75 * E_rms
    assert conf_d <= 2 * conf_E + 1e-4
    # depth: where the GPU picks another plane than the oracle, the oracle's cost there is within
    # the two planes' cost bounds of its maximum (c_o(p_g) >= c_g(p_g) - b(p_g) >= c_g(p_o) - b(p_g)
    # >= c_o(p_o) - b(p_o) - b(p_g)): a near-tie, not a wrong plane
    dv = c["dv"]
    B, D = dv.shape
    pg = (out["depth"].unsqueeze(1) - dv.view(B, D, 1, 1)).abs().argmin(1, keepdim=True)
    assert torch.equal(torch.gather(dv.view(B, D, 1, 1).expand_as(cost), 1, pg).squeeze(1), out["depth"])
    po = ref["cost"].argmax(1, keepdim=True)
    gap = torch.gather(ref["cost"], 1, po) - torch.gather(ref["cost"], 1, pg)
    allow = torch.gather(bound, 1, po) + torch.gather(bound, 1, pg)
    moved = pg != po
    print(f"[{tag}] planes moved {float(moved.float().mean()):.2e}, depth rel-L1 "
          f"{rel_l1(out['depth'], ref['depth']):.3e}, worst gap / allowance "
          f"{float((gap / allow)[moved].max()) if moved.any() else 0.0:.3f}")
    assert bool((gap[moved] <= allow[moved]).all())
    return E_rms


# ---------------------------------------------------------------------------------------
# 1. cell-level rounding
# ---------------------------------------------------------------------------------------
def test_cell0_matches_the_emulation_per_step():
    """B = 2, 36x68 (partial tiles), three aarmvs_unet_step_p steps on x ~ N(0, 1): cell 0's h and
    c after each step against the emulation, within 0.1 E_rms (the CPU's own one-ulp sensitivity
    there is 0.02; truncation instead of rounding, or a silently split run, would give >= 1)."""
    from oracle import sweep_oracle as orc
    B, H, W = 2, 36, 68
    P = weights("syn")
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(B, 32, H, W, generator=g) for _ in range(3)]
    st_ref, st_emu = orc.init_state(B, H, W), orc.init_state(B, H, W)
    sw = sweeper("syn")
    sw.precision = "fp16"
    try:
        for t, x in enumerate(xs):
            _, st_ref = orc.unet_step(x, st_ref, P)
            with fref.fp16_operands():
                _, st_emu = orc.unet_step(x, st_emu, P)
            sw.unet_step(x.to(DEV), t)
            torch.cuda.synchronize()
            for which, name in ((0, "h"), (1, "c")):
                got = sw.state(B, H, W, 1, t + 1, 0, which).cpu()
                E_rms = fref.rms(st_emu[0][which] - st_ref[0][which])
                d = fref.rms(got - st_emu[0][which])
                print(f"step {t} cell 0 {name}: E_rms {E_rms:.3e}, gpu - emulation rms {d:.3e} ({d / E_rms:.3f} E_rms)")
                assert E_rms > 0 and d <= 0.1 * E_rms
    finally:
        sw.precision = "split"


# ---------------------------------------------------------------------------------------
# 2, 3. step and sweep against the oracle; depth
# ---------------------------------------------------------------------------------------
SWEEP_CASES = [((1, 3, 32, 48, 16), "real"), ((1, 5, 48, 64, 24), "real"),
               ((2, 4, 36, 68, 8), "syn"), ((1, 2, 4, 4, 4), "syn")]


@pytest.mark.parametrize("shape,kind", SWEEP_CASES)
def test_sweep_against_oracle_and_emulation(shape, kind):
    c = case(shape, kind)
    out = run(c, kind, "fp16")
    check_against_oracle(c, out, f"{shape} {kind}")
    if kind == "real":   # the project's bar; the emulation gives <= 3.5e-4 there
        assert rel_l1(c["emu"]["depth"], c["ref"]["depth"]) <= 3.5e-4
        assert rel_l1(out["depth"], c["ref"]["depth"]) <= 1e-3


# ---------------------------------------------------------------------------------------
# 4. range guard
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [100.0, 0.01])
def test_range_guard_under_scaled_features(scale):
    """Features x100 drive the cost slice above fp16's largest finite value (65504), x0.01 far
    below its usual range.  The emulation rounds relative to each value, so the bounds above
    hold only if the 1-product cells keep the staging scales (a dropped scale: inf or flushed)."""
    from oracle import sweep_oracle as orc
    shape = (1, 3, 32, 48, 8)
    c = case(shape, "real", scale)
    if scale > 1:
        views = _views(c["feats"], c["proj"])
        rels = [orc.relative_projection(sp, views[2]) for sp in views[3]]
        assert float(orc.cost_slice(views[0], views[1], rels, c["dv"][:, 0], c["P"]).abs().max()) > 65504.0
    out = run(c, "real", "fp16")
    check_against_oracle(c, out, f"{shape} x{scale:g}")


# ---------------------------------------------------------------------------------------
# 5. determinism and schedules
# ---------------------------------------------------------------------------------------
def test_fp16_mode_is_schedule_independent_and_leaves_no_trace():
    from aarmvs import ops
    shape, kind = (2, 3, 36, 68, 8), "syn"
    c = case(shape, kind)
    B, N, H, W, D = shape
    sw = sweeper(kind)
    keys = ("cost", "depth", "conf")
    split_before = run(c, kind, "split")
    a = run(c, kind, "fp16")
    sw.overlap = False
    try:
        b = run(c, kind, "fp16")
    finally:
        sw.overlap = True
    # a d_range split at plane 3 of 8 into one cost buffer
    cost = torch.empty(B, D, H, W, device=DEV)
    run(c, kind, "fp16", d_range=(0, 3), cost_out=cost, want_depth=False)
    d = run(c, kind, "fp16", d_range=(3, D), cost_out=cost)
    again = run(c, kind, "fp16")
    for k in keys:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], d[k]), k
        assert torch.equal(a[k], again[k]), k
    # the default mode after fp16 calls on the same object, and on a fresh object
    split_after = run(c, kind, "split")
    fresh = ops.DepthSweep({n: v.to(DEV) for n, v in c["P"].items()}, DEV)
    assert fresh.precision == "split"
    split_fresh = run(c, kind, "split", sw=fresh)
    for k in keys:
        assert torch.equal(split_before[k], split_after[k]), k
        assert torch.equal(split_before[k], split_fresh[k]), k
    # an object constructed in the mode gives the mode's result
    made = ops.DepthSweep({n: v.to(DEV) for n, v in c["P"].items()}, DEV, precision="fp16")
    out = made(*_views(c["feats"].to(DEV), c["proj"]), c["dv"], want_cost=True)
    assert made.precision == "fp16" and torch.equal(out["cost"].cpu(), a["cost"])


# ---------------------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------------------
def test_modes_differ_and_the_profiler_names_the_fp16_kernels():
    from aarmvs import ops
    shape, kind = (1, 3, 32, 48, 16), "real"
    c = case(shape, kind)
    D = shape[4]
    split = run(c, kind, "split")
    ops.profile_enable(True)
    try:
        ops.profile_reset()
        fp16 = run(c, kind, "fp16")
        prof16 = ops.profile_read()
        ops.profile_reset()
        run(c, kind, "split")
        prof3 = ops.profile_read()
    finally:
        ops.profile_enable(False)
        ops.profile_reset()
    assert not torch.equal(split["cost"], fp16["cost"])
    cells = [f"lstm_cell{k}" for k in range(5)] + ["deconv0", "deconv1"]
    for name in cells:
        assert prof16.get(name + "_fp16", (0, 0.0))[0] == D, (name, prof16)
        assert name not in prof16
        assert prof3.get(name, (0, 0.0))[0] == D and name + "_fp16" not in prof3
    # the stages outside the mode run under their usual names in both
    rest16 = {k: v[0] for k, v in prof16.items() if not k.endswith("_fp16")}
    rest3 = {k: v[0] for k, v in prof3.items() if k not in cells}
    assert rest16 == rest3 and rest3["head_wta"] == D


def test_record_with_fp16_raises():
    from aarmvs import AarmvsError, ops
    shape, kind = (1, 3, 32, 48, 16), "real"
    c = case(shape, kind)
    B, N, H, W, D = shape
    sw = sweeper(kind)
    rec = ops.DepthSweep.record_buffers(B, H, W, D, DEV, nsrc=N - 1)
    sw.precision = "fp16"
    try:
        with pytest.raises(AarmvsError, match="inference mode"):
            sw(*_views(c["feats"].to(DEV), c["proj"]), c["dv"], want_cost=True, record=rec)
    finally:
        sw.precision = "split"
    with pytest.raises(AarmvsError, match="precision"):
        sw.precision = "bf16"
    assert sw.precision == "split"


def _emvsnet(shape, P, **kw):
    from models import EMVSNet
    B, N, H, W, D = shape
    m = EMVSNet(disparity_level=D, image_scale=1.0, max_h=H, max_w=W, evidential=False, **kw)
    missing = m.load_state_dict(P, strict=False).missing_keys
    assert all(k.startswith("feature.") for k in missing)
    m.feature = nn.Identity()
    return m.to(DEV)


def test_emvsnet_sweep_precision():
    shape, kind = (1, 3, 32, 48, 16), "real"
    c = case(shape, kind)
    want = run(c, kind, "fp16")
    imgs = c["feats"].transpose(0, 1).contiguous().to(DEV)
    proj, dv = c["proj"].to(DEV), c["dv"].to(DEV)
    m = _emvsnet(shape, c["P"], return_depth=True, sweep_precision="fp16").eval()
    plain = _emvsnet(shape, c["P"], return_depth=True).eval()
    with torch.no_grad():
        out = m(imgs, proj, dv)
        assert torch.equal(out["depth"].cpu(), want["depth"])
        assert torch.equal(out["photometric_confidence"].cpu(), want["conf"])
        assert not torch.equal(plain(imgs, proj, dv)["photometric_confidence"].cpu(), want["conf"])
        # the other forwards stay split: eval without return_depth, and the training forward
        m.return_depth = plain.return_depth = False
        assert torch.equal(m(imgs, proj, dv)[0], plain(imgs, proj, dv)[0])
    m.train()
    plain.train()
    p16, p3 = m(imgs, proj, dv)[0], plain(imgs, proj, dv)[0]
    assert p16.requires_grad and torch.equal(p16, p3)
