"""GPU tests of the opt-in depth-posterior statistics of the sweep (DepthSweep(...)(
want_posterior=True), aarmvs_sweep_ex; the standalone aarmvs_wta_posterior_update / _finalize
pair; aarmvs_posterior_from_cost; EMVSNet(posterior_stats=True) and the drivers).

Shapes: 20x36 frames (not a multiple of the head kernel's 8x32 tile: partial tiles in both
directions, six blocks per batch element), B = 2, two source views, random parameters, D = 5
and 17 (17 crosses a 16-plane group).  The float64 reference is tests/posterior_ref.py on the
cost volume the GPU produced; its bounds come from the number formats (posterior_ref.bounds),
never from a GPU result.
"""
import functools
import math
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from aarmvs import synthetic as syn

import posterior_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, H, W = 2, 3, 20, 36
KEYS = pr.KEYS
RKEYS = ("depth_refined", "conf_window", "index")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _views(feats, proj):
    n = feats.shape[0]
    return feats[0], [feats[v] for v in range(1, n)], proj[:, 0], [proj[:, v] for v in range(1, n)]


@functools.lru_cache(maxsize=None)
def weights():
    return {k: torch.from_numpy(v) for k, v in syn.sweep_weights(7).items()}


@functools.lru_cache(maxsize=None)
def scene(D):
    sc = syn.scene(B, N, H, W, D, seed=N * 100 + D)
    return (torch.from_numpy(sc["features"]), torch.from_numpy(sc["proj_matrices"]),
            torch.from_numpy(sc["depth_values"]))


@functools.lru_cache(maxsize=None)
def sweeper():
    from aarmvs import ops
    return ops.DepthSweep({n: v.to(DEV) for n, v in weights().items()}, DEV)


def run(D, precision="split", **kw):
    feats, proj, dv = scene(D)
    sw = sweeper()
    sw.precision = precision
    try:
        out = sw(*_views(feats.to(DEV), proj), dv, want_cost=True, **kw)
        torch.cuda.synchronize()
    finally:
        sw.precision = "split"
    return {k: v for k, v in out.items() if k != "_keepalive"}


@functools.lru_cache(maxsize=None)
def posterior_sweep(D):
    """One sweep with the statistics per D, shared (read-only) by the tests."""
    return run(D, want_posterior=True)


def same(a, b):
    """Bit-for-bit equality that also holds where both are NaN."""
    if a.dtype.is_floating_point:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def standalone(cost, dv, n=None):
    """The standalone pair plane by plane over cost [B,D,h,w]; also the WTA images' depth and
    confidence."""
    from aarmvs import ops
    Bc, D = cost.shape[:2]
    n = D if n is None else n
    mp, dm, es = (torch.zeros_like(cost[:, 0]).contiguous() for _ in range(3))
    st = ops.posterior_state(Bc, cost[0, 0].numel(), cost.device)
    for d in range(n):
        ops.wta_posterior_update(cost[:, d].contiguous(), d, dv[:, d], mp, dm, es, st)
    out = ops.wta_posterior_finalize(es, st)
    out.update(depth=dm, conf=mp / es)
    torch.cuda.synchronize()
    return out


def check_bounds(got, cost, dv, what):
    """Every pixel of the four outputs within posterior_ref.bounds of the float64 definition on
    ``cost``; prints and returns the worst error / bound per output."""
    ref = pr.from_volume64(cost, dv)
    got = {k: got[k].cpu().numpy() for k in KEYS}
    for k in KEYS:
        assert np.isfinite(got[k]).all(), k
    ratio = pr.error_over_bound(got, ref)
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratio.items()))
    assert all(r <= 1.0 for r in ratio.values()), ratio
    return ratio


# ---------------------------------------------------------------------------------------
# 1. off changes nothing; refine and posterior do not see each other
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["split", "fp16"])
def test_the_statistics_leave_the_other_outputs_bit_identical(precision):
    off = run(5, precision)
    on = run(5, precision, want_posterior=True)
    again = run(5, precision)
    assert set(KEYS).isdisjoint(off) and set(KEYS) <= set(on)
    for k in ("depth", "conf", "cost"):
        assert torch.equal(off[k], on[k]), k
        assert torch.equal(off[k], again[k]), k
    for k in KEYS:
        assert on[k].dtype == torch.float32 and tuple(on[k].shape) == (B, H, W)
    refined = run(5, precision, want_refined=True)
    both = run(5, precision, want_refined=True, want_posterior=True)
    for k in ("depth", "conf", "cost"):
        assert torch.equal(off[k], both[k]), k
    for k in KEYS:
        assert same(on[k], both[k]), k
    for k in RKEYS:
        assert same(refined[k], both[k]), k


# ---------------------------------------------------------------------------------------
# 2. online == from the volume == the standalone pair
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 17])
def test_online_equals_the_volume_form_and_the_standalone_pair(D):
    from aarmvs import ops
    out = posterior_sweep(D)
    dv = scene(D)[2].to(DEV)
    vol = ops.posterior_from_cost(out["cost"], dv)
    pair = standalone(out["cost"], dv)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], vol[k]), k
        assert torch.equal(out[k], pair[k]), k
    assert torch.equal(pair["depth"], out["depth"]) and torch.equal(pair["conf"], out["conf"])
    # the statistics are real: a spread, an entropy below ln D, a runner-up below the winner
    assert (out["depth_std"] > 0).all() and (out["entropy"] >= 0).all() and (out["entropy"] > 0).any()
    assert (out["entropy"] <= math.log(D) + 1e-5).all()
    assert (out["runner_up"] <= out["conf"]).all() and (out["runner_up"] > 0).all()


# ---------------------------------------------------------------------------------------
# 3. against float64
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 17])
def test_against_the_float64_definition(D):
    out = posterior_sweep(D)
    check_bounds(out, out["cost"].cpu().numpy(), scene(D)[2].numpy(), f"sweep D={D}")


def test_volume_form_against_float64_at_512_planes():
    from aarmvs import ops
    rng = np.random.default_rng(512)
    dv = np.stack([np.linspace(425.0, 935.0, 512), 1.0 / np.linspace(1 / 425.0, 1 / 935.0, 512)]).astype(np.float32)
    cost = (rng.standard_normal((2, 512, 3, 5)) * 3).astype(np.float32)
    got = ops.posterior_from_cost(torch.from_numpy(cost).to(DEV), torch.from_numpy(dv).to(DEV))
    check_bounds(got, cost, dv, "volume D=512, randn * 3")
    # a late plane holds all but ~1e-8 of the mass: the input on which rescaling the variance by
    # 1 - k instead of S0 / S1 loses the standard deviation (tests/test_posterior_ref.py)
    late = pr.late_dominant(rng, 2, 512, 15).reshape(2, 512, 3, 5)
    ref = pr.from_volume64(late, dv)
    naive = pr.error_over_bound(pr.sequential32(late, dv, naive=True), ref)
    assert naive["depth_std"] > 1.0
    got = ops.posterior_from_cost(torch.from_numpy(late).to(DEV), torch.from_numpy(dv).to(DEV))
    check_bounds(got, late, dv, f"volume D=512, late-dominant (the naive form: std {naive['depth_std']:.0f})")


# ---------------------------------------------------------------------------------------
# 4. schedules and ranges
# ---------------------------------------------------------------------------------------
def test_schedules_and_plane_ranges():
    D = 5
    whole = posterior_sweep(D)
    sw = sweeper()
    sw.overlap = False
    try:
        serial = run(D, want_posterior=True)
    finally:
        sw.overlap = True
    for k in KEYS + ("depth", "conf", "cost"):
        assert torch.equal(whole[k], serial[k]), k
    # (0, 3) + (3, 5) through the sweeper's one state buffer
    cost = torch.empty(B, D, H, W, device=DEV)
    first = run(D, d_range=(0, 3), cost_out=cost, want_posterior=True)
    first = {k: first[k].clone() for k in KEYS}
    second = run(D, d_range=(3, D), cost_out=cost, want_posterior=True)
    for k in KEYS + ("depth", "conf"):
        assert torch.equal(whole[k], second[k]), k
    assert torch.equal(whole["cost"], cost)
    # after (0, 3) alone the outputs describe planes 0..2
    dv = scene(D)[2].to(DEV)
    part = standalone(whole["cost"], dv, n=3)
    for k in KEYS:
        assert torch.equal(first[k], part[k]), k
    assert not torch.equal(first["depth_mean"], whole["depth_mean"])


# ---------------------------------------------------------------------------------------
# 5. hand-made planes through the standalone pair
# ---------------------------------------------------------------------------------------
NAN = float("nan")
HAND = np.array([          # one row per pixel, one column per plane
    [0.0, 0.0, 0.0, 0.0],       # 0 uniform
    [0.0, 30.0, 0.0, 0.0],      # 1 one plane holds nearly everything
    [0.0, 100.0, 0.0, 0.0],     # 2 exp overflows
    [-200.0] * 4,               # 3 p == 0 on every plane
    [0.0, 2.0, NAN, 0.0],       # 4 a NaN plane
    [1.0, 0.5, 3.0, 0.0],       # 5 a late larger winner: the old winner becomes the runner-up
], np.float32)


def test_hand_made_planes():
    cost = torch.from_numpy(HAND.T.copy()).view(1, 4, 1, -1).to(DEV)
    dv = torch.tensor([[1.0, 2.0, 3.0, 4.0]], device=DEV)
    o = {k: v.reshape(-1).cpu() for k, v in standalone(cost, dv).items()}
    mean, sd, ent, ru, conf = (o[k] for k in KEYS + ("conf",))
    # uniform: mean 2.5, std sqrt(1.25) within a few ulp, entropy ln 4, and the tie rule
    assert abs(float(mean[0]) - 2.5) <= 4 * 2.0 ** -23 * 2.5
    assert abs(float(sd[0]) - math.sqrt(1.25)) <= 4 * 2.0 ** -23 * math.sqrt(1.25)
    assert abs(float(ent[0]) - math.log(4.0)) <= 1e-6
    assert float(ru[0]) == float(conf[0]) == 0.25
    # [0, 30, 0, 0]: a small positive std, entropy >= 0
    p = np.exp(HAND[1].astype(np.float64))
    q = p / p.sum()
    want_sd = math.sqrt(float((q * (np.arange(1, 5) - (q * np.arange(1, 5)).sum()) ** 2).sum()))
    assert 0.0 < float(sd[1]) < 1e-5 and abs(float(sd[1]) - want_sd) <= 1e-5 * want_sd
    assert float(ent[1]) >= 0.0 and abs(float(mean[1]) - 2.0) <= 2.0 ** -22
    assert abs(float(ru[1]) - q[0]) <= 1e-5 * q[0]
    # overflow, no mass, NaN: all four are NaN exactly where conf is
    assert torch.isnan(conf).tolist() == [False, False, True, True, True, False]
    for k in KEYS:
        assert torch.equal(torch.isnan(o[k]), torch.isnan(conf)), k
    # the late winner: the runner-up is the former maximum, plane 0
    p = np.exp(HAND[5].astype(np.float64))
    assert abs(float(ru[5]) - p[0] / p.sum()) <= 1e-6 and abs(float(conf[5]) - p[2] / p.sum()) <= 1e-6


def test_a_single_plane():
    from aarmvs import ops
    cost = torch.zeros(2, 1, 3, 5, device=DEV)
    dv = torch.tensor([[425.0], [935.0]], device=DEV)
    o = standalone(cost, dv)
    v = ops.posterior_from_cost(cost, dv)
    for k in KEYS:
        assert torch.equal(o[k], v[k]), k
    assert torch.equal(o["depth_mean"], dv.view(2, 1, 1).expand(2, 3, 5))
    for k in ("depth_std", "entropy", "runner_up"):
        assert bool((o[k] == 0).all()), k


# ---------------------------------------------------------------------------------------
# 6. model and drivers
# ---------------------------------------------------------------------------------------
def _emvsnet(D, **kw):
    from models import EMVSNet
    m = EMVSNet(disparity_level=D, image_scale=1.0, max_h=H, max_w=W, evidential=False, **kw)
    missing = m.load_state_dict(weights(), strict=False).missing_keys
    assert all(k.startswith("feature.") for k in missing)
    m.feature = nn.Identity()
    return m.to(DEV).eval()


def test_emvsnet_posterior_stats():
    D = 5
    feats, proj, dv = scene(D)
    want = posterior_sweep(D)
    imgs = feats.transpose(0, 1).contiguous().to(DEV)
    with torch.no_grad():
        plain = _emvsnet(D, return_depth=True)(imgs, proj.to(DEV), dv.to(DEV))
        out = _emvsnet(D, return_depth=True, posterior_stats=True)(imgs, proj.to(DEV), dv.to(DEV))
        both = _emvsnet(D, return_depth=True, posterior_stats=True, refine_depth=True)(imgs, proj.to(DEV),
                                                                                       dv.to(DEV))
    assert set(plain) == {"depth", "photometric_confidence", "evidential_prediction"}
    assert set(out) == set(plain) | set(KEYS)
    assert set(both) == set(out) | {"depth_refined", "photometric_confidence_window"}
    assert torch.equal(out["depth"], plain["depth"]) and torch.equal(out["depth"], want["depth"])
    assert torch.equal(out["photometric_confidence"], plain["photometric_confidence"])
    for k in KEYS:
        assert torch.equal(out[k], want[k]) and torch.equal(both[k], want[k]), k


def _eval_tree(tmp_path):
    """tests/golden/dtu_mini (the training layout) laid out as eval.py reads a scan: images/,
    cams/ and pair.txt under the scan's folder."""
    mini = os.path.join(GOLDEN, "dtu_mini")
    scan = tmp_path / "scan9"
    (scan / "images").mkdir(parents=True)
    (scan / "cams").mkdir()
    shutil.copy(os.path.join(mini, "Cameras", "pair.txt"), scan / "pair.txt")
    for v in range(4):
        shutil.copy(os.path.join(mini, "Rectified", "scan9_train", f"rect_{v + 1:0>3}_3_r5000.png"),
                    scan / "images" / f"{v:0>8}.jpg")
        shutil.copy(os.path.join(mini, "Cameras", "train", f"{v:0>8}_cam.txt"), scan / "cams" / f"{v:0>8}_cam.txt")
    (tmp_path / "list.txt").write_text("scan9\n")
    return tmp_path


def test_eval_driver(tmp_path):
    from aarmvs import eval_sharded, fusion
    from models import EMVSNet
    root = _eval_tree(tmp_path)
    common = ["--testpath", str(root), "--testlist", str(root / "list.txt"), "--max_h", "64", "--max_w", "80",
              "--numdepth", "8", "--view_num", "3", "--interval_scale", "1.06"]
    torch.manual_seed(0)
    model = EMVSNet(disparity_level=8, image_scale=1.0, max_h=64, max_w=80, return_depth=True,
                    evidential=False, posterior_stats=True)
    args = eval_sharded.parse_args(common + ["--outdir", str(root / "out"), "--posterior_stats"])
    ranges = []   # the depth range of every sample, as the model is given it (batch size 1)
    hook = model.register_forward_pre_hook(
        lambda m, a: ranges.extend((float(r.min()), float(r.max())) for r in a[2]))
    written = eval_sharded.save_depth(args, 0, 1, torch.device("cuda", 0), model=model)
    hook.remove()
    assert len(written) == 4 and len(ranges) == 4
    scan_out = root / "out" / "scan9"
    assert sorted(os.listdir(scan_out)) == ["confidence_0", "depth_est_0", "depth_mean_0", "depth_std_0",
                                            "entropy_0", "runner_up_0"]
    for v in range(4):
        maps = {k: fusion.read_pfm(str(scan_out / k / f"{v:0>8}.pfm"))[0] for k in os.listdir(scan_out)}
        assert all(m.shape == (64, 80) and np.isfinite(m).all() for m in maps.values())
        assert (maps["depth_std_0"] >= 0).all() and (maps["entropy_0"] >= 0).all()
        assert (maps["runner_up_0"] <= maps["confidence_0"]).all()
        # the mean lies inside the sample's depth range (one ulp of the far end for its rounding)
        lo, hi = ranges[written.index(f"scan9/{{}}/{v:0>8}{{}}")]
        ulp = float(np.spacing(np.float32(hi)))
        assert (maps["depth_mean_0"] >= lo - ulp).all() and (maps["depth_mean_0"] <= hi + ulp).all()
    # without the flag the tree is exactly what it was
    model.posterior_stats = False
    plain = eval_sharded.parse_args(common + ["--outdir", str(root / "plain")])
    eval_sharded.save_depth(plain, 0, 1, torch.device("cuda", 0), model=model)
    assert sorted(os.listdir(root / "plain" / "scan9")) == ["confidence_0", "depth_est_0"]
    for k in ("depth_est_0", "confidence_0"):
        a = fusion.read_pfm(str(root / "plain" / "scan9" / k / "00000002.pfm"))[0]
        np.testing.assert_array_equal(a, fusion.read_pfm(str(scan_out / k / "00000002.pfm"))[0])


def test_train_driver_uncertainty_metrics(tmp_path):
    """The test pass with uncertainty=True reports four AUSE values beside the same numbers as
    without it; they are the numpy restatement's on the first sample; --uncertainty_metrics
    prints them on their own line."""
    from torch.utils.data import DataLoader
    from aarmvs import ops, train_ddp
    from datasets import find_dataset_def
    from models import EMVSNet
    mini = os.path.join(GOLDEN, "dtu_mini")
    scans = os.path.join(mini, "scans.txt")
    tds = find_dataset_def("dtu_yao")(mini, scans, "test", 3, 8, 1.06, False, False, 3, 0.25)
    loader = DataLoader(tds, 1, shuffle=False, num_workers=0)
    torch.manual_seed(0)
    model = EMVSNet(disparity_level=8, image_scale=0.25, max_h=64, max_w=80, return_cost=True,
                    evidential=False).to(DEV)
    quiet = lambda *a: None
    plain = train_ddp.run_test_pass(model, loader, torch.device(DEV), True, log=quiet)
    both = train_ddp.run_test_pass(model, loader, torch.device(DEV), True, log=quiet, uncertainty=True)
    assert {k: v for k, v in both.items() if not k.startswith(train_ddp.AUSE)} == plain
    au = {k[len(train_ddp.AUSE):]: v for k, v in both.items() if k.startswith(train_ddp.AUSE)}
    assert tuple(au) == train_ddp.RANKINGS == ("conf", "depth_std", "entropy", "runner_up")
    assert all(np.isfinite(v) for v in au.values())
    # the first sample against numpy, from the model's own cost volume
    s = {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in next(iter(loader)).items()}
    with torch.no_grad():
        out = model.eval()(s["imgs"], s["proj_matrices"], s["depth_values"])
    depth_est = train_ddp._loss_and_depth(out, s, True)[1]
    got = train_ddp.sparsification_errors(depth_est, s["depth"], s["mask"], out[0], s["depth_values"])
    # (the rankings are the device's own maps: AUSE is what is restated here, and a last-bit
    # difference in a map could swap two pixels of a ranking)
    post = ops.posterior_from_cost(out[0].float(), s["depth_values"].float())
    unc = {k: post[k].cpu().numpy() for k in ("depth_std", "entropy", "runner_up")}
    unc["conf"] = (1.0 - torch.softmax(out[0].float(), 1).amax(1)).cpu().numpy()
    err = np.abs(depth_est.float().cpu().numpy() - s["depth"].float().cpu().numpy())
    mask = s["mask"].cpu().numpy()
    assert (mask[0] > 0.5).sum() >= 2 and err[0][mask[0] > 0.5].mean() > 0   # the fixture has few valid pixels
    for k in train_ddp.RANKINGS:
        want = pr.ause(err[0], unc[k][0], mask[0])
        print(f"AUSE[{k}] first sample: driver {float(got[k][0]):.6f}, numpy {want:.6f}")
        assert abs(float(got[k][0]) - want) <= 1e-5, k
    # the command-line flag, through one tiny epoch
    lines = []
    args = train_ddp.parse_args([
        "--trainpath", mini, "--trainlist", scans, "--numdepth", "8", "--max_h", "64", "--max_w", "80",
        "--image_scale", "0.25", "--epochs", "1", "--max_steps", "1", "--summary_freq", "1",
        "--train_light_idx", "3", "--testpath", mini, "--testlist", scans, "--fused_loss",
        "--uncertainty_metrics", "--logdir", str(tmp_path / "ck")])
    res = train_ddp.train(args, 0, 1, DEV, log=lambda *a: lines.append(" ".join(map(str, a))))
    assert len(res["test_scalars"]) == 1 and len(res["test_scalars_uncertainty"]) == 1
    assert "test_scalars_refined" not in res
    assert not any(k.startswith(train_ddp.AUSE) for k in res["test_scalars"][0])
    assert sum(ln.startswith("avg_test_scalars:") for ln in lines) == 1
    assert sum(ln.startswith("avg_test_scalars_uncertainty:") for ln in lines) == 1
