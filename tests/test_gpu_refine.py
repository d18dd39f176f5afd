"""GPU tests of the opt-in sub-plane refinement of the sweep's winner-take-all
(DepthSweep(...)(want_refined=True), aarmvs_sweep_r; the standalone aarmvs_wta_refine_update /
_finalize pair; aarmvs_refine_from_cost; EMVSNet(refine_depth=True) and the drivers).

Shapes: 20x36 frames (not a multiple of the head kernel's 8x32 tile: partial tiles in both
directions, six blocks per batch element), B = 2, two source views, random parameters.  The
float64 reference is tests/refine_ref.py on the cost volume the GPU produced; its bound comes
from the number formats (refine_ref.depth_bound), never from a GPU result.
"""
import functools
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from aarmvs import synthetic as syn

import refine_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, H, W = 2, 3, 20, 36
KEYS = ("depth_refined", "conf_window", "index")


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
def refined_sweep(D):
    """One refined sweep per D, shared (read-only) by the tests."""
    return run(D, want_refined=True)


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
    st = ops.refine_state(Bc, cost[0, 0].numel(), cost.device)
    for d in range(n):
        ops.wta_refine_update(cost[:, d].contiguous(), d, dv[:, d], mp, dm, es, st)
    out = ops.wta_refine_finalize(mp, dm, es, st, dv, n)
    out.update(depth=dm, conf=mp / es, max_prob=mp)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------
# 1. off changes nothing
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["split", "fp16"])
def test_refinement_leaves_the_other_outputs_bit_identical(precision):
    off = run(5, precision)
    on = run(5, precision, want_refined=True)
    again = run(5, precision)
    assert set(KEYS).isdisjoint(off) and set(KEYS) <= set(on)
    for k in ("depth", "conf", "cost"):
        assert torch.equal(off[k], on[k]), k
        assert torch.equal(off[k], again[k]), k
    assert on["index"].dtype == torch.int32 and tuple(on["index"].shape) == (B, H, W)


# ---------------------------------------------------------------------------------------
# 2. online == from the volume == the standalone pair
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 17])
def test_online_equals_the_volume_form_and_the_standalone_pair(D):
    from aarmvs import ops
    out = refined_sweep(D)
    dv = scene(D)[2].to(DEV)
    vol = ops.refine_from_cost(out["cost"], dv)
    pair = standalone(out["cost"], dv)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], vol[k]), k
        assert torch.equal(out[k], pair[k]), k
    assert torch.equal(pair["depth"], out["depth"]) and torch.equal(pair["conf"], out["conf"])
    # the refinement is on: some pixels moved off their plane, the border winners did not
    moved = out["depth_refined"] != out["depth"]
    assert moved.any()
    border = (out["index"] <= 0) | (out["index"] == D - 1)
    assert not moved[border].any()
    assert (out["conf_window"] >= out["conf"]).all()


# ---------------------------------------------------------------------------------------
# 3. against float64
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 17])
def test_against_the_float64_definition(D):
    out = refined_sweep(D)
    dv = scene(D)[2].numpy()
    ref = rr.from_volume64(out["cost"].cpu().numpy(), dv)
    keep = ~ref["near_tie"]
    excluded = 1.0 - float(keep.mean())
    idx = out["index"].cpu().numpy()
    got = out["depth_refined"].cpu().numpy().astype(np.float64)
    err = np.abs(got - ref["depth_refined"])
    bound = rr.depth_bound(ref)
    print(f"D={D}: near-ties excluded {excluded:.4%}, refined {float(ref['refined'].mean()):.2%}, "
          f"worst err / bound {float((err[keep] / np.maximum(bound[keep], 1e-300)).max()):.3f}")
    assert excluded <= 0.01
    assert np.array_equal(idx[keep], ref["index"][keep])
    assert ref["refined"][keep].any()
    assert (err[keep] <= bound[keep]).all()
    cw = out["conf_window"].cpu().numpy().astype(np.float64)
    assert np.allclose(cw[keep], ref["conf_window"][keep], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------
# 4. schedules and ranges
# ---------------------------------------------------------------------------------------
def test_schedules_and_plane_ranges():
    D = 5
    whole = refined_sweep(D)
    sw = sweeper()
    sw.overlap = False
    try:
        serial = run(D, want_refined=True)
    finally:
        sw.overlap = True
    for k in KEYS + ("depth", "conf", "cost"):
        assert torch.equal(whole[k], serial[k]), k
    # (0, 3) + (3, 5) through the sweeper's one state buffer
    cost = torch.empty(B, D, H, W, device=DEV)
    first = run(D, d_range=(0, 3), cost_out=cost, want_refined=True)
    first = {k: first[k].clone() for k in KEYS}
    second = run(D, d_range=(3, D), cost_out=cost, want_refined=True)
    for k in KEYS + ("depth", "conf"):
        assert torch.equal(whole[k], second[k]), k
    assert torch.equal(whole["cost"], cost)
    # after (0, 3) alone the outputs describe planes 0..2: a winner on plane 2 has no right
    # neighbour yet and keeps its plane's depth
    dv = scene(D)[2].to(DEV)
    last = first["index"] == 2
    assert last.any()
    assert torch.equal(first["depth_refined"][last], dv[:, 2].view(B, 1, 1).expand(B, H, W)[last])
    part = standalone(whole["cost"], dv, n=3)
    for k in KEYS:
        assert torch.equal(first[k], part[k]), k
    # ... and is refined once plane 3 has been seen, unless a later plane took over
    still = last & (whole["index"] == 2)
    assert still.any() and (whole["depth_refined"][still] != dv[:, 2].view(B, 1, 1).expand(B, H, W)[still]).any()


# ---------------------------------------------------------------------------------------
# 5. hand-made planes through the standalone pair
# ---------------------------------------------------------------------------------------
NAN = float("nan")
HAND = np.array([          # one row per pixel, one column per plane
    [2.0, 0.0, 0.0, 0.0],       # 0 winner on plane 0
    [0.0, 0.0, 0.0, 2.0],       # 1 winner on the last plane
    [0.0, 1.0, 1.0, 0.0],       # 2 a tie at planes 1 and 2: the first wins
    [1.0, 0.5, 3.0, 0.0],       # 3 a late larger winner
    [0.0, 100.0, 0.0, 0.0],     # 4 exp overflows
    [-200.0] * 4,               # 5 p == 0 on every plane
    [0.0, 2.0, NAN, 0.0],       # 6 a NaN plane beside the winner
    [0.0, 2.0, 1.0, 0.0],       # 7 plainly refinable
], np.float32)


def _hand(dv_row):
    cost = torch.from_numpy(HAND.T.copy()).view(1, 4, 1, 8).to(DEV)
    dv = torch.tensor([dv_row], dtype=torch.float32, device=DEV)
    out = standalone(cost, dv)
    return {k: v.reshape(-1).cpu() for k, v in out.items()}


def test_hand_made_planes():
    o = _hand([1.0, 2.0, 3.0, 4.0])
    dr, cw, idx, wta, conf, mp = (o[k] for k in ("depth_refined", "conf_window", "index", "depth", "conf",
                                                 "max_prob"))
    assert idx.tolist() == [0, 3, 1, 2, 1, -1, 1, 1]
    unrefined = [0, 1, 4, 5, 6]
    assert same(dr[unrefined], wta[unrefined])
    assert dr[unrefined].tolist() == [1.0, 4.0, 2.0, 0.0, 2.0]
    # the tie: p[1] = p[2] = e (max_prob holds it), p[0] = exp(0) = 1 exactly; float32 by hand
    e = mp[2].numpy()
    one = np.float32(1.0)
    s = (one + e) + e
    num = one * np.float32(1.0 - 2.0) + e * np.float32(3.0 - 2.0)
    assert dr[2].numpy() == np.float32(2.0) + num / s and dr[2] > 2.0
    assert cw[2].numpy() == s / (((one + e) + e) + one)
    # the late winner: plane 2 takes p_left from plane 1 (not from the old winner, plane 0) and
    # its right neighbour is plane 3 (the old winner's p_right = p[1] is dropped)
    p = np.exp(HAND[3].astype(np.float64))
    want = 3.0 + (p[1] * (2.0 - 3.0) + p[3] * (4.0 - 3.0)) / (p[1] + p[2] + p[3])
    assert abs(float(dr[3]) - want) <= 2.0 ** -23 * 3.0 + 2.0 ** -19
    assert abs(float(cw[3]) - (p[1] + p[2] + p[3]) / p.sum()) <= 1e-6
    # borders: one-sided sums
    p0 = np.exp(HAND[0].astype(np.float64))
    assert abs(float(cw[0]) - (p0[0] + p0[1]) / p0.sum()) <= 1e-6
    assert abs(float(cw[1]) - (p0[0] + p0[1]) / p0.sum()) <= 1e-6      # the mirrored pixel
    # overflow, no winner, NaN: conf_window is NaN exactly where conf is
    assert torch.isnan(conf).tolist() == [False, False, False, False, True, True, True, False]
    assert torch.equal(torch.isnan(cw), torch.isnan(conf))
    assert bool((cw[~torch.isnan(cw)] >= conf[~torch.isnan(conf)]).all())
    # the plain pixel, against float64
    p7 = np.exp(HAND[7].astype(np.float64))
    want = 2.0 + (p7[0] * -1.0 + p7[2] * 1.0) / (p7[0] + p7[1] + p7[2])
    assert abs(float(dr[7]) - want) <= 2.0 ** -23 * 2.0 + 2.0 ** -19 and 2.0 < float(dr[7]) < 3.0


def test_hand_made_planes_with_inverse_depth_spacing():
    dv = (1.0 / np.linspace(1.0 / 400.0, 1.0 / 1000.0, 4)).astype(np.float32)     # 400 .. 1000, uneven
    o = _hand(dv.tolist())
    dr, idx = o["depth_refined"], o["index"]
    for px in (2, 3, 7):
        w = int(idx[px])
        lo, hi = float(dv[w - 1]), float(dv[w + 1])
        assert lo < float(dr[px]) < hi and float(dr[px]) != float(dv[w])
        p = np.exp(HAND[px].astype(np.float64))
        d64 = dv.astype(np.float64)
        want = d64[w] + (p[w - 1] * (d64[w - 1] - d64[w]) + p[w + 1] * (d64[w + 1] - d64[w])) / p[w - 1:w + 2].sum()
        spread = max(abs(d64[w - 1] - d64[w]), abs(d64[w + 1] - d64[w]))
        assert abs(float(dr[px]) - want) <= 2.0 ** -23 * d64[w] + 2.0 ** -19 * spread
    assert same(dr[[0, 1, 4, 5, 6]], o["depth"][[0, 1, 4, 5, 6]])


@pytest.mark.parametrize("D", [1, 2])
def test_one_and_two_planes_are_never_refined(D):
    from aarmvs import ops
    g = torch.Generator().manual_seed(D)
    cost = torch.randn(2, D, 3, 5, generator=g).to(DEV)
    dv = torch.linspace(425.0, 935.0, 4)[:D].repeat(2, 1).to(DEV)
    o = standalone(cost, dv)
    v = ops.refine_from_cost(cost, dv)
    assert torch.equal(o["depth_refined"], o["depth"]) and torch.equal(v["depth_refined"], o["depth"])
    assert torch.equal(o["index"], cost.argmax(1).int())
    assert bool((o["conf_window"] == 1.0).all()) if D == 1 else bool((o["conf_window"] >= o["conf"]).all())
    for k in KEYS:
        assert torch.equal(o[k], v[k])


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


def test_emvsnet_refine_depth():
    D = 5
    feats, proj, dv = scene(D)
    want = refined_sweep(D)
    imgs = feats.transpose(0, 1).contiguous().to(DEV)
    with torch.no_grad():
        plain = _emvsnet(D, return_depth=True)(imgs, proj.to(DEV), dv.to(DEV))
        out = _emvsnet(D, return_depth=True, refine_depth=True)(imgs, proj.to(DEV), dv.to(DEV))
    assert set(plain) == {"depth", "photometric_confidence", "evidential_prediction"}
    assert set(out) == set(plain) | {"depth_refined", "photometric_confidence_window"}
    assert torch.equal(out["depth"], plain["depth"]) and torch.equal(out["depth"], want["depth"])
    assert torch.equal(out["photometric_confidence"], plain["photometric_confidence"])
    assert out["evidential_prediction"] is None and plain["evidential_prediction"] is None
    assert torch.equal(out["depth_refined"], want["depth_refined"])
    assert torch.equal(out["photometric_confidence_window"], want["conf_window"])


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


def test_eval_and_fusion_drivers(tmp_path):
    from aarmvs import eval_sharded, fusion
    from models import EMVSNet
    root = _eval_tree(tmp_path)
    common = ["--testpath", str(root), "--testlist", str(root / "list.txt"), "--max_h", "64", "--max_w", "80",
              "--numdepth", "8", "--view_num", "3", "--interval_scale", "1.06"]
    torch.manual_seed(0)
    model = EMVSNet(disparity_level=8, image_scale=1.0, max_h=64, max_w=80, return_depth=True,
                    evidential=False, refine_depth=True)
    args = eval_sharded.parse_args(common + ["--outdir", str(root / "out"), "--refine_depth"])
    written = eval_sharded.save_depth(args, 0, 1, torch.device("cuda", 0), model=model)
    assert len(written) == 4
    scan_out = root / "out" / "scan9"
    for v in range(4):
        maps = {k: fusion.read_pfm(str(scan_out / k / f"{v:0>8}.pfm"))[0]
                for k in ("depth_est_0", "confidence_0", "depth_refined_0", "confidence_window_0")}
        assert all(m.shape == (64, 80) for m in maps.values())
        assert (maps["confidence_window_0"] >= maps["confidence_0"]).all()
        assert (maps["depth_refined_0"] != maps["depth_est_0"]).any()
    # without the flag the two folders are not written, and the two others hold the same maps
    model.refine_depth = False
    plain = eval_sharded.parse_args(common + ["--outdir", str(root / "plain")])
    eval_sharded.save_depth(plain, 0, 1, torch.device("cuda", 0), model=model)
    assert sorted(os.listdir(root / "plain" / "scan9")) == ["confidence_0", "depth_est_0"]
    for k in ("depth_est_0", "confidence_0"):
        a = fusion.read_pfm(str(root / "plain" / "scan9" / k / "00000002.pfm"))[0]
        np.testing.assert_array_equal(a, fusion.read_pfm(str(scan_out / k / "00000002.pfm"))[0])
    # fusion: the default arguments read depth_est_0 / confidence_0 as before ...
    base = ["--test_dataset", "dtu", "--testpath", str(root), "--testlist", str(root / "list.txt"),
            "--outdir", str(root / "out"), "--photo_threshold", "0.0"]
    ply = root / "out" / "mvsnet_009_l3.ply"
    fusion.main(base)
    default = ply.read_bytes()
    n = fusion.filter_depth(str(root / "scan9"), str(scan_out), str(root / "positional.ply"), 0.0)
    assert (root / "positional.ply").read_bytes() == default and n >= 0
    shutil.copytree(scan_out / "depth_est_0", scan_out / "depth_copy")
    shutil.copytree(scan_out / "confidence_0", scan_out / "conf_copy")
    fusion.main(base + ["--depth_dir", "depth_copy", "--conf_dir", "conf_copy"])
    assert ply.read_bytes() == default
    # ... and the refined maps fuse through the same path
    fusion.main(base + ["--depth_dir", "depth_refined_0", "--conf_dir", "confidence_window_0"])
    refined = ply.read_bytes()
    assert refined.startswith(b"ply\n")
    n_ref = fusion.filter_depth(str(root / "scan9"), str(scan_out), str(root / "kw.ply"), 0.0,
                                depth_dir="depth_refined_0", conf_dir="confidence_window_0")
    assert (root / "kw.ply").read_bytes() == refined and n_ref >= 0
    # the folders are really the ones read: other maps give other points, a missing one none
    assert n > 0 and refined != default
    assert fusion.filter_depth(str(root / "scan9"), str(scan_out), str(root / "none.ply"), 0.0,
                               depth_dir="depth_missing_0") == 0


def test_train_driver_refine_metrics(tmp_path):
    """The test pass with refine=True reports the refined depth's six metrics beside the same
    numbers as without it, in both loss modes; --refine_metrics prints them on their own line."""
    from torch.utils.data import DataLoader
    from aarmvs import ops, train_ddp
    from datasets import find_dataset_def
    from models import EMVSNet
    mini = os.path.join(GOLDEN, "dtu_mini")
    scans = os.path.join(mini, "scans.txt")
    tds = find_dataset_def("dtu_yao")(mini, scans, "test", 3, 8, 1.06, False, False, 3, 0.25)
    loader = DataLoader(tds, 1, shuffle=False, num_workers=0)
    for fused in (True, False):
        torch.manual_seed(0)
        model = EMVSNet(disparity_level=8, image_scale=0.25, max_h=64, max_w=80, return_cost=fused,
                        evidential=False).to(DEV)
        plain = train_ddp.run_test_pass(model, loader, torch.device(DEV), fused, log=lambda *a: None)
        both = train_ddp.run_test_pass(model, loader, torch.device(DEV), fused, log=lambda *a: None, refine=True)
        assert {k: v for k, v in both.items() if not k.startswith(train_ddp.REFINED)} == plain
        ref = {k[len(train_ddp.REFINED):]: v for k, v in both.items() if k.startswith(train_ddp.REFINED)}
        assert set(ref) == set(plain) - {"loss"} and all(np.isfinite(v) for v in ref.values())
    # the numbers are aarmvs_depth_metrics of refine_from_cost's depth (last model: probabilities)
    s = {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in next(iter(loader)).items()}
    with torch.no_grad():
        prob = model.eval()(s["imgs"], s["proj_matrices"], s["depth_values"])[0]
    r = ops.refine_from_cost(torch.log(prob), s["depth_values"].float())
    assert (r["depth_refined"] != train_ddp._loss_and_depth((prob, None, None), s, False)[1]).any()
    # the command-line flag, through one tiny epoch
    lines = []
    args = train_ddp.parse_args([
        "--trainpath", mini, "--trainlist", scans, "--numdepth", "8", "--max_h", "64", "--max_w", "80",
        "--image_scale", "0.25", "--epochs", "1", "--max_steps", "1", "--summary_freq", "1",
        "--train_light_idx", "3", "--testpath", mini, "--testlist", scans, "--fused_loss",
        "--refine_metrics", "--logdir", str(tmp_path / "ck")])
    out = train_ddp.train(args, 0, 1, DEV, log=lambda *a: lines.append(" ".join(map(str, a))))
    assert len(out["test_scalars"]) == 1 and len(out["test_scalars_refined"]) == 1
    assert not any(k.startswith(train_ddp.REFINED) for k in out["test_scalars"][0])
    assert sum(ln.startswith("avg_test_scalars:") for ln in lines) == 1
    assert sum(ln.startswith("avg_test_scalars_refined:") for ln in lines) == 1
