"""GPU tests of the loss from the cost volume (aarmvs_cls_loss / _backward) and of the masked depth
metrics (aarmvs_depth_metrics).

Loss, WTA depth, max-probability map and dL/dcost are checked against the outputs of the
reference's mvsnet_cls_loss on torch.softmax, run on the CPU in float32 and float64 by
tests/golden/make_cls_loss_golden.py (tests/golden/cls_loss.npz; inputs regenerated from seeds,
tests/cls_loss_cases.py).  Bounds, each against the reference and none against the code under test:

* loss: |gpu - ref64| <= max(2 |ref32 - ref64|, 1e-6 |ref64|) (1e-6: the project's tightest
  scalar bound, the per-plane mean probability of test_gpu_long.py);
* dL/dcost: relative L2 against float64 <= max(2 x the float32 autograd's, 1e-6); exactly 0
  under a zero mask;
* max-probability map: 1e-5 absolute (the sampled-softmax bound);
* WTA depth and ground-truth index: bit-equal to the float64 run outside pixels whose float64
  top-two probabilities differ by less than 1e-6 relative, which may be at most 1% of a case
  (the generator asserts there are none but in the deliberate tie, which must take the lower
  index);
* loss and gradient bit-identical over two calls and across two processes.

The depth metrics' expectations are a float64 numpy restatement of utils.py:150-175 written
here: the reference's utils.py imports torchvision and tensorboardX, which are not installed, so
it cannot be run (as tests/fusion_tnt_ref.py restates what could not be run there).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cls_loss_cases as cases
from conftest import GOLDEN, ROOT
from aarmvs import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cls_loss.npz"), allow_pickle=False)


def _dev(inp):
    return {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def _rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / den) if den > 0 else float(np.abs(a).max())


def _run(name):
    """loss, gradient and the kernel's per-pixel outputs of a case, as numpy."""
    from aarmvs import ops
    t = _dev(cases.build(name))
    cost = t["cost"].clone().requires_grad_(True)
    loss, wta, pmap = ops.cls_loss(cost, t["depth_gt"], t["mask"], t["depth_values"], want_prob_map=True)
    assert not wta.requires_grad and not pmap.requires_grad
    loss.backward()
    raw = ops.cls_loss_forward(t["cost"], t["depth_gt"], t["mask"], t["depth_values"])
    assert raw["max_prob"] is None
    torch.cuda.synchronize()
    return {"loss": loss.detach().cpu().numpy(), "wta": wta.cpu().numpy(), "pmap": pmap.cpu().numpy(),
            "grad": cost.grad.cpu().numpy(), "gt": raw["gt"].cpu().numpy(),
            "raw_loss": raw["loss"].cpu().numpy()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_loss_and_gradient_match_the_reference(name, golden):
    z = {k: golden[f"{name}/{k}"] for k in ("loss32", "loss64", "wta64", "prob64", "grad64",
                                            "grad32_rel_l2", "gt64", "gap64")}
    inp = cases.build(name)
    B, D, H, W = inp["cost"].shape
    out = _run(name)
    assert out["loss"].dtype == np.float32 and out["loss"].tobytes() == out["raw_loss"].tobytes()

    l64 = float(z["loss64"])
    err, lim = abs(float(out["loss"]) - l64), max(2.0 * abs(float(z["loss32"]) - l64), 1e-6 * abs(l64))
    print(f"\n{name}: loss {float(out['loss']):.9g} ref64 {l64:.9g} err {err:.3e} (bound {lim:.3e})")
    assert err <= lim

    sel = slice(None, None, cases.GRAD_STRIDE.get(name, 1))
    g = out["grad"].reshape(B, D, H * W)
    e_g, lim_g = _rel_l2(g[:, :, sel], z["grad64"]), max(2.0 * float(z["grad32_rel_l2"]), 1e-6)
    print(f"{name}: dL/dcost rel L2 {e_g:.3e} (float32 autograd {float(z['grad32_rel_l2']):.3e}, "
          f"bound {lim_g:.3e})")
    assert e_g <= lim_g
    zero = np.broadcast_to((inp["mask"] == 0)[:, None], (B, D, H, W))
    assert np.all(out["grad"][zero] == 0.0)
    assert np.all(np.isfinite(out["grad"]))

    e_p = float(np.abs(out["pmap"].astype(np.float64) - z["prob64"]).max())
    print(f"{name}: max-probability map max |err| {e_p:.3e}")
    assert e_p <= 1e-5

    excluded = z["gap64"] < 1e-6
    assert excluded.mean() <= 0.01 or name == "tied_maximum"
    keep = ~excluded
    assert np.array_equal(out["wta"].astype(np.float64)[keep], z["wta64"][keep])
    assert np.array_equal(out["gt"], z["gt64"])
    if name == "tied_maximum":   # maxima at planes 3 and 7, bit-equal: the lower index
        assert excluded.all()
        assert np.array_equal(out["wta"], np.broadcast_to(inp["depth_values"][:, 3, None, None], (B, H, W)))


def test_index_rule_corner_cases():
    """What the corner cases are there to show, read off the kernel's index map: the first
    minimum on a midway tie, the end planes outside the range, plane 0 under a zero mask, and
    half-to-even rounding of 0.5 x argmin."""
    from aarmvs import ops

    def gt_of(name):
        t = _dev(cases.build(name))
        return ops.cls_loss_forward(t["cost"], t["depth_gt"], t["mask"], t["depth_values"])["gt"].cpu().numpy()

    for name in ("midway", "out_of_range", "gt0_under_mask0", "half_mask", "on_hypothesis"):
        inp = cases.build(name)
        dist = np.abs(inp["depth_values"][:, :, None, None] - inp["depth_gt"][:, None])   # float32
        first = np.argmin(dist, axis=1)                                                 # first minimum
        want = np.rint(inp["mask"] * first.astype(np.float32)).astype(np.int32)         # half to even
        got = gt_of(name)
        assert np.array_equal(got, want), name
        if name == "midway":
            tie = np.sort(dist, axis=1)
            assert (tie[:, 0] == tie[:, 1]).mean() > 0.5       # most pixels are exact ties
        if name == "out_of_range":
            assert set(np.unique(got[inp["mask"] == 1])) == {0, 15}
        if name == "gt0_under_mask0":
            assert np.all(got[inp["mask"] == 0] == 0)
        if name == "half_mask":
            half = inp["mask"] == 0.5
            odd = first[half] % 2 == 1                 # 0.5 x odd = k + 0.5: to the even neighbour
            assert np.any(odd) and np.all(got[half][odd] % 2 == 0)
            assert np.array_equal(got[half], np.rint(0.5 * first[half]).astype(np.int32))


def test_zero_mask_element_contributes_nothing(golden):
    out = _run("all_zero_mask")
    inp = cases.build("all_zero_mask")
    assert np.all(out["grad"][1] == 0.0) and np.any(out["grad"][0] != 0.0)
    # the loss is half of element 0's own (element 1's term is 0 / 1e-6 = 0)
    from aarmvs import ops
    t = _dev({k: v[:1] for k, v in inp.items()})
    alone = ops.cls_loss(t["cost"], t["depth_gt"], t["mask"], t["depth_values"])[0].item()
    assert abs(float(out["loss"]) - 0.5 * alone) <= 1e-6 * abs(0.5 * alone)


def _digest(name):
    out = _run(name)
    return hashlib.sha256(out["loss"].tobytes() + out["grad"].tobytes()).hexdigest()


def test_loss_and_gradient_are_bit_identical_across_calls_and_processes():
    name = "b2_d48_52x84"   # 18 blocks per element: the fixed-order reduce
    a, b = _digest(name), _digest(name)
    assert a == b
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [os.path.join(ROOT, "aa-rmvsnet_amd"), os.path.join(ROOT, "tests"), ROOT,
         os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c",
                        "import test_gpu_cls_loss as t; print('DIGEST', t._digest(%r))" % name],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"DIGEST {a}" in r.stdout


# -- depth metrics -------------------------------------------------------------------------
def _metrics_ref(est, gt, mask, thresholds):
    """utils.py:150-175 restated in float64 numpy: per batch element over mask > 0.5 the mean of
    the float32 |est - gt| and the share above each threshold, then the mean over elements."""
    rows = []
    for b in range(est.shape[0]):
        m = mask[b] > 0.5
        e = np.abs(est[b][m] - gt[b][m]).astype(np.float64)      # the float32 difference, as torch
        n = e.size
        rows.append([n, e.sum() / n if n else np.nan] + [(e > t).sum() / n if n else np.nan
                                                          for t in thresholds])
    rows = np.array(rows, np.float64)
    return rows[:, 0], rows[:, 1:].mean(axis=0)


def _metric_inputs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(425, 935, (B, H, W)).astype(np.float32)
    # errors on both sides of every threshold, some exactly on one (not counted: strict >)
    err = rng.choice(np.array([0, 1, 2, 3, 4, 7, 8, 9, 16, 20, 32, 40], np.float32), (B, H, W))
    est = (gt + err * rng.choice(np.array([-1, 1], np.float32), (B, H, W))).astype(np.float32)
    mask = rng.choice(np.array([0, 0.5, 0.75, 1], np.float32), (B, H, W))
    return est, gt, mask


@pytest.mark.parametrize("shape", [(1, 4, 4), (1, 4, 132), (2, 52, 84), (3, 16, 20)])
def test_depth_metrics_match_the_restatement(shape):
    from aarmvs import ops
    thr = (2, 4, 8, 16, 32)
    est, gt, mask = _metric_inputs(*shape, seed=sum(shape))
    res = ops.depth_metrics(*(torch.from_numpy(a).to(DEV) for a in (est, gt, mask)), thresholds=thr)
    assert list(res) == ["abs_depth_error"] + [f"thres{t}mm_error" for t in thr]
    n, want = _metrics_ref(est, gt, mask, thr)
    got = np.array([v.item() for v in res.values()])
    assert abs(got[0] - want[0]) <= 1e-6 * want[0]
    # counts exact: the shares are count / n in float64 on both sides
    assert np.array_equal(got[1:], want[1:])
    if shape[0] > 1:   # the mean of the per-element values
        each = [ops.depth_metrics(*(torch.from_numpy(a[b:b + 1]).to(DEV) for a in (est, gt, mask)),
                                  thresholds=thr) for b in range(shape[0])]
        for k in res:
            assert abs(res[k].item() - np.mean([e[k].item() for e in each])) <= 1e-15 * max(1.0, abs(res[k].item()))


def test_depth_metrics_empty_mask_is_nan_and_threshold_count_is_free():
    from aarmvs import AarmvsError, ops
    est, gt, mask = _metric_inputs(2, 8, 12, seed=5)
    mask[1] = 0.5   # not above 0.5: no valid pixel in element 1
    t = [torch.from_numpy(a).to(DEV) for a in (est, gt, mask)]
    res = ops.depth_metrics(*t)
    assert all(np.isnan(v.item()) for v in res.values())
    res0 = ops.depth_metrics(*(a[:1] for a in t), thresholds=(0.5, 1, 2, 4, 8, 16, 32, 64))
    assert len(res0) == 9 and "thres0.5mm_error" in res0 and all(np.isfinite(v.item()) for v in res0.values())
    assert list(ops.depth_metrics(*(a[:1] for a in t), thresholds=())) == ["abs_depth_error"]
    with pytest.raises(AarmvsError):
        ops.depth_metrics(*t, thresholds=range(9))


# -- end to end ------------------------------------------------------------------------------
def _model(D, H, W, wseed, **kw):
    import torch.nn as nn
    from models import EMVSNet
    m = EMVSNet(disparity_level=D, image_scale=1.0, max_h=H, max_w=W, return_depth=False, **kw)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.init_weights(shapes, seed=wseed).items()},
                      strict=True)
    m.feature = nn.Identity()
    return m.to(DEV)


def test_model_with_return_cost_matches_the_default_path():
    """EMVSNet(return_cost=True) + mvsnet_cls_loss_from_cost against the default EMVSNet +
    mvsnet_cls_loss at 32x48, N = 3, D = 8: the loss and the tensor handed to
    _SweepTrain.backward, each within the bounds above of a float64 CPU evaluation of the same
    cost volume, with the default (float32) path in the place of the float32 reference."""
    from models import mvsnet_cls_loss, mvsnet_cls_loss_from_cost
    B, N, H, W, D = 1, 3, 32, 48, 8
    sc = syn.scene(B, N, H, W, D, seed=31)
    gt, mask = (torch.from_numpy(a) for a in syn.depth_targets(sc["depth_values"], H, W, seed=31))
    imgs = torch.from_numpy(np.moveaxis(sc["features"], 0, 1).copy()).to(DEV)
    proj, dv = torch.from_numpy(sc["proj_matrices"]).to(DEV), torch.from_numpy(sc["depth_values"]).to(DEV)
    got = {}

    unfused = _model(D, H, W, 3, evidential=False)
    prob, ev, pc = unfused(imgs, proj, dv)
    assert ev is None and pc is None
    prob.grad_fn.next_functions[0][0].register_prehook(lambda g: got.__setitem__("unfused", g[0].clone()))
    loss_u, wta_u = mvsnet_cls_loss(prob, gt.to(DEV), mask.to(DEV), dv)
    loss_u.backward()

    fused = _model(D, H, W, 3, evidential=False, return_cost=True)
    cost, ev, pc = fused(imgs, proj, dv)
    assert ev is None and pc is None and tuple(cost.shape) == (B, D, H, W)
    cost.register_hook(lambda g: got.__setitem__("fused", g.clone()))
    loss_f, wta_f = mvsnet_cls_loss_from_cost(cost, gt.to(DEV), mask.to(DEV), dv)
    loss_f.backward()
    torch.cuda.synchronize()
    assert torch.equal(torch.softmax(cost.detach(), 1).argmax(1), prob.detach().argmax(1))
    assert torch.equal(wta_f, wta_u)
    for (ku, pu), (kf, pf) in zip(unfused.named_parameters(), fused.named_parameters()):
        assert (pu.grad is None) == (pf.grad is None), ku

    c64 = cost.detach().cpu().double().requires_grad_(True)
    l64, _ = mvsnet_cls_loss(torch.softmax(c64, 1), gt.double(), mask.double(), dv.cpu().double())
    l64.backward()
    l64, g64 = l64.item(), c64.grad.numpy()
    err_f, err_u = abs(loss_f.item() - l64), abs(loss_u.item() - l64)
    e_f, e_u = _rel_l2(got["fused"].cpu().numpy(), g64), _rel_l2(got["unfused"].cpu().numpy(), g64)
    print(f"\nloss: fused err {err_f:.3e}, default {err_u:.3e}; dL/dcost rel L2: fused {e_f:.3e}, "
          f"default {e_u:.3e}")
    assert err_f <= max(2.0 * err_u, 1e-6 * abs(l64))
    assert e_f <= max(2.0 * e_u, 1e-6)


def test_return_cost_feeds_the_evidential_head_the_softmax():
    """Where the head runs (B = 1, D = 32) a return_cost model still gives it softmax(cost):
    its evidential outputs equal the default model's, and the first slot is the raw cost."""
    B, N, H, W, D = 1, 3, 32, 48, 32
    sc = syn.scene(B, N, H, W, D, seed=32)
    imgs = torch.from_numpy(np.moveaxis(sc["features"], 0, 1).copy()).to(DEV)
    proj, dv = torch.from_numpy(sc["proj_matrices"]).to(DEV), torch.from_numpy(sc["depth_values"]).to(DEV)
    with torch.no_grad():
        prob, ev, pc = _model(D, H, W, 4).eval()(imgs, proj, dv)
        cost, ev_c, pc_c = _model(D, H, W, 4, return_cost=True).eval()(imgs, proj, dv)
    assert ev is not None and torch.equal(ev, ev_c) and torch.equal(pc, pc_c)
    assert torch.equal(torch.softmax(cost, 1).argmax(1), prob.argmax(1))
    assert not torch.allclose(cost.sum(1), torch.ones_like(cost.sum(1)))


# -- the training driver ---------------------------------------------------------------------
MINI = os.path.join(ROOT, "tests", "golden", "dtu_mini")


def _train_argv(tmp_path, tag, extra=()):
    return ["--trainpath", MINI, "--trainlist", os.path.join(MINI, "scans.txt"), "--numdepth", "8",
            "--max_h", "64", "--max_w", "80", "--image_scale", "0.25", "--max_steps", "1",
            "--logdir", str(tmp_path / tag), "--summary_freq", "1", "--train_light_idx", "3", *extra]


def _train(tmp_path, tag, extra=()):
    from aarmvs import train_ddp
    lines = []
    out = train_ddp.train(train_ddp.parse_args(_train_argv(tmp_path, tag, extra)), 0, 1, DEV,
                          log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    return out, lines


TEST_FLAGS = ["--testpath", MINI, "--testlist", os.path.join(MINI, "scans.txt")]
KEYS = ["loss", "abs_depth_error"] + [f"thres{t}mm_error" for t in (2, 4, 8, 16, 32)]


def test_train_driver_default_path_is_unchanged_by_the_new_flags(tmp_path):
    """Two epochs of one step: without the new flags the driver returns the same losses as with
    a test pass between the epochs (which must leave the training untouched), no test scalars,
    and a fused first step within 1e-6 relative of the unfused one.

    Step 0 is compared bit for bit.  The second loss follows an optimiser step, and the training
    step is not bit-reproducible from run to run with or without this change: for one, FeatNet's
    deformable-conv backward adds dL/dx with fp32 atomics in no fixed order (include/aarmvs.h,
    aarmvs_deform_sample_backward).  Two runs of this test on one tree gave 2.076565742 twice,
    then 2.076565742 against 2.076565981: one float32 ulp, 1.1e-7 relative.  Its bound is 1e-5
    relative: reordered fp32 sums move a gradient by ~1e-7 relative, and Adam's first step,
    g / (|g| + 1e-8), can amplify that for near-zero gradients; two orders of magnitude are left
    for that, far below what a disturbed training (another sample, another mode) would show."""
    base, _ = _train(tmp_path, "a", ["--epochs", "2"])
    assert set(base) == {"losses", "checkpoints", "test_scalars"} and base["test_scalars"] == []
    assert len(base["losses"]) == 2 and all(np.isfinite(base["losses"]))
    again, lines = _train(tmp_path, "b", ["--epochs", "2", *TEST_FLAGS])
    print("\nlosses without / with the test pass:", base["losses"], again["losses"])
    assert again["losses"][0] == base["losses"][0]
    assert abs(again["losses"][1] - base["losses"][1]) <= 1e-5 * abs(base["losses"][1])
    assert len(again["test_scalars"]) == 2 and all(list(s) == KEYS for s in again["test_scalars"])
    assert sum(ln.startswith("avg_test_scalars:") for ln in lines) == 2
    fused, _ = _train(tmp_path, "c", ["--epochs", "1", "--fused_loss"])
    print("step 0 loss unfused / fused:", base["losses"][0], fused["losses"][0])
    assert abs(fused["losses"][0] - base["losses"][0]) <= 1e-6 * abs(base["losses"][0])


def test_train_driver_test_pass_one_rank_equals_two_ranks(tmp_path):
    """--testpath at lr 0 (the weights stay the seeded initial ones on every rank): one rank and
    two ranks (shared-GPU rehearsal, gloo) return the same test scalars up to fp64 summation
    order, the two ranks' batch counts add up to the 8 test samples, and the fused and the
    unfused test pass agree (loss to 1e-6, the depth metrics exactly: the same WTA depth)."""
    import socket
    flags = ["--epochs", "1", "--lr", "0", *TEST_FLAGS]
    one, lines = _train(tmp_path, "one", flags + ["--fused_loss"])
    s1 = one["test_scalars"][0]
    assert list(s1) == KEYS and all(np.isfinite(list(s1.values())))
    assert any("8 of 8 test batches" in ln for ln in lines), lines
    plain, _ = _train(tmp_path, "plain", flags)
    s0 = plain["test_scalars"][0]
    assert abs(s1["loss"] - s0["loss"]) <= 1e-6 * abs(s0["loss"])
    assert all(s1[k] == s0[k] for k in KEYS[1:])

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "aarmvs.train_ddp", *_train_argv(tmp_path, "two", flags + ["--fused_loss"])]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), AARMVS_SHARED_GPU="1",
                   PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "aa-rmvsnet_amd"), ROOT,
                                               os.environ.get("PYTHONPATH", "")]))
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=150)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
        assert p.returncode == 0, out[-3000:]
    counts = [int(ln.split(" ran ")[1].split(" of ")[0]) for out in outs for ln in out.splitlines()
              if ln.startswith("test pass: rank")]
    assert counts == [4, 4], outs
    line = [ln for ln in outs[0].splitlines() if ln.startswith("avg_test_scalars:")]
    assert len(line) == 1 and not any(ln.startswith("avg_test_scalars:") for ln in outs[1].splitlines())
    s2 = eval(line[0].split(":", 1)[1], {"nan": float("nan")})
    assert list(s2) == KEYS
    for k in KEYS:
        assert abs(s2[k] - s1[k]) <= 1e-12 * abs(s1[k]), (k, s1[k], s2[k])
