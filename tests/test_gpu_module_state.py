"""GPU tests of EMVSNet over time (cases and references: tests/module_state_cases.py; the CPU
side: tests/test_module_state_cases.py).

1. A parameter change between two calls of one model, in every idiom of the case list: the
   next forward, inference and training, runs on the current values -- bit-equal to a fresh twin.
2. copy.deepcopy, pickle / torch.save and swa_utils.AveragedModel of a model before any forward,
   after an inference forward and after a training step: no error, equal outputs, independent.
3. Graphs that outlive a change: a backward after the weights moved differentiates at its own
   forward's weights; two forwards and one backward; accumulation; frozen parameters.
4. Three steps of plain SGD against the float64 oracle's trajectory.

Everything but 4 is compared with torch.equal: the sweep is bit-reproducible across objects
(DESIGN.md §6).  Frame 1 x 3 x 16 x 24, D = 4 (D = 20 with checkpoint_planes = 16).
"""
import os

import pytest
import torch

import module_state_cases as msc

pytestmark = pytest.mark.gpu
DEV = "cuda"
_, _, H, W, D = msc.FRAME


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def s():
    return msc.sample(DEV)


def _model(D=D, **kw):
    return msc.build(D, H, W, DEV, **kw)


def _differs(a, b) -> bool:
    return not torch.equal(a, b)


# ---------------------------------------------------------------------------------------
# 1. parameter changes between calls
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", msc.CASE_NAMES)
def test_forward_after_a_parameter_change_equals_the_fresh_twin(name, s):
    m = _model()
    c = msc.case(name)
    state = c.prepare(m)
    before = msc.observe(m, s)   # the warm-up: an inference forward, a training forward + backward
    c.apply(m, state, DEV)
    after = msc.observe(m, s)
    assert _differs(after["cost"], before["cost"]), "the change did not reach the cost volume"
    msc.same_bits(after, msc.observe(msc.fresh(m, DEV), s), name)


def test_depth_sweep_snapshots_its_parameters_at_construction(s):
    """DepthSweep(params, dev) followed at once by in-place changes to params (nothing
    synchronised in between): the sweep runs on the values at construction."""
    from aarmvs import ops
    imgs, proj, dv, _ = s
    args = (imgs[:, 0], [imgs[:, v] for v in range(1, imgs.shape[1])], proj[:, 0],
            [proj[:, v] for v in range(1, imgs.shape[1])], dv)
    P = {k: torch.from_numpy(v).to(DEV) for k, v in msc.syn.sweep_weights(msc.WSEED).items()}
    want = ops.DepthSweep({k: v.clone() for k, v in P.items()}, DEV)(*args, want_cost=True)
    sw = ops.DepthSweep(P, DEV)
    for k, v in P.items():
        v.copy_(msc.new_value(v, k), non_blocking=True)
    got = sw(*args, want_cost=True)
    moved = ops.DepthSweep(P, DEV)(*args, want_cost=True)
    for k in ("depth", "conf", "cost"):
        assert torch.equal(got[k], want[k]), k
    assert _differs(moved["cost"], want["cost"])


# ---------------------------------------------------------------------------------------
# 2. copies of a model that has run
# ---------------------------------------------------------------------------------------
def _reach(m, state, s):
    if state == "after_inference":
        msc.infer(m, s)
    elif state == "after_training":
        msc.observe(m, s)
    else:
        assert state == "new"


@pytest.mark.parametrize("state", msc.STATES)
@pytest.mark.parametrize("how", list(msc.COPIES))
def test_copy_of_a_model_runs_equal_and_independent(how, state, s):
    m = _model()
    keys = list(m.state_dict())
    _reach(m, state, s)
    assert list(m.state_dict()) == keys
    c = msc.COPIES[how](m)   # must not raise
    assert c is not m and list(c.state_dict()) == keys
    want = msc.observe(m, s)
    msc.same_bits(msc.observe(c, s), want, f"{how} {state}: the copy")
    assert list(c.state_dict()) == keys == list(m.state_dict())
    # independent: the copy's weights move, the original's outputs do not ...
    msc.scale_weights(c, 1.25)
    moved = msc.observe(c, s)
    assert _differs(moved["cost"], want["cost"])
    msc.same_bits(moved, msc.observe(msc.fresh(c, DEV), s), f"{how} {state}: the changed copy")
    msc.same_bits(msc.observe(m, s), want, f"{how} {state}: the original after the copy changed")
    # ... and the reverse
    msc.scale_weights(m, 0.75)
    assert _differs(msc.infer(m, s)["cost"], want["cost"])
    msc.same_bits(msc.observe(c, s), moved, f"{how} {state}: the copy after the original changed")


# ---------------------------------------------------------------------------------------
# 3. graphs that outlive a change
# ---------------------------------------------------------------------------------------
CKPT = [(D, 0), (msc.CKPT_D, msc.CKPT_S)]   # (planes, checkpoint_planes)


def _forward(m, smp):
    imgs, proj, dv, R = smp
    x = imgs.detach().clone().requires_grad_(True)
    prob = m(x, proj, dv)[0]
    return x, prob, (prob * R).sum()


def _grads(m, x=None) -> dict:
    out = {"grad:" + k: None if p.grad is None else p.grad.detach().clone()
           for k, p in msc.sweep_params(m).items()}
    if x is not None:
        out["imgs.grad"] = None if x.grad is None else x.grad.clone()
    return out


@pytest.mark.parametrize("forward_between", [False, True])
@pytest.mark.parametrize("planes,ckpt", CKPT)
def test_backward_after_a_weight_change_uses_its_forwards_weights(planes, ckpt, forward_between):
    """forward, in-place change under no_grad (and, ``forward_between``, another forward of the
    model on the new weights), backward of the old graph: the gradients of the same forward and
    backward with no change in between, bit for bit."""
    smp = msc.sample(DEV, D=planes)
    ref = _model(planes, checkpoint_planes=ckpt)
    x, _, loss = _forward(ref, smp)
    loss.backward()
    want = _grads(ref, x)
    m = _model(planes, checkpoint_planes=ckpt)
    x, _, loss = _forward(m, smp)
    msc.scale_weights(m, 1.25)
    if forward_between:
        assert _differs(msc.infer(m, smp)["cost"], msc.infer(ref, smp)["cost"])
    loss.backward()
    msc.same_bits(_grads(m, x), want, "backward after a weight change")


@pytest.mark.parametrize("planes,ckpt,batches", [(D, 0, (1, 1)), (msc.CKPT_D, msc.CKPT_S, (1, 1)),
                                                 (D, 0, (1, 2)), (msc.CKPT_D, msc.CKPT_S, (1, 2))])
def test_two_forwards_one_backward_adds_the_two_gradients(planes, ckpt, batches):
    """(La + Lb).backward() over two samples: ga + gb of the separate runs (two-term addition is
    exact in either order).  Batches (1, 2): the second forward evicts the first's workspace
    before either backward runs."""
    sa = msc.sample(DEV, B=batches[0], D=planes, seed=5, rseed=3)
    sb = msc.sample(DEV, B=batches[1], D=planes, seed=6, rseed=4)
    m = _model(planes, checkpoint_planes=ckpt)
    sep = []
    for smp in (sa, sb):
        for p in m.parameters():
            p.grad = None
        x, _, loss = _forward(m, smp)
        loss.backward()
        sep.append(_grads(m, x))
    for p in m.parameters():
        p.grad = None
    xa, _, la = _forward(m, sa)
    xb, _, lb = _forward(m, sb)
    (la + lb).backward()
    got = _grads(m)
    want = {k: sep[0][k] + sep[1][k] for k in got}
    msc.same_bits(got, want, "two forwards, one backward")
    assert torch.equal(xa.grad, sep[0]["imgs.grad"]) and torch.equal(xb.grad, sep[1]["imgs.grad"])
    # accumulation: two backward calls without zero_grad leave ga + gb as well
    for p in m.parameters():
        p.grad = None
    _forward(m, sa)[2].backward()
    _forward(m, sb)[2].backward()
    msc.same_bits(_grads(m), want, "two backward calls without zero_grad")


@pytest.mark.parametrize("frozen", ["omega.", "cost_regularization.", ""])
def test_frozen_parameters_get_no_gradient_and_change_no_other(frozen, s):
    """``frozen``: the prefix of the sweep tensors with requires_grad False ("" freezes them all:
    only imgs.requires_grad remains)."""
    want = msc.train(_model(), s)
    m = _model()
    for k, p in msc.sweep_params(m).items():
        if k.startswith(frozen):
            p.requires_grad_(False)
    got = msc.train(m, s)
    for k in msc.SWEEP_KEYS:
        if k.startswith(frozen):
            assert got.pop("grad:" + k) is None, k
            want.pop("grad:" + k)
    assert len(want) > 2 or frozen == ""
    msc.same_bits(got, want, f"frozen {frozen!r}")


# ---------------------------------------------------------------------------------------
# 4. three steps of SGD against float64
# ---------------------------------------------------------------------------------------
def test_three_sgd_steps_follow_the_float64_trajectory():
    """Plain SGD (lr 1e-2, no momentum), three steps on L = sum(R * softmax(cost)), scene seed 5,
    sweep_weights(2), R seed 3.  At each step, per tensor: rel_l2(theta_k - theta_0, float64's)
    <= test_gpu_bptt.bound(name, float32's own error over F32_THREADS); conv_0.bias (true
    gradient 0): max |displacement| <= 2 x float32's + 1e-6; the loss: |L - L64| <=
    max(1e-5 sum|R|, 2 |L32 - L64|).  A stale trajectory misses every tensor's bound at step 3 by
    237x or more (tests/test_module_state_cases.py)."""
    smp = msc.sample(DEV, seed=5, rseed=3)
    m = _model(wseed=msc.WSEED)
    theta0 = {k: p.detach().double().cpu() for k, p in msc.sweep_params(m).items()}
    P0 = msc.trajectory_inputs()[3]
    for k in msc.SWEEP_KEYS:   # the model's sweep tensors are the oracle's theta_0
        assert torch.equal(theta0[k], P0[k].double()), k
    ref = msc.trajectory_reference()
    bad = []
    for step in range(msc.TRAJ_STEPS):
        for p in m.parameters():
            p.grad = None
        _, prob, loss = _forward(m, smp)
        loss.backward()
        loss = float((prob.detach().double() * smp[3].double()).sum())   # (summed as the oracle's)
        ps = msc.sweep_params(m)
        new = msc.sgd_step({k: p.detach() for k, p in ps.items()}, {k: p.grad for k, p in ps.items()})
        with torch.no_grad():
            for k, p in ps.items():
                p.copy_(new[k])
        disp = {k: (p.detach().double().cpu() - theta0[k]).numpy() for k, p in ps.items()}
        worst = max(msc.rel_l2(disp[k], ref["f64"][step][1][k]) for k in msc.SWEEP_KEYS if k != msc.BIAS)
        print(f"step {step + 1}: loss {loss:.6f} (float64 {ref['f64'][step][0]:.6f}), worst displacement "
              f"rel_l2 {worst:.3e} (float32's {max(v for k, v in ref['e32'][step].items() if k != msc.BIAS):.3e})")
        bad += msc.trajectory_misses(step, disp, loss)
    assert not bad, bad
