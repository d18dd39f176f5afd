"""Cases, builders and CPU references of the module-state tests (tests/test_gpu_module_state.py,
tests/test_module_state_cases.py): EMVSNet over time -- parameter updates between two calls of
one model, copies of a model that has run, autograd graphs that outlive a weight change, and a
three-step SGD trajectory against float64.

The oracle of everything but the trajectory is the fresh twin: the sweep is bit-reproducible
across objects and processes, so a model that has a history must give, bit for
bit, what a new model loaded with its current state_dict gives (``fresh``, ``observe``,
``same_bits``).

A case of §1 is a ``Case(prepare, apply)``: ``prepare(m)`` runs before the warm-up forwards
(only the aliased vector needs it: the aliasing itself moves every data pointer, the write
through the alias afterwards moves nothing), ``apply(m, state, dev)`` is the change between the
warm-up and the forward under test.  Both work on CPU parameters too, where
``tabulate`` records what a (data_ptr, _version) key would have seen of the change.
"""
from __future__ import annotations

import copy
import functools
import io
import pickle
from collections import namedtuple

import numpy as np

from aarmvs import synthetic as syn

SWEEP_KEYS = tuple(syn.SWEEP_SHAPES)
FRAME = (1, 3, 16, 24, 4)        # B, N, H, W, D
CKPT_D, CKPT_S = 20, 16          # checkpoint_planes=16 over D=20: segments of 16 and 4 planes
WSEED = 2

Case = namedtuple("Case", "prepare apply")


# ---------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------
def _make(args: dict):
    import torch.nn as nn
    from models import EMVSNet
    m = EMVSNet(**args)
    m.ctor_args = dict(args)   # (a plain attribute: copies carry it along)
    return m, nn.Identity()


def build(D, H, W, dev, wseed=WSEED, **kw):
    """The sweep-only model of tests/test_gpu_training.py::_model (feature = nn.Identity(), so the
    images are the 32-channel features and MIOpen is not in the path)."""
    import torch
    m, identity = _make(dict(disparity_level=D, image_scale=1.0, max_h=H, max_w=W, **kw))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    wts = syn.init_weights(shapes, seed=wseed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()}, strict=True)
    m.feature = identity
    return m.to(dev)


def fresh(m, dev):
    """The fresh twin: a new EMVSNet with the same constructor arguments and feature replacement,
    loaded with a clone of ``m.state_dict()``, on ``dev``.  It has no history."""
    t, identity = _make(m.ctor_args)
    t.feature = identity
    t.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    return t.to(dev)


def sweep_params(m) -> dict:
    from models.drmvsnet import _sweep_params
    return dict(zip(SWEEP_KEYS, _sweep_params(m)))


def sample(dev, B=FRAME[0], D=FRAME[4], seed=5, rseed=3):
    """(imgs [B,N,32,H,W], proj [B,N,4,4], depth_values [B,D], R [B,D,H,W]) on ``dev``."""
    import torch
    _, N, H, W, _ = FRAME
    sc = syn.scene(B, N, H, W, D, seed=seed)
    imgs = torch.from_numpy(np.moveaxis(sc["features"], 0, 1).copy())
    R = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(rseed))
    return tuple(t.to(dev) for t in (imgs, torch.from_numpy(sc["proj_matrices"]),
                                     torch.from_numpy(sc["depth_values"]), R))


# ---------------------------------------------------------------------------------------
# what a model computes: every output the twin is compared on
# ---------------------------------------------------------------------------------------
def infer(m, s) -> dict:
    """The inference outputs (return_depth=True, no_grad) and the raw cost volume
    (return_cost=True) of ``m`` on sample ``s``; the model's flags are put back."""
    import torch
    imgs, proj, dv, _ = s
    flags = (m.return_depth, m.return_cost)
    out = {}
    try:
        with torch.no_grad():
            m.return_depth, m.return_cost = True, False
            res = m(imgs, proj, dv)
            out["depth"], out["conf"] = res["depth"].clone(), res["photometric_confidence"].clone()
            m.return_depth, m.return_cost = False, True
            out["cost"] = m(imgs, proj, dv)[0].clone()
    finally:
        m.return_depth, m.return_cost = flags
    return out


def train(m, s, zero=True) -> dict:
    """One training forward and the backward of sum(prob * R): prob, d/d imgs and the gradient of
    every sweep tensor (None where autograd left none).  ``zero``: drop the gradients first."""
    imgs, proj, dv, R = s
    if zero:
        for p in m.parameters():
            p.grad = None
    x = imgs.detach().clone().requires_grad_(True)
    prob = m(x, proj, dv)[0]
    (prob * R).sum().backward()
    out = {"prob": prob.detach().clone(), "imgs.grad": None if x.grad is None else x.grad.clone()}
    for k, p in sweep_params(m).items():
        out["grad:" + k] = None if p.grad is None else p.grad.detach().clone()
    return out


def observe(m, s) -> dict:
    return {**infer(m, s), **train(m, s)}


def same_bits(got: dict, want: dict, what: str) -> None:
    """torch.equal on every entry (None must meet None)."""
    import torch
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    bad = []
    for k, w in want.items():
        g = got[k]
        if (g is None) != (w is None):
            bad.append(f"{k} (None on one side)")
        elif w is not None and not torch.equal(g, w):
            n = int((g != w).sum()) if g.shape == w.shape else -1
            bad.append(f"{k} ({n} of {w.numel()} elements differ)")
    assert not bad, f"{what}: not bit-equal: {bad}"


# ---------------------------------------------------------------------------------------
# §1: parameter changes between two calls
# ---------------------------------------------------------------------------------------
def new_value(p, key: str):
    """A new value for a sweep tensor: a fixed function of the old one and the key, clearly
    different (a quarter of its scale), on the tensor's device and dtype."""
    import torch
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    old = p.detach().cpu().double()
    scale = float(old.abs().max())
    return (old + 0.25 * scale * torch.randn(old.shape, generator=g, dtype=torch.float64)).to(p.device, p.dtype)


def seed_grads(m) -> None:
    """Gradients for the optimiser cases where no backward has run (the CPU tabulation)."""
    for k, p in sweep_params(m).items():
        if p.grad is None:
            p.grad = (new_value(p, "grad:" + k) - p.detach())


def _optimizer(cls, **kw):
    def apply(m, state, dev):
        opt = cls(list(sweep_params(m).values()), lr=1e-2, **kw)
        opt.step()
    return apply


def _load_state_dict(assign: bool):
    def apply(m, state, dev):
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for k, p in sweep_params(m).items():
            sd[k] = new_value(p, k)
        m.load_state_dict(sd, strict=True, assign=assign)
    return apply


def _each(fn, no_grad: bool):
    def apply(m, state, dev):
        import torch
        with torch.no_grad() if no_grad else torch.enable_grad():
            for k, p in sweep_params(m).items():
                fn(p, k)
    return apply


def _setattr_parameter(m, state, dev):
    import torch.nn as nn
    for k, p in sweep_params(m).items():
        *path, leaf = k.split(".")
        mod = m
        for part in path:
            mod = getattr(mod, part)
        setattr(mod, leaf, nn.Parameter(new_value(p, k)))


def _alias_prepare(m):
    from torch.nn.utils import parameters_to_vector, vector_to_parameters
    ps = list(sweep_params(m).values())
    vec = parameters_to_vector(ps).detach().clone()
    vector_to_parameters(vec, ps)   # every parameter is now a view of vec (same values)
    return vec


def _dtype_round_trip(m, state, dev):
    import torch
    m.to(torch.float64)
    with torch.no_grad():
        for p in sweep_params(m).values():
            p.mul_(1.25)
    m.to(torch.float32)


def _cpu_round_trip(m, state, dev):
    import torch
    m.cpu()
    with torch.no_grad():
        for p in sweep_params(m).values():
            p.mul_(1.25)
    m.to(dev)


# The element a one-element case moves: the middle one, except where that one cannot reach the
# cost volume at this frame and these weights -- channels 0, 1 and 8 of deconv_0's output are
# negative before the ReLU at every pixel and plane, so their GroupNorm affine and cell 3's
# weights on them have exactly no effect, in the float64 oracle too.  There: channel 3 (cell 3:
# output channel 32, input channel 3, the centre tap).  tests/test_module_state_cases.py checks
# every choice against the float64 oracle.
ONE_ELEMENT = {"cost_regularization.deconv_0.gn.weight": 3, "cost_regularization.deconv_0.gn.bias": 3,
               "cost_regularization.cell_list.3.conv.weight": (32 * 48 + 3) * 9 + 4}


def one_element_index(key: str) -> int:
    return ONE_ELEMENT.get(key, int(np.prod(syn.SWEEP_SHAPES[key])) // 2)


def one_element_moved(p, key: str):
    """``p`` with its chosen element moved by 1/8 of the tensor's max |value| (a new tensor)."""
    q = p.detach().clone()
    q.view(-1)[one_element_index(key)] += float(q.abs().max()) / 8
    return q


def _one_element(key: str):
    def apply(m, state, dev):
        import torch
        p = sweep_params(m)[key]
        with torch.no_grad():
            p.view(-1)[one_element_index(key)] += float(p.detach().abs().max()) / 8
    return apply


def oracle_cost(P: dict):
    """The float64 oracle's cost volume [B,D,H,W] of the trajectory's scene on parameters P."""
    from oracle import sweep_oracle as orc
    feats, proj, dv, _, _ = trajectory_inputs()
    f = feats.double()
    return orc.sweep(f[0], list(f[1:]), proj[:, 0], list(proj[:, 1:].unbind(1)), dv,
                     {k: v.double() for k, v in P.items()})["cost"]


def _cases() -> dict:
    import torch
    none = lambda m: None   # noqa: E731
    c = {
        "sgd_step": Case(none, _optimizer(torch.optim.SGD)),
        "adam_step": Case(none, _optimizer(torch.optim.Adam)),
        "adam_fused_step": Case(none, _optimizer(torch.optim.Adam, fused=True)),
        "load_state_dict": Case(none, _load_state_dict(False)),
        "load_state_dict_assign": Case(none, _load_state_dict(True)),
        "no_grad_copy_": Case(none, _each(lambda p, k: p.copy_(new_value(p, k)), True)),
        "no_grad_mul_": Case(none, _each(lambda p, k: p.mul_(1.25), True)),
        "data_mul_": Case(none, _each(lambda p, k: p.data.mul_(1.25), False)),
        "data_copy_": Case(none, _each(lambda p, k: p.data.copy_(new_value(p, k)), False)),
        "data_assign": Case(none, _each(lambda p, k: setattr(p, "data", new_value(p, k)), False)),
        "aliased_vector_mul_": Case(_alias_prepare, lambda m, vec, dev: vec.mul_(1.25)),
        "setattr_parameter": Case(none, _setattr_parameter),
        "dtype_round_trip": Case(none, _dtype_round_trip),
        "cpu_round_trip": Case(none, _cpu_round_trip),
    }
    for k in SWEEP_KEYS:
        c["one_element:" + k] = Case(none, _one_element(k))
    return c


CASE_NAMES = ("sgd_step", "adam_step", "adam_fused_step", "load_state_dict", "load_state_dict_assign",
              "no_grad_copy_", "no_grad_mul_", "data_mul_", "data_copy_", "data_assign",
              "aliased_vector_mul_", "setattr_parameter", "dtype_round_trip", "cpu_round_trip"
              ) + tuple("one_element:" + k for k in SWEEP_KEYS)
# the changes that neither bump a version counter nor move a data pointer
UNSEEN_BY_A_KEY = {"data_mul_", "data_copy_", "aliased_vector_mul_"}
# whether a key sees it is the torch build's choice (the fused kernels write through tensor lists)
KEY_DEPENDS_ON_TORCH = {"adam_fused_step"}


def case(name: str) -> Case:
    return _cases()[name]


def tabulate(name: str) -> dict:
    """The case on CPU parameters: {'version': a sweep tensor's _version changed, 'pointer': a
    data_ptr() changed, 'values': the names of the sweep tensors whose values changed}."""
    import torch
    _, _, H, W, D = FRAME
    m = build(D, H, W, "cpu", evidential=False)
    seed_grads(m)
    c = case(name)
    state = c.prepare(m)
    before = {k: (p._version, p.data_ptr(), p.detach().clone()) for k, p in sweep_params(m).items()}
    c.apply(m, state, "cpu")
    after = sweep_params(m)
    return {"version": any(after[k]._version != v for k, (v, _, _) in before.items()),
            "pointer": any(after[k].data_ptr() != q for k, (_, q, _) in before.items()),
            "values": [k for k, (_, _, old) in before.items()
                       if after[k].dtype != old.dtype or not torch.equal(after[k].detach(), old)]}


# ---------------------------------------------------------------------------------------
# §2: copies
# ---------------------------------------------------------------------------------------
def _pickle_round_trip(m):
    return pickle.loads(pickle.dumps(m))


def _torch_save_load(m):
    import torch
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _averaged(m):
    from torch.optim.swa_utils import AveragedModel
    return AveragedModel(m).module


COPIES = {"deepcopy": copy.deepcopy, "pickle": _pickle_round_trip, "torch_save": _torch_save_load,
          "averaged_model": _averaged}
STATES = ("new", "after_inference", "after_training")


def scale_weights(m, factor: float) -> None:
    import torch
    with torch.no_grad():
        for p in sweep_params(m).values():
            p.mul_(factor)


# ---------------------------------------------------------------------------------------
# §4: the three-step SGD trajectory on the CPU oracle
# ---------------------------------------------------------------------------------------
TRAJ_STEPS, TRAJ_LR = 3, 1e-2
BIAS = "cost_regularization.conv_0.bias"   # true gradient 0 (softmax over D)


def rel_l2(a, ref) -> float:
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))


def trajectory_inputs():
    """(features [N,B,C,H,W], proj, depth_values, {sweep tensor: value}, R), CPU float32."""
    import torch
    B, N, H, W, D = FRAME
    sc = syn.scene(B, N, H, W, D, seed=5)
    P = {k: torch.from_numpy(v) for k, v in syn.sweep_weights(WSEED).items()}
    R = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(3))
    return (torch.from_numpy(sc["features"]), torch.from_numpy(sc["proj_matrices"]),
            torch.from_numpy(sc["depth_values"]), P, R)


def sgd_step(theta: dict, grads: dict, lr: float = TRAJ_LR) -> dict:
    """The hand-written SGD of every trajectory, the device's included: theta - lr * g in the
    tensors' own precision."""
    return {k: theta[k] - lr * grads[k] for k in theta}


def _oracle_trajectory(dtype, stale=False):
    """[(loss, {name: theta_k - theta_0 as float64})] for k = 1..TRAJ_STEPS.  ``stale``: every
    step takes the gradient at theta_0 (what a model that never repacked would train on)."""
    from test_gpu_bptt import _oracle_grads
    feats, proj, dv, P0, R = trajectory_inputs()
    theta0 = {k: v.to(dtype) for k, v in P0.items()}
    theta, out = theta0, []
    for _ in range(TRAJ_STEPS):
        prob, _, gp, _ = _oracle_grads(feats, proj, dv, theta0 if stale else theta, R, dtype)
        loss = float((prob.double() * R.double()).sum())
        theta = sgd_step(theta, gp)
        out.append((loss, {k: (theta[k].double() - theta0[k].double()).numpy() for k in theta}))
    return out


@functools.lru_cache(maxsize=None)
def trajectory_reference() -> dict:
    """{'f64': the float64 trajectory, 'stale': the stale one (float64), 'e32': per step {name:
    max over F32_THREADS of float32's rel_l2 displacement error}, 'bias32': per step float32's
    max |conv_0.bias displacement|, 'loss32': per step float32's max |L32 - L64|, 'sum_abs_R'}.
    Computed once and shared; callers do not modify it."""
    import torch
    from test_gpu_bptt import F32_THREADS
    f64 = _oracle_trajectory(torch.float64)
    e32 = [dict() for _ in range(TRAJ_STEPS)]
    bias32, loss32 = [0.0] * TRAJ_STEPS, [0.0] * TRAJ_STEPS
    prev = torch.get_num_threads()
    try:
        for n in F32_THREADS:
            torch.set_num_threads(n)
            for k, (loss, disp) in enumerate(_oracle_trajectory(torch.float32)):
                for name, d in disp.items():
                    e32[k][name] = max(e32[k].get(name, 0.0), rel_l2(d, f64[k][1][name]))
                bias32[k] = max(bias32[k], float(np.abs(disp[BIAS]).max()))
                loss32[k] = max(loss32[k], abs(loss - f64[k][0]))
    finally:
        torch.set_num_threads(prev)
    R = trajectory_inputs()[4]
    return {"f64": f64, "stale": _oracle_trajectory(torch.float64, stale=True), "e32": e32,
            "bias32": bias32, "loss32": loss32, "sum_abs_R": float(R.double().abs().sum())}


def trajectory_misses(step: int, disp: dict, loss) -> list:
    """The checks of §4 on a trajectory's step (0-based): [(what, value, limit)] of those missed.
    Every tensor but conv_0.bias: rel_l2 of the displacement against float64's <=
    test_gpu_bptt.bound(name, float32's own error); conv_0.bias: max |displacement| <= 2 x
    float32's + 1e-6; the loss (None: not checked): |L - L64| <= max(1e-5 sum|R|, 2 |L32 - L64|)."""
    from test_gpu_bptt import bound
    ref = trajectory_reference()
    bad = []
    for name in SWEEP_KEYS:
        if name == BIAS:
            v, lim = float(np.abs(disp[name]).max()), 2.0 * ref["bias32"][step] + 1e-6
        else:
            v, lim = rel_l2(disp[name], ref["f64"][step][1][name]), bound(name, ref["e32"][step][name])
        if not v <= lim:
            bad.append((f"step {step + 1} {name}", v, lim))
    if loss is not None:
        v = abs(loss - ref["f64"][step][0])
        lim = max(1e-5 * ref["sum_abs_R"], 2.0 * ref["loss32"][step])
        if not v <= lim:
            bad.append((f"step {step + 1} loss", v, lim))
    return bad
