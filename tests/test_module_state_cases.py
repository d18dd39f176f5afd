"""The module-state cases without a device (tests/module_state_cases.py): each case of
tests/test_gpu_module_state.py reaches the regime it is there for.

* Which parameter changes a (data_ptr, _version) key would have seen, tabulated on CPU
  parameters: exactly the ``.data`` in-place cases and the write through an aliased vector leave
  both unchanged -- and every case changes values, so the forward after it must differ.  (The
  fused Adam is tabulated and printed but not asserted either way: torch 2.10's CPU
  implementation bumps no version counter, other builds' and the device's may.)
* Copies drop the sweep cache (no device needed: a stand-in object that cannot be copied).
* The trajectory check is honest: the stale trajectory (every step on theta_0's gradient, what a
  model that never repacked would give) misses every checked tensor's bound at step 3 by at
  least 10x, and the float32 oracle passes its own check.
"""
import numpy as np
import pytest
import torch

import module_state_cases as msc


def test_case_list_is_complete():
    assert set(msc.CASE_NAMES) == set(msc._cases()) and len(set(msc.CASE_NAMES)) == len(msc.CASE_NAMES)
    from aarmvs import ops
    assert msc.SWEEP_KEYS == ops.SWEEP_KEYS
    assert sum(n.startswith("one_element:") for n in msc.CASE_NAMES) == len(ops.SWEEP_KEYS)
    assert msc.UNSEEN_BY_A_KEY < set(msc.CASE_NAMES)


@pytest.mark.parametrize("name", msc.CASE_NAMES)
def test_case_changes_values_and_is_seen_by_a_key_or_not(name):
    t = msc.tabulate(name)
    print(name, "version", t["version"], "pointer", t["pointer"], "changed", len(t["values"]))
    assert t["values"], "the case changes no sweep tensor"
    seen = t["version"] or t["pointer"]
    if name not in msc.KEY_DEPENDS_ON_TORCH:
        assert seen == (name not in msc.UNSEEN_BY_A_KEY)
    if name.startswith("one_element:"):
        assert t["values"] == [name.split(":", 1)[1]]
    else:
        assert t["values"] == list(msc.SWEEP_KEYS)


def test_one_element_moves_by_an_eighth_of_the_tensors_scale():
    _, _, H, W, D = msc.FRAME
    for key in msc.SWEEP_KEYS:
        m = msc.build(D, H, W, "cpu", evidential=False)
        old = msc.sweep_params(m)[key].detach().clone()
        msc.case("one_element:" + key).apply(m, None, "cpu")
        diff = (msc.sweep_params(m)[key].detach() - old).abs()
        assert int((diff != 0).sum()) == 1
        assert float(diff.max()) == pytest.approx(float(old.abs().max()) / 8, rel=1e-5)


def test_every_one_element_change_reaches_the_float64_cost_volume():
    """The GPU test asserts that the cost volume differs after each change.  That holds only if
    the element matters: in the float64 oracle each chosen element moves the cost volume by at
    least 1e-5 of its largest value, 80 times float32's resolution of that value."""
    P = msc.trajectory_inputs()[3]
    c0 = msc.oracle_cost(P)
    scale = float(c0.abs().max())
    reach = {}
    for key in msc.SWEEP_KEYS:
        assert 0 <= msc.one_element_index(key) < P[key].numel()
        reach[key] = float((msc.oracle_cost({**P, key: msc.one_element_moved(P[key], key)}) - c0).abs().max()) / scale
    print("smallest reach:", min(reach, key=reach.get), f"{min(reach.values()):.3e}")
    assert all(v >= 1e-5 for v in reach.values()), {k: v for k, v in reach.items() if v < 1e-5}


def test_fresh_twin_has_the_same_arguments_and_state():
    _, _, H, W, _ = msc.FRAME
    m = msc.build(msc.CKPT_D, H, W, "cpu", checkpoint_planes=msc.CKPT_S, return_cost=True)
    t = msc.fresh(m, "cpu")
    assert t.ctor_args == m.ctor_args and t.ctor_args is not m.ctor_args and t is not m
    assert t.checkpoint_planes == msc.CKPT_S and t.return_cost and isinstance(t.feature, torch.nn.Identity)
    sd, st = m.state_dict(), t.state_dict()
    assert list(sd) == list(st)
    for k in sd:
        assert torch.equal(sd[k], st[k]) and sd[k].data_ptr() != st[k].data_ptr()


class _Uncopyable:
    """Stands for a DepthSweep: neither copy nor pickle can take it (as a stream handle)."""

    def __reduce_ex__(self, protocol):
        raise TypeError("a sweep object must not be copied")


@pytest.mark.parametrize("how", list(msc.COPIES))
def test_copies_drop_the_sweep_cache(how):
    _, _, H, W, D = msc.FRAME
    m = msc.build(D, H, W, "cpu", evidential=False)
    cache = (torch.device("cpu"), _Uncopyable())
    m._sweep_cache = cache
    keys = list(m.state_dict())
    c = msc.COPIES[how](m)
    assert c._sweep_cache is None and m._sweep_cache is cache
    assert list(c.state_dict()) == keys == list(m.state_dict())
    for (k, a), b in zip(msc.sweep_params(m).items(), msc.sweep_params(c).values()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), k


def test_trajectory_guard_the_stale_trajectory_misses_every_bound_tenfold():
    from test_gpu_bptt import bound
    ref = msc.trajectory_reference()
    last = msc.TRAJ_STEPS - 1
    worst32 = max(v for k, v in ref["e32"][last].items() if k != msc.BIAS)
    margins = {}
    for name in msc.SWEEP_KEYS:
        if name == msc.BIAS:
            continue
        e = msc.rel_l2(ref["stale"][last][1][name], ref["f64"][last][1][name])
        margins[name] = e / bound(name, ref["e32"][last][name])
    print(f"float32's worst displacement error at step {last + 1}: {worst32:.3e}; "
          f"the stale trajectory's smallest margin: {min(margins.values()):.1f}x")
    assert all(v >= 10.0 for v in margins.values()), {k: v for k, v in margins.items() if v < 10.0}
    assert len(msc.trajectory_misses(last, ref["stale"][last][1], None)) == len(msc.SWEEP_KEYS) - 1
    # step 1 is the same for both (one gradient at theta_0): the check must not fire there
    assert msc.trajectory_misses(0, ref["stale"][0][1], ref["stale"][0][0]) == []


def test_trajectory_check_passes_the_float64_trajectory_itself():
    ref = msc.trajectory_reference()
    for k, (loss, disp) in enumerate(ref["f64"]):
        assert msc.trajectory_misses(k, disp, loss) == []
    assert ref["sum_abs_R"] > 0 and all(np.isfinite(l) for l, _ in ref["f64"])
