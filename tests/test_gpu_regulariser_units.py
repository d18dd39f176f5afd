"""GPU tests of the regulariser's units against float64 on the GPU's own inputs
(tests/regulariser_unit_cases.py: the units, the frames, the injected states, the bounds).

Inference path (aarmvs_unet_step_p, the pooled cell kinds 5/6/7 -- the library's default): the
injected h- and c- are written into the workspace through DepthSweep.state(..., planes=k, cell,
which) and one step k is run.  csrc/convlstm.hip unet_io_ws: step k reads h- from ring slot
k % r (what state(planes=k) returns) and writes slot (k + 1) % r (state(planes=k + 1)); c has one
buffer per cell, updated in place, so c- is read back before the step and c after it from the same
view.  The slot of the step before (planes=k - 1) is filled with other values ('stale'), so a cell
reading the wrong slot sees plausible numbers, not zeros.  Every unit is then recomputed in float64
from the tensors read back: |got - ref64| <= 2e-5 max(1, max|ref64|) per tensor.

fp16 mode: the reference is the float64 unit with tests/fp16_mode_ref.py's operand rounding
(round11 on the operands of the seven convs; fp16_operands() itself patches float32-only
functions), the bound test_gpu_fp16_mode.py's per-step one: rms(got - emulation) <= 0.1 E_rms, E_rms
= rms(emulation - float64 unit).  The head conv is not one of the seven (E_rms = 0): it keeps the
split bound.

Training path: a segment record of planes 1 and 2 (record_d0 = 1) from an injected state in slab
0; every record tensor of both planes against its float64 unit, the statistics (fp64 sums of fp32
values) within 1e-6 relative.

Each case prints every tensor's error with the float32 CPU evaluation's beside it, then one line:
the case, the worst tensor, its pixel, its error and float32's (profiles/regulariser_unit_errors.txt
holds a run).  No bound comes from the library.  The split-precision and training tests also put each
planted fault of the case's frame into the reference built from the GPU's tensors and assert that
the GPU's result then lies outside the bound: the comparison would have caught that fault.
"""
import functools
import os

import pytest
import torch

from aarmvs import synthetic as syn

import regulariser_unit_cases as ruc

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [c.id for c in ruc.CASES]
MS_FRAME = (1, 36, 68)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


@functools.lru_cache(maxsize=None)
def sweeper(kind):
    from aarmvs import ops
    return ops.DepthSweep({n: v.to(DEV) for n, v in ruc.weights(kind).items()}, DEV)


def _step(case, precision="split"):
    """Injects the case's state, runs step k, reads everything back -> the float32 CPU tensors in
    infer_units' form ('x', 'hp', 'cp', 'stale', 'h') and the GPU's outputs by name."""
    B, H, W = case.frame
    k = case.k
    t = ruc.inputs(case.frame, case.sset)
    sw = sweeper(case.wkind)
    st = lambda planes, cell, which: sw.state(B, H, W, 1, planes, cell, which)   # noqa: E731
    for cell in range(5):
        st(k - 1, cell, 0).copy_(t["stale"][cell])
        st(k, cell, 0).copy_(t["hp"][cell])
        st(k, cell, 1).copy_(t["cp"][cell])
    back = {"x": t["x"], "stale": t["stale"],
            "hp": [st(k, cell, 0).cpu().contiguous() for cell in range(5)],
            "cp": [st(k, cell, 1).cpu().contiguous() for cell in range(5)]}
    for cell in range(5):   # the views are writable slices of the workspace
        assert torch.equal(back["hp"][cell], t["hp"][cell]) and torch.equal(back["cp"][cell], t["cp"][cell])
    sw.precision = precision
    try:
        cost = sw.unet_step(t["x"].to(DEV), k)
        torch.cuda.synchronize()
    finally:
        sw.precision = "split"
    got = {"cost": cost.cpu()}
    for cell in range(5):
        got[f"h{cell}"] = st(k + 1, cell, 0).cpu().contiguous()
        got[f"c{cell}"] = st(k + 1, cell, 1).cpu().contiguous()
    back["h"] = [got[f"h{cell}"] for cell in range(5)]
    return back, got


def _report(tag, rows):
    """rows: (ratio, name, idx, err, err32).  Prints the worst, returns the tensors over the bound."""
    r, name, idx, err, e32 = max(rows)
    print(f"[{tag}] worst {name} at {idx}: |gpu - f64| {err:.3e} = {r:.3f} of the bound; float32 CPU {e32:.3e}")
    return [(n, i, e, rr) for rr, n, i, e, _ in rows if rr > 1.0]


def _planted_faults_fail(case, P64, t64, got, units, training):
    """Every planted fault of the frame, put into the reference of the GPU's own tensors, puts the
    GPU's result outside the bound in the unit it targets: the comparison would have caught it."""
    with torch.no_grad():
        for fault in ruc.applicable(case.frame):
            bad = units(P64, t64, case.frame, fault=fault)
            m = max(ruc.worst(n, got[n], bad[n])[0] for n in ruc.fault_target(fault, training))
            assert m > 1.0, (fault, m)


def _check_split(case, tag, faults=False):
    back, got = _step(case)
    P64, P32 = ruc.weights(case.wkind, torch.float64), ruc.weights(case.wkind, torch.float32)
    with torch.no_grad():
        ref64 = ruc.infer_units(P64, ruc.to_dtype(back, torch.float64), case.frame, oracle=True)
        ref32 = ruc.infer_units(P32, back, case.frame, oracle=True)
    if faults:
        _planted_faults_fail(case, P64, ruc.to_dtype(back, torch.float64), got, ruc.infer_units, False)
    rows = []
    for unit, names in ruc.INFER_UNITS.items():
        for n in names:
            assert torch.isfinite(got[n]).all(), (unit, n)
            r, idx, err = ruc.worst(n, got[n], ref64[n])
            rows.append((r, f"{unit}:{n}", idx, err, float((ref32[n].double() - ref64[n]).abs().max())))
    print()
    for r, n, idx, err, e32 in rows:
        print(f"  [{tag}] {n:8s} {err:.3e} ({r:.3f} of the bound)  float32 CPU {e32:.3e}")
    bad = _report(tag, rows)
    assert not bad, bad


@pytest.mark.parametrize("cid", IDS)
def test_inference_units_match_float64(cid):
    """All six units of one step, split precision, pooled cell kinds, on every frame, state set and
    weight set, at a step index that wraps some cell's ring; and each planted fault, put into the
    reference, would have failed the comparison."""
    _check_split(ruc.BY_ID[cid], cid, faults=True)


@pytest.mark.parametrize("ms", ["0", "1", "2"])
@pytest.mark.parametrize("sset", ruc.STATE_SETS)
def test_inference_units_match_float64_in_every_cell_shape(monkeypatch, sset, ms):
    """AARMVS_CELL_MS = 0, 1, 2 (convlstm.hip cell_shape) on 36x68, each against the reference --
    a fault common to the three tile shapes passes their bit-identity tests."""
    case = next(c for c in ruc.CASES if c.frame == MS_FRAME and c.sset == sset)
    monkeypatch.setenv("AARMVS_CELL_MS", ms)
    _check_split(case, f"{case.id} MS={ms}")


@pytest.mark.parametrize("cid", [c.id for c in ruc.CASES if c.sset == "plain"])
def test_inference_units_fp16_mode_match_the_emulation(cid):
    """The 1-product mode per unit: against the float64 unit with the operands of its convs rounded
    to 11 bits, within 0.1 E_rms (see the module docstring); the head within the split bound."""
    case = ruc.BY_ID[cid]
    back, got = _step(case, "fp16")
    P64 = ruc.weights(case.wkind, torch.float64)
    t64 = ruc.to_dtype(back, torch.float64)
    with torch.no_grad():
        ref64 = ruc.infer_units(P64, t64, case.frame, oracle=True)
        emu = ruc.infer_units(P64, t64, case.frame, rnd=ruc.round_operand)
    bad, rows = [], []
    for unit, names in ruc.INFER_UNITS.items():
        for n in names:
            assert torch.isfinite(got[n]).all(), (unit, n)
            if unit == "head":
                r, idx, err = ruc.worst(n, got[n], ref64[n])
                rows.append((r, f"{unit}:{n}", err, 0.0))
                continue
            E_rms = ruc.fref.rms(emu[n] - ref64[n])
            d = ruc.fref.rms(got[n].double() - emu[n])
            assert E_rms > 0
            rows.append((d / (0.1 * E_rms), f"{unit}:{n}", d, E_rms))
    print()
    for r, n, d, E in rows:
        print(f"  [{cid} fp16] {n:8s} gpu - emulation {d:.3e} ({r:.3f} of the bound), E_rms {E:.3e}")
        if r > 1.0:
            bad.append((n, d, E))
    r, n, d, E = max(rows)
    print(f"[{cid} fp16] worst {n}: {d:.3e} = {r:.3f} of the bound (E_rms {E:.3e})")
    assert not bad, bad


@pytest.mark.parametrize("cid", IDS)
def test_training_record_units_match_float64(cid):
    """A segment-record sweep over planes 1 and 2 (the training cell kinds 0-2 with SRC_POOL, the
    PRECISE gates, z_out) from the injected state: every record tensor of both planes, and
    cost_out, against its float64 unit on the record's own tensors."""
    from aarmvs import _lib
    case = ruc.BY_ID[cid]
    B, H, W = case.frame
    N, D = 3, 3
    t = ruc.inputs(case.frame, case.sset)
    sw = sweeper(case.wkind)
    L = _lib.lib()
    lay = ruc.record_layout(case.frame)
    for which, key, size in ((0, "x_plane", 4), (1, "state_slab", 4), (2, "z_slab", 4), (3, "u_slab", 4),
                             (4, "stats_slab", 8)):
        assert L.aarmvs_train_record_bytes(B, H, W, which) == lay[key] * size, key
    sc = syn.scene(B, N, H, W, D, seed=100 * H + W)
    feats = torch.from_numpy(sc["features"]).to(DEV)
    proj = torch.from_numpy(sc["proj_matrices"])
    dv = torch.from_numpy(sc["depth_values"])
    rec = sw.record_buffers(B, H, W, D, DEV, nsrc=N - 1, planes=3)
    for buf in rec.values():
        buf.zero_()
    hs, cs = ruc.state_views(rec["state"].view(torch.float32), case.frame, 0)
    for k in range(5):
        hs[k].copy_(t["hp"][k])
        cs[k].copy_(t["cp"][k])
    cost = torch.zeros(B, D, H, W, device=DEV)
    sw(feats[0], [feats[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)], dv,
       want_depth=False, cost_out=cost, d_range=(1, 3), record=rec, record_d0=1)
    torch.cuda.synchronize()
    cost = cost.cpu()
    P64, P32 = ruc.weights(case.wkind, torch.float64), ruc.weights(case.wkind, torch.float32)
    rows = []
    for i in (0, 1):
        r = ruc.parse_record(rec, case.frame, i)
        r["stale"] = t["stale"]
        if i == 0:   # the sweep started from the injected state
            for k in range(5):
                assert torch.equal(r["hp"][k], t["hp"][k]) and torch.equal(r["cp"][k], t["cp"][k])
        got = {"cost": cost[:, 1 + i: 2 + i]}
        for k in range(5):
            got[f"z{k}"], got[f"h{k}"], got[f"c{k}"] = r["z"][k], r["h"][k], r["c"][k]
        for j in range(2):
            got[f"u{j}"], got[f"stats{j}"] = r["u"][j], r["stats"][j]
        with torch.no_grad():
            ref64 = ruc.train_units(P64, ruc.to_dtype(r, torch.float64), case.frame)
            ref32 = ruc.train_units(P32, ruc.to_dtype(r, torch.float32), case.frame)
        _planted_faults_fail(case, P64, ruc.to_dtype(r, torch.float64), got, ruc.train_units, True)
        for n in ruc.TRAIN_TENSORS:
            assert torch.isfinite(got[n]).all() and float(ref64[n].abs().max()) > 0, n
            ratio, idx, err = ruc.worst(n, got[n], ref64[n])
            rows.append((ratio, f"plane{1 + i}:{n}", idx, err, float((ref32[n].double() - ref64[n]).abs().max())))
    print()
    for ratio, n, idx, err, e32 in rows:
        print(f"  [{cid} train] {n:14s} {err:.3e} ({ratio:.3f} of the bound)  float32 CPU {e32:.3e}")
    bad = _report(f"{cid} train", rows)
    assert not bad, bad
