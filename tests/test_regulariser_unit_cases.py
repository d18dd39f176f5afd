"""CPU checks of tests/regulariser_unit_cases.py: what keeps tests/test_gpu_regulariser_units.py
honest.  No GPU, no library.

* The restated primitives without a fault equal oracle.sweep_oracle's lstm_cell / deconv_gn_relu /
  head conv, which the true references go through.
* Every planted fault, on every frame on which it exists, moves the unit it targets by at least
  10x the GPU test's bound at one pixel or more, in the inference decomposition and in the
  training record's; the smallest margins are printed (profiles/regulariser_unit_errors.txt).
* The inputs have the properties the cases claim.
* The float32 CPU evaluation of every unit is inside the GPU test's bound on every case.
"""
import numpy as np
import pytest
import torch

import regulariser_unit_cases as ruc

IDS = [c.id for c in ruc.CASES]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(min(8, prev))
    yield
    torch.set_num_threads(prev)


def test_cases_cover_every_frame_state_set_and_ring_position():
    assert {c.frame for c in ruc.CASES} == set(ruc.FRAMES)
    for f in ruc.FRAMES:   # no state set of any frame has been removed
        assert {c.sset for c in ruc.CASES if c.frame == f and c.wkind == "real"} == set(ruc.STATE_SETS)
    assert any(c.wkind == "syn" and c.frame == (2, 8, 36) for c in ruc.CASES)
    assert {1, 2, 5, 6} <= {c.k for c in ruc.CASES} and all(c.k >= 1 for c in ruc.CASES)
    for k, ring in enumerate((6, 4, 3, 3, 2)):   # every ring wraps in some case
        assert any((c.k + 1) % ring == 0 for c in ruc.CASES), k
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("cid", IDS)
def test_restated_primitives_equal_the_oracle(cid):
    case = ruc.BY_ID[cid]
    P64 = ruc.weights(case.wkind, torch.float64)
    ref = ruc.cpu_reference(case)
    t64 = ruc.to_dtype(ref["t"], torch.float64)
    with torch.no_grad():
        own = ruc.infer_units(P64, t64, case.frame)
    for name, want in ref["inf64"].items():
        err = float((own[name] - want).abs().max())
        # (the variance as ss / n - mean^2 against mean((x - mean)^2): float64 rounding only)
        assert err <= 1e-11 * max(1.0, float(want.abs().max())), (name, err)
    # the training decomposition of the same (float32-rounded) tensors agrees with the units to
    # the rounding of its inputs
    for k in range(5):
        for n in (f"h{k}", f"c{k}"):
            d = float((ref["trn64"][n] - ref["inf64"][n]).abs().max())
            assert d <= 1e-4 * max(1.0, float(ref["inf64"][n].abs().max())), (n, d)


@pytest.mark.parametrize("cid", IDS)
def test_input_properties(cid):
    case = ruc.BY_ID[cid]
    B, H, W = case.frame
    t = ruc.inputs(case.frame, case.sset)
    assert t["x"].dtype == torch.float32 and tuple(t["x"].shape) == (B, 32, H, W)
    rms = float(torch.sqrt((t["x"].double() ** 2).mean()))
    assert 0.5 * ruc.x_scale() <= rms <= 2.0 * ruc.x_scale() and ruc.x_scale() > 0
    for k in range(5):
        hp, cp, stale = t["hp"][k], t["cp"][k], t["stale"][k]
        assert tuple(hp.shape) == tuple(cp.shape) == ruc.level_shape(case.frame, k)
        assert float(hp.abs().max()) < 1.0
        assert not torch.equal(hp, stale)
    if B > 1:   # the batch elements differ in every tensor
        for v in [t["x"]] + t["hp"] + t["cp"] + t["stale"]:
            assert not torch.equal(v[0], v[1])
    if case.sset == "plain":
        assert all(float(c.abs().max()) <= 4.0 for c in t["cp"])
        return
    for k in range(5):
        hp, cp = t["hp"][k], t["cp"][k]
        Hk = hp.shape[2]
        assert float(cp.abs().max()) > 20.0 and float(cp.abs().max()) <= 30.0     # tanh(c) saturates
        for b in range(B):
            assert float(cp[b].abs().max()) > 20.0
        assert float(hp[:, ruc.ZERO_CHANNEL].abs().max()) == 0.0                  # one full channel
        assert float(hp[:, :, ruc.zero_row(Hk)].abs().max()) == 0.0               # one full row
    # the checkerboard of h0-'s last two columns: in every 2x2 window (but the zeroed row's) the
    # signs alternate, and over the windows the maximum falls on each position that exists
    h0 = t["hp"][0]
    pos = set()
    for wy in range(H // 2):
        if ruc.zero_row(H) // 2 == wy:
            continue
        for ch in (0, 5, 15):   # (the zero channel aside, every channel has the pattern)
            win = h0[:, ch, 2 * wy: 2 * wy + 2, W - 2:]
            assert bool((win[:, 0, 0] * win[:, 0, 1] < 0).all()) and bool((win[:, 0, 0] * win[:, 1, 0] < 0).all())
            assert bool((win[:, 0, 0] * win[:, 1, 1] > 0).all())
            pos.add(int(win[0].reshape(-1).argmax()))
    assert len(pos) == min(4, H // 2 - 1), pos


_margins = {}


@pytest.mark.parametrize("cid", IDS)
def test_planted_faults_are_visible(cid):
    """Every fault that exists on the frame, applied to the reference, differs from the true one by
    >= 10x the bound in the unit it targets -- so reverting it into the reference fails the GPU
    test (the GPU's tensors replace the CPU chain's there; both feed the same functions)."""
    case = ruc.BY_ID[cid]
    P64 = ruc.weights(case.wkind, torch.float64)
    ref = ruc.cpu_reference(case)
    t64 = ruc.to_dtype(ref["t"], torch.float64)
    faults = ruc.applicable(case.frame)
    assert {f[0] for f in faults} >= {"pool", "stale", "swap_if"}
    low = []
    with torch.no_grad():
        for fault in faults:
            for training, true in ((False, ref["inf64"]), (True, ref["trn64"])):
                bad = (ruc.train_units if training else ruc.infer_units)(P64, t64, case.frame, fault=fault)
                m = max(ruc.worst(n, bad[n], true[n])[0] for n in ruc.fault_target(fault, training))
                key = (fault[0], "training" if training else "inference")
                _margins[key] = min(_margins.get(key, (np.inf, None)), (m, f"{cid} cell {fault[1]}"))
                if m < ruc.FAULT_FACTOR:
                    low.append((fault, training, m))
    assert not low, low


def test_every_fault_is_planted_somewhere_and_print_the_margins():
    """(after the cases above) each of the seven faults exists on some frame, in both
    decompositions; prints the smallest margin of each, in units of the GPU test's bound."""
    if len(_margins) < 2 * len(ruc.FAULTS):   # run alone: fill the table
        for cid in IDS:
            test_planted_faults_are_visible(cid)
    assert {k[0] for k in _margins} == set(ruc.FAULTS)
    print("\nplanted-fault margins: min over cases and cells of max|faulty - true| / bound")
    for (name, path), (m, where) in sorted(_margins.items()):
        print(f"  {name:10s} {path:9s} {m:12.1f}x  ({where})")
        assert m >= ruc.FAULT_FACTOR
    on_frame = {f: {n for n, _ in ruc.applicable(f)} for f in ruc.FRAMES}
    assert on_frame[(1, 4, 4)] == {"pool", "stale", "swap_if"}
    assert "deconv_col" in on_frame[(2, 12, 132)] and "gn_elem0" in on_frame[(2, 8, 36)]
    assert "seam" in on_frame[(1, 36, 68)] and "c_elem0" in on_frame[(2, 12, 132)]


@pytest.mark.parametrize("cid", IDS)
def test_float32_stays_inside_the_bound(cid):
    """The float32 CPU evaluation of every unit, on the same inputs, is within the GPU test's
    bound of float64 -- a case where float32 itself is outside it would not belong in the GPU test.
    The statistics are exempt by construction: they are fp64 sums of fp32 values and their bound
    (1e-6 relative) lies below what a float32 sum can hold."""
    case = ruc.BY_ID[cid]
    ref = ruc.cpu_reference(case)
    out = []
    for path, names in (("inf", ref["inf64"].keys()), ("trn", [n for n in ruc.TRAIN_TENSORS if not n.startswith("stats")])):
        for n in names:
            r, idx, err = ruc.worst(n, ref[path + "32"][n], ref[path + "64"][n])
            out.append((r, path, n, idx, err))
    r, path, n, idx, err = max(out)
    print(f"\n{cid}: float32 worst {path}:{n} {err:.3e} = {r:.3f} of the bound at {idx}")
    assert r <= 1.0, (path, n, idx, err)
