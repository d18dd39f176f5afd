"""The sub-plane refinement's C ABI and Python surface without a GPU: the symbols, the state
size, and the rejections that happen before any device work."""
import ctypes

import pytest

FAKE = 0x1000   # never dereferenced: validation fails first
INVALID = 1


def _err():
    from aarmvs import lib
    return lib().aarmvs_last_error().decode()


def _sweep_args(D=4, rec=None):
    from aarmvs import _lib
    a = _lib.SweepArgs()
    a.B, a.C, a.H, a.W, a.nsrc, a.D = 1, 32, 8, 8, 1, D
    a.d_begin, a.d_end = 0, D
    a.ref_fea = a.rel_proj = a.depth_values = a.packed_params = a.workspace = FAKE
    a.src_fea[0] = FAKE
    if rec is not None:
        a.record = ctypes.pointer(rec)
    return a


def _refine(state=FAKE):
    from aarmvs import _lib
    r = _lib.RefineArgs()
    r.state = state
    r.depth_refined_out = r.conf_window_out = r.index_out = FAKE
    return r


def test_symbols_exist():
    from aarmvs import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("aarmvs_refine_state_bytes", "aarmvs_sweep_r", "aarmvs_wta_refine_update",
                 "aarmvs_wta_refine_finalize", "aarmvs_refine_from_cost"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES
    assert [f[0] for f in _lib.RefineArgs._fields_] == ["state", "depth_refined_out", "conf_window_out",
                                                        "index_out"]
    assert ctypes.sizeof(_lib.RefineArgs) == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_state_bytes():
    from aarmvs import lib
    L = lib()
    assert L.aarmvs_refine_state_bytes(2, 720) == 23040
    assert L.aarmvs_refine_state_bytes(1, 1600 * 1184) == 16 * 1600 * 1184
    for B, HW in ((0, 720), (2, 0), (-1, 720), (2, -5)):
        assert L.aarmvs_refine_state_bytes(B, HW) == 0


def test_the_workspace_and_the_sweep_struct_did_not_change():
    from aarmvs import _lib
    assert [f[0] for f in _lib.SweepArgs._fields_][-3:] == ["record", "record_d0", "record_planes"]


@pytest.mark.parametrize("precision", [0, 1])
def test_sweep_r_rejects_a_null_state(precision):
    from aarmvs import lib
    a, r = _sweep_args(), _refine(state=None)
    assert lib().aarmvs_sweep_r(ctypes.byref(a), precision, ctypes.byref(r), None) == INVALID
    assert "state" in _err() and "aarmvs_refine_state_bytes" in _err()


def test_sweep_r_rejects_a_training_record():
    from aarmvs import _lib, lib
    rec = _lib.TrainRecord()
    rec.x = rec.state = rec.z = rec.u = rec.stats = rec.t1 = rec.ostats = FAKE
    a, r = _sweep_args(rec=rec), _refine()
    assert lib().aarmvs_sweep_r(ctypes.byref(a), 0, ctypes.byref(r), None) == INVALID
    assert "record" in _err() and "inference" in _err()


def test_sweep_r_without_refinement_is_sweep_p():
    """refine == NULL goes through aarmvs_sweep_p's checks with their messages."""
    from aarmvs import lib
    L = lib()
    a = _sweep_args()
    a.C = 16
    assert L.aarmvs_sweep_r(ctypes.byref(a), 0, None, None) == INVALID
    assert _err() == "sweep: feature channels C must be 32"
    assert L.aarmvs_sweep_r(ctypes.byref(a), 7, None, None) == INVALID and "unknown precision" in _err()
    a = _sweep_args()
    a.d_end = 9
    assert L.aarmvs_sweep_r(ctypes.byref(a), 0, ctypes.byref(_refine()), None) == INVALID
    assert _err() == "sweep: need 0 <= d_begin < d_end <= D"


def test_standalone_entries_validate_before_launching():
    from aarmvs import lib
    L = lib()
    assert L.aarmvs_wta_refine_update(FAKE, 0, FAKE, FAKE, FAKE, None, FAKE, 1, 8, None) == INVALID
    assert "wta_refine_update" in _err()
    assert L.aarmvs_wta_refine_update(FAKE, -1, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 8, None) == INVALID
    assert L.aarmvs_wta_refine_update(FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 0, None) == INVALID
    assert L.aarmvs_wta_refine_finalize(FAKE, FAKE, FAKE, None, FAKE, 1, 4, 4, 8, FAKE, FAKE, FAKE, None) == INVALID
    assert "null" in _err()
    for n in (0, 5):   # 1 <= n <= D
        assert L.aarmvs_wta_refine_finalize(FAKE, FAKE, FAKE, FAKE, FAKE, 1, 4, n, 8, FAKE, FAKE, FAKE,
                                            None) == INVALID
        assert "1 <= n <= D" in _err()
    assert L.aarmvs_refine_from_cost(None, FAKE, 1, 4, 8, FAKE, FAKE, FAKE, None) == INVALID
    assert L.aarmvs_refine_from_cost(FAKE, FAKE, 1, 0, 8, FAKE, FAKE, FAKE, None) == INVALID
    assert "refine_from_cost" in _err()


def test_profiler_name_comes_after_the_existing_ones():
    from aarmvs import lib
    L = lib()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    assert names[-1] == "refine" and names.index("head_wta") == 12 and len(set(names)) == len(names)


def test_python_surface():
    import torch
    from aarmvs import AarmvsError, eval_sharded, fusion, ops, train_ddp
    from models import EMVSNet
    with pytest.raises(ValueError, match="refine_depth"):
        EMVSNet(disparity_level=8, evidential=False, refine_depth=True, return_depth=False)
    assert EMVSNet(disparity_level=8, evidential=False, return_depth=True, refine_depth=True).refine_depth
    assert EMVSNet(disparity_level=8, evidential=False, return_depth=True).refine_depth is False
    assert eval_sharded.parse_args([]).refine_depth is False
    assert eval_sharded.parse_args(["--refine_depth"]).refine_depth is True
    assert train_ddp.parse_args([]).refine_metrics is False
    assert train_ddp.parse_args(["--refine_metrics"]).refine_metrics is True
    base = ["--test_dataset", "dtu", "--testpath", "p", "--testlist", "l", "--outdir", "o"]
    a = fusion.parse_args(base)
    assert (a.depth_dir, a.conf_dir) == ("depth_est_0", "confidence_0")
    a = fusion.parse_args(base + ["--depth_dir", "depth_refined_0", "--conf_dir", "confidence_window_0"])
    assert (a.depth_dir, a.conf_dir) == ("depth_refined_0", "confidence_window_0")
    # CPU tensors are refused: there is no CPU fallback
    with pytest.raises(AarmvsError):
        ops.refine_from_cost(torch.zeros(1, 3, 2, 4), torch.ones(1, 3))
