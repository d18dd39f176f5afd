"""The depth-posterior statistics' C ABI and Python surface without a GPU: the symbols, the
structs, the state size, aarmvs_sweep_ex's size rule, and the rejections that happen before any
device work."""
import ctypes

import pytest

FAKE = 0x1000   # never dereferenced: validation fails first
INVALID = 1
PTR = ctypes.sizeof(ctypes.c_void_p)


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


def _posterior(state=FAKE):
    from aarmvs import _lib
    p = _lib.PosteriorArgs()
    p.state = state
    p.mean_out = p.std_out = p.entropy_out = p.runner_up_out = FAKE
    return p


def _options(precision=0, posterior=None, refine=None, size=None):
    from aarmvs import _lib
    o = _lib.SweepOptions()
    o.size = ctypes.sizeof(o) if size is None else size
    o.precision = precision
    if posterior is not None:
        o.posterior = ctypes.pointer(posterior)
    if refine is not None:
        o.refine = ctypes.pointer(refine)
    return o


def _sweep_ex(a, o):
    from aarmvs import lib
    return lib().aarmvs_sweep_ex(ctypes.byref(a), ctypes.byref(o) if o is not None else None, None)


def test_symbols_and_structs():
    from aarmvs import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("aarmvs_posterior_state_bytes", "aarmvs_sweep_ex", "aarmvs_wta_posterior_update",
                 "aarmvs_wta_posterior_finalize", "aarmvs_posterior_from_cost"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES
    assert [f[0] for f in _lib.PosteriorArgs._fields_] == ["state", "mean_out", "std_out", "entropy_out",
                                                           "runner_up_out"]
    assert ctypes.sizeof(_lib.PosteriorArgs) == 5 * PTR
    assert [f[0] for f in _lib.SweepOptions._fields_] == ["size", "precision", "refine", "posterior"]
    assert ctypes.sizeof(_lib.SweepOptions) == ctypes.sizeof(ctypes.c_size_t) + 8 + 2 * PTR
    assert _lib.SweepOptions.posterior.offset == ctypes.sizeof(_lib.SweepOptions) - PTR
    int_, ptr = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["aarmvs_sweep_ex"] == (int_, [ctypes.POINTER(_lib.SweepArgs),
                                                         ctypes.POINTER(_lib.SweepOptions), ptr])
    assert _lib.SIGNATURES["aarmvs_posterior_state_bytes"] == (ctypes.c_size_t, [int_, int_])
    assert _lib.SIGNATURES["aarmvs_wta_posterior_update"] == (int_, [ptr, int_] + [ptr] * 5 + [int_, int_, ptr])
    assert _lib.SIGNATURES["aarmvs_wta_posterior_finalize"] == (int_, [ptr, ptr, int_, int_] + [ptr] * 5)
    assert _lib.SIGNATURES["aarmvs_posterior_from_cost"] == (int_, [ptr, ptr, int_, int_, int_] + [ptr] * 5)


def test_state_bytes():
    from aarmvs import lib
    L = lib()
    assert L.aarmvs_posterior_state_bytes(2, 720) == 23040
    assert L.aarmvs_posterior_state_bytes(1, 1600 * 1184) == 16 * 1600 * 1184
    for B, HW in ((0, 720), (2, 0), (-1, 720), (2, -5)):
        assert L.aarmvs_posterior_state_bytes(B, HW) == 0


WORKSPACE_HEADLINE = 14101997568   # aarmvs_sweep_workspace_bytes(1, 1184, 1600, 6) before this feature
WORKSPACE_SMALL = 8606720          # ... and of (2, 20, 36, 2)


def test_the_workspace_and_the_sweep_struct_did_not_change():
    from aarmvs import _lib, lib
    assert [f[0] for f in _lib.SweepArgs._fields_][-3:] == ["record", "record_d0", "record_planes"]
    # the workspace of the headline and of the tests' shape: the values of the parent commit
    assert lib().aarmvs_sweep_workspace_bytes(1, 1184, 1600, 6) == WORKSPACE_HEADLINE
    assert lib().aarmvs_sweep_workspace_bytes(2, 20, 36, 2) == WORKSPACE_SMALL


@pytest.mark.parametrize("precision", [0, 1])
def test_sweep_ex_rejects_a_null_state(precision):
    a = _sweep_args()
    assert _sweep_ex(a, _options(precision, posterior=_posterior(state=None))) == INVALID
    assert "state" in _err() and "aarmvs_posterior_state_bytes" in _err()


def test_sweep_ex_rejects_a_training_record_with_a_posterior():
    from aarmvs import _lib
    rec = _lib.TrainRecord()
    rec.x = rec.state = rec.z = rec.u = rec.stats = rec.t1 = rec.ostats = FAKE
    a = _sweep_args(rec=rec)
    assert _sweep_ex(a, _options(posterior=_posterior())) == INVALID
    assert "record" in _err() and "inference" in _err() and "aarmvs_posterior_from_cost" in _err()


def test_sweep_ex_rejects_an_unknown_precision():
    assert _sweep_ex(_sweep_args(), _options(precision=7, posterior=_posterior())) == INVALID
    assert "unknown precision" in _err()


def test_sweep_ex_size_rule():
    """Any size from the first version's up to the library's own; everything else is refused
    before the struct's other fields are looked at."""
    from aarmvs import _lib
    full = ctypes.sizeof(_lib.SweepOptions)
    for size in (0, 8, full - 1, full + 1, full + 8, 1 << 20):
        o = _options(size=size)
        assert _sweep_ex(_sweep_args(), o) == INVALID, size
        assert "aarmvs_sweep_options.size" in _err(), size
    # a right-sized struct gets past the rule, to the checks of the arguments
    a = _sweep_args()
    a.C = 16
    assert _sweep_ex(a, _options()) == INVALID and _err() == "sweep: feature channels C must be 32"
    # NULL options are the defaults
    assert _sweep_ex(a, None) == INVALID and _err() == "sweep: feature channels C must be 32"
    from aarmvs import lib
    assert lib().aarmvs_sweep_ex(None, ctypes.byref(_options()), None) == INVALID and "null args" in _err()


def test_the_older_entries_are_wrappers():
    """aarmvs_sweep / _p / _r reach the same checks with the same messages."""
    from aarmvs import _lib, lib
    L = lib()
    a = _sweep_args()
    a.d_end = 9
    for call in (lambda: L.aarmvs_sweep(ctypes.byref(a), None), lambda: L.aarmvs_sweep_p(ctypes.byref(a), 1, None),
                 lambda: L.aarmvs_sweep_r(ctypes.byref(a), 0, None, None), lambda: _sweep_ex(a, _options())):
        assert call() == INVALID and _err() == "sweep: need 0 <= d_begin < d_end <= D"
    r = _lib.RefineArgs()
    assert _sweep_ex(_sweep_args(), _options(refine=r)) == INVALID and "aarmvs_refine_state_bytes" in _err()


def test_standalone_entries_validate_before_launching():
    from aarmvs import lib
    L = lib()
    assert L.aarmvs_wta_posterior_update(FAKE, 0, FAKE, FAKE, FAKE, None, FAKE, 1, 8, None) == INVALID
    assert "wta_posterior_update" in _err()
    assert L.aarmvs_wta_posterior_update(FAKE, -1, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 8, None) == INVALID
    assert L.aarmvs_wta_posterior_update(FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 0, None) == INVALID
    assert L.aarmvs_wta_posterior_finalize(FAKE, None, 1, 8, FAKE, FAKE, FAKE, FAKE, None) == INVALID
    assert "null" in _err()
    assert L.aarmvs_wta_posterior_finalize(FAKE, FAKE, 0, 8, FAKE, FAKE, FAKE, FAKE, None) == INVALID
    assert L.aarmvs_posterior_from_cost(None, FAKE, 1, 4, 8, FAKE, FAKE, FAKE, FAKE, None) == INVALID
    assert L.aarmvs_posterior_from_cost(FAKE, FAKE, 1, 0, 8, FAKE, FAKE, FAKE, FAKE, None) == INVALID
    assert "posterior_from_cost" in _err()


def test_profiler_names_are_unchanged():
    from aarmvs import lib
    L = lib()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    assert names.index("head_wta") == 12 and names.index("refine") == 57 and len(set(names)) == len(names)


def test_python_surface():
    import torch
    from aarmvs import AarmvsError, eval_sharded, ops, train_ddp
    from models import EMVSNet
    with pytest.raises(ValueError, match="posterior_stats"):
        EMVSNet(disparity_level=8, evidential=False, posterior_stats=True, return_depth=False)
    m = EMVSNet(disparity_level=8, evidential=False, return_depth=True, posterior_stats=True, refine_depth=True)
    assert m.posterior_stats and m.refine_depth
    assert EMVSNet(disparity_level=8, evidential=False, return_depth=True).posterior_stats is False
    assert eval_sharded.parse_args([]).posterior_stats is False
    assert eval_sharded.parse_args(["--posterior_stats"]).posterior_stats is True
    assert train_ddp.parse_args([]).uncertainty_metrics is False
    assert train_ddp.parse_args(["--uncertainty_metrics"]).uncertainty_metrics is True
    assert ops.POSTERIOR_KEYS == ("depth_mean", "depth_std", "entropy", "runner_up")
    # CPU tensors are refused: there is no CPU fallback
    with pytest.raises(AarmvsError):
        ops.posterior_from_cost(torch.zeros(1, 3, 2, 4), torch.ones(1, 3))
    with pytest.raises(AarmvsError):
        ops.wta_posterior_finalize(torch.zeros(1, 2, 4), torch.zeros(32))
