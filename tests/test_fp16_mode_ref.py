"""The fp16 mode without a device: the CPU emulation the GPU tests are bounded by
(tests/fp16_mode_ref.py), and the C ABI / Python surface of the mode (every call here is refused
before the library touches the GPU, as in test_checkpoint_host.py).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from aarmvs import synthetic as syn

import fp16_mode_ref as fref

FAKE = 0x1000   # never dereferenced: validation fails first
INVALID = 1
SPLIT, FP16 = 0, 1


def _err():
    from aarmvs import lib
    return lib().aarmvs_last_error().decode()


def real_P():
    g = np.load(os.path.join(GOLDEN, "real_weights_sweep.npz"), allow_pickle=False)
    return {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}


# ---------------------------------------------------------------------------------------
# emulation sanity
# ---------------------------------------------------------------------------------------
def test_round11_is_fp16_rounding_in_the_normal_range():
    g = torch.Generator().manual_seed(3)
    mag = torch.exp2(torch.rand(20000, generator=g) * 29.0 - 14.0)          # 2^-14 .. 2^15
    sign = torch.where(torch.rand(20000, generator=g) < 0.5, -1.0, 1.0)
    ties = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2048.0 + 1.0, 2048.0 + 3.0, 65504.0, 2.0 ** -14,
                         0.0, -0.0, 1.0, -3.0])                             # half-way cases: to even
    v = torch.cat([mag * sign, ties])
    assert torch.equal(fref.round11(v), v.half().float())
    # and past fp16's range the same relative rounding (the library rescales instead)
    big = v * 2.0 ** 20
    assert torch.equal(fref.round11(big), (v.half().float()) * 2.0 ** 20)


def test_context_restores_the_oracle():
    from oracle import sweep_oracle as orc
    before = orc.lstm_cell, orc.deconv_gn_relu
    with fref.fp16_operands():
        assert orc.lstm_cell is not before[0] and orc.deconv_gn_relu is not before[1]
    assert (orc.lstm_cell, orc.deconv_gn_relu) == before
    with pytest.raises(RuntimeError):
        with fref.fp16_operands():
            raise RuntimeError("x")
    assert (orc.lstm_cell, orc.deconv_gn_relu) == before


def test_emulated_sweep_error_is_the_measured_one():
    """(1,3,32,48,16) with the real weights: the emulation differs from the fp32 oracle by an rms
    cost error within a factor 2 of 1.5e-3 (the mode's measured error)."""
    from oracle import sweep_oracle as orc
    B, N, H, W, D = 1, 3, 32, 48, 16
    sc = syn.scene(B, N, H, W, D, seed=41)
    feats = torch.from_numpy(sc["features"])
    proj = torch.from_numpy(sc["proj_matrices"])
    dv = torch.from_numpy(sc["depth_values"])
    views = (feats[0], [feats[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)])
    P = real_P()
    ref = orc.sweep(*views, dv, P)
    with fref.fp16_operands():
        emu = orc.sweep(*views, dv, P)
    again = orc.sweep(*views, dv, P)
    assert torch.equal(again["cost"], ref["cost"])          # the swap left nothing behind
    assert not torch.equal(emu["cost"], ref["cost"])
    e = fref.rms(emu["cost"] - ref["cost"])
    print(f"emulated fp16 mode: cost rms error {e:.3e} (cost rms {fref.rms(ref['cost']):.3g})")
    assert 0.75e-3 <= e <= 3.0e-3


# ---------------------------------------------------------------------------------------
# ABI, no GPU needed
# ---------------------------------------------------------------------------------------
def _record(fill=FAKE):
    from aarmvs import _lib
    r = _lib.TrainRecord()
    r.x = r.state = r.z = r.u = r.stats = r.t1 = r.ostats = fill
    return r


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


@pytest.mark.parametrize("precision", [2, -1, 16])
def test_sweep_p_rejects_an_unknown_precision(precision):
    from aarmvs import lib
    a = _sweep_args()
    assert lib().aarmvs_sweep_p(ctypes.byref(a), precision, None) == INVALID
    assert "unknown precision" in _err() and str(precision) in _err()
    assert lib().aarmvs_unet_step_p(FAKE, 1, 8, 8, 1, 0, FAKE, FAKE, FAKE, precision, None) == INVALID
    assert "unet_step: unknown precision" in _err()


def test_sweep_p_rejects_fp16_with_a_training_record():
    from aarmvs import lib
    rec = _record()
    a = _sweep_args(rec=rec)
    assert lib().aarmvs_sweep_p(ctypes.byref(a), FP16, None) == INVALID
    assert "AARMVS_PREC_FP16" in _err() and "record" in _err()


def test_sweep_p_split_keeps_the_old_rejections():
    """aarmvs_sweep_p(a, 0, s) is aarmvs_sweep(a, s): the rejections of
    test_checkpoint_host.py::test_zeroed_new_fields_keep_the_old_rejections with their exact
    messages, through both entries; the FP16 value meets the same argument checks."""
    from aarmvs import _lib, lib
    L = lib()
    for call in (lambda a: L.aarmvs_sweep_p(ctypes.byref(a), SPLIT, None),
                 lambda a: L.aarmvs_sweep(ctypes.byref(a), None),
                 lambda a: L.aarmvs_sweep_p(ctypes.byref(a), FP16, None)):
        a = _lib.SweepArgs()
        a.B, a.C, a.H, a.W, a.nsrc, a.D, a.d_begin, a.d_end = 1, 32, 8, 8, 1, 4, 0, 4
        assert call(a) == INVALID and _err() == "sweep: null pointer argument"
        a = _sweep_args(D=4)
        a.C = 16
        assert call(a) == INVALID and _err() == "sweep: feature channels C must be 32"
        a.C, a.d_end = 32, 5
        assert call(a) == INVALID and _err() == "sweep: need 0 <= d_begin < d_end <= D"
        a.d_end, a.d_begin = 4, 4
        assert call(a) == INVALID and _err() == "sweep: need 0 <= d_begin < d_end <= D"
        a.d_begin, a.nsrc = 0, 2
        assert call(a) == INVALID and _err() == "sweep: null src_fea pointer"
        a.nsrc, a.H = 1, 6
        assert call(a) == INVALID and "multiples of 4" in _err()
    null_rec = _lib.TrainRecord()
    a = _sweep_args(D=4, rec=null_rec)
    assert L.aarmvs_sweep_p(ctypes.byref(a), SPLIT, None) == INVALID
    assert _err() == "sweep: training record with a null buffer"
    a = _sweep_args(D=40, rec=_record())
    a.d_begin, a.d_end, a.record_d0, a.record_planes = 16, 32, 0, 16
    assert L.aarmvs_sweep_p(ctypes.byref(a), SPLIT, None) == INVALID
    assert "sweep: the record holds planes [0, 16) and does not cover the range [16, 32)" in _err()
    assert L.aarmvs_unet_step_p(None, 1, 8, 8, 1, 0, FAKE, FAKE, FAKE, SPLIT, None) == INVALID
    assert _err() == "unet_step: null pointer or negative step"
    # the struct did not grow for the mode
    assert [f[0] for f in _lib.SweepArgs._fields_][-3:] == ["record", "record_d0", "record_planes"]


def test_profiler_names_of_the_fp16_kernels():
    from aarmvs import lib
    L = lib()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    for k in range(5):
        assert f"lstm_cell{k}" in names and f"lstm_cell{k}_fp16" in names
    assert "deconv0_fp16" in names and "deconv1_fp16" in names
    # existing names keep their ids: the new ones come after them
    assert names.index("lstm_cell0") == 5 and names.index("deconv0") == 10
    assert names.index("lstm_cell0_fp16") > names.index("depth_metrics")
    assert len(set(names)) == len(names)


def test_python_surface_rejects_unknown_modes():
    from aarmvs import AarmvsError, eval_sharded, ops
    with pytest.raises(AarmvsError, match="precision"):
        ops.DepthSweep({}, "cuda", precision="bf16")     # refused before the parameters or the device
    from models import EMVSNet
    with pytest.raises(ValueError, match="sweep_precision"):
        EMVSNet(disparity_level=8, evidential=False, sweep_precision="bf16")
    assert EMVSNet(disparity_level=8, evidential=False).sweep_precision == "split"
    assert EMVSNet(disparity_level=8, evidential=False, sweep_precision="fp16").sweep_precision == "fp16"
    assert eval_sharded.parse_args([]).sweep_precision == "split"
    assert eval_sharded.parse_args(["--sweep_precision", "fp16"]).sweep_precision == "fp16"
    with pytest.raises(SystemExit):
        eval_sharded.parse_args(["--sweep_precision", "bf16"])
