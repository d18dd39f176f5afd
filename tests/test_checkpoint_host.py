"""Host-side checks of plane-segment checkpointing (no device: every call here is refused or
answered before the library touches the GPU).

* aarmvs_sweep_backward rejects a misaligned range, a range outside [0, D] and a record that
  does not cover the range, each with a message naming the rule; aarmvs_sweep rejects a record
  that does not cover its planes.
* Structs whose new fields are zero (the old form) are accepted or rejected exactly as before:
  the same status and the same message for every case tools/asan/abi_host.cpp walks through.
* aarmvs_train_segment_bytes against bytes computed by hand.
* EMVSNet(checkpoint_planes=24) raises ValueError.
"""
import ctypes

import pytest

FAKE = 0x1000   # never dereferenced: validation fails first
INVALID = 1


def _err():
    from aarmvs import lib
    return lib().aarmvs_last_error().decode()


def _record(fill=FAKE):
    from aarmvs import _lib
    r = _lib.TrainRecord()
    r.x = r.state = r.z = r.u = r.stats = r.t1 = r.ostats = fill
    return r


def _backward_args(D=40, H=8, W=8, rec=None):
    from aarmvs import _lib
    a = _lib.BackwardArgs()
    a.B, a.C, a.H, a.W, a.nsrc, a.D = 1, 32, H, W, 1, D
    a.ref_fea = a.rel_proj = a.depth_values = a.packed_params = FAKE
    a.src_fea[0] = FAKE
    a.grad_cost = a.workspace = a.scratch = a.grad_ref = FAKE
    a.record = ctypes.pointer(rec if rec is not None else _record())
    return a


def _sweep_args(D=40, rec=None):
    from aarmvs import _lib
    a = _lib.SweepArgs()
    a.B, a.C, a.H, a.W, a.nsrc, a.D = 1, 32, 8, 8, 1, D
    a.d_begin, a.d_end = 0, D
    a.ref_fea = a.rel_proj = a.depth_values = a.packed_params = a.workspace = FAKE
    a.src_fea[0] = FAKE
    if rec is not None:
        a.record = ctypes.pointer(rec)
    return a


def _bwd(a):
    from aarmvs import lib
    return lib().aarmvs_sweep_backward(ctypes.byref(a), None)


@pytest.mark.parametrize("d_begin,d_end", [(8, 40), (16, 24), (0, 39), (17, 32)])
def test_backward_rejects_a_misaligned_range(d_begin, d_end):
    a = _backward_args()
    a.d_begin, a.d_end = d_begin, d_end
    assert _bwd(a) == INVALID
    msg = _err()
    assert "misaligned" in msg and "multiples of 16" in msg and f"[{d_begin}, {d_end})" in msg


@pytest.mark.parametrize("d_begin,d_end", [(0, 48), (32, 64), (-16, 16), (32, 32), (32, 16)])
def test_backward_rejects_a_range_outside_the_planes(d_begin, d_end):
    a = _backward_args()
    a.d_begin, a.d_end = d_begin, d_end
    assert _bwd(a) == INVALID
    msg = _err()
    assert "outside [0, D = 40]" in msg and "misaligned" not in msg


@pytest.mark.parametrize("rng,rec_d0,rec_n,held", [((16, 32), 0, 16, "[0, 16)"), ((0, 32), 16, 16, "[16, 32)"),
                                                   ((16, 40), 16, 16, "[16, 32)"), ((0, 0), 16, 0, "[16, 40)"),
                                                   ((32, 40), 0, 32, "[0, 32)")])
def test_backward_rejects_a_record_that_does_not_cover_the_range(rng, rec_d0, rec_n, held):
    a = _backward_args()
    a.d_begin, a.d_end = rng
    a.record_d0, a.record_planes = rec_d0, rec_n
    assert _bwd(a) == INVALID
    msg = _err()
    assert "does not cover the range" in msg and held in msg


@pytest.mark.parametrize("rec_d0,rec_n", [(-1, 0), (40, 0), (32, 16), (0, -4)])
def test_backward_rejects_a_record_outside_the_planes(rec_d0, rec_n):
    a = _backward_args()
    a.d_begin, a.d_end = 32, 40
    a.record_d0, a.record_planes = rec_d0, rec_n
    assert _bwd(a) == INVALID
    assert "record's planes" in _err() and "outside [0, D = 40]" in _err()


def test_sweep_rejects_a_record_that_does_not_cover_its_planes():
    from aarmvs import lib
    a = _sweep_args(rec=_record())
    a.d_begin, a.d_end = 16, 32
    a.record_d0, a.record_planes = 0, 16
    assert lib().aarmvs_sweep(ctypes.byref(a), None) == INVALID
    assert "sweep: the record holds planes [0, 16) and does not cover the range [16, 32)" in _err()
    a.record_d0, a.record_planes = 32, 8
    assert lib().aarmvs_sweep(ctypes.byref(a), None) == INVALID
    assert "does not cover the range" in _err()
    a.record_d0, a.record_planes = 24, 32
    assert lib().aarmvs_sweep(ctypes.byref(a), None) == INVALID
    assert "record's planes" in _err()


def test_zeroed_new_fields_keep_the_old_rejections():
    """The cases of tools/asan/abi_host.cpp with the appended fields zero, as a caller of the old
    form leaves them: the status and the message of each rejection are those of the library
    before the fields existed."""
    from aarmvs import _lib, lib
    L = lib()
    null_rec = _lib.TrainRecord()
    # sweep
    a = _lib.SweepArgs()
    a.B, a.C, a.H, a.W, a.nsrc, a.D, a.d_begin, a.d_end = 1, 32, 8, 8, 1, 4, 0, 4
    assert (a.record_d0, a.record_planes) == (0, 0)
    assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID and _err() == "sweep: null pointer argument"
    a = _sweep_args(D=4)
    a.C = 16
    assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID and _err() == "sweep: feature channels C must be 32"
    a.C, a.d_end = 32, 5
    assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID and _err() == "sweep: need 0 <= d_begin < d_end <= D"
    a.d_end, a.d_begin = 4, 4
    assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID and _err() == "sweep: need 0 <= d_begin < d_end <= D"
    a.d_begin, a.nsrc = 0, 2
    assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID and _err() == "sweep: null src_fea pointer"
    a.nsrc, a.record = 1, ctypes.pointer(null_rec)
    assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID
    assert _err() == "sweep: training record with a null buffer"
    # backward
    b = _lib.BackwardArgs()
    b.B, b.C, b.H, b.W, b.nsrc, b.D = 1, 32, 8, 8, 1, 4
    assert (b.d_begin, b.d_end, b.record_d0, b.record_planes) == (0, 0, 0, 0)
    assert _bwd(b) == INVALID and _err() == "sweep_backward: null pointer argument or D < 1"
    b = _backward_args(D=4, rec=null_rec)
    assert _bwd(b) == INVALID and _err() == "sweep_backward: training record with a null buffer"
    half = _record()
    half.t1 = half.ostats = None
    b = _backward_args(D=4, rec=half)
    assert _bwd(b) == INVALID and _err() == "sweep_backward: training record with a null buffer"
    b = _backward_args(D=4)
    b.grad_ref = None
    assert _bwd(b) == INVALID and _err() == "sweep_backward: grad_ref is required (the cost-slice part)"
    b.C = 16
    assert _bwd(b) == INVALID and _err() == "sweep_backward: feature channels C must be 32"
    b.C, b.H = 32, 6
    assert _bwd(b) == INVALID and "multiples of 4" in _err()


def test_struct_mirrors_grew_by_the_appended_fields_only():
    """The ctypes mirrors end with the new fields, after every field of the old layout (the C
    structs: include/aarmvs.h)."""
    from aarmvs import _lib
    names = [f[0] for f in _lib.SweepArgs._fields_]
    assert names[-3:] == ["record", "record_d0", "record_planes"]
    names = [f[0] for f in _lib.BackwardArgs._fields_]
    assert names[-5:] == ["regulariser_only", "d_begin", "d_end", "record_d0", "record_planes"]
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert _lib.SweepArgs.record_d0.offset == _lib.SweepArgs.record.offset + ptr
    assert _lib.BackwardArgs.d_begin.offset == _lib.BackwardArgs.regulariser_only.offset + 4


def _al64(n):
    return -(-n // 64) * 64


def test_segment_bytes_match_hand_computed_sizes():
    """B = 2, 32x48, two source views.  Per plane: x 32 floats per pixel; z the five cells' 4 hid
    gate values at their resolutions; u the two deconv outputs (16 channels at 1/4 and 1 of the
    pixels); stats [B][4][kSlots][2] doubles; t1 4 floats and ostats [B][3][kSlots][2] doubles
    per view.  State: h and c of the five cells (hid 16, 16, 16, 16, 8 at 1, 1/4, 1/16, 1/4, 1 of
    the pixels): 264 B per pixel.  Every section is a multiple of 64 floats here."""
    from aarmvs import lib, ops
    L = lib()
    B, H, W, nsrc = 2, 32, 48, 2
    px = B * H * W
    cells = [(16, px), (16, px // 4), (16, px // 16), (16, px // 4), (8, px)]
    x = px * 32 * 4
    state = sum(2 * _al64(hid * n) for hid, n in cells) * 4
    z = sum(_al64(4 * hid * n) for hid, n in cells) * 4
    u = (_al64(16 * px // 4) + _al64(16 * px)) * 4
    assert state == 264 * px and x == 128 * px and z == 528 * px and u == 80 * px
    stats = L.aarmvs_train_record_bytes(B, H, W, 4)
    ostats = L.aarmvs_train_record_bytes(B, H, W, 6)
    assert stats % (B * 4 * 2 * 8) == 0 and ostats * 4 == stats * 3   # [B][4] against [B][3] slots
    t1 = px * 16
    for planes in (1, 16, 40):
        rec, ck = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert L.aarmvs_train_segment_bytes(B, H, W, nsrc, planes, ctypes.byref(rec), ctypes.byref(ck)) == 0
        want = planes * (x + z + u + stats) + (planes + 1) * state + planes * nsrc * (t1 + ostats)
        assert rec.value == want and ck.value == state
        assert ops.DepthSweep.record_bytes(B, H, W, planes, nsrc=nsrc) == (want, state)
        assert sum(ops.DepthSweep._record_sizes(B, H, W, planes, nsrc).values()) == want
    # either output may be omitted; bad arguments are refused with a message
    only = ctypes.c_size_t(0)
    assert L.aarmvs_train_segment_bytes(B, H, W, nsrc, 16, None, ctypes.byref(only)) == 0 and only.value == state
    assert L.aarmvs_train_segment_bytes(B, H, W, nsrc, 0, ctypes.byref(only), None) == INVALID
    assert "planes" in _err()
    assert L.aarmvs_train_segment_bytes(B, 30, W, nsrc, 16, ctypes.byref(only), None) == INVALID
    assert "multiples of 4" in _err()
    # the figures of the issue: config 4's record and the evaluation frame's
    gb4 = ops.DepthSweep.record_bytes(1, 512, 640, 192, nsrc=2)[0] / 1e9
    gbe = ops.DepthSweep.record_bytes(1, 1184, 1600, 192, nsrc=2)[0] / 1e9
    assert 60 < gb4 < 70 and 350 < gbe < 400


def test_checkpoint_planes_must_be_a_multiple_of_16():
    from models import EMVSNet
    for bad in (24, 8, -16):
        with pytest.raises(ValueError, match="multiple of 16"):
            EMVSNet(disparity_level=48, evidential=False, checkpoint_planes=bad)
    assert EMVSNet(disparity_level=48, evidential=False).checkpoint_planes == 0
    assert EMVSNet(disparity_level=48, evidential=False, checkpoint_planes=32).checkpoint_planes == 32


def test_train_ddp_takes_checkpoint_planes():
    from aarmvs import train_ddp
    src = open(train_ddp.__file__).read()
    assert "--checkpoint_planes" in src and "checkpoint_planes=args.checkpoint_planes" in src
