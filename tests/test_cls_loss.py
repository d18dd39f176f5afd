"""CPU checks of the loss-from-cost path: host-side argument rejection of the new C-ABI entries
(no device work, so they run here), the ``return_cost`` constructor keyword, the refusal of CPU
tensors, and the fixture's input digests."""
import os

import numpy as np
import pytest
import torch

import cls_loss_cases as cases
from conftest import GOLDEN

FAKE = 0x1000   # never dereferenced: validation fails first


def test_cls_loss_scratch_query_is_host_only():
    from aarmvs import lib
    from aarmvs import _lib
    L = lib()
    one = L.aarmvs_cls_loss_scratch_bytes(1, 256)
    assert one == 10 * 8 and L.aarmvs_cls_loss_scratch_bytes(1, 257) == 2 * one
    assert L.aarmvs_cls_loss_scratch_bytes(3, 640 * 512) == 3 * 1280 * one
    for B, HW in ((0, 64), (1, 0), (-1, 64), (1, -5), (65536, 64)):
        assert L.aarmvs_cls_loss_scratch_bytes(B, HW) == 0
        assert L.aarmvs_last_error()
    assert "aarmvs_cls_loss_scratch_bytes" in _lib.SIGNATURES


def test_cls_loss_rejects_bad_arguments_before_launching():
    from aarmvs import lib
    L = lib()
    ok = [FAKE] * 4 + [1, 4, 64] + [FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, None]
    for i in (0, 1, 2, 3, 7, 8, 10, 11, 12, 13):   # every pointer but max_prob and the stream
        a = list(ok)
        a[i] = None
        assert L.aarmvs_cls_loss(*a) != 0, i
        assert b"null" in L.aarmvs_last_error()
    for i in (4, 5, 6):                            # B, D, HW < 1
        a = list(ok)
        a[i] = 0
        assert L.aarmvs_cls_loss(*a) != 0, i
        assert b">= 1" in L.aarmvs_last_error()


def test_cls_loss_backward_rejects_bad_arguments_before_launching():
    from aarmvs import lib
    L = lib()
    ok = [FAKE] * 6 + [1, 4, 64] + [FAKE, None]
    for i in (0, 1, 2, 3, 4, 5, 9):
        a = list(ok)
        a[i] = None
        assert L.aarmvs_cls_loss_backward(*a) != 0, i
        assert b"null" in L.aarmvs_last_error()
    for i in (6, 7, 8):
        a = list(ok)
        a[i] = 0
        assert L.aarmvs_cls_loss_backward(*a) != 0, i
        assert b">= 1" in L.aarmvs_last_error()


def test_depth_metrics_rejects_bad_arguments_before_launching():
    import ctypes
    from aarmvs import lib
    L = lib()
    thr = (ctypes.c_float * 9)(*range(1, 10))
    ok = [FAKE] * 3 + [1, 64, thr, 5, FAKE, FAKE, None]
    for i in (0, 1, 2, 5, 7, 8):
        a = list(ok)
        a[i] = None
        assert L.aarmvs_depth_metrics(*a) != 0, i
        assert b"null" in L.aarmvs_last_error()
    for i in (3, 4):
        a = list(ok)
        a[i] = 0
        assert L.aarmvs_depth_metrics(*a) != 0, i
        assert b">= 1" in L.aarmvs_last_error()
    a = list(ok)
    a[6] = 9
    assert L.aarmvs_depth_metrics(*a) != 0
    assert b"8 thresholds" in L.aarmvs_last_error()


def test_profile_table_names_the_new_kernels():
    from aarmvs import lib
    L = lib()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    for n in ("cls_loss_fwd", "cls_loss_reduce", "cls_loss_bwd", "depth_metrics"):
        assert n in names


def test_return_cost_keeps_the_checkpoint_keys():
    import json
    from models import EMVSNet
    with open(os.path.join(GOLDEN, "ckpt_layout.json")) as f:
        layout = json.load(f)["keys"]
    m = EMVSNet(disparity_level=48, evidential=False, return_cost=True)
    assert m.return_cost is True and m.return_depth is False
    sd = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert sd == layout and len(sd) == 90
    assert EMVSNet(disparity_level=48, evidential=False).return_cost is False


def test_loss_from_cost_refuses_cpu_tensors():
    import models
    from aarmvs import AarmvsError, ops
    import models.drmvsnet as drm
    assert "mvsnet_cls_loss_from_cost" in drm.__all__
    inp = {k: torch.from_numpy(v) for k, v in cases.build("d5_4x4").items()}
    with pytest.raises(AarmvsError):
        models.mvsnet_cls_loss_from_cost(inp["cost"], inp["depth_gt"], inp["mask"], inp["depth_values"])
    with pytest.raises(AarmvsError):
        ops.depth_metrics(inp["depth_gt"], inp["depth_gt"], inp["mask"])


def test_fixture_inputs_match_their_digests():
    """The seeded inputs regenerate bit for bit (numpy PCG64): the reference outputs in
    cls_loss.npz belong to the inputs the GPU tests run."""
    from aarmvs import synthetic as syn
    z = np.load(os.path.join(GOLDEN, "cls_loss.npz"), allow_pickle=False)
    assert {k.split("/")[0] for k in z.files} == set(cases.CASES)
    for name in cases.CASES:
        inp = cases.build(name)
        assert all(v.dtype == np.float32 for v in inp.values())
        assert syn.array_digest(*(inp[k] for k in sorted(inp))) == str(z[f"{name}/digest"]), name


def test_train_driver_parses_the_new_flags():
    from aarmvs import train_ddp
    a = train_ddp.parse_args([])
    assert a.fused_loss is False and a.testpath is None and a.testlist is None and a.test_light_idx == 3
    a = train_ddp.parse_args(["--fused_loss", "--testpath", "x", "--testlist", "y", "--test_light_idx", "5"])
    assert a.fused_loss is True and (a.testpath, a.testlist, a.test_light_idx) == ("x", "y", 5)
