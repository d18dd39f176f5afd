"""GPU tests of plane-segment checkpointing of the training sweep's BPTT.

The reference of every comparison is the whole-record path (one recorded aarmvs_sweep over all D
planes, one aarmvs_sweep_backward on its record; EMVSNet() with checkpoint_planes = 0), never the
code under test.  Comparisons are torch.equal: the segment forward writes the whole record's
slabs, the ranged backward runs the whole backward's 16-plane groups and carries everything
between its calls in fixed-order accumulators, so the bits must match.  The one exception is
FeatNet's parameter gradients at the model level (MIOpen's backward is not pinned bitwise):
assert_close at torch's float32 defaults (rtol 1.3e-6, atol 1e-5).
"""
import functools
import os

import numpy as np
import pytest
import torch

from aarmvs import synthetic as syn

import geometry_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLABBED = ("x", "state", "z", "u", "stats", "t1", "ostats")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _slab_bytes(B, H, W, nsrc):
    """bytes per plane of each record buffer (t1 / ostats: all views of the plane)"""
    from aarmvs import lib
    L = lib()
    return {k: L.aarmvs_train_record_bytes(B, H, W, i) * (nsrc if k in ("t1", "ostats") else 1)
            for i, k in enumerate(SLABBED)}


def _zeroed_record(sw, B, H, W, D, nsrc, planes=None):
    rec = sw.record_buffers(B, H, W, D, DEV, nsrc=nsrc, planes=planes)
    for t in rec.values():   # (alignment padding is never written)
        t.zero_()
    return rec


@functools.lru_cache(maxsize=None)
def _whole(shape, kind=None):
    """The whole-record forward and backward of a shape (the reference), computed once."""
    from aarmvs import ops
    B, N, H, W, D = shape
    sc = syn.scene(B, N, H, W, D, seed=31)
    P = {k: torch.from_numpy(v).to(DEV) for k, v in syn.sweep_weights(6).items()}
    proj = torch.from_numpy(sc["proj_matrices"])
    if kind is not None:
        proj = gc.apply(proj, [(0, 1, kind)], H, W)
    dv = torch.from_numpy(sc["depth_values"])
    fd = torch.from_numpy(sc["features"]).to(DEV)
    sw = ops.DepthSweep(P, DEV)
    ref, srcs = fd[0], [fd[v] for v in range(1, N)]
    ref_proj, src_projs = proj[:, 0], [proj[:, v] for v in range(1, N)]
    rel = sw.relative(ref_proj, src_projs, B)
    rec = _zeroed_record(sw, B, H, W, D, N - 1)
    cost = torch.empty(B, D, H, W, device=DEV)
    sw(ref, srcs, ref_proj, src_projs, dv, want_depth=False, cost_out=cost, rel=rel, record=rec)
    gcost = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
    g_ref, g_src, g_par, g_x = sw.backward(ref, srcs, rel, dv, rec, gcost, want_grad_x=True)
    torch.cuda.synchronize()
    return dict(P=P, ref=ref, srcs=srcs, ref_proj=ref_proj, src_projs=src_projs, dv=dv, rel=rel, rec=rec,
                cost=cost, gcost=gcost, g_ref=g_ref, g_src=g_src, g_par=g_par, g_x=g_x, fd=fd)


def _segment_forward(sw, w, shape, seg, s0, s1, cost):
    """planes [s0, s1) recorded into the segment record `seg`, from the whole record's state"""
    B, N, H, W, D = shape
    slab = _slab_bytes(B, H, W, N - 1)["state"]
    seg["state"][:slab].copy_(w["rec"]["state"][s0 * slab:(s0 + 1) * slab])
    sw(w["ref"], w["srcs"], w["ref_proj"], w["src_projs"], w["dv"], want_depth=False, cost_out=cost,
       rel=w["rel"], record=seg, record_d0=s0, d_range=(s0, s1))


def test_segment_forward_writes_the_whole_records_slabs():
    """B=2, N=3, 32x48, D=40: planes [16, 32) into a 16-plane record whose state slab 0 is the whole
    record's slab 16.  The cost planes, every slab (16..31) and the state slabs (16..32) equal the
    whole record's; again after an unrelated sweep (other features, from plane 0) has used the
    same DepthSweep and its workspace in between."""
    from aarmvs import ops
    shape = (2, 3, 32, 48, 40)
    B, N, H, W, D = shape
    w = _whole(shape)
    sw = ops.DepthSweep(w["P"], DEV)
    sizes = _slab_bytes(B, H, W, N - 1)
    other = torch.from_numpy(syn.scene(B, N, H, W, D, seed=77)["features"]).to(DEV)
    for unrelated_first in (False, True):
        if unrelated_first:
            sw(other[0], [other[1], other[2]], w["ref_proj"], w["src_projs"], w["dv"], want_cost=True)
        seg = _zeroed_record(sw, B, H, W, D, N - 1, planes=16)
        cost = torch.zeros(B, D, H, W, device=DEV)
        _segment_forward(sw, w, shape, seg, 16, 32, cost)
        torch.cuda.synchronize()
        assert torch.equal(cost[:, 16:32], w["cost"][:, 16:32]), unrelated_first
        assert not cost[:, :16].any() and not cost[:, 32:].any()
        for k, n in sizes.items():
            slabs = 17 if k == "state" else 16
            assert seg[k].numel() >= slabs * n
            assert torch.equal(seg[k][:slabs * n], w["rec"][k][16 * n:(16 + slabs) * n]), (k, unrelated_first)


def _ranged_backward(shape, S, kind=None):
    """The backward of `shape` as a chain of ranged calls on S-plane segment records (each
    segment's forward recomputed from the whole record's state), against the whole backward."""
    from aarmvs import ops
    B, N, H, W, D = shape
    w = _whole(shape, kind)
    sw = ops.DepthSweep(w["P"], DEV)
    seg = _zeroed_record(sw, B, H, W, D, N - 1, planes=min(S, D))
    gx = torch.zeros(D, B, H, W, 32, device=DEV)
    segs = [(s0, min(s0 + S, D)) for s0 in range(0, D, S)]
    out = None
    for s0, s1 in reversed(segs):
        assert out is None   # only the final call returns gradients
        _segment_forward(sw, w, shape, seg, s0, s1, None)
        out = sw.backward(w["ref"], w["srcs"], w["rel"], w["dv"], seg, w["gcost"], d_range=(s0, s1),
                          record_d0=s0, grad_x_out=gx)
    torch.cuda.synchronize()
    g_ref, g_src, g_par, g_x = out
    assert g_x is gx
    assert torch.equal(g_ref, w["g_ref"])
    for v in range(N - 1):
        assert torch.equal(g_src[v], w["g_src"][v]), v
    for k, g in w["g_par"].items():
        assert torch.equal(g_par[k], g), k
    assert torch.equal(gx, w["g_x"])
    assert float(w["g_ref"].abs().max()) > 0 and float(w["g_x"].abs().max()) > 0
    return sw, w, seg


@pytest.mark.parametrize("S", [16, 32])
def test_ranged_backward_equals_the_whole_backward(S):
    """B=2, N=3, 32x48, D=40, seeded dL/dcost: [32,40), [16,32), [0,16) (S=16) and [32,40), [0,32)
    (S=32) on segment records: grad_ref, every grad_src, every parameter gradient and grad_x."""
    _ranged_backward((2, 3, 32, 48, 40), S)


def test_ranged_backward_refuses_calls_out_of_order():
    """A range that does not end at D must continue the call before it on the same DepthSweep."""
    from aarmvs import ops
    from aarmvs._lib import AarmvsError
    shape = (2, 3, 32, 48, 40)
    B, N, H, W, D = shape
    w = _whole(shape)
    sw = ops.DepthSweep(w["P"], DEV)
    seg = _zeroed_record(sw, B, H, W, D, N - 1, planes=16)
    args = (w["ref"], w["srcs"], w["rel"], w["dv"], seg, w["gcost"])
    _segment_forward(sw, w, shape, seg, 16, 32, None)
    with pytest.raises(AarmvsError, match="does not continue"):   # nothing before it
        sw.backward(*args, d_range=(16, 32), record_d0=16)
    _segment_forward(sw, w, shape, seg, 32, 40, None)
    assert sw.backward(*args, d_range=(32, 40), record_d0=32) is None
    _segment_forward(sw, w, shape, seg, 0, 16, None)
    with pytest.raises(AarmvsError, match="does not continue"):   # skips [16, 32)
        sw.backward(*args, d_range=(0, 16), record_d0=0)
    with pytest.raises(AarmvsError, match="does not cover"):      # the record holds [0, 16)
        sw.backward(*args, d_range=(32, 40), record_d0=0)
    with pytest.raises(AarmvsError, match="misaligned"):          # (on the whole record)
        sw.backward(w["ref"], w["srcs"], w["rel"], w["dv"], w["rec"], w["gcost"], d_range=(8, 40))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 3, 64, 96, 36), (1, 3, 256, 320, 36)])
def test_ranged_backward_under_both_stream_schedules(shape):
    """S=16 at 64x96 (the small-frame schedule: cost stage on the caller's stream) and at 256x320
    (more than 65,536 px: the cost stage on the aux stream), D=36: [32,36), [16,32), [0,16)."""
    _ranged_backward(shape, 16)


@pytest.mark.parametrize("S", [16, 32])
def test_ranged_backward_under_minifying_geometry(S):
    """Source view 1 under tests/geometry_cases.py's `minify` (overflowing gather cells, the
    fixed-point atomic path) at the 36x52 of that file's users, D=40: still bit-equal, since
    those sums do not depend on their order."""
    _ranged_backward((1, 3, 36, 52, 40), S, kind="minify")


# -- model level -----------------------------------------------------------------------------
MODEL_SHAPE = (1, 3, 32, 48, 40)


def _model(like=None, **kw):
    from models import EMVSNet
    B, N, H, W, D = MODEL_SHAPE
    torch.manual_seed(11)
    m = EMVSNet(D, image_scale=1.0, max_h=H, max_w=W, evidential=False, **kw)
    if like is not None:
        m.load_state_dict(like.state_dict(), strict=True)
    return m.to(DEV).train()


def _sample(seed):
    B, N, H, W, D = MODEL_SHAPE
    sc = syn.scene(B, N, H, W, D, seed=seed)
    imgs = torch.randn(B, N, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
    gt, mask = (torch.from_numpy(a).to(DEV) for a in syn.depth_targets(sc["depth_values"], H, W, seed=seed))
    return imgs, torch.from_numpy(sc["proj_matrices"]).to(DEV), torch.from_numpy(sc["depth_values"]).to(DEV), gt, mask


def _loss(model, sample):
    from models import mvsnet_cls_loss, mvsnet_cls_loss_from_cost
    imgs, proj, dv, gt, mask = sample
    out = model(imgs, proj, dv)[0]
    return (mvsnet_cls_loss_from_cost if model.return_cost else mvsnet_cls_loss)(out, gt, mask, dv)[0]


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _assert_same_grads(got, want):
    assert set(got) == set(want)
    assert any(k.startswith("omega.") for k in want) and any(k.startswith("feature.") for k in want)
    for k, g in want.items():
        if k.startswith(("omega.", "cost_regularization.")):
            assert torch.equal(got[k], g), k
        else:
            torch.testing.assert_close(got[k], g, msg=lambda m, k=k: f"{k}: {m}")


@functools.lru_cache(maxsize=None)
def _model_reference(return_cost):
    """loss and gradients of the un-checkpointed model on sample 21 (the reference of the
    model-level tests)"""
    m = _model(return_cost=return_cost)
    loss = _loss(m, _sample(21))
    loss.backward()
    torch.cuda.synchronize()
    return m, loss.detach().clone(), _grads(m)


@pytest.mark.parametrize("return_cost", [False, True])
@pytest.mark.parametrize("S", [16, 48])
def test_model_with_checkpointing_equals_the_whole_record_model(S, return_cost):
    """EMVSNet(checkpoint_planes=S) against EMVSNet() with equal weights and images at 1x3x32x48,
    D=40, mvsnet_cls_loss (or mvsnet_cls_loss_from_cost on return_cost=True) on seeded gt and
    mask: S=16 is three segments, S=48 one segment (S >= D).  The losses and every omega.* and
    cost_regularization.* gradient are equal; FeatNet's are close at float32 tolerances."""
    m0, loss0, g0 = _model_reference(return_cost)
    m = _model(like=m0, return_cost=return_cost, checkpoint_planes=S)
    loss = _loss(m, _sample(21))
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), loss0)
    _assert_same_grads(_grads(m), g0)


def test_two_forwards_then_one_backward_of_the_summed_loss():
    """Two samples through one checkpointed model (each forward keeps its own 16-plane record and
    checkpoints; both share the DepthSweep's workspace and backward scratch), one backward of the
    summed loss: the un-checkpointed model's gradients."""
    m0 = _model()
    (_loss(m0, _sample(21)) + _loss(m0, _sample(22))).backward()
    m = _model(like=m0, checkpoint_planes=16)
    la, lb = _loss(m, _sample(21)), _loss(m, _sample(22))
    (la + lb).backward()
    torch.cuda.synchronize()
    assert torch.equal(la.detach(), _model_reference(False)[1])
    _assert_same_grads(_grads(m), _grads(m0))


def test_second_backward_through_a_retained_graph_repeats_the_first():
    """After a backward the record holds segment 0, not the last segment: a second backward
    through the retained graph recomputes it and gives the same gradients (never a stale read)."""
    _, _, g0 = _model_reference(False)
    m = _model(like=_model_reference(False)[0], checkpoint_planes=16)
    loss = _loss(m, _sample(21))
    loss.backward(retain_graph=True)
    first = _grads(m)
    m.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    second = _grads(m)
    _assert_same_grads(first, g0)
    for k, g in first.items():
        if k.startswith(("omega.", "cost_regularization.")):
            assert torch.equal(second[k], g), k
    with pytest.raises(RuntimeError):   # the graph is freed now: autograd's own error
        loss.backward()


def test_checkpointing_saves_the_records_memory():
    """1x3x64x96, D=64, S=16: max_memory_allocated over one forward + backward, reset before each
    variant (after one warm-up step, so that the sweep's workspace and scratch exist).  With
    Delta = record(D) - record(S) - 4 checkpoints from the size helper and m =
    max_memory_allocated over a checkpointed step with S = D (allocator rounding and the extra
    saved tensors), the bound is peak(off) - peak(S=16) >= Delta - m.  (m is a whole step's peak,
    so the bound is loose; the figures are printed.  On an MI355X: Delta 298,106,880 B, saved
    299,032,576 B, 1.003 of Delta.)"""
    from aarmvs import ops
    from models import EMVSNet, mvsnet_cls_loss
    B, N, H, W, D, S = 1, 3, 64, 96, 64, 16
    sc = syn.scene(B, N, H, W, D, seed=5)
    imgs = torch.randn(B, N, 3, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
    proj, dv = torch.from_numpy(sc["proj_matrices"]).to(DEV), torch.from_numpy(sc["depth_values"]).to(DEV)
    gt, mask = (torch.from_numpy(a).to(DEV) for a in syn.depth_targets(sc["depth_values"], H, W, seed=5))

    def peak(ckpt):
        torch.manual_seed(3)
        m = EMVSNet(D, image_scale=1.0, max_h=H, max_w=W, evidential=False, checkpoint_planes=ckpt).to(DEV).train()

        def step():
            m.zero_grad(set_to_none=True)
            mvsnet_cls_loss(m(imgs, proj, dv)[0], gt, mask, dv)[0].backward()

        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated()
        del m
        torch.cuda.empty_cache()
        return p

    p_off, p_s, m_full = peak(0), peak(S), peak(D)
    rec_d, ck = ops.DepthSweep.record_bytes(B, H, W, D, nsrc=N - 1)
    rec_s, _ = ops.DepthSweep.record_bytes(B, H, W, S, nsrc=N - 1)
    delta = rec_d - rec_s - 4 * ck
    print(f"\npeak off {p_off} B, S={S} {p_s} B, S=D {m_full} B; record(D) {rec_d} B, record(S) {rec_s} B, "
          f"checkpoint {ck} B; Delta {delta} B, saved {p_off - p_s} B ({(p_off - p_s) / delta:.3f} of Delta)")
    assert delta > 0
    assert p_off - p_s >= delta - m_full
