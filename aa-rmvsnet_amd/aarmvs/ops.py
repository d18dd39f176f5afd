"""Torch-facing wrappers of the HIP depth-sweep library.

Tensors stay on the device (PyTorch's caching allocator owns every buffer);
launches go to ``torch.cuda.current_stream()``.  All functions raise
``AarmvsError`` for CPU tensors or when libaarmvs.so is missing: the product
path has no CPU fallback.
"""
from __future__ import annotations

import ctypes
import functools

import torch

from . import _lib
from ._lib import AarmvsError, check, lib
from .synthetic import SWEEP_SHAPES

SWEEP_KEYS = tuple(SWEEP_SHAPES.keys())  # raw-blob order (include/aarmvs.h)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _device_of(args, kwargs):
    for a in list(args) + list(kwargs.values()):
        if isinstance(a, DepthSweep):
            return a.device
        if torch.is_tensor(a) and a.is_cuda:
            return a.device
        if isinstance(a, torch.device):
            return a
    return None


def _on_tensor_device(fn):
    """Runs ``fn`` with the current device set to its first device tensor's (or its
    DepthSweep's) device, so ``_stream()`` is that device's current stream and the library's
    hipGetDevice() agrees with the tensors, whatever device the caller left current."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = _device_of(args, kwargs)
        if dev is None or dev.type != "cuda" or dev.index is None:
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _home(t: torch.Tensor) -> torch.Tensor:
    """Marks a cached buffer with the stream it was allocated under (``_use`` compares with it)."""
    t._aarmvs_stream = torch.cuda.current_stream(t.device)
    return t


def _use(t: torch.Tensor) -> torch.Tensor:
    """A cached buffer about to be used on the current stream.  The caching allocator returns a
    freed block to the pool of the stream it was allocated under and hands it out again at once
    there; used under another stream, the buffer is recorded on that stream, so that a block
    dropped while work is queued on it is reused only after that work."""
    s = torch.cuda.current_stream(t.device)
    if s != getattr(t, "_aarmvs_stream", None):   # (a buffer of unknown origin: recorded too)
        t.record_stream(s)
    return t


def _require_device(*ts: torch.Tensor) -> None:
    for t in ts:
        if not t.is_cuda:
            raise AarmvsError("aarmvs: the HIP sweep needs ROCm device tensors (got a CPU tensor); "
                              "there is no CPU fallback")
        if t.dtype != torch.float32:
            raise AarmvsError(f"aarmvs: expected float32 tensors, got {t.dtype}")


def _check_proj(p: torch.Tensor, B: int, what: str) -> None:
    if tuple(p.shape) != (B, 4, 4):
        raise AarmvsError(f"aarmvs: {what} must be [B={B},4,4], got {tuple(p.shape)}")


def relative_projection(src_proj: torch.Tensor, ref_proj: torch.Tensor) -> torch.Tensor:
    """rows 0..2 of src_proj @ inverse(ref_proj) (module.py:16-18), [B,3,4] fp32.

    Computed on the host in fp32, exactly as the reference's CPU path does; the
    4x4 matrices are tiny and this keeps the sampling grid bit-compatible.
    """
    s = src_proj.detach().float().cpu()
    r = ref_proj.detach().float().cpu()
    return torch.matmul(s, torch.inverse(r))[:, :3, :4].contiguous()


def pack_params(params: dict, device) -> torch.Tensor:
    """Flatten the sweep tensors (checkpoint keys) and pack them on the device."""
    missing = [k for k in SWEEP_KEYS if k not in params]
    if missing:
        raise KeyError(f"aarmvs.pack_params: missing parameters {missing[:3]}...")
    return pack_flat([params[k] for k in SWEEP_KEYS], device)


@_on_tensor_device
def pack_flat(tensors, device) -> torch.Tensor:
    """``pack_params`` of the sweep tensors given in SWEEP_KEYS order: a NEW packed buffer holding
    their values as of this call on the current stream (one concatenation and one pack kernel,
    both asynchronous; later in-place changes to the tensors do not reach it).  EMVSNet calls
    this on every forward, so the per-tensor host work is one reshape each."""
    with torch.no_grad():
        raw = torch.cat([t.reshape(-1) for t in tensors]).to(device, torch.float32)
    if raw.numel() != lib().aarmvs_param_count():
        raise AarmvsError("aarmvs.pack_params: parameter count mismatch with libaarmvs")
    nbytes = lib().aarmvs_packed_param_bytes()
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    check(lib().aarmvs_pack_params(raw.data_ptr(), packed.data_ptr(), _stream()), "pack_params")
    packed._aarmvs_raw = raw  # keep the source alive until the async pack has run
    return _home(packed)


@_on_tensor_device
def homo_warp(src_fea: torch.Tensor, rel: torch.Tensor, depth: torch.Tensor) -> torch.Tensor:
    """homo_warping_depthwise on the GPU for precomputed rel [B,3,4] and depth [B]."""
    _require_device(src_fea)
    src = src_fea.contiguous()
    B, C, H, W = src.shape
    rel_d = rel.reshape(B, 12).to(src.device, torch.float32).contiguous()
    dep = depth.reshape(B).to(src.device, torch.float32).contiguous()
    out = torch.empty_like(src)
    check(lib().aarmvs_homo_warp(src.data_ptr(), rel_d.data_ptr(), dep.data_ptr(), B, C, H, W,
                                 out.data_ptr(), _stream()), "homo_warp")
    return out


@_on_tensor_device
def homo_warp_backward(grad_out: torch.Tensor, rel: torch.Tensor, depth: torch.Tensor,
                       src_shape) -> torch.Tensor:
    """d loss / d src_fea of homo_warp: bilinear scatter-add of grad_out, summed in 64-bit fixed
    point (bit-reproducible, aarmvs_homo_warp_backward; fp32 atomics for a batch element whose
    grad_out is not finite).  Workspace: min(B, 64) * C * H * W * 8 bytes + 256."""
    _require_device(grad_out)
    g = grad_out.contiguous()
    B, C, H, W = src_shape
    rel_d = rel.reshape(B, 12).to(g.device, torch.float32).contiguous()
    dep = depth.reshape(B).to(g.device, torch.float32).contiguous()
    grad_src = torch.zeros(B, C, H, W, device=g.device)
    n = lib().aarmvs_homo_warp_backward_workspace_bytes(B, C, H, W)
    if n == 0:
        raise AarmvsError(f"aarmvs: homo_warp_backward geometry B={B} C={C} H={H} W={W}")
    ws = torch.empty(n, dtype=torch.uint8, device=g.device)
    check(lib().aarmvs_homo_warp_backward(g.data_ptr(), rel_d.data_ptr(), dep.data_ptr(), B, C, H,
                                          W, grad_src.data_ptr(), ws.data_ptr(), _stream()),
          "homo_warp_backward")
    return grad_src


class _GroupNormHip(torch.autograd.Function):
    """GroupNorm on NCHW fp32 device tensors through aarmvs_group_norm_forward/_backward
    (fixed-order fp64 statistics).  Once differentiable (no double backward)."""

    @staticmethod
    @_on_tensor_device
    def forward(ctx, x, weight, bias, groups: int, eps: float):
        _require_device(x)
        xc = x.contiguous()
        B, C = xc.shape[:2]
        HW = xc[0, 0].numel()
        y = torch.empty_like(xc)
        mr = torch.empty(B, groups, 2, device=xc.device)
        scratch = torch.empty(lib().aarmvs_group_norm_scratch_bytes(B, C, HW), dtype=torch.uint8,
                              device=xc.device)
        w = weight.contiguous() if weight is not None else None
        bb = bias.contiguous() if bias is not None else None
        check(lib().aarmvs_group_norm_forward(xc.data_ptr(), w.data_ptr() if w is not None else None,
                                              bb.data_ptr() if bb is not None else None, B, C, HW,
                                              groups, float(eps), y.data_ptr(), mr.data_ptr(),
                                              scratch.data_ptr(), _stream()), "group_norm_forward")
        ctx.save_for_backward(xc, w if w is not None else xc.new_empty(0), mr)
        ctx.groups, ctx.has_w, ctx.has_b = groups, w is not None, bb is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    @_on_tensor_device
    def backward(ctx, gy):
        xc, w, mr = ctx.saved_tensors
        g = gy.contiguous()
        B, C = xc.shape[:2]
        HW = xc[0, 0].numel()
        dx = torch.empty_like(xc)
        s1 = torch.empty(B, C, device=xc.device)
        s2 = torch.empty(B, C, device=xc.device)
        scratch = torch.empty(lib().aarmvs_group_norm_scratch_bytes(B, C, HW), dtype=torch.uint8,
                              device=xc.device)
        check(lib().aarmvs_group_norm_backward(g.data_ptr(), xc.data_ptr(),
                                               w.data_ptr() if ctx.has_w else None, mr.data_ptr(),
                                               B, C, HW, ctx.groups, dx.data_ptr(), s1.data_ptr(),
                                               s2.data_ptr(), scratch.data_ptr(), _stream()),
              "group_norm_backward")
        dw = s1.sum(0) if ctx.has_w else None
        db = s2.sum(0) if ctx.has_b else None
        return dx, dw, db, None, None


class _LstmGatesHip(torch.autograd.Function):
    """ConvLSTMCell gates (module.py:83-90) on the HIP kernels: (z, c_prev) -> (h, c)."""

    @staticmethod
    @_on_tensor_device
    def forward(ctx, z, c_prev):
        _require_device(z, c_prev)
        zc, cp = z.contiguous(), c_prev.contiguous()
        B, C4 = zc.shape[:2]
        hid = C4 // 4
        HW = zc[0, 0].numel()
        if C4 != 4 * hid or tuple(cp.shape) != (B, hid) + tuple(zc.shape[2:]):
            raise AarmvsError(f"aarmvs.lstm_gates: z {tuple(zc.shape)} vs c {tuple(cp.shape)}")
        h = torch.empty_like(cp)
        c = torch.empty_like(cp)
        check(lib().aarmvs_lstm_gates_forward(zc.data_ptr(), cp.data_ptr(), B, hid, HW, h.data_ptr(),
                                              c.data_ptr(), _stream()), "lstm_gates_forward")
        ctx.save_for_backward(zc, cp)
        return h, c

    @staticmethod
    @torch.autograd.function.once_differentiable
    @_on_tensor_device
    def backward(ctx, dh, dc):
        zc, cp = ctx.saved_tensors
        B, C4 = zc.shape[:2]
        hid, HW = C4 // 4, zc[0, 0].numel()
        dh = dh.contiguous() if dh is not None else None
        dc = dc.contiguous() if dc is not None else None
        dz = torch.empty_like(zc)
        dcp = torch.empty_like(cp)
        check(lib().aarmvs_lstm_gates_backward(zc.data_ptr(), cp.data_ptr(),
                                               dh.data_ptr() if dh is not None else None,
                                               dc.data_ptr() if dc is not None else None, B, hid, HW,
                                               dz.data_ptr(), dcp.data_ptr(), _stream()),
              "lstm_gates_backward")
        return dz, dcp


def lstm_gates(z: torch.Tensor, c_prev: torch.Tensor):
    """(h, c) = ConvLSTMCell's gate math on the conv output z [B,4*hid,H,W] and c_prev
    [B,hid,H,W] (fp32 device tensors), forward and backward on the HIP kernels."""
    return _LstmGatesHip.apply(z, c_prev)


def group_norm(x: torch.Tensor, groups: int, weight=None, bias=None, eps: float = 1e-5):
    """F.group_norm(x, groups, weight, bias, eps) for fp32 device tensors on the HIP kernels
    (forward and backward)."""
    if x.dtype != torch.float32:
        raise AarmvsError(f"aarmvs.group_norm: expected float32, got {x.dtype}")
    return _GroupNormHip.apply(x, weight, bias, groups, eps)


@_on_tensor_device
def softmax_depth(cost: torch.Tensor) -> torch.Tensor:
    _require_device(cost)
    c = cost.contiguous()
    B, D = c.shape[:2]
    out = torch.empty_like(c)
    check(lib().aarmvs_softmax_depth(c.data_ptr(), out.data_ptr(), B, D, c[0, 0].numel(),
                                     _stream()), "softmax_depth")
    return out


def _cls_scratch(B: int, HW: int, device) -> torch.Tensor:
    n = lib().aarmvs_cls_loss_scratch_bytes(B, HW)
    if n == 0:
        raise AarmvsError(f"aarmvs: cls_loss geometry B={B} HW={HW}: "
                          + lib().aarmvs_last_error().decode(errors="replace"))
    return torch.empty(n // 8, dtype=torch.float64, device=device)


@_on_tensor_device
def cls_loss_forward(cost: torch.Tensor, depth_gt: torch.Tensor, mask: torch.Tensor,
                     depth_values: torch.Tensor, want_prob_map: bool = False) -> dict:
    """aarmvs_cls_loss on cost [B,D,H,W], depth_gt / mask [B,H,W], depth_values [B,D]: every
    output of the kernel, {'cost' (contiguous), 'mask', 'loss' (0-dim), 'wta_depth' [B,H,W],
    'max_prob' [B,H,W] or None, 'lse' [2,B,H,W], 'gt' [B,H,W] int32, 'coef' [B]}.  No autograd:
    ``cls_loss`` is the differentiable form."""
    _require_device(cost, depth_gt, mask, depth_values)
    c, gtd, mk, dv = (t.detach().contiguous() for t in (cost, depth_gt, mask, depth_values))
    if c.dim() != 4:
        raise AarmvsError(f"aarmvs: cls_loss cost must be [B,D,H,W], got {tuple(c.shape)}")
    B, D, H, W = c.shape
    if tuple(gtd.shape) != (B, H, W) or tuple(mk.shape) != (B, H, W) or tuple(dv.shape) != (B, D):
        raise AarmvsError(f"aarmvs: cls_loss shapes: cost {tuple(c.shape)}, depth_gt "
                          f"{tuple(gtd.shape)}, mask {tuple(mk.shape)}, depth_values {tuple(dv.shape)}")
    dev = c.device
    if any(t.device != dev for t in (gtd, mk, dv)):
        raise AarmvsError("aarmvs: cls_loss tensors must be on one device")
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"cost": c, "mask": mk, "loss": torch.empty((), **f32), "wta_depth": torch.empty(B, H, W, **f32),
           "max_prob": torch.empty(B, H, W, **f32) if want_prob_map else None,
           "lse": torch.empty(2, B, H, W, **f32),
           "gt": torch.empty(B, H, W, dtype=torch.int32, device=dev), "coef": torch.empty(B, **f32)}
    scratch = _cls_scratch(B, H * W, dev)
    check(lib().aarmvs_cls_loss(c.data_ptr(), gtd.data_ptr(), mk.data_ptr(), dv.data_ptr(), B, D, H * W,
                                out["loss"].data_ptr(), out["wta_depth"].data_ptr(),
                                _ptr(out["max_prob"]), out["lse"].data_ptr(), out["gt"].data_ptr(),
                                out["coef"].data_ptr(), scratch.data_ptr(), _stream()), "cls_loss")
    return out


class _ClsLoss(torch.autograd.Function):
    """loss (and the non-differentiable WTA depth / max probability) from the cost volume on
    aarmvs_cls_loss; the backward is aarmvs_cls_loss_backward (p - onehot, scaled), which reads
    the upstream gradient on the device.  Saves cost, lse, gt, mask and coef only."""

    @staticmethod
    def forward(ctx, cost, depth_gt, mask, depth_values, want_prob_map):
        o = cls_loss_forward(cost, depth_gt, mask, depth_values, want_prob_map)
        ctx.save_for_backward(o["cost"], o["lse"], o["gt"], o["mask"], o["coef"])
        outs = (o["loss"], o["wta_depth"]) + ((o["max_prob"],) if want_prob_map else ())
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, *_):
        cost, lse, gt, mask, coef = ctx.saved_tensors
        B, D, H, W = cost.shape
        g = g_loss.detach().to(cost.device, torch.float32).reshape(1).contiguous()
        grad = torch.empty_like(cost)
        with torch.cuda.device(cost.device):
            check(lib().aarmvs_cls_loss_backward(cost.data_ptr(), lse.data_ptr(), gt.data_ptr(),
                                                 mask.data_ptr(), coef.data_ptr(), g.data_ptr(), B, D,
                                                 H * W, grad.data_ptr(), _stream()), "cls_loss_backward")
        return grad, None, None, None, None


def cls_loss(cost: torch.Tensor, depth_gt: torch.Tensor, mask: torch.Tensor, depth_values: torch.Tensor,
             want_prob_map: bool = False):
    """mvsnet_cls_loss(softmax(cost, 1), depth_gt, mask, depth_values) without the probability
    volume: (loss, wta_depth[, max_prob]); ``loss`` is differentiable w.r.t. ``cost``."""
    _require_device(cost, depth_gt, mask, depth_values)
    return _ClsLoss.apply(cost, depth_gt, mask, depth_values, bool(want_prob_map))


@_on_tensor_device
def depth_metrics(depth_est: torch.Tensor, depth_gt: torch.Tensor, mask: torch.Tensor,
                  thresholds=(2, 4, 8, 16, 32)) -> dict:
    """The test pass's masked metrics (utils.py:150-175 over mask > 0.5, the mean over batch
    elements of each element's masked mean) under the reference's key names: abs_depth_error and
    thres{t}mm_error per threshold, as 0-dim float64 device tensors (no host synchronisation)."""
    _require_device(depth_est, depth_gt, mask)
    est, gtd, mk = (t.detach().contiguous() for t in (depth_est, depth_gt, mask))
    if est.dim() != 3 or gtd.shape != est.shape or mk.shape != est.shape:
        raise AarmvsError(f"aarmvs: depth_metrics needs three [B,H,W] tensors, got {tuple(est.shape)}, "
                          f"{tuple(gtd.shape)}, {tuple(mk.shape)}")
    if gtd.device != est.device or mk.device != est.device:
        raise AarmvsError("aarmvs: depth_metrics tensors must be on one device")
    thr = list(thresholds)
    if len(thr) > 8:
        raise AarmvsError(f"aarmvs: depth_metrics takes at most 8 thresholds, got {len(thr)}")
    B, H, W = est.shape
    out = torch.empty(1 + len(thr), dtype=torch.float64, device=est.device)
    scratch = _cls_scratch(B, H * W, est.device)
    check(lib().aarmvs_depth_metrics(est.data_ptr(), gtd.data_ptr(), mk.data_ptr(), B, H * W,
                                     (ctypes.c_float * max(1, len(thr)))(*thr), len(thr),
                                     out.data_ptr(), scratch.data_ptr(), _stream()), "depth_metrics")
    res = {"abs_depth_error": out[0]}
    for k, t in enumerate(thr):
        res[f"thres{t:g}mm_error"] = out[1 + k]
    return res


def _ptr3(ts) -> ctypes.Array:
    return (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])


class _EvidentialEpilogue(torch.autograd.Function):
    """The evidential head's epilogue on HIP (aarmvs_evidential_epilogue, evidential/models.py:
    385-459): the three classifier outputs [1,4,D,H,W] -> (evidential [4,H,W], prob_combine
    [1,D,H,W]); backward through aarmvs_evidential_epilogue_backward (no gradient to the depths)."""

    @staticmethod
    def forward(ctx, dv, h0, h1, h2):
        heads = [h.contiguous() for h in (h0, h1, h2)]
        _require_device(*heads)
        B, C, D, H, W = heads[0].shape
        if B != 1 or C != 4 or any(tuple(h.shape) != (1, 4, D, H, W) for h in heads):
            raise ValueError(f"evidential epilogue: heads must be [1, 4, D, H, W], got "
                             f"{[tuple(h.shape) for h in heads]}")
        dev = heads[0].device
        if any(h.device != dev for h in heads):
            raise AarmvsError("aarmvs: evidential epilogue heads must be on one device")
        if not dv.is_cuda or dv.device != dev:
            raise AarmvsError(f"aarmvs: evidential epilogue depth values must be on {dev} "
                              f"(got {dv.device}); the kernel reads them in place")
        dvc = dv.reshape(-1).float().contiguous()
        if dvc.numel() != D:
            raise ValueError(f"evidential epilogue: {dvc.numel()} depth values for D = {D}")
        ev = torch.empty(4, H, W, device=dev, dtype=torch.float32)
        pc = torch.empty(1, D, H, W, device=dev, dtype=torch.float32)
        check(lib().aarmvs_evidential_epilogue(_ptr3(heads), dvc.data_ptr(), D, H * W, ev.data_ptr(),
                                               pc.data_ptr(), _stream()), "evidential_epilogue")
        ctx.save_for_backward(dvc, *heads)
        return ev, pc

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ev, g_pc):
        dvc, *heads = ctx.saved_tensors
        D, H, W = heads[0].shape[2:]
        g_ev = g_ev.contiguous() if g_ev is not None else None
        g_pc = g_pc.contiguous() if g_pc is not None else None
        for gt in (g_ev, g_pc):
            if gt is not None:
                _require_device(gt)
                if gt.device != heads[0].device:
                    raise AarmvsError("aarmvs: evidential epilogue gradients on another device")
        gh = [torch.empty_like(h) for h in heads]
        check(lib().aarmvs_evidential_epilogue_backward(_ptr3(heads), dvc.data_ptr(), D, H * W,
                                                        _ptr(g_ev), _ptr(g_pc), _ptr3(gh), _stream()),
              "evidential_epilogue_backward")
        return (None, *gh)


class _DeformSample(torch.autograd.Function):
    """The sampling half of DeformConv2d (aarmvs_deform_sample, the reference's
    models/module.py:160-219): x NHWC [B,H,W,32], offset [B,18,h,w], mask [B,9,h,w] or None ->
    val [B,h*w,9*32], the A operand of the (tap, channel) contraction; differentiable in x,
    offset and mask."""

    @staticmethod
    def forward(ctx, x_nhwc, offset, mask, stride, pad):
        x_nhwc, offset = x_nhwc.contiguous(), offset.contiguous()
        mask = mask.contiguous() if mask is not None else None
        ts = [x_nhwc, offset] + ([mask] if mask is not None else [])
        _require_device(*ts)
        if any(t.device != x_nhwc.device for t in ts):
            raise AarmvsError("aarmvs: deform_sample tensors must be on one device")
        B, H, W, C = x_nhwc.shape
        h, w = offset.shape[2:]
        if tuple(offset.shape) != (B, 18, h, w) or (mask is not None and tuple(mask.shape) != (B, 9, h, w)):
            raise ValueError(f"deform_sample: offset / mask shapes {tuple(offset.shape)} / "
                             f"{None if mask is None else tuple(mask.shape)} for x {tuple(x_nhwc.shape)}")
        val = torch.empty(B, h * w, 9 * C, device=x_nhwc.device, dtype=torch.float32)
        check(lib().aarmvs_deform_sample(x_nhwc.data_ptr(), offset.data_ptr(), _ptr(mask), B, C, H, W,
                                         h, w, stride, pad, val.data_ptr(), _stream()), "deform_sample")
        ctx.save_for_backward(x_nhwc, offset, mask)
        ctx.geom = (stride, pad)
        return val

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_val):
        x_nhwc, offset, mask = ctx.saved_tensors
        stride, pad = ctx.geom
        g_val = g_val.contiguous()
        _require_device(g_val)
        if g_val.device != x_nhwc.device:
            raise AarmvsError("aarmvs: deform_sample gradient on another device")
        B, H, W, C = x_nhwc.shape
        h, w = offset.shape[2:]
        gx = torch.zeros_like(x_nhwc)
        goff = torch.empty_like(offset)
        gm = torch.empty_like(mask) if mask is not None else None
        check(lib().aarmvs_deform_sample_backward(x_nhwc.data_ptr(), offset.data_ptr(), _ptr(mask), B, C,
                                                  H, W, h, w, stride, pad, g_val.data_ptr(),
                                                  gx.data_ptr(), goff.data_ptr(), _ptr(gm), _stream()),
              "deform_sample_backward")
        return gx, goff, gm, None, None


@_on_tensor_device
def deform_sample(x_nhwc: torch.Tensor, offset: torch.Tensor, mask: torch.Tensor | None, stride: int = 1,
                  pad: int = 1) -> torch.Tensor:
    """val [B, h*w, 9*C] of DeformConv2d's sampling (C == 32), differentiable (see _DeformSample)."""
    return _DeformSample.apply(x_nhwc, offset, mask, int(stride), int(pad))


@_on_tensor_device
def evidential_epilogue(h0: torch.Tensor, h1: torch.Tensor, h2: torch.Tensor, depth_values: torch.Tensor):
    """(evidential [4,H,W], prob_combine [1,D,H,W]) from classif0/1/2's outputs [1,4,D,H,W]
    (D = 32), differentiable w.r.t. the three head outputs."""
    return _EvidentialEpilogue.apply(depth_values, h0, h1, h2)


@_on_tensor_device
def wta_update(cost: torch.Tensor, depth_d: torch.Tensor, max_prob: torch.Tensor,
               depth_map: torch.Tensor, exp_sum: torch.Tensor) -> None:
    """In-place online WTA update of one plane (aarmvs_wta_update, drmvsnet.py:324-334):
    cost/max_prob/depth_map/exp_sum [B,H,W] fp32 device tensors, depth_d [B]."""
    ts = (cost, max_prob, depth_map, exp_sum)
    _require_device(*ts)
    B = cost.shape[0]
    for t in ts:
        if t.shape != cost.shape or not t.is_contiguous():
            raise AarmvsError("aarmvs: wta_update needs contiguous tensors of one [B,H,W] shape")
    dep = depth_d.reshape(-1).to(cost.device, torch.float32).contiguous()
    if dep.numel() != B:
        raise AarmvsError(f"aarmvs: depth_d must hold B={B} values")
    check(lib().aarmvs_wta_update(cost.data_ptr(), dep.data_ptr(), max_prob.data_ptr(),
                                  depth_map.data_ptr(), exp_sum.data_ptr(), B, cost[0].numel(),
                                  _stream()), "wta_update")


def refine_state(B: int, HW: int, device) -> torch.Tensor:
    """A state buffer of the sub-plane refinement (aarmvs_refine_state_bytes: 16 B per pixel)."""
    n = lib().aarmvs_refine_state_bytes(B, HW)
    if n == 0:
        raise AarmvsError(f"aarmvs: refine state geometry B={B} HW={HW}")
    return torch.empty(n // 4, dtype=torch.int32, device=device)


def _check_refine_state(state: torch.Tensor, B: int, HW: int, device) -> None:
    if (not torch.is_tensor(state) or not state.is_cuda or state.device != device or not state.is_contiguous()
            or state.numel() * state.element_size() < lib().aarmvs_refine_state_bytes(B, HW)):
        raise AarmvsError(f"aarmvs: the refine state must be a contiguous tensor of {16 * B * HW} B on {device} "
                          "(ops.refine_state(B, HW, device))")


@_on_tensor_device
def wta_refine_update(cost: torch.Tensor, d: int, depth_d: torch.Tensor, max_prob: torch.Tensor,
                      depth_map: torch.Tensor, exp_sum: torch.Tensor, state: torch.Tensor) -> None:
    """``wta_update`` of plane ``d`` (planes in order from 0) that also keeps the sub-plane
    refinement's ``state`` (``refine_state(B, H*W, device)``; d == 0 resets it), in place
    (aarmvs_wta_refine_update)."""
    ts = (cost, max_prob, depth_map, exp_sum)
    _require_device(*ts)
    B = cost.shape[0]
    for t in ts:
        if t.shape != cost.shape or not t.is_contiguous() or t.device != cost.device:
            raise AarmvsError("aarmvs: wta_refine_update needs contiguous tensors of one [B,H,W] shape")
    HW = cost[0].numel()
    _check_refine_state(state, B, HW, cost.device)
    dep = depth_d.reshape(-1).to(cost.device, torch.float32).contiguous()
    if dep.numel() != B:
        raise AarmvsError(f"aarmvs: depth_d must hold B={B} values")
    if int(d) < 0:
        raise AarmvsError(f"aarmvs: plane index {d} < 0")
    check(lib().aarmvs_wta_refine_update(cost.data_ptr(), int(d), max_prob.data_ptr(), depth_map.data_ptr(),
                                         exp_sum.data_ptr(), state.data_ptr(), dep.data_ptr(), B, HW,
                                         _stream()), "wta_refine_update")


@_on_tensor_device
def wta_refine_finalize(max_prob: torch.Tensor, depth_map: torch.Tensor, exp_sum: torch.Tensor,
                        state: torch.Tensor, depth_values: torch.Tensor, n: int) -> dict:
    """{'depth_refined', 'conf_window' (float32), 'index' (int32)}, each shaped like ``max_prob``
    [B,H,W], after ``n`` planes of ``wta_refine_update`` (aarmvs_wta_refine_finalize);
    depth_values [B,D]."""
    ts = (max_prob, depth_map, exp_sum)
    _require_device(*ts)
    for t in ts:
        if t.shape != max_prob.shape or not t.is_contiguous() or t.device != max_prob.device:
            raise AarmvsError("aarmvs: wta_refine_finalize needs contiguous tensors of one [B,H,W] shape")
    B, HW = max_prob.shape[0], max_prob[0].numel()
    _check_refine_state(state, B, HW, max_prob.device)
    if depth_values.dim() != 2 or depth_values.shape[0] != B:
        raise AarmvsError(f"aarmvs: depth_values must be [B={B},D], got {tuple(depth_values.shape)}")
    dv = depth_values.to(max_prob.device, torch.float32).contiguous()
    D = dv.shape[1]
    if not 1 <= int(n) <= D:
        raise AarmvsError(f"aarmvs: n = {n} planes outside [1, D={D}]")
    out = {"depth_refined": torch.empty_like(max_prob), "conf_window": torch.empty_like(max_prob),
           "index": torch.empty(max_prob.shape, dtype=torch.int32, device=max_prob.device)}
    check(lib().aarmvs_wta_refine_finalize(max_prob.data_ptr(), depth_map.data_ptr(), exp_sum.data_ptr(),
                                           state.data_ptr(), dv.data_ptr(), B, D, int(n), HW,
                                           out["depth_refined"].data_ptr(), out["conf_window"].data_ptr(),
                                           out["index"].data_ptr(), _stream()), "wta_refine_finalize")
    return out


@_on_tensor_device
def refine_from_cost(cost: torch.Tensor, depth_values: torch.Tensor) -> dict:
    """The sub-plane refinement from a whole cost volume [B,D,H,W] and depth_values [B,D]
    (aarmvs_refine_from_cost): {'depth_refined', 'conf_window' [B,H,W] float32, 'index' [B,H,W]
    int32}, bit for bit what a sweep with ``want_refined`` gives on the same cost values."""
    _require_device(cost)
    c = cost.detach().contiguous()
    if c.dim() != 4:
        raise AarmvsError(f"aarmvs: refine_from_cost cost must be [B,D,H,W], got {tuple(c.shape)}")
    B, D, H, W = c.shape
    if tuple(depth_values.shape) != (B, D):
        raise AarmvsError(f"aarmvs: depth_values must be [B={B},D={D}], got {tuple(depth_values.shape)}")
    dv = depth_values.detach().to(c.device, torch.float32).contiguous()
    out = {"depth_refined": torch.empty(B, H, W, device=c.device),
           "conf_window": torch.empty(B, H, W, device=c.device),
           "index": torch.empty(B, H, W, dtype=torch.int32, device=c.device)}
    check(lib().aarmvs_refine_from_cost(c.data_ptr(), dv.data_ptr(), B, D, H * W,
                                        out["depth_refined"].data_ptr(), out["conf_window"].data_ptr(),
                                        out["index"].data_ptr(), _stream()), "refine_from_cost")
    return out


POSTERIOR_KEYS = ("depth_mean", "depth_std", "entropy", "runner_up")


def posterior_state(B: int, HW: int, device) -> torch.Tensor:
    """A state buffer of the depth-posterior statistics (aarmvs_posterior_state_bytes: 16 B per
    pixel)."""
    n = lib().aarmvs_posterior_state_bytes(B, HW)
    if n == 0:
        raise AarmvsError(f"aarmvs: posterior state geometry B={B} HW={HW}")
    return torch.empty(n // 4, dtype=torch.float32, device=device)


def _check_posterior_state(state: torch.Tensor, B: int, HW: int, device) -> None:
    if (not torch.is_tensor(state) or not state.is_cuda or state.device != device or not state.is_contiguous()
            or state.numel() * state.element_size() < lib().aarmvs_posterior_state_bytes(B, HW)):
        raise AarmvsError(f"aarmvs: the posterior state must be a contiguous tensor of {16 * B * HW} B on "
                          f"{device} (ops.posterior_state(B, HW, device))")


@_on_tensor_device
def wta_posterior_update(cost: torch.Tensor, d: int, depth_d: torch.Tensor, max_prob: torch.Tensor,
                         depth_map: torch.Tensor, exp_sum: torch.Tensor, state: torch.Tensor) -> None:
    """``wta_update`` of plane ``d`` (planes in order from 0) that also keeps the posterior
    statistics' ``state`` (``posterior_state(B, H*W, device)``; d == 0 resets it), in place
    (aarmvs_wta_posterior_update)."""
    ts = (cost, max_prob, depth_map, exp_sum)
    _require_device(*ts)
    B = cost.shape[0]
    for t in ts:
        if t.shape != cost.shape or not t.is_contiguous() or t.device != cost.device:
            raise AarmvsError("aarmvs: wta_posterior_update needs contiguous tensors of one [B,H,W] shape")
    HW = cost[0].numel()
    _check_posterior_state(state, B, HW, cost.device)
    dep = depth_d.reshape(-1).to(cost.device, torch.float32).contiguous()
    if dep.numel() != B:
        raise AarmvsError(f"aarmvs: depth_d must hold B={B} values")
    if int(d) < 0:
        raise AarmvsError(f"aarmvs: plane index {d} < 0")
    check(lib().aarmvs_wta_posterior_update(cost.data_ptr(), int(d), max_prob.data_ptr(), depth_map.data_ptr(),
                                            exp_sum.data_ptr(), state.data_ptr(), dep.data_ptr(), B, HW,
                                            _stream()), "wta_posterior_update")


@_on_tensor_device
def wta_posterior_finalize(exp_sum: torch.Tensor, state: torch.Tensor) -> dict:
    """{'depth_mean', 'depth_std', 'entropy', 'runner_up'}, each shaped like ``exp_sum`` [B,H,W],
    of the planes given to ``wta_posterior_update`` so far (aarmvs_wta_posterior_finalize)."""
    _require_device(exp_sum)
    if exp_sum.dim() < 2 or not exp_sum.is_contiguous() or exp_sum.dtype != torch.float32:
        raise AarmvsError("aarmvs: wta_posterior_finalize needs a contiguous float32 [B,H,W] exp_sum")
    B, HW = exp_sum.shape[0], exp_sum[0].numel()
    _check_posterior_state(state, B, HW, exp_sum.device)
    out = {k: torch.empty_like(exp_sum) for k in POSTERIOR_KEYS}
    check(lib().aarmvs_wta_posterior_finalize(exp_sum.data_ptr(), state.data_ptr(), B, HW,
                                              *[out[k].data_ptr() for k in POSTERIOR_KEYS], _stream()),
          "wta_posterior_finalize")
    return out


@_on_tensor_device
def posterior_from_cost(cost: torch.Tensor, depth_values: torch.Tensor) -> dict:
    """The depth-posterior statistics from a whole cost volume [B,D,H,W] and depth_values [B,D]
    (aarmvs_posterior_from_cost): {'depth_mean', 'depth_std', 'entropy', 'runner_up'} [B,H,W]
    float32, bit for bit what a sweep with ``want_posterior`` gives on the same cost values."""
    _require_device(cost)
    c = cost.detach().contiguous()
    if c.dim() != 4 or c.dtype != torch.float32:
        raise AarmvsError(f"aarmvs: posterior_from_cost cost must be float32 [B,D,H,W], got {tuple(c.shape)}")
    B, D, H, W = c.shape
    if tuple(depth_values.shape) != (B, D):
        raise AarmvsError(f"aarmvs: depth_values must be [B={B},D={D}], got {tuple(depth_values.shape)}")
    dv = depth_values.detach().to(c.device, torch.float32).contiguous()
    out = {k: torch.empty(B, H, W, device=c.device) for k in POSTERIOR_KEYS}
    check(lib().aarmvs_posterior_from_cost(c.data_ptr(), dv.data_ptr(), B, D, H * W,
                                           *[out[k].data_ptr() for k in POSTERIOR_KEYS], _stream()),
          "posterior_from_cost")
    return out


def aux_stream(device) -> torch.cuda.ExternalStream:
    """The library's aux stream of ``device`` (aarmvs_aux_stream): one per device, shared by every
    DepthSweep.  The process gets four hardware queues and streams beyond four share them (a
    stream's event wait then stalls its queue partner); with this stream, the default stream and
    the library's two unit / backward streams, a sweep or a training step uses exactly four."""
    device = torch.device(device)
    ptr = ctypes.c_void_p()
    with torch.cuda.device(device):
        check(lib().aarmvs_aux_stream(ctypes.byref(ptr)), "aux_stream")
    return torch.cuda.ExternalStream(ptr.value, device=device)


class DepthSweep:
    """Runs EMVSNet's depth loop (drmvsnet.py:273-291 / :306-342) on the HIP library.

    Holds the packed parameters and a workspace per (B, H, W, nsrc) geometry.

    Streams.  Every call launches on ``torch.cuda.current_stream()`` and is ordered there like a
    kernel: after what the stream held, before what is enqueued on it next (the library's own
    streams are forked from it and joined back before the call returns).  The packed parameters
    are ready on the stream that was current at construction; using the object under another
    stream needs the caller's ``wait_stream`` first, as for any tensor.  One object serves one
    stream at a time: it owns one workspace (the recurrent state lives there), so calls on two
    streams need the caller's ordering between them, and the pieces of one sweep's ``d_range``
    go to one stream.  Two objects may be in flight on two streams, or in two host threads, at
    once: the library's unit / backward streams and its aux stream are shared per device, so
    their work is serialised there and the results do not change.

    The cached buffers (workspace, backward scratch, refine / posterior state: one live geometry
    at a time) are safe across streams through ``record_stream``: a buffer used under a stream
    other than the one it was allocated under is recorded on it on every such use, so when a new
    geometry drops it, the caching allocator reuses the block only after the work queued on it.
    Nothing is held back by the object itself, which keeps "one live geometry" bounded.
    """

    PRECISIONS = {"split": 0, "fp16": 1}  # aarmvs_precision (include/aarmvs.h)

    def __init__(self, params: dict, device, overlap: bool = True, precision: str = "split"):
        """``precision``: ``"split"`` (the default, the parity mode: three fp16 matrix products
        per fp32 product of the regulariser's convs) or ``"fp16"`` (opt-in, inference only: one
        product, the conv operands rounded once to fp16).  Settable afterwards;
        ``__call__`` and ``unet_step`` use the current value.

        ``overlap``: run the next plane group's cost stage on a second stream (the library's
        aux stream, aux_stream()) beside the current group's regulariser steps, and spread each
        plane's U-Net step over the library's streams so that the steps of neighbouring planes
        overlap (four streams in all; small frames move the cost stage to the current stream;
        same results, bit for bit)."""
        self.precision = precision  # (validated before anything touches the device)
        self.device = torch.device(device)
        self.packed = pack_params(params, self.device)
        self._ws = {}
        self._refine = {}
        self._posterior = {}
        self._aux = None
        self.overlap = overlap

    @property
    def precision(self) -> str:
        return self._precision

    @precision.setter
    def precision(self, mode: str):
        if mode not in self.PRECISIONS:
            raise AarmvsError(f"aarmvs: precision must be one of {sorted(self.PRECISIONS)}, got {mode!r}")
        self._precision = mode

    @property
    def overlap(self) -> bool:
        return self._aux is not None

    @overlap.setter
    def overlap(self, on: bool):
        if on and self._aux is None:
            self._aux = aux_stream(self.device)
        elif not on:
            self._aux = None

    def _packed_arg(self, packed) -> torch.Tensor:
        """``self.packed``, or a caller's ``pack_params`` buffer after checking it (the kernels read
        aarmvs_packed_param_bytes from it without bounds)."""
        if packed is None:
            return self.packed
        if (not torch.is_tensor(packed) or packed.dtype != torch.float32 or packed.device != self.device
                or not packed.is_contiguous() or packed.numel() * 4 < lib().aarmvs_packed_param_bytes()):
            raise AarmvsError(f"aarmvs: packed must be a pack_params buffer on {self.device}")
        return packed

    def workspace(self, B, H, W, nsrc) -> torch.Tensor:
        key = (B, H, W, nsrc)
        ws = self._ws.get(key)
        if ws is None:
            n = lib().aarmvs_sweep_workspace_bytes(B, H, W, nsrc)
            if n == 0:
                raise AarmvsError(f"aarmvs: invalid sweep geometry B={B} H={H} W={W} nsrc={nsrc} "
                                  "(H and W must be multiples of 4, 1 <= nsrc <= 16)")
            self._ws = {k: v for k, v in self._ws.items() if k[0] == "bwd" and k[1:] == key}
            # one live geometry at a time keeps HBM use bounded
            ws = _home(torch.empty(n, dtype=torch.uint8, device=self.device))
            self._ws[key] = ws
        return _use(ws)

    def refine_state(self, B, H, W) -> torch.Tensor:
        """The sub-plane refinement's state of a (B, H, W) sweep (16 B per pixel), cached beside
        the workspace, one geometry at a time: d_range calls with ``want_refined`` continue it."""
        key = (B, H, W)
        st = self._refine.get(key)
        if st is None:
            st = _home(refine_state(B, H * W, self.device))
            self._refine = {key: st}
        return _use(st)

    def posterior_state(self, B, H, W) -> torch.Tensor:
        """The posterior statistics' state of a (B, H, W) sweep (16 B per pixel), cached beside
        the workspace, one geometry at a time: d_range calls with ``want_posterior`` continue it."""
        key = (B, H, W)
        st = self._posterior.get(key)
        if st is None:
            st = _home(posterior_state(B, H * W, self.device))
            self._posterior = {key: st}
        return _use(st)

    def relative(self, ref_proj, src_projs, B: int) -> torch.Tensor:
        """[nsrc,B,12] device tensor of rows 0..2 of src_proj @ inv(ref_proj) per source view
        (module.py:16-18): one host round trip, reusable across d_range calls."""
        _check_proj(ref_proj, B, "ref_proj")
        for sp in src_projs:
            _check_proj(sp, B, "src_proj")
        rel = torch.stack([relative_projection(sp, ref_proj) for sp in src_projs])  # [nsrc,B,3,4]
        return rel.reshape(len(src_projs), B, 12).to(self.device).contiguous()

    RECORD_KEYS = ("x", "state", "z", "u", "stats", "t1", "ostats")

    @staticmethod
    def _record_sizes(B: int, H: int, W: int, D: int, nsrc: int) -> dict:
        L = lib()
        counts = (D, D + 1, D, D, D, D * nsrc, D * nsrc)
        out = {}
        for i, (name, count) in enumerate(zip(DepthSweep.RECORD_KEYS, counts)):
            n = L.aarmvs_train_record_bytes(B, H, W, i)
            if n == 0:
                raise AarmvsError(f"aarmvs: invalid record geometry B={B} H={H} W={W}")
            out[name] = n * count
        return out

    @staticmethod
    def record_buffers(B: int, H: int, W: int, D: int, device, *, nsrc: int, planes: int | None = None) -> dict:
        """Device buffers of a training record (aarmvs_train_record) for D planes and nsrc
        source views: the cost slices, D + 1 regulariser state slabs, the gate pre-activations,
        the deconv outputs and their GroupNorm statistics, the omega conv output and its
        statistics (~1 KB per pixel and plane at B = 1, N = 3).  ``planes``: a segment record of
        that many planes (at most D) instead, for ``record_d0`` calls (plane-segment
        checkpointing; ``record_bytes`` gives the sizes)."""
        n_planes = D if planes is None else int(planes)
        if not 1 <= n_planes <= D:
            raise AarmvsError(f"aarmvs: a segment record holds 1..D={D} planes, got {planes}")
        return {k: torch.empty(n, dtype=torch.uint8, device=device)
                for k, n in DepthSweep._record_sizes(B, H, W, n_planes, nsrc).items()}

    @staticmethod
    def record_bytes(B: int, H: int, W: int, planes: int, *, nsrc: int) -> tuple:
        """(bytes of a record of ``planes`` planes, bytes of one state checkpoint), from
        aarmvs_train_segment_bytes.  No device needed."""
        rec, ck = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(lib().aarmvs_train_segment_bytes(B, H, W, nsrc, planes, ctypes.byref(rec), ctypes.byref(ck)),
              "train_segment_bytes")
        return int(rec.value), int(ck.value)

    @staticmethod
    def _record_planes(rec: dict, B: int, H: int, W: int, nsrc: int) -> int:
        """The planes a record's buffers have room for (the smallest over the seven)."""
        L = lib()
        planes = None
        for i, name in enumerate(DepthSweep.RECORD_KEYS):
            slab = L.aarmvs_train_record_bytes(B, H, W, i)
            t = rec.get(name)
            if slab == 0 or t is None:
                raise AarmvsError(f"aarmvs: training record '{name}' missing or invalid geometry B={B} H={H} W={W}")
            n = t.numel() * t.element_size() // slab
            n = n - 1 if name == "state" else n // nsrc if name in ("t1", "ostats") else n
            planes = n if planes is None else min(planes, n)
        return planes

    @staticmethod
    def _record_struct(rec: dict, B: int, H: int, W: int, D: int, nsrc: int, device=None):
        """ctypes view of a record, after checking every buffer holds this geometry's bytes,
        is contiguous and lives on the sweep's device (the library writes them without bounds)."""
        for k, n in DepthSweep._record_sizes(B, H, W, D, nsrc).items():
            t = rec.get(k)
            if t is None or not t.is_cuda or t.numel() * t.element_size() < n or not t.is_contiguous():
                raise AarmvsError(f"aarmvs: training record '{k}' missing, non-contiguous or smaller "
                                  f"than {n} B (record_buffers(B, H, W, D, nsrc={nsrc}))")
            if device is not None and t.device != torch.device(device):
                raise AarmvsError(f"aarmvs: training record '{k}' is on {t.device}, the sweep on {device}")
        r = _lib.TrainRecord()
        (r.x, r.state, r.z, r.u, r.stats, r.t1, r.ostats) = (rec[k].data_ptr() for k in DepthSweep.RECORD_KEYS)
        return r

    def _segment_struct(self, a, record: dict, record_d0, d0: int, d1: int, device):
        """Points ``a`` (SweepArgs or BackwardArgs with its geometry set) at ``record`` as the
        record of the planes from ``record_d0`` on, after checking that the buffers hold the
        planes d0..d1-1 of the call; returns the ctypes record (to be kept alive)."""
        record_d0 = int(record_d0)
        if not 0 <= record_d0 < a.D:
            raise AarmvsError(f"aarmvs: record_d0 {record_d0} outside [0, D={a.D})")
        n = min(self._record_planes(record, a.B, a.H, a.W, a.nsrc), a.D - record_d0)
        if n < 1 or d0 < record_d0 or d1 > record_d0 + n:
            raise AarmvsError(f"aarmvs: the training record holds planes [{record_d0}, {record_d0 + max(n, 0)}) "
                              f"and does not cover the range [{d0}, {d1}) (record_buffers(B, H, W, D, "
                              f"nsrc={a.nsrc}[, planes=S]) and record_d0)")
        rs = self._record_struct(record, a.B, a.H, a.W, n, a.nsrc, device)
        a.record = ctypes.pointer(rs)
        a.record_d0, a.record_planes = record_d0, n
        return rs

    @_on_tensor_device
    def __call__(self, ref_fea, src_feas, ref_proj, src_projs, depth_values, *,
                 want_depth=True, want_cost=False, d_range=None, debug=False, cost_out=None,
                 rel=None, record=None, record_d0=0, want_refined=False, want_posterior=False,
                 packed=None):
        """Returns dict(depth, conf, cost, slice, omega) (entries None when not requested).

        ``packed``: a ``pack_params`` buffer to run on instead of ``self.packed`` (an autograd
        graph passes the buffer of its own forward to the checkpoint recompute, whatever the
        object holds by then).

        ``want_refined`` (opt-in, inference only) adds ``depth_refined`` and ``conf_window``
        [B,H,W] and ``index`` [B,H,W] int32: the local expectation of depth over the winning
        plane and its two neighbours, the probability mass of that window, and the winner's
        plane (include/aarmvs.h, aarmvs_sweep_r).  They describe the planes up to the call's
        last one; with ``d_range`` every call of the sweep must pass ``want_refined``, which
        carries the state in ``self.refine_state(B, H, W)``.  The other outputs do not change.

        ``want_posterior`` (opt-in, inference only, combinable with ``want_refined``) adds
        ``depth_mean``, ``depth_std``, ``entropy`` (nats) and ``runner_up`` [B,H,W]: the moments of
        the softmax over the planes' costs, its entropy and its second largest probability
        (include/aarmvs.h, aarmvs_posterior_args), NaN exactly where ``conf`` is NaN or the sum
        overflowed.  Same rules as ``want_refined``; the state is ``self.posterior_state(B, H, W)``.

        ``d_range=(d0, d1)`` runs planes d0..d1-1 only (d0 == 0 resets the hidden state;
        later ranges continue from the state the previous call left in the workspace).
        ``cost_out`` is an optional caller-owned [B,D,H,W] buffer for the regulariser output.
        ``rel`` is an optional precomputed ``self.relative(ref_proj, src_projs, B)``.
        ``record`` (``record_buffers(B, H, W, D, nsrc=...)``) keeps every plane's tensors for
        ``backward`` (the training forward).  ``record_d0``: ``record`` is a segment record
        (``record_buffers(..., planes=S)``) whose slab i is plane ``record_d0 + i``; the call's
        planes must lie inside it, and it starts from the state in the record's state slab
        ``d0 - record_d0`` (the caller's checkpoint; zeroed by the library when d0 == 0).
        """
        ref = ref_fea.contiguous()
        srcs = [s.contiguous() for s in src_feas]
        _require_device(ref, *srcs)
        if ref.dim() != 4:
            raise AarmvsError(f"aarmvs: ref_fea must be [B,C,H,W], got {tuple(ref.shape)}")
        B, C, H, W = ref.shape
        nsrc = len(srcs)
        if nsrc < 1 or nsrc > _lib.MAX_SRC:
            raise AarmvsError(f"aarmvs: need 1..{_lib.MAX_SRC} source views, got {nsrc}")
        if len(src_projs) != nsrc:
            raise AarmvsError(f"aarmvs: {nsrc} source features but {len(src_projs)} projections")
        for s in srcs:
            if s.shape != ref.shape:
                raise AarmvsError("aarmvs: source features must match the reference feature shape")
        # the kernels index depth_values[b * D + d] and rel[v][b]: reject mismatches here
        if depth_values.dim() != 2 or depth_values.shape[0] != B or depth_values.shape[1] < 1:
            raise AarmvsError(f"aarmvs: depth_values must be [B={B},D], got {tuple(depth_values.shape)}")
        dv = depth_values.to(ref.device, torch.float32).contiguous()
        D = dv.shape[1]
        if d_range is not None and not (0 <= d_range[0] < d_range[1] <= D):
            raise AarmvsError(f"aarmvs: bad d_range {d_range} for D={D}")
        if rel is None:
            rel = self.relative(ref_proj, src_projs, B)
        elif tuple(rel.shape) != (nsrc, B, 12) or not rel.is_cuda:
            raise AarmvsError(f"aarmvs: rel must be a device [nsrc={nsrc},B={B},12] tensor")
        ws = self.workspace(B, H, W, nsrc)
        out = {"depth": None, "conf": None, "cost": None, "slice": None, "omega": None}
        if want_depth:
            out["depth"] = torch.empty(B, H, W, device=ref.device)
            out["conf"] = torch.empty(B, H, W, device=ref.device)
        if cost_out is not None:
            if tuple(cost_out.shape) != (B, D, H, W) or not cost_out.is_contiguous():
                raise AarmvsError("aarmvs: cost_out must be a contiguous [B,D,H,W] tensor")
            _require_device(cost_out)
            out["cost"] = cost_out
        elif want_cost:
            out["cost"] = torch.empty(B, D, H, W, device=ref.device)
        if debug:
            out["slice"] = torch.empty(B, C, H, W, device=ref.device)
            out["omega"] = torch.empty(nsrc, B, H, W, device=ref.device)
        a = _lib.SweepArgs()
        a.B, a.C, a.H, a.W, a.nsrc, a.D = B, C, H, W, nsrc, D
        d0, d1 = (0, D) if d_range is None else d_range
        a.d_begin, a.d_end = d0, d1
        a.ref_fea = ref.data_ptr()
        for i, s in enumerate(srcs):
            a.src_fea[i] = s.data_ptr()
        a.rel_proj = rel.data_ptr()
        a.depth_values = dv.data_ptr()
        packed = self._packed_arg(packed)
        a.packed_params = _use(packed).data_ptr()
        a.workspace = ws.data_ptr()
        a.depth_out = _ptr(out["depth"])
        a.conf_out = _ptr(out["conf"])
        a.cost_out = _ptr(out["cost"])
        a.slice_out = _ptr(out["slice"])
        a.omega_out = _ptr(out["omega"])
        a.aux_stream = self._aux.cuda_stream if self._aux is not None else None
        rec_struct = None
        refine = None
        if want_refined:
            if record is not None:
                raise AarmvsError("aarmvs: want_refined is an inference output; a recorded (training) sweep "
                                  "has none (ops.refine_from_cost works on its cost volume)")
            out["depth_refined"] = torch.empty(B, H, W, device=ref.device)
            out["conf_window"] = torch.empty(B, H, W, device=ref.device)
            out["index"] = torch.empty(B, H, W, dtype=torch.int32, device=ref.device)
            refine = _lib.RefineArgs()
            refine.state = self.refine_state(B, H, W).data_ptr()
            refine.depth_refined_out = out["depth_refined"].data_ptr()
            refine.conf_window_out = out["conf_window"].data_ptr()
            refine.index_out = out["index"].data_ptr()
        posterior = None
        if want_posterior:
            if record is not None:
                raise AarmvsError("aarmvs: want_posterior is an inference output; a recorded (training) sweep "
                                  "has none (ops.posterior_from_cost works on its cost volume)")
            posterior = _lib.PosteriorArgs()
            posterior.state = self.posterior_state(B, H, W).data_ptr()
            for k, f in zip(POSTERIOR_KEYS, ("mean_out", "std_out", "entropy_out", "runner_up_out")):
                out[k] = torch.empty(B, H, W, device=ref.device)
                setattr(posterior, f, out[k].data_ptr())
        if record is not None:
            if self._precision != "split":
                raise AarmvsError(f"aarmvs: precision {self._precision!r} is an inference mode; a recorded "
                                  "(training) sweep needs precision 'split'")
            rec_struct = self._segment_struct(a, record, record_d0, d0, d1, ref.device)
        elif record_d0:
            raise AarmvsError("aarmvs: record_d0 without a record")
        opts = _lib.SweepOptions()
        opts.size = ctypes.sizeof(opts)
        opts.precision = self.PRECISIONS[self._precision]
        if refine is not None:
            opts.refine = ctypes.pointer(refine)
        if posterior is not None:
            opts.posterior = ctypes.pointer(posterior)
        check(lib().aarmvs_sweep_ex(ctypes.byref(a), ctypes.byref(opts), _stream()), "sweep")
        out["_keepalive"] = (rel, dv, srcs, ref, rec_struct, packed)
        return out

    @_on_tensor_device
    def backward(self, ref_fea, src_feas, rel, depth_values, record, grad_cost, *,
                 regulariser_only=False, want_grad_x=False, d_range=None, record_d0=0, grad_x_out=None,
                 packed=None):
        """Backward of a recorded training sweep (aarmvs_sweep_backward): from dL/dcost
        [B,D,H,W] to (grad_ref [B,32,H,W], [grad_src [B,32,H,W]] per view, {sweep parameter
        name: gradient}, grad_x [D,B,H,W,32] NHWC or None).  ``regulariser_only`` stops after
        the regulariser (debug: grad_ref/grad_src are None, the omega.* gradients zero).

        ``d_range=(d0, d1)`` runs the planes d0..d1-1 only, on a ``record`` that holds the planes
        from ``record_d0`` on (a segment record).  d0 and d1 must be multiples of 16 (d1 may be
        D).  One backward is a chain of such calls, last range first (d1 == D), each ending
        where the one before began, down to d0 == 0; only the recompute forward of the next
        segment may use this object in between.  The calls before the final one return None; the
        final one (d0 == 0) returns the gradients of the whole sweep, bit for bit those of one
        call on a whole record.  ``grad_x_out``: a caller-owned [D,B,H,W,32] buffer for grad_x
        (each call fills its planes).  ``packed``: the ``pack_params`` buffer the recorded forward
        ran on, when that is no longer ``self.packed`` (a graph differentiates at its own
        forward's weights)."""
        ref = ref_fea.contiguous()
        srcs = [t.contiguous() for t in src_feas]
        _require_device(ref, *srcs, grad_cost)
        B, C, H, W = ref.shape
        nsrc = len(srcs)
        dv = depth_values.to(ref.device, torch.float32).contiguous()
        D = dv.shape[1]
        g = grad_cost.contiguous()
        if tuple(g.shape) != (B, D, H, W):
            raise AarmvsError(f"aarmvs: grad_cost must be [B={B},D={D},H={H},W={W}], got {tuple(g.shape)}")
        d0, d1 = (0, D) if d_range is None else (int(d_range[0]), int(d_range[1]))
        if not 0 <= d0 < d1 <= D:
            raise AarmvsError(f"aarmvs: bad backward d_range {d_range} for D={D}")
        ws = self.workspace(B, H, W, nsrc)
        L = lib()
        key = ("bwd", B, H, W, nsrc)
        scratch = self._ws.get(key)
        # a call that continues a backward needs the scratch the call before it left: the same
        # buffer, and the range that ends where that one began
        chain = getattr(self, "_bwd_chain", None)
        self._bwd_chain = None
        if d1 != D and (scratch is None or chain != (key, d1, bool(regulariser_only))):
            raise AarmvsError(f"aarmvs: backward over [{d0}, {d1}) does not continue a backward of this "
                              f"geometry that stopped at plane {d1} (the calls come last range first, "
                              "contiguous, with nothing but the recompute forward between them)")
        if scratch is None:
            n = L.aarmvs_backward_scratch_bytes(B, H, W, nsrc)
            if n == 0:
                raise AarmvsError(f"aarmvs: invalid backward geometry B={B} H={H} W={W} nsrc={nsrc}")
            scratch = _home(torch.empty(n, dtype=torch.uint8, device=ref.device))
            self._ws[key] = scratch
        _use(scratch)
        final = d0 == 0
        grad_ref = torch.empty_like(ref) if final and not regulariser_only else None
        grad_src = [torch.empty_like(t) for t in srcs] if final and not regulariser_only else None
        grad_params = torch.empty(L.aarmvs_param_count(), device=ref.device) if final else None
        grad_x = None
        if grad_x_out is not None:
            _require_device(grad_x_out)
            if tuple(grad_x_out.shape) != (D, B, H, W, C) or not grad_x_out.is_contiguous():
                raise AarmvsError(f"aarmvs: grad_x_out must be a contiguous [D={D},B,H,W,{C}] tensor")
            grad_x = grad_x_out
        elif want_grad_x:
            if (d0, d1) != (0, D):
                raise AarmvsError("aarmvs: a ranged backward returns grad_x through grad_x_out")
            grad_x = torch.empty(D, B, H, W, C, device=ref.device)
        a = _lib.BackwardArgs()
        a.B, a.C, a.H, a.W, a.nsrc, a.D = B, C, H, W, nsrc, D
        a.ref_fea = ref.data_ptr()
        for i, t in enumerate(srcs):
            a.src_fea[i] = t.data_ptr()
            if grad_src is not None:
                a.grad_src[i] = grad_src[i].data_ptr()
        a.rel_proj = rel.data_ptr()
        a.depth_values = dv.data_ptr()
        a.packed_params = _use(self._packed_arg(packed)).data_ptr()
        if (not torch.is_tensor(rel) or tuple(rel.shape) != (nsrc, B, 12) or rel.dtype != torch.float32
                or rel.device != ref.device or not rel.is_contiguous()):
            raise AarmvsError(f"aarmvs: rel must be a contiguous float32 [nsrc={nsrc}, B={B}, 12] tensor on "
                              f"{ref.device} (DepthSweep.relative), got "
                              f"{tuple(rel.shape) if torch.is_tensor(rel) else type(rel)}")
        rs = self._segment_struct(a, record, record_d0, d0, d1, ref.device)
        a.d_begin, a.d_end = d0, d1
        a.grad_cost = g.data_ptr()
        a.grad_ref = _ptr(grad_ref)
        a.grad_params = _ptr(grad_params)
        a.grad_x = _ptr(grad_x)
        a.workspace = ws.data_ptr()
        a.scratch = scratch.data_ptr()
        a.regulariser_only = 1 if regulariser_only else 0
        check(L.aarmvs_sweep_backward(ctypes.byref(a), _stream()), "sweep_backward")
        del rs
        if not final:
            self._bwd_chain = (key, d0, bool(regulariser_only))
            return None
        grads, off = {}, 0
        for k in SWEEP_KEYS:
            n = 1
            for d in SWEEP_SHAPES[k]:
                n *= d
            grads[k] = grad_params[off: off + n].view(SWEEP_SHAPES[k])
            off += n
        return grad_ref, grad_src, grads, grad_x

    def state(self, B, H, W, nsrc, planes, cell, which) -> torch.Tensor:
        """View of a hidden/cell state inside the workspace after the sweep has processed
        ``planes`` planes (or ``unet_step`` steps): the state those planes left."""
        ws = self.workspace(B, H, W, nsrc)
        ptr = lib().aarmvs_state_ptr(ws.data_ptr(), B, H, W, nsrc, planes, cell, which)
        if not ptr:
            raise AarmvsError("aarmvs: bad state query")
        hid = (16, 16, 16, 16, 8)[cell]
        sc = (1, 2, 4, 2, 1)[cell]
        off = ptr - ws.data_ptr()
        # stored NHWC (include/aarmvs.h); returned as the reference's NCHW view
        return ws[off: off + B * hid * (H // sc) * (W // sc) * 4].view(torch.float32).view(
            B, H // sc, W // sc, hid).permute(0, 3, 1, 2)

    @_on_tensor_device
    def cost_slice(self, ref_fea, src_feas, ref_proj, src_projs, depth, want_omega=False):
        """One plane's cost slice x [B,32,H,W] (aarmvs_cost_slice; drmvsnet.py:307-319) at
        depth [B]; returns (x, omega [nsrc,B,H,W] or None).  Uses this object's workspace."""
        ref = ref_fea.contiguous()
        srcs = [s.contiguous() for s in src_feas]
        _require_device(ref, *srcs)
        B, C, H, W = ref.shape
        nsrc = len(srcs)
        if nsrc < 1 or nsrc > _lib.MAX_SRC or len(src_projs) != nsrc:
            raise AarmvsError(f"aarmvs: need 1..{_lib.MAX_SRC} source views with projections")
        for s in srcs:
            if s.shape != ref.shape:
                raise AarmvsError("aarmvs: source features must match the reference feature shape")
        dep = depth.reshape(-1).to(ref.device, torch.float32).contiguous()
        if dep.numel() != B:
            raise AarmvsError(f"aarmvs: depth must hold B={B} values")
        rel = self.relative(ref_proj, src_projs, B)
        ws = self.workspace(B, H, W, nsrc)
        x = torch.empty(B, C, H, W, device=ref.device)
        om = torch.empty(nsrc, B, H, W, device=ref.device) if want_omega else None
        ptrs = (ctypes.c_void_p * nsrc)(*[s.data_ptr() for s in srcs])
        check(lib().aarmvs_cost_slice(ref.data_ptr(), ptrs, rel.data_ptr(), dep.data_ptr(),
                                      _use(self.packed).data_ptr(), B, C, H, W, nsrc, ws.data_ptr(),
                                      x.data_ptr(), _ptr(om), _stream()), "cost_slice")
        return x, om

    @_on_tensor_device
    def unet_step(self, x: torch.Tensor, step: int, nsrc: int = 1) -> torch.Tensor:
        _require_device(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        ws = self.workspace(B, H, W, nsrc)
        cost = torch.empty(B, 1, H, W, device=x.device)
        check(lib().aarmvs_unet_step_p(x.data_ptr(), B, H, W, nsrc, step, _use(self.packed).data_ptr(),
                                       ws.data_ptr(), cost.data_ptr(), self.PRECISIONS[self._precision],
                                       _stream()), "unet_step")
        return cost


# ----------------------------------------------------------------------------------
# opt-in per-kernel timing (aarmvs_profile_*): hipEvents on the launch stream
# ----------------------------------------------------------------------------------
def profile_enable(on: bool = True) -> None:
    lib().aarmvs_profile_enable(1 if on else 0)


def profile_reset() -> None:
    lib().aarmvs_profile_reset()


def profile_read() -> dict:
    """{kernel name: (launches, total device ms)} since the last reset."""
    L = lib()
    out = {}
    for i in range(L.aarmvs_profile_kernel_count()):
        n = ctypes.c_longlong(0)
        ms = ctypes.c_double(0.0)
        check(L.aarmvs_profile_read(i, ctypes.byref(n), ctypes.byref(ms)), "profile_read")
        if n.value:
            out[L.aarmvs_profile_kernel_name(i).decode()] = (int(n.value), float(ms.value))
    return out
