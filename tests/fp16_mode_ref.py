"""CPU emulation of the sweep's fp16 mode (AARMVS_PREC_FP16), for the tests only.

``fp16_operands()`` swaps ``oracle.sweep_oracle.lstm_cell`` and ``deconv_gn_relu`` for versions
that round the operands of their convolutions to 11 significant bits (fp16's precision, without
its range: the library stages every operand at a power-of-two scale that keeps it in range, so
its rounding is relative too) and restores them on exit.  ``unet_step`` looks both up at call
time, so ``orc.unet_step`` / ``orc.sweep`` inside the block run the emulated mode.  Everything
else (accumulation, bias, gates, state, GroupNorm, head, WTA, the cost slice) stays fp32.

Operands: ``cat[x, h]`` and the weight of a cell; the input and the weight of a deconv.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import sweep_oracle as orc


def round11(t: torch.Tensor) -> torch.Tensor:
    """t rounded to 11 significant bits, round to nearest even, any exponent."""
    m, e = torch.frexp(t.float())              # t = m 2^e, |m| in [0.5, 1)
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)   # torch.round: half to even


def _lstm_cell(x, h, c, w, b):
    z = F.conv2d(round11(torch.cat([x, h], 1)), round11(w), b, padding=1)
    if orc.GATE_HOOK is not None:
        orc.GATE_HOOK(z)
    i, f, o, g = torch.split(z, h.shape[1], dim=1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return h2, c2


def _deconv_gn_relu(x, P, name, fast=False):
    k = "cost_regularization." + name + "."
    y = F.conv_transpose2d(round11(x), round11(P[k + "conv.weight"]), P[k + "conv.bias"], stride=2,
                           padding=1, output_padding=1)
    return F.relu(orc.group_norm(y, 2, P[k + "gn.weight"], P[k + "gn.bias"], fast=fast))


@contextlib.contextmanager
def fp16_operands():
    saved = orc.lstm_cell, orc.deconv_gn_relu
    orc.lstm_cell, orc.deconv_gn_relu = _lstm_cell, _deconv_gn_relu
    try:
        yield
    finally:
        orc.lstm_cell, orc.deconv_gn_relu = saved


def rms(t) -> float:
    t = torch.as_tensor(t).double()
    return float(torch.sqrt((t * t).mean()))
