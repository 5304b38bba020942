"""Restatement, for the tests, of `native_2d_fp32_split: true` on a UNet2D: the arithmetic of csrc/u3d_conv2d_f32s.h on the CPU — a
float64 2-D convolution of the exactly split operands, six partial products, smallest class first — and the routing rule of the engine
(`_split2d`), written down a second time from the description of the feature, without the engine."""
import torch
import torch.nn.functional as F
from torch import nn

import f32s_emul as FE

NEW_NAMES = ("u3d_conv2d_f32s_supported", "u3d_conv2d_wgrad_f32s_supported", "u3d_packed_weight2d_f32s_elems", "u3d_pack_weights2d_f32s",
             "u3d_conv2d_f32s", "u3d_conv2d_f32s_dgrad", "u3d_wgrad2d_f32s_workspace_floats", "u3d_conv2d_wgrad_f32s")


def conv2d_six_products(x, w):
    """conv2d(x, w, padding=1) as the kernels form it, in float64: both fp32 operands split into (h, m, l), the six partial
    convolutions hh, hm, mh, hl, lh, mm added smallest class first"""
    px, pw = [t.double() for t in FE.split3(x)], [t.double() for t in FE.split3(w)]
    out = None
    for i, j in reversed(FE.PRODUCTS):
        term = F.conv2d(px[i], pw[j], None, padding=1)
        out = term if out is None else out + term
    return out


def rule(C0, C1, Cout):
    """a 3x3 layer is routed when the key is on and — a single source (C1 == 0) — both counts are multiples of 32, or — a decoder's
    virtual concat — C0, C1 and Cout all are"""
    if Cout <= 0 or Cout % 32 or C0 <= 0 or C0 % 32:
        return False
    return C1 == 0 or (C1 > 0 and C1 % 32 == 0)


def routed(model, key=True):
    """[(parameter name of the weight, C0, C1, Cout)] of the 3x3 layers of a UNet2D that run forward, data gradient and weight gradient on
    the new kernels, in module order: one launch of each direction per entry.  A decoder's first convolution reads cat(skip, nearest(low)):
    C0 = the skip's channels (the output of the encoder at its level), C1 = the rest."""
    if not key:
        return []
    names = {id(p): n for n, p in model.named_parameters()}
    L = len(model.encoders)
    first = {}
    for j, dec in enumerate(model.decoders):
        c1 = dec.basic_module.SingleConv1.conv
        first[id(c1)] = model.encoders[L - 2 - j].basic_module.SingleConv2.conv.out_channels
    out = []
    for mod in model.modules():
        if not isinstance(mod, nn.Conv2d) or tuple(mod.kernel_size) != (3, 3):
            continue
        C0 = first.get(id(mod), mod.in_channels)
        C1 = mod.in_channels - C0
        if rule(C0, C1, mod.out_channels):
            out.append((names[id(mod.weight)], C0, C1, mod.out_channels))
    return out
