"""Restatement, for the tests, of the opt-in split weight gradient (`fp32_split_wgrad: true`): the arithmetic of csrc/u3d_wgrad_f32s.hip
on the CPU — the exact three-way bf16 split and the six partial products — and the routing rule of the engine (`_split_wgrad`, asked
inside `_wgrad_fp32` and `_wgrad_subpixel`), written down a second time from the description of the feature, without the engine."""
import torch
from torch import nn

PRODUCTS = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))  # (part of a, part of b): hh, hm, mh, hl, lh, mm; h = 0, m = 1, l = 2


def split3(x):
    """fp32 tensor -> (h, m, l) bf16-representable fp32 tensors: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), nearest even"""
    assert x.dtype == torch.float32
    h = x.bfloat16().float()
    r = x - h
    m = r.bfloat16().float()
    l = (r - m).bfloat16().float()
    return h, m, l


def six_products(a, b):
    """sum of the six partial products of the split operands, in float64 (every product of two bf16 values is exact there)"""
    pa, pb = [t.double() for t in split3(a)], [t.double() for t in split3(b)]
    out = torch.zeros_like(pa[0])
    for i, j in reversed(PRODUCTS):  # smallest class first
        out += pa[i] * pb[j]
    return out


def in_envelope(Cin, Cout):
    return Cin > 0 and Cout > 0 and Cin % 32 == 0 and Cout % 32 == 0


def level_dims(size, levels):
    dims = [tuple(size)]
    for _ in range(levels - 1):
        dims.append(tuple(d // 2 for d in dims[-1]))
    return dims


def routed(model, size, key=True):
    """[(parameter name of the weight, Cin of the routed launch, Cout, dw_cin_stride)] of the layers whose weight gradient — for a UNet3D's
    decoder first convolution: whose skip slice — runs on u3d_conv3d_wgrad_f32s in a backward at input size `size` (D, H, W): one launch
    each.  A 3x3x3 convolution over one real tensor with both counts % 32; the skip slice (C0, Cout) of a decoder's first convolution
    when the level upsamples by exactly 2 (or n -> 2n + 1) on every axis, where the sub-pixel kernels read skip and low-res tensor apart;
    a decoder's first convolution on a virtual concat (any other level) is not routed.  Residual nets join by summation: every 3x3x3
    layer reads one tensor."""
    if not key:
        return []
    names = {id(p): n for n, p in model.named_parameters()}
    first = {}
    if not model._residual:
        L = len(model.encoders)
        dims = level_dims(size, L)
        for j, dec in enumerate(model.decoders):
            c1 = dec.basic_module.SingleConv1.conv
            C0 = model.encoders[L - 2 - j].basic_module.SingleConv2.conv.out_channels
            ratio = [a - 2 * b for a, b in zip(dims[L - 2 - j], dims[L - 1 - j])]
            first[id(c1)] = (C0, all(r in (0, 1) for r in ratio))
    out = []
    for mod in model.modules():
        if not isinstance(mod, nn.Conv3d) or tuple(mod.kernel_size) != (3, 3, 3):
            continue
        Cin, Cout = mod.in_channels, mod.out_channels
        if id(mod) in first:
            C0, subpixel = first[id(mod)]
            if subpixel and in_envelope(C0, Cout):
                out.append((names[id(mod.weight)], C0, Cout, Cin))
        elif in_envelope(Cin, Cout):
            out.append((names[id(mod.weight)], Cin, Cout, Cin))
    return out
