"""Restatement, for the tests, of `native_2d_residual_fp32_split: true` on a ResidualUNet2D: which 3x3 convolutions run on the six-product
kernels of csrc/u3d_conv2d_f32s.h and which of them carry the residual in their epilogue (u3d_conv2d_f32s_res), written down a second time
from the description of the feature, without the engine.

A ResNetBlock (one per encoder and per decoder) is conv1 (1x1, or the identity) -> conv2 (3x3) -> conv3 (3x3) + residual -> non-linearity;
conv2 and conv3 are width -> width on one real tensor.  Both are routed when the block's width is a multiple of 32.  `out += residual`
follows the block's last norm: in a pre-norm order (a norm letter before the `c`) that is conv3's own epilogue; in a post-norm or norm-free
order the residual is added by the pass that applies conv3's norm / bias, and conv3 is a plain convolution."""
NEW_NAME = "u3d_conv2d_f32s_res"
KEY = "native_2d_residual_fp32_split"


def pre_norm(order: str) -> bool:
    """a GroupNorm / BatchNorm letter stands before the convolution's"""
    c = order.index("c")
    return any(ch in order[:c] for ch in "gb")


def rule(width: int) -> bool:
    return width > 0 and width % 32 == 0


def routed(model, key=True):
    """[(parameter name of the weight, width, carries the epilogue residual)] of the 3x3 convolutions on the six-product kernels, in module
    order: one forward, one data-gradient and one weight-gradient launch per entry"""
    if not key:
        return []
    names = {id(p): n for n, p in model.named_parameters()}
    pre = pre_norm(model.layer_order)
    out = []
    for level in list(model.encoders) + list(model.decoders):
        bm = level.basic_module
        for which in ("conv2", "conv3"):
            conv = getattr(bm, which).conv
            assert tuple(conv.kernel_size) == (3, 3) and conv.in_channels == conv.out_channels
            if rule(conv.out_channels):
                out.append((names[id(conv.weight)], conv.out_channels, which == "conv3" and pre))
    return out


def conv3x3(model):
    """every 3x3 convolution of the net, routed or not"""
    return [getattr(level.basic_module, which).conv for level in list(model.encoders) + list(model.decoders) for which in ("conv2", "conv3")]
