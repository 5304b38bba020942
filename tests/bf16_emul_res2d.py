"""Float64 CPU emulation of a ResidualUNet2D under `native_2d_residual_bf16`: the product's module tree in float64, with every 3x3 Conv2d
that the executor routes to the bf16 kernels (csrc/u3d_conv2d_bf16.hip) replaced by bf16_emul_2d.Bf16Conv2d — the operands of its three
GEMMs (forward: the convolution input after the norm in front of it and w; data gradient: dz and w; weight gradient: the input and dz)
rounded to bf16, accumulated in float64.  The residual add (`out += residual`, never rounded: the kernel adds the fp32 residual to its
fp32 accumulator), the 1x1 convolutions, ConvTranspose2d, the norms, pooling, joining and the head are exact.

The eligibility rule is RESTATED here, not imported from the engine (tests/test_native2d_residual_bf16.py holds the two against each
other): a 3x3 convolution with both channel counts multiples of 32.  Every 3x3 convolution of a ResNetBlock (conv2, conv3) maps
out_channels -> out_channels and reads one real tensor — with `upsample: deconv` the concat is consumed by the block's 1x1 conv1 — so no
layer is excluded for its source, and the layer order does not matter."""
import torch

from bf16_emul_2d import Bf16Conv2d


def conv3x3(model):
    """every 3x3 Conv2d of `model` in module order"""
    return [m for m in model.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]


def eligible(model):
    """the 3x3 Conv2d modules of `model` (a ResidualUNet2D) that run on the bf16 kernels under native_2d_residual_bf16, in module order"""
    return [m for m in conv3x3(model) if m.in_channels % 32 == 0 and m.out_channels % 32 == 0]


def build(cfg, sd, emulate: bool):
    """the float64 module tree of `cfg` with the parameters `sd`; emulate: the eligible convolutions round their operands"""
    from pytorch3dunet_amd.unet3d.model import get_model

    drop = ("native_2d", "native_2d_residual", "native_2d_residual_bf16", "compute_dtype", "activation_dtype")
    model = get_model({k: v for k, v in cfg.items() if k not in drop}).double()
    model.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    if emulate:
        for conv in eligible(model):
            def fwd(x, conv=conv):
                y = Bf16Conv2d.apply(x, conv.weight)
                return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1)

            conv.forward = fwd
    return model.train()


def run(cfg, sd, x, target, loss_name: str, emulate: bool):
    """(logits, loss, {name: grad}) of one training step in float64"""
    from conftest import loss_by_name

    model = build(cfg, sd, emulate)
    probs, logits = model(x.double(), return_logits=True)
    loss = loss_by_name(loss_name, probs, logits, target.double())
    loss.backward()
    return logits.detach(), loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}
