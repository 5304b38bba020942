"""Float64 CPU emulation of a UNet2D under `native_2d_bf16` + `native_2d_stem`: the module tree in float64, with every 3x3 Conv2d the
executor routes to the bf16 kernels replaced by the autograd function of tests/bf16_emul_2d.py, which rounds the operands of its three
GEMMs to bf16 and accumulates in float64.  Every other layer is exact.

The eligibility rule of the mode is RESTATED here, not imported from the engine (tests/test_native2d_stem.py holds the two against each
other):
  * a small-family layer — a single real source with Cin <= 4 and Cout <= 32, the net's first convolution — stays exact (fp32 kernels of
    csrc/u3d_conv2d.hip);
  * any other 3x3 convolution with BOTH channel counts multiples of 16 whose input is a single tensor rounds its operands — with a
    norm-first layer order the decoders' first convolutions qualify too (their concat is written out);
  * everything else (a virtual concat, an 8-channel layer) stays exact."""
import torch

from bf16_emul_2d import Bf16Conv2d, norm_first


def _conv3x3(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]


def small(model):
    """the 3x3 Conv2d modules of `model` (a UNet2D) on the small-Cin kernels under native_2d_stem, in module order"""
    first_of_decoder = {id(dec.basic_module.SingleConv1.conv) for dec in model.decoders}  # (their input is a concat)
    return [m for m in _conv3x3(model) if m.in_channels <= 4 and m.out_channels <= 32 and id(m) not in first_of_decoder]


def eligible(model):
    """the 3x3 Conv2d modules of `model` that run on the bf16 kernels under native_2d_bf16 + native_2d_stem, in module order"""
    first_of_decoder = {id(dec.basic_module.SingleConv1.conv) for dec in model.decoders}
    pre = norm_first(model.layer_order)
    exact = {id(m) for m in small(model)}
    out = []
    for mod in _conv3x3(model):
        if id(mod) in exact or mod.in_channels % 16 or mod.out_channels % 16:
            continue
        if id(mod) in first_of_decoder and not pre:
            continue  # (its input stays a virtual concat: fp32 kernels)
        out.append(mod)
    return out


def c16(model):
    """... those among them outside the rule of native_2d_bf16 alone (both counts multiples of 32): the `_c16` entry points"""
    return [m for m in eligible(model) if m.in_channels % 32 or m.out_channels % 32]


_KEYS = ("native_2d", "native_2d_bf16", "native_2d_stem", "compute_dtype")


def build(cfg, sd, emulate: bool):
    """the float64 module tree of `cfg` with the parameters `sd`; emulate: the eligible convolutions round their operands"""
    from pytorch3dunet_amd.unet3d.model import get_model

    model = get_model({k: v for k, v in cfg.items() if k not in _KEYS}).double()
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
