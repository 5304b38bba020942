"""Float64 CPU emulation of a ResidualUNet2D under `native_2d_residual_bf16_deconv`: the tree of tests/bf16_emul_res2d.py (every eligible
3x3 Conv2d rounds the operands of its three GEMMs to bf16) in which, in addition, every eligible ConvTranspose2d of the decoders is
replaced by an autograd function that does the same for the transposed convolution (csrc/u3d_conv2d_bf16.hip, u3d_convtr2d_*_bf16):
  forward:          x and w,
  data gradient:    dt and w,
  weight gradient:  x and dt —
rounded to nearest even, accumulated in float64.  The nearest resize, the join, the 1x1 convolutions, the norms, pooling and the head are
exact.

The eligibility rule is RESTATED here, not imported from the engine (tests/test_native2d_residual_bf16_deconv.py holds the two against
each other): a ConvTranspose2d with both channel counts multiples of 32."""
import torch
import torch.nn.functional as F

import bf16_emul_res2d as E3
from bf16_emul_2d import Bf16Conv2d, r16


class Bf16ConvTranspose2d(torch.autograd.Function):
    """conv_transpose2d(x, w, stride=2, padding=1) whose three GEMMs see bf16-rounded operands (`round_ops` False: exact operands)"""

    @staticmethod
    def forward(ctx, x, w, round_ops=True):
        ctx.save_for_backward(x, w)
        ctx.rnd = r16 if round_ops else (lambda t: t)
        return F.conv_transpose2d(ctx.rnd(x), ctx.rnd(w), stride=2, padding=1)

    @staticmethod
    def backward(ctx, dt):
        x, w = ctx.saved_tensors
        rnd = ctx.rnd
        dtr = rnd(dt)
        # the operator is bilinear: each gradient is autograd's own of the same operator with the OTHER operand rounded (so that with
        # the rounding switched off this is the plain float64 backward, bit for bit)
        with torch.enable_grad():
            xa, wa = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
            dx, = torch.autograd.grad(F.conv_transpose2d(xa, rnd(w).detach(), stride=2, padding=1), xa, dtr)
            dw, = torch.autograd.grad(F.conv_transpose2d(rnd(x).detach(), wa, stride=2, padding=1), wa, dtr)
        return dx, dw, None


def convtr(model):
    """every ConvTranspose2d of `model` in module order"""
    return [m for m in model.modules() if isinstance(m, torch.nn.ConvTranspose2d)]


def eligible_convtr(model):
    """the ConvTranspose2d modules of `model` (a ResidualUNet2D) that run on the bf16 kernels under native_2d_residual_bf16_deconv"""
    return [m for m in convtr(model) if m.in_channels % 32 == 0 and m.out_channels % 32 == 0]


_DROP = ("native_2d", "native_2d_residual", "native_2d_residual_bf16", "native_2d_residual_bf16_deconv", "compute_dtype",
         "activation_dtype")


def build(cfg, sd, emulate: bool, round_ops: bool = True):
    """the float64 module tree of `cfg` with the parameters `sd`; emulate: the eligible 3x3 and transposed convolutions go through the
    emulating functions (`round_ops` False: through the same functions with the rounding switched off)"""
    from pytorch3dunet_amd.unet3d.model import get_model

    model = get_model({k: v for k, v in cfg.items() if k not in _DROP}).double()
    model.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    if emulate:
        if round_ops:
            for conv in E3.eligible(model):
                def fwd(x, conv=conv):
                    y = Bf16Conv2d.apply(x, conv.weight)
                    return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1)

                conv.forward = fwd
        for ct in eligible_convtr(model):
            assert ct.kernel_size == (3, 3) and ct.stride == (2, 2) and ct.padding == (1, 1) and ct.bias is None

            def fwd_t(x, output_size=None, ct=ct):  # (the module's own output size IS 2n - 1: no output padding)
                return Bf16ConvTranspose2d.apply(x, ct.weight, round_ops)

            ct.forward = fwd_t
    return model.train()


def run(cfg, sd, x, target, loss_name: str, emulate: bool, round_ops: bool = True):
    """(logits, loss, {name: grad}) of one training step in float64"""
    from conftest import loss_by_name

    model = build(cfg, sd, emulate, round_ops)
    probs, logits = model(x.double(), return_logits=True)
    loss = loss_by_name(loss_name, probs, logits, target.double())
    loss.backward()
    return logits.detach(), loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}
