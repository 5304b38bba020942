"""TEST HELPER (not a test): float64 CPU emulation of a UNet2D under `native_2d_bf16_subpixel`, extending tests/bf16_emul_2d.py.  The first
convolution of an ELIGIBLE decoder becomes an autograd function with the rounding points of the sub-pixel bf16 kernels
(csrc/u3d_conv2d_bf16.hip), built on the identities of tests/subpixel2d_ref.py:
  weights      the pre-summed taps are added in fp32 from the fp32 master weight (ascending (ty, tx) order), then rounded ONCE to bf16;
               the skip half's taps are rounded one by one (the 9-tap kernels);
  activations  the convolution input (after the norm in front of it) and dz are rounded once;
  accumulation float64.
After the norm the upsampled half of the concat is an exact 2x replication, so the low-res operand is x[:, C0:, ::2, ::2]; the low-res
gradient (children sum included) is placed on ONE child of every low-res pixel — the norm backward in front depends on the children sums
only.  Every other eligible layer rounds as in bf16_emul_2d.py.

The eligibility rule is RESTATED here, not imported from the engine (tests/test_native2d_bf16_subpixel.py holds the two against each
other): a decoder's first convolution qualifies when the layer order is norm-first, its level upsamples by exactly 2 on both axes at this
input size (H == 2 * H1 and W == 2 * W1 under floor pooling), and C0 % 32 == C1 % 32 == Cout % 32 == 0."""
import itertools

import torch
import torch.nn.functional as F

import bf16_emul_2d as E
import subpixel2d_ref as S


def identity(t):
    return t


def presum_fwd(w1, rnd=E.r16):
    """{(py, px): (Cout, C1, 2, 2) float64}: the 2x2 kernels of the four parity classes as the pack kernel writes them — fp32 sums of the
    fp32 taps, rounded once (rnd = identity: float64 sums, no rounding)"""
    if rnd is identity:
        return S.presum_weights(w1.double())
    return {p: rnd(k).double() for p, k in S.presum_weights(w1.float()).items()}


def presum_dgrad(w1, rnd=E.r16):
    """{(ey, ex): (Cout, C1) float64}: the sixteen matrices of the 4 x 4 stride-2 gather, summed and rounded the same way"""
    w = w1.double() if rnd is identity else w1.float()
    out = {}
    for ey, ex in itertools.product(range(4), repeat=2):
        k = torch.zeros_like(w[:, :, 0, 0])
        for ty in S.DGRAD_TAPS[ey]:
            for tx in S.DGRAD_TAPS[ex]:
                k = k + w[:, :, ty, tx]
        out[(ey, ex)] = rnd(k).double()
    return out


def up_forward(low, kernels):
    """the four parity-class 2x2 convolutions of `low` (N, C1, H1, W1; already rounded) with the kernels of presum_fwd"""
    N, _, H1, W1 = low.shape
    y = torch.zeros(N, next(iter(kernels.values())).shape[0], 2 * H1, 2 * W1, dtype=torch.float64)
    for p, k in kernels.items():
        y[:, :, p[0]::2, p[1]::2] = F.conv2d(S._shifted(low.double(), p), k)
    return y


def up_dgrad(dz, mats):
    """dlow (N, C1, H1, W1) from dz (N, Cout, 2 H1, 2 W1; already rounded) with the matrices of presum_dgrad"""
    N, _, H, W = dz.shape
    H1, W1 = H // 2, W // 2
    dzp = F.pad(dz.double(), [1, 1, 1, 1])
    dlow = torch.zeros(N, mats[(0, 0)].shape[1], H1, W1, dtype=torch.float64)
    for (ey, ex), k in mats.items():
        dlow += torch.einsum("nkyx,kc->ncyx", dzp[:, :, ey:ey + 2 * H1:2, ex:ex + 2 * W1:2], k)
    return dlow


def up_wgrad(low, dz):
    """dw (Cout, C1, 3, 3) of the upsampled half from the already rounded operands (the sixteen matrices folded 4 per tap)"""
    return S.wgrad(low.double(), dz.double())


class SubpixelBf16Conv2d(torch.autograd.Function):
    """conv2d(cat(skip, nearest2x(low)), w, padding=1) as the executor runs it under `native_2d_bf16_subpixel`; x is the normed concat"""

    @staticmethod
    def forward(ctx, x, w, C0, rnd):
        ctx.save_for_backward(x, w)
        ctx.C0, ctx.rnd = C0, rnd
        skip, low = x[:, :C0], x[:, C0:, ::2, ::2]
        return F.conv2d(rnd(skip), rnd(w[:, :C0]), padding=1) + up_forward(rnd(low), presum_fwd(w[:, C0:], rnd)).to(x.dtype)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        C0, rnd = ctx.C0, ctx.rnd
        skip, low = x[:, :C0], x[:, C0:, ::2, ::2]
        dzr = rnd(dz)
        dx = torch.zeros_like(x)
        dx[:, :C0] = torch.nn.grad.conv2d_input(skip.shape, rnd(w[:, :C0]), dzr, padding=1)
        dx[:, C0:, ::2, ::2] = up_dgrad(dzr, presum_dgrad(w[:, C0:], rnd)).to(x.dtype)
        dw0 = torch.nn.grad.conv2d_weight(rnd(skip), w[:, :C0].shape, dzr, padding=1)
        dw1 = up_wgrad(rnd(low), dzr).to(x.dtype)
        return dx, torch.cat((dw0, dw1), dim=1), None, None


def level_sizes(model, size):
    """(H, W) of every encoder level at input `size` (N, C, H, W): floor pooling by 2 per level"""
    dims = [tuple(size[2:])]
    for _ in range(len(model.encoders) - 1):
        dims.append(tuple(d // 2 for d in dims[-1]))
    return dims


def eligible_subpixel(model, size):
    """{conv module of a decoder's first convolution: (C0, C1)} for the decoders that take the sub-pixel bf16 path at this input size"""
    if not E.norm_first(model.layer_order):
        return {}
    dims = level_sizes(model, size)
    L = len(model.encoders)
    out = {}
    for j, dec in enumerate(model.decoders):
        conv = dec.basic_module.SingleConv1.conv
        skip_lvl, low_lvl = L - 2 - j, L - 1 - j
        C0 = model.encoders[skip_lvl].basic_module.SingleConv2.conv.out_channels
        C1 = conv.in_channels - C0
        exact2x = all(a == 2 * b for a, b in zip(dims[skip_lvl], dims[low_lvl]))
        if exact2x and C0 > 0 and C1 > 0 and C0 % 32 == 0 and C1 % 32 == 0 and conv.out_channels % 32 == 0:
            out[conv] = (C0, C1)
    return out


def build(cfg, sd, size, emulate: bool, rnd=E.r16):
    """the float64 module tree of `cfg` with the parameters `sd`; emulate: the eligible decoder convolutions run in the sub-pixel form,
    every other eligible convolution as in bf16_emul_2d.  rnd = identity switches every rounding of the sub-pixel layers off."""
    drop = ("native_2d_bf16_subpixel", "native_2d_bf16_vcat", "native_2d_stem")
    model = E.build({k: v for k, v in cfg.items() if k not in drop}, sd, emulate and rnd is not identity)
    if emulate:
        for conv, (C0, _) in eligible_subpixel(model, size).items():
            def fwd(x, conv=conv, C0=C0):
                y = SubpixelBf16Conv2d.apply(x, conv.weight, C0, rnd)
                return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1)

            conv.forward = fwd
    return model.train()


def run(cfg, sd, x, target, loss_name: str, emulate: bool, rnd=E.r16):
    """(logits, loss, {name: grad}) of one training step in float64"""
    from conftest import loss_by_name

    model = build(cfg, sd, tuple(x.shape), emulate, rnd)
    probs, logits = model(x.double(), return_logits=True)
    loss = loss_by_name(loss_name, probs, logits, target.double())
    loss.backward()
    return logits.detach(), loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


# ---- the model cases of tests/test_native2d_bf16_subpixel.py (emulation alone, CPU) and tests/test_gpu_model2d_bf16_subpixel.py ----------
BF16_LOGITS_TOL = 3e-2  # the stated bf16 tolerances of tests/test_gpu_model2d_bf16.py: logits within 3 % of their range ...
BF16_GRAD_TOL = 0.15    # ... and the global relative L2 distance of all parameter gradients within 15 % of the plain run
_NET3 = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="gce", num_groups=8)
MODEL_CASES = [
    (_NET3, (2, 1, 32, 40), {}),                                 # both decoders eligible
    (_NET3, (2, 1, 36, 42), {}),                                 # top decoder eligible, bottom 10 -> 21 is not: written-out concat ...
    (_NET3, (2, 1, 36, 42), dict(native_2d_bf16_vcat=True)),     # ... or the `_src` entry points
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="bcr"), (2, 1, 32, 32), {}),
    (dict(name="UNet2D", in_channels=2, out_channels=3, f_maps=[32, 64], final_sigmoid=False, num_groups=8), (1, 2, 24, 40), {}),
]
NO_ELIGIBLE_SHAPE = (2, 1, 35, 45)  # _NET3 here: 35 -> 17 -> 8 and 45 -> 22 -> 11, every level upsamples n -> 2n + 1 on some axis


def prep(cfg, shape, **extra):
    """model, parameters, input and target of one case: seed 99, as `_prep` of tests/test_gpu_model2d_bf16.py prepares them"""
    from pytorch3dunet_amd.unet3d.model import get_model

    torch.manual_seed(99)
    model = get_model(dict(cfg, **extra))
    with torch.no_grad():  # a trained-like net: the default norm init (gamma 1, beta 0) hides half of the gradient paths
        for k, p in model.named_parameters():
            if "groupnorm" in k or "batchnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(shape)
    target = (torch.rand((shape[0], cfg["out_channels"]) + tuple(shape[2:])) > 0.5).float()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model, sd, x, target


def loss_name_of(cfg):
    return "bce_dice" if cfg.get("final_sigmoid", True) else "probs_sum"


def distances(a, b):
    """(logits distance relative to the range of b's logits, global gradient rel-L2) of two run() results"""
    import unet3d_oracle as orc

    keys = list(b[2])
    cat = lambda d: torch.cat([d[k].flatten().double() for k in keys])  # noqa: E731
    ga, gb = cat(a[2]), cat(b[2])
    return orc.rel_err(a[0].double(), b[0]), ((ga - gb).norm() / gb.norm()).item()
