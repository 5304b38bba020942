"""TEST HELPER (not a test): float64 CPU emulation of a UNet3D under `bf16_stem` (on top of `compute_dtype: bf16`, optionally next to
`bf16_subpixel`), built on tests/bf16_emul_3d_subpixel.py.  A 16-channel layer on the kernels of csrc/u3d_c16_bf16.hip has the rounding
points of every 27-tap bf16 layer, restated:
  weights      every tap of the fp32 master weight rounded ONCE to bf16, nearest even (forward and data gradient read the same values);
  activations  the convolution input — after the fp32 affine of the norm in front of it — and dz rounded once; zero padding stays 0;
  accumulation float64 here (fp32 on the device).
So the emulation is `SE.Bf16Conv3d` on a wider set of layers, and that set — THE rule — is restated here, not imported from the engine
(tests/test_bf16_stem3d.py holds the two against each other): a 3x3x3 convolution of a UNet3D (DoubleConv blocks) runs on the new kernels
when the key is on, both channel counts are multiples of 16 but not both of 32, and its input is one real tensor — a decoder's first
convolution qualifies with a norm-first layer order only (its concat is then written out); in a post-norm order it stays a virtual concat
on the fp32 kernels.  8-channel layers (8 -> 16 at `f_maps: 16`) and the Cin <= 4 first layer stay on the fp32 / small-Cin kernels.

Model cases: the emulation's own distance from the plain float64 run, measured on the CPU by tests/test_bf16_stem3d.py (logits relative
to their range / global gradient rel-L2), against the bars 3e-2 / 0.15 — a case is held to gate 2 on the GPU only if both figures are
inside 2/3 of the bars (2e-2 / 0.10): `GATE2` lists those cases, computed there and asserted."""
import torch

import bf16_emul_3d_subpixel as SE

BF16_LOGITS_TOL, BF16_GRAD_TOL = SE.BF16_LOGITS_TOL, SE.BF16_GRAD_TOL


def _is_3x3x3(mod):
    return isinstance(mod, torch.nn.Conv3d) and mod.kernel_size == (3, 3, 3)


def _first_of_decoder(model):
    return {id(dec.basic_module.SingleConv1.conv) for dec in model.decoders}


def routed_c16(model, key=True):
    """the Conv3d modules of `model` on the 16-channel bf16 kernels under `bf16_stem`, in module order ([]: key off, residual classes)"""
    if not key or type(model).__name__ != "UNet3D":
        return []
    pre, first = SE.norm_first(model.layer_order), _first_of_decoder(model)
    out = []
    for mod in model.modules():
        if not _is_3x3x3(mod):
            continue
        ci, co = mod.in_channels, mod.out_channels
        if ci % 16 or co % 16 or (ci % 32 == 0 and co % 32 == 0):
            continue
        if id(mod) in first and not pre:
            continue  # (its input stays a virtual concat: fp32 kernels)
        out.append(mod)
    return out


def fp32_mfma_layers(model, key=True):
    """the 3x3x3 Conv3d modules that stay on the fp32 MFMA kernels in bf16 mode: outside both channel rules (or a post-norm decoder's first
    convolution), and not the Cin <= 4 first layer of the small-Cin kernels"""
    bf16 = {id(m) for m in SE.eligible(model)} | {id(m) for m in routed_c16(model, key)}
    return [m for m in model.modules() if _is_3x3x3(m) and id(m) not in bf16 and not (m.in_channels <= 4 and m.out_channels <= 32)]


_DROP = SE._DROP + ("bf16_stem",)


def build(cfg, sd, size, emulate: bool):
    """the float64 module tree of `cfg` with the parameters `sd`; emulate: every convolution the executor routes to a bf16 kernel under
    the keys of `cfg` (`bf16_stem`, `bf16_subpixel`) rounds its operands as that kernel does"""
    from pytorch3dunet_amd.unet3d.model import get_model

    model = get_model({k: v for k, v in cfg.items() if k not in _DROP}).double()
    model.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    if emulate:
        # (`bf16_subpixel` asks `_cat_bf16` first: under both keys a level with 16-channel halves keeps its written-out concat — the
        # restated sub-pixel rule wants C0 % 32 == C1 % 32 == Cout % 32 == 0 already)
        sub = SE.eligible_subpixel(model, size) if cfg.get("bf16_subpixel") else {}
        for conv in SE.eligible(model) + routed_c16(model, cfg.get("bf16_stem", False)):
            if conv in sub:
                continue

            def fwd(x, conv=conv):
                y = SE.Bf16Conv3d.apply(x, conv.weight)
                return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1, 1)

            conv.forward = fwd
        for conv, (C0, _) in sub.items():
            def fwd(x, conv=conv, C0=C0):
                y = SE.SubpixelBf16Conv3d.apply(x, conv.weight, C0, SE.r16)
                return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1, 1)

            conv.forward = fwd
    return model.train()


def run(cfg, sd, x, target, loss_name: str, emulate: bool):
    """(logits, loss, {name: grad}) of one training step in float64"""
    from conftest import loss_by_name

    model = build(cfg, sd, tuple(x.shape), emulate)
    probs, logits = model(x.double(), return_logits=True)
    loss = loss_by_name(loss_name, probs, logits, target.double())
    loss.backward()
    return logits.detach(), loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


loss_name_of, distances = SE.loss_name_of, SE.distances


def prep(cfg, shape, seed=99, **extra):
    """model, parameters, input and target of one case (SE.prep with the case's seed)"""
    from pytorch3dunet_amd.unet3d.model import get_model

    torch.manual_seed(seed)
    model = get_model(dict(cfg, **extra))
    with torch.no_grad():  # a trained-like net: the default norm init (gamma 1, beta 0) hides half of the gradient paths
        for k, p in model.named_parameters():
            if "groupnorm" in k or "batchnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(shape)
    target = (torch.rand((shape[0], cfg["out_channels"]) + tuple(shape[2:])) > 0.5).float()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model, sd, x, target


_NET16 = dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=[16, 32, 64], layer_order="gcr", num_groups=8)
# (cfg with the keys of the case, shape, seed).  Shapes are the issue's.  Seeds: a ReLU net's gradient jumps where bf16 rounding flips a
# mask, and at seed 99 (the seed of the other bf16 model tests) the emulation ALONE sits outside 2/3 of a bar in three cases — logits
# 0.0200 / gradient 0.088 (case 0), 0.0147 / 0.170 (case 1), 0.0189 / 0.168 (case 4) — so, as the issue prescribes (seeds, not bars), each
# case takes the first seed from 99 upward at which its emulation is inside 2/3 of both bars; seeds 100 .. 103 gave gradient distances
# between 0.07 and 0.18 for the [16, 32, 64] net.  The measured distances are in tests/test_gpu_model_bf16_stem.py's docstring.
MODEL_CASES = [
    (dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=32, num_levels=3, layer_order="gcr", num_groups=8, bf16_stem=True),
     (2, 1, 16, 32, 32), 102),   # the headline net: encoders.0's 16 -> 32 layer
    (dict(_NET16, bf16_stem=True), (2, 1, 16, 32, 32), 101),   # 16 -> 16, 16 -> 32 and the 48 -> 16 layer on its written-out concat
    (dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=[16, 32], layer_order="bcr", bf16_stem=True), (2, 1, 8, 16, 16), 99),
    (dict(name="UNet3D", in_channels=2, out_channels=2, f_maps=[16, 32], final_sigmoid=False, num_groups=8, bf16_stem=True),
     (1, 2, 8, 12, 20), 99),
    (dict(_NET16, bf16_stem=True, bf16_subpixel=True), (2, 1, 16, 32, 32), 101),   # ... with the bottom decoder on the sub-pixel bf16 kernels
]
# the cases whose emulation alone stays inside 2/3 of both bars: held to gate 2 on the GPU (tests/test_bf16_stem3d.py asserts this list
# against the measured distances; at least three of the five)
GATE2 = (0, 1, 2, 3, 4)
# (f_maps [32, 64], the issue's example, HAS the 16 -> 32 layer: a DoubleConv encoder's first convolution produces max(out / 2, in) channels)
NET_WITHOUT_C16_LAYER = dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=[64, 128], layer_order="gcr", num_groups=8)


def keys_of(cfg):
    return {k: cfg[k] for k in ("bf16_stem", "bf16_subpixel") if k in cfg}


def base_of(cfg):
    return {k: v for k, v in cfg.items() if k not in ("bf16_stem", "bf16_subpixel")}
