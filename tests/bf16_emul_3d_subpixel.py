"""TEST HELPER (not a test): float64 CPU emulation of a UNet3D under `bf16_subpixel` (on top of `compute_dtype: bf16`), the 3-D twin of
tests/bf16_emul_2d_subpixel.py.  Every 3x3x3 Conv3d the executor routes to the bf16 kernels (csrc/u3d_bf16.hip) rounds the operands of
its three GEMMs to bf16 and accumulates in float64; the first convolution of an ELIGIBLE decoder becomes an autograd function with the
rounding points of the sub-pixel bf16 kernels (csrc/u3d_subpix_bf16.hip):
  weights      the pre-summed taps are added in fp32 from the fp32 master weight (ascending (tz, ty, tx) order), then rounded ONCE to
               bf16; the skip half's taps are rounded one by one (the 27-tap kernels);
  activations  the convolution input (after the norm in front of it) and dz are rounded once;
  accumulation float64.
After the norm the upsampled half of the concat is an exact 2x replication, so the low-res operand is x[:, C0:, ::2, ::2, ::2]; the
low-res gradient (children sum included) is placed on ONE child of every low-res voxel — the norm backward in front depends on the
children sums only.

The eligibility rules are RESTATED here, not imported from the engine (tests/test_bf16_subpixel3d.py holds the two against each other):
a 3x3x3 convolution runs on the bf16 kernels when both channel counts are multiples of 32 and its input is a single tensor — with a
norm-first layer order the decoders' first convolutions qualify too; a decoder's first convolution takes the sub-pixel path when the layer
order is norm-first, its level upsamples by exactly 2 on all three axes at this input size (floor pooling) and C0 % 32 == C1 % 32 ==
Cout % 32 == 0.

Model cases: chosen on the CPU so that the emulation's own distance from the plain float64 run is at most 2/3 of each bar (logits 3e-2
of their range, global gradient rel-L2 0.15, i.e. 2e-2 and 0.10).  Two starting cases were dropped for sitting near the gradient bar on
the emulation alone — the 3-level f_maps-32 net at (1, 1, 16, 32, 32): 0.101, and at (1, 1, 12, 20, 26): 0.137 (a ReLU net's gradient
jumps where bf16 rounding flips a mask, and few voxels average few flips) — and replaced by the same net on more voxels: (2, 1, 16, 32,
32): 0.073, and (2, 1, 16, 32, 26), which keeps the 6 -> 13 axis: 0.082.  The bars themselves are untouched."""
import itertools

import torch
import torch.nn.functional as F

# per axis: taps of parity p that read low-res offset (p - 1 + e); taps that dz[2j - 1 + r], r = 0..3, carries in the gradient of low[j]
TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
DGRAD_TAPS = ((2,), (1, 2), (0, 1), (0,))
P3 = tuple(itertools.product((0, 1), repeat=3))


def identity(t):
    return t


def r16(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def _shifted(low, p):
    """zero-padded low-res tensor such that a VALID 2x2x2 correlation yields, at j, the sum over e of low[j + p - 1 + e]"""
    return F.pad(low, [1 - p[2], p[2], 1 - p[1], p[1], 1 - p[0], p[0]])  # F.pad order: last dimension first


def _presum(w):
    """w (Cout, C1, 3, 3, 3) -> {(pz, py, px): (Cout, C1, 2, 2, 2)}, the taps added in ascending (tz, ty, tx) order in w's dtype"""
    out = {}
    for p in P3:
        k = torch.zeros(w.shape[0], w.shape[1], 2, 2, 2, dtype=w.dtype)
        for e in P3:
            for tz in TAPS[(p[0], e[0])]:
                for ty in TAPS[(p[1], e[1])]:
                    for tx in TAPS[(p[2], e[2])]:
                        k[:, :, e[0], e[1], e[2]] += w[:, :, tz, ty, tx]
        out[p] = k
    return out


def presum_fwd(w1, rnd=r16):
    """the 2x2x2 kernels of the eight parity classes as the pack kernel writes them — fp32 sums of the fp32 taps, rounded once (rnd =
    identity: float64 sums, no rounding)"""
    if rnd is identity:
        return _presum(w1.double())
    return {p: rnd(k).double() for p, k in _presum(w1.float()).items()}


def presum_dgrad(w1, rnd=r16):
    """{(ez, ey, ex): (Cout, C1) float64}: the 64 matrices of the 4 x 4 x 4 stride-2 gather, summed and rounded the same way"""
    w = w1.double() if rnd is identity else w1.float()
    out = {}
    for e in itertools.product(range(4), repeat=3):
        k = torch.zeros_like(w[:, :, 0, 0, 0])
        for tz in DGRAD_TAPS[e[0]]:
            for ty in DGRAD_TAPS[e[1]]:
                for tx in DGRAD_TAPS[e[2]]:
                    k = k + w[:, :, tz, ty, tx]
        out[e] = rnd(k).double()
    return out


def up_forward(low, kernels):
    """the eight parity-class 2x2x2 convolutions of `low` (N, C1, D1, H1, W1; already rounded) with the kernels of presum_fwd"""
    N, _, D1, H1, W1 = low.shape
    y = torch.zeros(N, next(iter(kernels.values())).shape[0], 2 * D1, 2 * H1, 2 * W1, dtype=torch.float64)
    for p, k in kernels.items():
        y[:, :, p[0]::2, p[1]::2, p[2]::2] = F.conv3d(_shifted(low.double(), p), k)
    return y


def up_dgrad(dz, mats):
    """dlow (N, C1, D1, H1, W1) from dz (N, Cout, 2 D1, 2 H1, 2 W1; already rounded) with the matrices of presum_dgrad"""
    N, _, D, H, W = dz.shape
    D1, H1, W1 = D // 2, H // 2, W // 2
    dzp = F.pad(dz.double(), [1, 1, 1, 1, 1, 1])
    dlow = torch.zeros(N, mats[(0, 0, 0)].shape[1], D1, H1, W1, dtype=torch.float64)
    for (ez, ey, ex), k in mats.items():
        dlow += torch.einsum("nkzyx,kc->nczyx", dzp[:, :, ez:ez + 2 * D1:2, ey:ey + 2 * H1:2, ex:ex + 2 * W1:2], k)
    return dlow


def up_wgrad(low, dz):
    """dw (Cout, C1, 3, 3, 3) of the upsampled half from the already rounded operands: the 64 (class, tap half) matrices folded 8 per tap"""
    low, dz = low.double(), dz.double()
    N, C1, D1, H1, W1 = low.shape
    dw = torch.zeros(dz.shape[1], C1, 3, 3, 3, dtype=torch.float64)
    for p in P3:
        dzp = dz[:, :, p[0]::2, p[1]::2, p[2]::2]
        lp = _shifted(low, p)
        for e in P3:
            a = lp[:, :, e[0]:e[0] + D1, e[1]:e[1] + H1, e[2]:e[2] + W1]
            m = torch.einsum("nkzyx,nczyx->kc", dzp, a)
            for tz in TAPS[(p[0], e[0])]:
                for ty in TAPS[(p[1], e[1])]:
                    for tx in TAPS[(p[2], e[2])]:
                        dw[:, :, tz, ty, tx] += m
    return dw


class Bf16Conv3d(torch.autograd.Function):
    """conv3d(x, w, padding=1) whose three GEMMs see bf16-rounded operands"""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return F.conv3d(r16(x), r16(w), padding=1)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        dzr = r16(dz)
        return torch.nn.grad.conv3d_input(x.shape, r16(w), dzr, padding=1), torch.nn.grad.conv3d_weight(r16(x), w.shape, dzr, padding=1)


class SubpixelBf16Conv3d(torch.autograd.Function):
    """conv3d(cat(skip, nearest2x(low)), w, padding=1) as the executor runs it under `bf16_subpixel`; x is the normed concat"""

    @staticmethod
    def forward(ctx, x, w, C0, rnd):
        ctx.save_for_backward(x, w)
        ctx.C0, ctx.rnd = C0, rnd
        skip, low = x[:, :C0], x[:, C0:, ::2, ::2, ::2]
        return F.conv3d(rnd(skip), rnd(w[:, :C0]), padding=1) + up_forward(rnd(low), presum_fwd(w[:, C0:], rnd)).to(x.dtype)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        C0, rnd = ctx.C0, ctx.rnd
        skip, low = x[:, :C0], x[:, C0:, ::2, ::2, ::2]
        dzr = rnd(dz)
        dx = torch.zeros_like(x)
        dx[:, :C0] = torch.nn.grad.conv3d_input(skip.shape, rnd(w[:, :C0]), dzr, padding=1)
        dx[:, C0:, ::2, ::2, ::2] = up_dgrad(dzr, presum_dgrad(w[:, C0:], rnd)).to(x.dtype)
        dw0 = torch.nn.grad.conv3d_weight(rnd(skip), w[:, :C0].shape, dzr, padding=1)
        dw1 = up_wgrad(rnd(low), dzr).to(x.dtype)
        return dx, torch.cat((dw0, dw1), dim=1), None, None


def norm_first(layer_order: str) -> bool:
    i = layer_order.index("c")
    return any(ch in layer_order[:i] for ch in "gb")


def eligible(model):
    """the 3x3x3 Conv3d modules of `model` (a UNet3D) that run on the bf16 kernels under `compute_dtype: bf16`, in module order"""
    first_of_decoder = {id(dec.basic_module.SingleConv1.conv) for dec in model.decoders}
    pre = norm_first(model.layer_order)
    out = []
    for mod in model.modules():
        if not (isinstance(mod, torch.nn.Conv3d) and mod.kernel_size == (3, 3, 3)):
            continue
        if mod.in_channels % 32 or mod.out_channels % 32:
            continue
        if id(mod) in first_of_decoder and not pre:
            continue  # (its input stays a virtual concat: fp32 kernels)
        out.append(mod)
    return out


def level_sizes(model, size):
    """(D, H, W) of every encoder level at input `size` (N, C, D, H, W): floor pooling by 2 per level"""
    dims = [tuple(size[2:])]
    for _ in range(len(model.encoders) - 1):
        dims.append(tuple(d // 2 for d in dims[-1]))
    return dims


def eligible_subpixel(model, size):
    """{conv module of a decoder's first convolution: (C0, C1)} for the decoders that take the sub-pixel bf16 path at this input size"""
    if not norm_first(model.layer_order) or type(model).__name__ != "UNet3D":
        return {}
    if any(getattr(dec.upsampling, "mode", "nearest") != "nearest" or hasattr(getattr(dec.upsampling, "upsample", None), "conv_transposed")
           for dec in model.decoders):
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


_DROP = ("bf16_subpixel", "compute_dtype", "checkpoint_encoders", "checkpoint_levels", "hip_graph")


def build(cfg, sd, size, emulate: bool, rnd=r16):
    """the float64 module tree of `cfg` with the parameters `sd`; emulate: the eligible decoder convolutions run in the sub-pixel form,
    every other bf16-routed convolution rounds its operands.  rnd = identity switches every rounding off."""
    from pytorch3dunet_amd.unet3d.model import get_model

    model = get_model({k: v for k, v in cfg.items() if k not in _DROP}).double()
    model.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    if emulate:
        sub = eligible_subpixel(model, size)
        if rnd is not identity:
            for conv in eligible(model):
                if conv in sub:
                    continue

                def fwd(x, conv=conv):
                    y = Bf16Conv3d.apply(x, conv.weight)
                    return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1, 1)

                conv.forward = fwd
        for conv, (C0, _) in sub.items():
            def fwd(x, conv=conv, C0=C0):
                y = SubpixelBf16Conv3d.apply(x, conv.weight, C0, rnd)
                return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1, 1)

            conv.forward = fwd
    return model.train()


def run(cfg, sd, x, target, loss_name: str, emulate: bool, rnd=r16):
    """(logits, loss, {name: grad}) of one training step in float64"""
    from conftest import loss_by_name

    model = build(cfg, sd, tuple(x.shape), emulate, rnd)
    probs, logits = model(x.double(), return_logits=True)
    loss = loss_by_name(loss_name, probs, logits, target.double())
    loss.backward()
    return logits.detach(), loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


# ---- the model cases of tests/test_bf16_subpixel3d.py (emulation alone, CPU) and tests/test_gpu_model_bf16_subpixel.py --------------------
BF16_LOGITS_TOL = 3e-2  # the stated bf16 tolerances of tests/test_gpu_bf16.py: logits within 3 % of their range ...
BF16_GRAD_TOL = 0.15    # ... and the global relative L2 distance of all parameter gradients within 15 % of the plain run
_NET3 = dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=32, num_levels=3, layer_order="gcr", num_groups=8)
MODEL_CASES = [
    (_NET3, (2, 1, 16, 32, 32)),   # both decoders eligible
    (_NET3, (2, 1, 16, 32, 26)),   # top decoder eligible; bottom: 6 -> 13 along x is n -> 2n + 1, its concat is written out
    (dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="bcr"), (2, 1, 8, 16, 16)),
    (dict(name="UNet3D", in_channels=2, out_channels=2, f_maps=[32, 64], final_sigmoid=False, num_groups=8), (1, 2, 8, 12, 20)),
]
NO_ELIGIBLE_SHAPE = (1, 1, 11, 15, 19)  # _NET3 here: 11 -> 5 -> 2, 15 -> 7 -> 3, 19 -> 9 -> 4: every level upsamples n -> 2n + 1
# a net with no level inside the channel rule at any size (C0 = 24 / 48).  (f_maps [16, 32, 64] is NOT such a net: its bottom decoder
# joins 32 skip and 64 upsampled channels into 32 — inside the rule wherever that level is an exact 2x.)
NET_OUTSIDE_CHANNEL_RULE = dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=[24, 48, 96], layer_order="gcr", num_groups=4)


def prep(cfg, shape, **extra):
    """model, parameters, input and target of one case: seed 99"""
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
