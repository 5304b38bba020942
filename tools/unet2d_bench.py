"""Training-step throughput of the reference's shipped 2-D configurations: forward + BCEDice + backward + FusedAdam, with
`native_2d: true` (csrc/u3d_conv2d.hip through the DoubleConv executor) and with the default path (the module tree on stock
PyTorch-ROCm operators, after its one-time warning) in the same process, alternating the two.  --bf16 adds the same step with
`native_2d_bf16: true` — on the ResidualUNet2D configurations `native_2d_residual_bf16: true` — (csrc/u3d_conv2d_bf16.hip for the layers
that fit) as a third path in the same alternation, and on the ResidualUNet2D configurations `native_2d_residual_bf16_deconv: true` (the
decoders' ConvTranspose2d on u3d_convtr2d_*_bf16 as well) as a fourth.  --stem adds, on the UNet2D configurations, `native_2d` +
`native_2d_stem: true` (the first layer on the small-Cin kernels of csrc/u3d_conv2d.hip) and, with --bf16, `native_2d_bf16` +
`native_2d_stem: true` (also the 16-channel layers on the `_c16` entry points) to the same alternation.

  confocal  resources/2DUnet_confocal_boundary/train_config.yml: 32 x 1 x 515 x 512, gcr, f_maps 32, 4 levels
  dsb2018   resources/2DUnet_dsb2018/train_config.yml: bcr, f_maps [32, 64, 128], batch 32 — DSB2018 images vary in size;
            32 x 1 x 256 x 256 is an ASSUMPTION of this tool, not a shape the configuration fixes
  resunet2d, resunet2d_515
            ResidualUNet2D at the reference defaults (f_maps 64, 5 levels, gcr, 8 groups) with `native_2d_residual: true`.  The reference
            ships no 2-D residual configuration: 16 x 1 x 256 x 256 and 8 x 1 x 515 x 512 are ASSUMPTIONS of this tool.  Their records
            add the transposed-convolution family (u3d_convtr2d_*: 2 * (9/4) * Cin * Cout FLOPs per output pixel and direction)

Prints one JSON line per configuration: images/s of both paths (device time over the steady-state steps only, after --warmup steps
per path), the conv2d family's ms per native step and its rate on executed FLOPs (18 * Cin * Cout * pixels per direction, from the
launches that declare them) as a fraction of the fp32 MFMA peak of 157.3 TFLOP/s.

With --bf16 the record adds the bf16 path's ms per step, images/s, its speed-up over the native fp32 step of the same process, and its
own conv2d family by entry point (the bf16 entry points' rate as TFLOP/s on executed FLOPs; the bf16 MFMA peak to hold it against is
measured with tools/mfma_bf16_peak.hip).  The ResidualUNet2D records add the deconv arm's ms per step, its speed-up over the
native_2d_residual_bf16 arm of the same run, and the transposed-convolution family of both arms by entry point (fp32 u3d_convtr2d_* in
the bf16 arm, u3d_convtr2d_*_bf16 in the deconv arm: ms per step and TFLOP/s on executed FLOPs).

With --stem the record adds each stem arm's ms per step and its speed-up over the arm it sits on in the same run, the per-call ms of
the new entry points next to the fp32 launches of the first two layers they replace (u3d_conv2d_ex_reps / u3d_conv2d_wgrad of the arm
without the key: the difference of the two arms' totals), and the new entry points' GB/s on the bytes each launch must move (inputs read
once, outputs written once) to hold against the chip's ~6.3 TB/s copy rate.

With --vcat (next to --bf16 --stem, UNet2D configurations) the alternation gains the arm `native_2d_bf16` + `native_2d_stem` +
`native_2d_bf16_vcat: true` (the decoders' first convolutions read their concat inside the bf16 kernels).  The record adds its ms per
step and its speed-up over the `native_2d_bf16` + stem arm of the same run, the per-call ms of the three `_src` entry points, of the
u3d_nearest_cat_fwd calls they replace and of the single-source bf16 calls of both arms (which the key must leave alone: the arm it sits
on has the decoders' first convolutions among them, so the comparison is on the difference of the totals), and
torch.cuda.max_memory_allocated over one step of every arm.

With --bf16-subpixel (next to --bf16 --stem --vcat) the alternation gains the arm `native_2d_bf16` + `native_2d_stem` + `native_2d_bf16_vcat` +
`native_2d_bf16_subpixel: true` (the decoders' first convolutions at exact-2x levels on the sub-pixel bf16 kernels).  The record adds its
ms per step, its speed-up over the vcat arm of the same run and the verdict against the project's bar for a speed mode (more than 5 %
faster than that arm), the levels it took, the per-call ms of the new entry points and of the `_src` calls they replace, and peak memory.

With --subpixel (UNet2D configurations) the alternation gains the arm `native_2d` + `native_2d_subpixel: true` (the upsampled half of the
decoders' first convolutions on the sub-pixel kernels of csrc/u3d_subpix2d.hip at the levels that upsample by exactly 2).  The record adds
its ms per step, its speed-up over the `native_2d` arm of the same run and the verdict against the project's bar for a speed mode (more
than 5 % faster), the decoder levels it took, the 3x3 FLOPs per image it executes (16 instead of 36 multiply-adds per low-res pixel for
the upsampled half of those levels) and the per-entry-point times of its convolution launches.

With --subpixel-plus (UNet2D configurations, next to --subpixel) the alternation gains the arm `native_2d_subpixel_plus: true` (also the
levels that upsample n -> 2n + 1 along H and / or W — two of the three levels of the 515 x 512 confocal patch — on the same kernels through a
shifted window, the 2-pixel slab on box launches of csrc/u3d_conv2d.hip).  The record adds its ms per step, its speed-up over the
`native_2d_subpixel` arm of the same run and the verdict against the same bar (more than 5 % faster than that arm), the levels it took, the
FLOPs it executes, its convolution launches by entry point and torch.cuda.max_memory_allocated over one step of every fp32 arm.

With --fp32-split (UNet2D configurations) the alternation gains the arm `native_2d_fp32_split: true` (the 3x3 layers with all channel counts
% 32 on the six-product bf16 MFMA kernels of csrc/u3d_conv2d_f32s.h, fp32 grade) and, next to --stem, the same with `native_2d_stem`.  The
record adds the arm's ms per step of every round with its median and range next to the `native_2d` arm's, whether the two ranges are
disjoint, the speed-up of the medians and the verdict against the project's bar for a speed mode (more than 5 % faster than the
`native_2d` arm of the same run), the new entry points per call next to the fp32 launches they replace (difference of the two arms'
totals), peak memory of one step per arm, and the three launches of ONE full-resolution 32 -> 32 layer on the new kernels against the
three fp32 launches they replace (HIP events around each launch, median of 5, same process).  On the ResidualUNet2D configurations
(`--configs resunet2d_515,resunet2d --fp32-split`) the arm is `native_2d_residual_fp32_split: true` against the `native_2d_residual` arm
(conv2 / conv3 of every block on the six-product kernels, conv3 with the residual epilogue u3d_conv2d_f32s_res): the same record — with
the stock arm's median and range next to them — without the one-layer timing.

  python tools/unet2d_bench.py [--configs confocal,dsb2018] [--fp32-split] [--batch N] [--steps 10] [--warmup 3] [--bf16] [--stem] [--vcat] [--bf16-subpixel] [--subpixel] [--subpixel-plus]   (--batch: every config's own default)"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-3dunet_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_TFLOPS = 157.3
CONFIGS = {
    "confocal": (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=32, num_levels=4, layer_order="gcr", num_groups=8),
                 (515, 512)),
    "dsb2018": (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="bcr"), (256, 256)),
    "resunet2d": (dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=64, num_levels=5, layer_order="gcr", num_groups=8),
                  (256, 256)),
    "resunet2d_515": (dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=64, num_levels=5, layer_order="gcr",
                           num_groups=8), (515, 512)),
}
BATCH = {"confocal": 32, "dsb2018": 32, "resunet2d": 16, "resunet2d_515": 8}


def _residual(cfg):
    return cfg["name"] == "ResidualUNet2D"


def layer_flops_per_image(cfg, hw):
    """(3x3 conv FLOPs, transposed-conv FLOPs) of one image and direction, from the layer shapes of a forward on the meta device:
    18 * Cin * Cout * pixels per 3x3 conv, 2 * (9/4) * Cin * Cout * output pixels per ConvTranspose2d"""
    from pytorch3dunet_amd.unet3d.model import get_model

    m = get_model(dict(cfg)).to("meta")
    tot = {"conv": 0.0, "convtr": 0.0}

    def hook(mod, inp, out):
        px = out.shape[-2] * out.shape[-1]
        if isinstance(mod, torch.nn.ConvTranspose2d):
            tot["convtr"] += 4.5 * mod.in_channels * mod.out_channels * px
        elif mod.kernel_size == (3, 3):
            tot["conv"] += 18.0 * mod.in_channels * mod.out_channels * px

    for mod in m.modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            mod.register_forward_hook(hook)
    with torch.no_grad():
        m._forward_modules(torch.empty((1, 1) + tuple(hw), device="meta"))
    return tot["conv"], tot["convtr"]


def conv_flops_per_image(cfg, hw, subpixel=False):
    """18 * Cin * Cout * pixels summed over the 3x3 layers (one direction), counted from the module tree.  `subpixel`: the FLOPs the
    `native_2d_subpixel` arm EXECUTES — at a decoder level that upsamples by exactly 2 (C0, C1, Cout multiples of 4) the C1 upsampled
    input channels of the first convolution cost 2 * 16 * C1 * Cout per LOW-RES pixel = 8 * C1 * Cout per output pixel instead of 18;
    `subpixel="plus"`: the `native_2d_subpixel_plus` arm — an n -> 2n + 1 level too, whose 2-pixel slab stays at 18 per output pixel"""
    from pytorch3dunet_amd.unet3d.model import get_model

    m = get_model(dict(cfg))
    H, W = hw
    tot = 0.0
    for enc in m.encoders:
        if enc.pooling is not None:
            H, W = H // 2, W // 2
        for sc in (enc.basic_module.SingleConv1, enc.basic_module.SingleConv2):
            tot += 18.0 * sc.conv.in_channels * sc.conv.out_channels * H * W
    sizes = []
    H, W = hw
    for enc in m.encoders:
        if enc.pooling is not None:
            H, W = H // 2, W // 2
        sizes.append((H, W))
    lows = sizes[1:][::-1]
    for dec, (h, w), (h1, w1) in zip(m.decoders, sizes[:-1][::-1], lows):
        for i, sc in enumerate((dec.basic_module.SingleConv1, dec.basic_module.SingleConv2)):
            ci, co = sc.conv.in_channels, sc.conv.out_channels
            c1 = (ci - co) if i == 0 else 0  # (a DoubleConv decoder's first conv: C0 = Cout skip channels, C1 = Cin - C0 upsampled)
            py, px = h - 2 * h1, w - 2 * w1
            fits = (py, px) == (0, 0) or (subpixel == "plus" and py in (0, 1) and px in (0, 1))
            if subpixel and i == 0 and fits and c1 > 0 and c1 % 4 == 0 and (ci - c1) % 4 == 0 and co % 4 == 0:
                slab = h * w - (h - 2 * py) * (w - 2 * px)  # output pixels d < 2 of the shifted axes: the plain 3x3 kernel
                tot += (18.0 * (ci - c1) * h * w + 8.0 * c1 * 4 * h1 * w1 + 18.0 * c1 * slab) * co
            else:
                tot += 18.0 * ci * co * h * w
    return tot


def make(cfg, native, dev):
    from pytorch3dunet_amd.optim import FusedAdam
    from pytorch3dunet_amd.unet3d.model import get_model

    torch.manual_seed(0)
    extra = {}
    if native == "f32s" and _residual(cfg):
        extra, native = dict(native_2d_residual_fp32_split=True), True
    elif native in ("f32s", "f32s_stem"):
        extra, native = dict(native_2d_fp32_split=True, **(dict(native_2d_stem=True) if native == "f32s_stem" else {})), True
    elif native == "subpixel":
        extra, native = dict(native_2d_subpixel=True), True
    elif native == "subpixel_plus":
        extra, native = dict(native_2d_subpixel_plus=True), True
    elif native == "bf16_stem_vcat":
        extra, native = dict(native_2d_stem=True, native_2d_bf16_vcat=True), "bf16"
    elif native == "bf16_stem_vcat_subpixel":
        extra, native = dict(native_2d_stem=True, native_2d_bf16_vcat=True, native_2d_bf16_subpixel=True), "bf16"
    elif native in ("stem", "bf16_stem"):
        extra, native = dict(native_2d_stem=True), ("bf16" if native == "bf16_stem" else True)
    if native == "bf16_deconv":
        key, native = "native_2d_residual_bf16_deconv", True
    elif native == "bf16":
        key, native = ("native_2d_residual_bf16" if _residual(cfg) else "native_2d_bf16"), True
    else:
        key = "native_2d_residual" if _residual(cfg) else "native_2d"
    m = get_model(dict(cfg, **{key: native}, **extra)).to(dev).train()
    return m, FusedAdam(m.parameters(), lr=1e-4, weight_decay=1e-5)


def step(model, opt, x, target, loss_fn):
    opt.zero_grad(set_to_none=True)
    _, logits = model(x, return_logits=True)
    loss = loss_fn(logits, target)
    loss.backward()
    opt.step()


def timed(model, opt, x, target, loss_fn, steps):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    st.record()
    for _ in range(steps):
        step(model, opt, x, target, loss_fn)
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / steps


def layer_times_f32s(batch, hw, C=32, reps=5):
    """ms of the three launches of one (C -> C) 3x3 layer at (batch, H, W) on the six-product kernels and on the fp32 kernels they
    replace: HIP events around each launch, median of `reps` after one warm-up launch"""
    import ctypes
    import statistics

    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd.engine import VSrc, _p, _stream

    dev = torch.device("cuda", 0)
    lib, ext, st = nat.get_lib(), nat.get_ext_lib(), _stream(dev)
    H, W = hw
    g = torch.Generator().manual_seed(2)
    x = torch.randn((batch, 1, H, W, C), generator=g).to(dev)
    dz = torch.randn((batch, 1, H, W, C), generator=g).to(dev)
    w = (torch.randn((C, C, 3, 3), generator=g) / (9 * C) ** 0.5).to(dev)
    aff = torch.stack((1.0 + 0.1 * torch.randn(batch, C, generator=g), 0.1 * torch.randn(batch, C, generator=g)), dim=-1).contiguous().to(dev)
    y, dw = torch.empty_like(x), torch.empty_like(w)
    stats = torch.zeros(8 * batch * C * 2, dtype=torch.float64, device=dev)
    img = {}
    for mode in (0, 1):
        img["s", mode] = torch.empty(ext.u3d_packed_weight2d_f32s_elems(C, C, mode), dtype=torch.bfloat16, device=dev)
        nat.call("u3d_pack_weights2d_f32s", 0, st, _p(w), C, C, mode, _p(img["s", mode]))
        img["f", mode] = torch.empty(lib.u3d_packed_weight2d_floats(C, C, mode), dtype=torch.float32, device=dev)
        nat.call("u3d_pack_weights2d", 0, st, _p(w), C, C, mode, _p(img["f", mode]))
    need = max(ext.u3d_wgrad2d_f32s_workspace_floats(batch, H, W, C, C), lib.u3d_wgrad2d_workspace_floats(batch, H, W, C, C),
               lib.u3d_conv2d_workspace_floats(batch, H, W, C, C), 4)
    ws = torch.empty(need, dtype=torch.float32, device=dev)
    sx, sdz, sgx = VSrc(x).struct(aff), VSrc(dz).struct(), VSrc(x).struct()
    single = (None, None, None, C, 0, 0, 0)
    launches = {
        "u3d_conv2d_f32s": lambda: nat.call("u3d_conv2d_f32s", 0, st, _p(x), *single, _p(aff), _p(img["s", 0]), _p(y), batch, H, W, C, 1,
                                            _p(stats), 8),
        "u3d_conv2d_f32s_dgrad": lambda: nat.call("u3d_conv2d_f32s_dgrad", 0, st, _p(dz), _p(img["s", 1]), _p(y), batch, H, W, C, _p(x),
                                                  *single, _p(stats), 8),
        "u3d_conv2d_wgrad_f32s": lambda: nat.call("u3d_conv2d_wgrad_f32s", 0, st, _p(x), *single, _p(aff), _p(dz), _p(dw), batch, H, W, C,
                                                  _p(ws), ws.numel()),
        "u3d_conv2d_ex_reps (forward)": lambda: nat.call("u3d_conv2d_ex_reps", 0, st, ctypes.byref(sx), _p(img["f", 0]), _p(y), batch, H, W,
                                                         C, 1, _p(stats), None, None, _p(ws), ws.numel(), 8),
        "u3d_conv2d_ex_reps (data gradient)": lambda: nat.call("u3d_conv2d_ex_reps", 0, st, ctypes.byref(sdz), _p(img["f", 1]), _p(y), batch,
                                                               H, W, C, 0, None, ctypes.byref(sgx), _p(stats), _p(ws), ws.numel(), 8),
        "u3d_conv2d_wgrad": lambda: nat.call("u3d_conv2d_wgrad", 0, st, ctypes.byref(sx), _p(dz), _p(dw), batch, H, W, C, _p(ws), ws.numel()),
    }
    out = {}
    for name, fn in launches.items():
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        out[name] = {"ms_median": round(statistics.median(ts), 4), "ms_range": [round(min(ts), 4), round(max(ts), 4)],
                     "tflops_executed": round(18.0 * C * C * batch * H * W / statistics.median(ts) / 1e9, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="confocal,dsb2018")
    ap.add_argument("--batch", type=int, default=None, help="images per step (default: the config's own, BATCH)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="alternating native / stock rounds of --steps each")
    ap.add_argument("--native-only", action="store_true", help="time the native path only (profiler runs)")
    ap.add_argument("--bf16", action="store_true", help="also time the step with native_2d_bf16 / native_2d_residual_bf16, alternated with the others")
    ap.add_argument("--stem", action="store_true", help="also time the UNet2D step with native_2d_stem next to native_2d (and, with --bf16, next to native_2d_bf16)")
    ap.add_argument("--vcat", action="store_true", help="with --bf16 --stem: also time the UNet2D step with native_2d_bf16_vcat on top of them")
    ap.add_argument("--bf16-subpixel", action="store_true", help="with --bf16 --stem --vcat: also time the UNet2D step with native_2d_bf16_subpixel on top of them")
    ap.add_argument("--subpixel", action="store_true", help="also time the UNet2D step with native_2d_subpixel next to native_2d")
    ap.add_argument("--subpixel-plus", action="store_true", help="also time the UNet2D step with native_2d_subpixel_plus (next to --subpixel)")
    ap.add_argument("--fp32-split", action="store_true", help="also time the UNet2D step with native_2d_fp32_split next to native_2d (and, with --stem, with native_2d_stem); "
                    "a ResidualUNet2D step with native_2d_residual_fp32_split next to native_2d_residual")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "unet2d_bench measures on the GPU"
    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd.unet3d.losses import BCEDiceLoss

    dev = torch.device("cuda", 0)
    loss_fn = BCEDiceLoss()  # the package's (fused u3d_bce_dice kernels on a HIP tensor), the same for both paths
    warnings.simplefilter("ignore")  # (the stock path's one-time "not covered" warning)
    for name in a.configs.split(","):
        cfg, hw = CONFIGS[name]
        batch = a.batch if a.batch is not None else BATCH[name]
        g = torch.Generator().manual_seed(1)
        x = torch.randn((batch, 1) + hw, generator=g).to(dev)
        target = (torch.rand((batch, 1) + hw, generator=g) > 0.5).float().to(dev)
        paths = [True] if a.native_only else [True, False]
        if a.bf16:
            paths.insert(1, "bf16")
            if _residual(cfg):
                paths.insert(2, "bf16_deconv")
        if a.stem and not _residual(cfg):
            paths.insert(1, "stem")
            if a.bf16:
                paths.insert(paths.index("bf16") + 1, "bf16_stem")
                if a.vcat:
                    paths.insert(paths.index("bf16_stem") + 1, "bf16_stem_vcat")
                    if a.bf16_subpixel:
                        paths.insert(paths.index("bf16_stem_vcat") + 1, "bf16_stem_vcat_subpixel")
        if a.fp32_split:  # (a ResidualUNet2D: `native_2d_residual_fp32_split`, no stem arm)
            paths.insert(1, "f32s")
            if a.stem and not _residual(cfg):
                paths.insert(2, "f32s_stem")
        if a.subpixel_plus and not _residual(cfg):
            paths.insert(1, "subpixel_plus")
        if a.subpixel and not _residual(cfg):
            paths.insert(1, "subpixel")
        runs = {p: make(cfg, p, dev) for p in paths}
        for p in paths:
            for _ in range(a.warmup):
                step(*runs[p], x, target, loss_fn)
        print(f"[unet2d_bench] {name}: warm-up done", file=sys.stderr, flush=True)
        ms = {p: [] for p in paths}
        for _ in range(a.rounds):
            for p in paths:
                ms[p].append(timed(*runs[p], x, target, loss_fn, a.steps))
        # conv2d family time in separate (event-bracketed) native steps: brackets cost a little device time each
        prof = nat.EventProfiler(flops_only=True, prealloc=4096)
        nat.profiler = prof
        step(*runs[True], x, target, loss_fn)
        torch.cuda.synchronize()
        nat.profiler = None
        fam = prof.summary()
        conv = {k: v for k, v in fam.items() if "conv2d" in k}
        c_ms = sum(v["ms"] for v in conv.values())
        c_fl = sum(v["flops"] for v in conv.values())
        fwd = {k: v for k, v in conv.items() if k in ("u3d_conv2d_ex_reps", "u3d_conv2d_res_reps")}
        per_img, tr_img = layer_flops_per_image(cfg, hw) if _residual(cfg) else (conv_flops_per_image(cfg, hw), 0.0)
        best = {p: min(v) for p, v in ms.items()}
        rec = {"config": name, "shape": [batch, 1, *hw], "order": cfg["layer_order"], "steps": a.steps, "warmup": a.warmup,
               "rounds": a.rounds, "native_ms_per_step": [round(v, 3) for v in ms[True]],
               "native_images_per_s": round(batch * 1000.0 / best[True], 2),
               "conv2d_gflop_fwd_per_image": round(per_img / 1e9, 2),
               "conv2d_family_ms_per_step": round(c_ms, 3), "conv2d_family_tflops_executed": round(c_fl / c_ms / 1e9, 2) if c_ms else None,
               "conv2d_family_fraction_of_peak": round(c_fl / c_ms / 1e9 / PEAK_TFLOPS, 3) if c_ms else None,
               "conv2d_calls": {k: {"calls": v["calls"], "ms": round(v["ms"], 3),
                                    "fraction_of_peak": round(v["flops"] / v["ms"] / 1e9 / PEAK_TFLOPS, 3) if v["ms"] else None}
                                for k, v in conv.items()},
               "conv2d_fwd_fraction_of_peak": round(sum(v["flops"] for v in fwd.values()) / sum(v["ms"] for v in fwd.values()) / 1e9 /
                                                    PEAK_TFLOPS, 3) if fwd else None,
               "device": torch.cuda.get_device_name(0)}
        if _residual(cfg):
            # the transposed-convolution family: forward, data and weight gradient (FLOPs as declared by the launches, 2 * (9/4) * Cin *
            # Cout per output pixel and direction) and everything else the native step launches, by entry point
            tr = {k: v for k, v in fam.items() if "convtr2d" in k}
            t_ms, t_fl = sum(v["ms"] for v in tr.values()), sum(v["flops"] for v in tr.values())
            rec.update(shape_is_assumption=True, convtr2d_gflop_fwd_per_image=round(tr_img / 1e9, 3),
                       convtr2d_family_ms_per_step=round(t_ms, 3),
                       convtr2d_family_fraction_of_peak=round(t_fl / t_ms / 1e9 / PEAK_TFLOPS, 3) if t_ms else None,
                       convtr2d_calls={k: {"calls": v["calls"], "ms": round(v["ms"], 3),
                                           "fraction_of_peak": round(v["flops"] / v["ms"] / 1e9 / PEAK_TFLOPS, 3) if v["ms"] and v["flops"] else None}
                                       for k, v in tr.items()},
                       other_declared_flop_ms_per_step=round(sum(v["ms"] for k, v in fam.items() if k not in conv and k not in tr), 3))
        def family_step(path):
            """entry-point summary of one event-bracketed step of `path`"""
            prof = nat.EventProfiler(flops_only=True, prealloc=4096)
            nat.profiler = prof
            step(*runs[path], x, target, loss_fn)
            torch.cuda.synchronize()
            nat.profiler = None
            return prof.summary()

        def calls(d):
            return {k: {"calls": v["calls"], "ms": round(v["ms"], 3), "tflops_executed": round(v["flops"] / v["ms"] / 1e9, 2) if v["ms"] else None}
                    for k, v in d.items()}

        if "f32s" in ms:
            # the fp32_split arm(s) against the native_2d arm of the same run: every round's ms, medians and ranges; the new entry points
            # per call and the fp32 launches they replace (difference of the two arms' totals); peak memory; one full-resolution layer
            import statistics

            def f32s_peak(path):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                step(*runs[path], x, target, loss_fn)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated(dev)

            def spread(v):
                return {"median": round(statistics.median(v), 3), "range": [round(min(v), 3), round(max(v), 3)]}

            base_med = statistics.median(ms[True])
            fp32_key = "native_2d_residual" if _residual(cfg) else "native_2d"
            rec.update(native_ms=spread(ms[True]), fp32_split_bar=f"more than 1.05x the {fp32_key} arm of the same run (medians)")
            if False in ms:
                rec.update(stock_ms=spread(ms[False]))
            for arm in [p for p in ("f32s", "f32s_stem") if p in ms]:
                afam = family_step(arm)
                new = {k: v for k, v in afam.items() if "f32s" in k}
                old = {k: {"calls": fam[k]["calls"] - afam.get(k, {"calls": 0})["calls"],
                           "ms": round(fam[k]["ms"] - afam.get(k, {"ms": 0.0})["ms"], 3)}
                       for k in ("u3d_conv2d_ex_reps", "u3d_conv2d_res_reps", "u3d_conv2d_wgrad") if k in fam}
                ratio = base_med / statistics.median(ms[arm])
                key = "fp32_split" if arm == "f32s" else "fp32_split_stem"
                rec.update({f"{key}_ms_per_step": [round(v, 3) for v in ms[arm]], f"{key}_ms": spread(ms[arm]),
                            f"{key}_images_per_s": round(batch * 1000.0 / statistics.median(ms[arm]), 2),
                            f"{key}_ranges_disjoint_from_native": bool(max(ms[arm]) < min(ms[True]) or min(ms[arm]) > max(ms[True])),
                            f"{key}_speedup_over_native_fp32": round(ratio, 4), f"{key}_meets_bar": bool(ratio > 1.05),
                            f"{key}_new_calls": calls(new), f"{key}_replaced_fp32_calls": old,
                            f"{key}_routed_layers": len(runs[arm][0]._get_engine()._split2d_weights())})
            rec.update(fp32_split_peak_memory_bytes={str(p): f32s_peak(p) for p in paths if p in (True, "stem", "f32s", "f32s_stem")})
            if not _residual(cfg):  # (a UNet2D's first routed layer; the residual configurations start at 64 channels)
                rec.update(fp32_split_layer_32_to_32_full_resolution=layer_times_f32s(batch, hw))
        if "subpixel" in ms:
            # the sub-pixel arm against the native_2d arm of the same run; its convolution launches by entry point (the three new ones
            # and the skip halves on the conv2d family), and the 3x3 FLOPs per image it executes
            spfam = family_step("subpixel")
            spconv = {k: v for k, v in spfam.items() if "conv2d" in k or "subpixel2d" in k}
            eng = runs["subpixel"][0]._get_engine()
            taken = eng._subpixel_layers((1,) + tuple(hw))
            ratio = best[True] / best["subpixel"]
            rec.update(subpixel_ms_per_step=[round(v, 3) for v in ms["subpixel"]],
                       subpixel_images_per_s=round(batch * 1000.0 / best["subpixel"], 2),
                       subpixel_speedup_over_native_fp32=round(ratio, 4),
                       subpixel_bar="more than 1.05x the native_2d arm of the same run",
                       subpixel_meets_bar=bool(ratio > 1.05),
                       subpixel_decoder_levels_taken=f"{len(taken)} of {len(eng.dec)}",
                       subpixel_conv2d_gflop_fwd_per_image_executed=round(conv_flops_per_image(cfg, hw, subpixel=True) / 1e9, 2),
                       subpixel_conv_family_ms_per_step=round(sum(v["ms"] for v in spconv.values()), 3),
                       subpixel_conv_calls=calls(spconv))
        if "subpixel_plus" in ms:
            # the plus arm against the native_2d_subpixel arm of the same run (against native_2d without --subpixel); peak memory of one
            # step per fp32 arm: a full-resolution slab scratch would show up here
            def peak_bytes(path):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                step(*runs[path], x, target, loss_fn)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated(dev)

            base = "subpixel" if "subpixel" in ms else True
            ppfam = family_step("subpixel_plus")
            ppconv = {k: v for k, v in ppfam.items() if "conv2d" in k or "subpixel2d" in k}
            eng = runs["subpixel_plus"][0]._get_engine()
            taken = eng._subpixel_layers((1,) + tuple(hw))
            ratio = best[base] / best["subpixel_plus"]
            rec.update(subpixel_plus_ms_per_step=[round(v, 3) for v in ms["subpixel_plus"]],
                       subpixel_plus_images_per_s=round(batch * 1000.0 / best["subpixel_plus"], 2),
                       subpixel_plus_speedup_over_subpixel=round(ratio, 4) if base == "subpixel" else None,
                       subpixel_plus_speedup_over_native_fp32=round(best[True] / best["subpixel_plus"], 4),
                       subpixel_plus_bar="more than 1.05x the native_2d_subpixel arm of the same run",
                       subpixel_plus_meets_bar=bool(ratio > 1.05) if base == "subpixel" else None,
                       subpixel_plus_decoder_levels_taken=f"{len(taken)} of {len(eng.dec)} ({len(taken.plus)} of them n -> 2n + 1)",
                       subpixel_plus_conv2d_gflop_fwd_per_image_executed=round(conv_flops_per_image(cfg, hw, subpixel="plus") / 1e9, 2),
                       subpixel_plus_conv_family_ms_per_step=round(sum(v["ms"] for v in ppconv.values()), 3),
                       subpixel_plus_conv_calls=calls(ppconv),
                       subpixel_plus_peak_memory_bytes={str(p): peak_bytes(p) for p in paths if p in (True, "subpixel", "subpixel_plus")})
        if "bf16" in ms:
            bfam = family_step("bf16")
            bconv = {k: v for k, v in bfam.items() if "conv2d" in k}
            rec.update(bf16_ms_per_step=[round(v, 3) for v in ms["bf16"]], bf16_images_per_s=round(batch * 1000.0 / best["bf16"], 2),
                       bf16_speedup_over_native_fp32=round(best[True] / best["bf16"], 3),
                       bf16_conv2d_family_ms_per_step=round(sum(v["ms"] for v in bconv.values()), 3),
                       bf16_conv2d_calls={k: {"calls": v["calls"], "ms": round(v["ms"], 3),
                                              "tflops_executed": round(v["flops"] / v["ms"] / 1e9, 2) if v["ms"] else None}
                                          for k, v in bconv.items()})
        if "bf16_deconv" in ms:
            # the transposed family of both bf16 arms in the same run: fp32 kernels in the bf16 arm, the bf16 twins in the deconv arm
            dfam = family_step("bf16_deconv")
            tr32 = {k: v for k, v in bfam.items() if "convtr2d" in k}
            tr16 = {k: v for k, v in dfam.items() if "convtr2d" in k}
            dconv = {k: v for k, v in dfam.items() if "conv2d" in k}
            rec.update(bf16_deconv_ms_per_step=[round(v, 3) for v in ms["bf16_deconv"]],
                       bf16_deconv_images_per_s=round(batch * 1000.0 / best["bf16_deconv"], 2),
                       bf16_deconv_speedup_over_bf16=round(best["bf16"] / best["bf16_deconv"], 3),
                       bf16_deconv_speedup_over_native_fp32=round(best[True] / best["bf16_deconv"], 3),
                       bf16_arm_convtr2d_family_ms_per_step=round(sum(v["ms"] for v in tr32.values()), 3),
                       bf16_arm_convtr2d_calls=calls(tr32),
                       bf16_deconv_convtr2d_family_ms_per_step=round(sum(v["ms"] for v in tr16.values()), 3),
                       bf16_deconv_convtr2d_calls=calls(tr16),
                       bf16_deconv_conv2d_calls=calls(dconv))
        if "stem" in ms:
            # the stem arms against the arms they sit on, in the same run; the new entry points per call, and the fp32 launches of the
            # first two layers they replace as the difference of the two arms' u3d_conv2d_ex_reps / u3d_conv2d_wgrad totals
            P = float(batch * hw[0] * hw[1])
            m0 = runs[True][0]
            c_in, c1, c2 = (m0.encoders[0].basic_module.SingleConv1.conv.in_channels, m0.encoders[0].basic_module.SingleConv1.conv.out_channels,
                            m0.encoders[0].basic_module.SingleConv2.conv.out_channels)
            must_move = {"u3d_conv2d_small_cin_fwd_reps": 4 * P * (c_in + c1), "u3d_conv2d_small_cin_bwd": 4 * P * (c_in + c1),
                         # one 16-channel layer c1 -> c2: forward (read c1, write c2) + data gradient (read dz c2, write c1, read x c1)
                         "u3d_conv2d_bf16_c16": 4 * P * (c1 + c2) + 4 * P * (c2 + 2 * c1), "u3d_conv2d_wgrad_bf16_c16": 4 * P * (c1 + c2)}
            want_calls = {"u3d_conv2d_small_cin_fwd_reps": 1, "u3d_conv2d_small_cin_bwd": 1, "u3d_conv2d_bf16_c16": 2, "u3d_conv2d_wgrad_bf16_c16": 1}

            def new_calls(d):
                out = {}
                for k, v in d.items():
                    if k in must_move:
                        gbs = must_move[k] / v["ms"] / 1e6 if v["ms"] and v["calls"] == want_calls[k] else None  # (else: not the one-layer stem)
                        out[k] = {"calls": v["calls"], "ms": round(v["ms"], 3), "gb_per_s_on_bytes_it_must_move": round(gbs, 1) if gbs else None}
                return out

            def replaced(base, stem):
                return {k: {"calls": base[k]["calls"] - stem.get(k, {"calls": 0})["calls"],
                            "ms": round(base[k]["ms"] - stem.get(k, {"ms": 0.0})["ms"], 3)}
                        for k in ("u3d_conv2d_ex_reps", "u3d_conv2d_wgrad") if k in base}

            sfam = family_step("stem")
            rec.update(stem_ms_per_step=[round(v, 3) for v in ms["stem"]], stem_speedup_over_native_fp32=round(best[True] / best["stem"], 3),
                       stem_new_calls=new_calls(sfam), stem_replaced_fp32_calls=replaced(fam, sfam))
            if "bf16_stem" in ms:
                bsfam = family_step("bf16_stem")
                rec.update(bf16_stem_ms_per_step=[round(v, 3) for v in ms["bf16_stem"]],
                           bf16_stem_images_per_s=round(batch * 1000.0 / best["bf16_stem"], 2),
                           bf16_stem_speedup_over_bf16=round(best["bf16"] / best["bf16_stem"], 3),
                           bf16_stem_new_calls=new_calls(bsfam), bf16_stem_replaced_fp32_calls=replaced(bfam, bsfam),
                           bf16_stem_conv2d_calls=calls({k: v for k, v in bsfam.items() if "conv2d" in k}))
        if "bf16_stem_vcat" in ms:
            # the vcat arm against the bf16 + stem arm of the same run: every bf16 conv entry point and the concat copy, bracketed by
            # name (u3d_nearest_cat_fwd declares no FLOPs); peak memory of one step per arm
            names = ("u3d_conv2d_bf16", "u3d_conv2d_wgrad_bf16", "u3d_conv2d_bf16_c16", "u3d_conv2d_wgrad_bf16_c16", "u3d_nearest_cat_fwd",
                     "u3d_conv2d_bf16_src", "u3d_conv2d_bf16_dgrad_src", "u3d_conv2d_wgrad_bf16_src")

            def named_step(path):
                prof = nat.EventProfiler(only=names, prealloc=512)
                nat.profiler = prof
                step(*runs[path], x, target, loss_fn)
                torch.cuda.synchronize()
                nat.profiler = None
                return {k: {"calls": v["calls"], "ms": round(v["ms"], 3), "ms_per_call": round(v["ms"] / v["calls"], 4)}
                        for k, v in prof.summary().items()}

            def peak_bytes(path):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                step(*runs[path], x, target, loss_fn)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated(dev)

            base, vc = named_step("bf16_stem"), named_step("bf16_stem_vcat")
            src_ms = sum(v["ms"] for k, v in vc.items() if k.endswith("_src"))
            single = ("u3d_conv2d_bf16", "u3d_conv2d_wgrad_bf16")
            rec.update(bf16_stem_vcat_ms_per_step=[round(v, 3) for v in ms["bf16_stem_vcat"]],
                       bf16_stem_vcat_images_per_s=round(batch * 1000.0 / best["bf16_stem_vcat"], 2),
                       bf16_stem_vcat_speedup_over_bf16_stem=round(best["bf16_stem"] / best["bf16_stem_vcat"], 4),
                       bf16_stem_arm_calls=base, bf16_stem_vcat_arm_calls=vc,
                       # what the three `_src` calls per decoder replace: the copy plus the same layers' single-source launches
                       vcat_src_calls_ms=round(src_ms, 3),
                       vcat_replaced_calls_ms=round(base.get("u3d_nearest_cat_fwd", {"ms": 0.0})["ms"] +
                                                    sum(base[k]["ms"] - vc.get(k, {"ms": 0.0})["ms"] for k in single if k in base), 3),
                       peak_memory_bytes={str(p): peak_bytes(p) for p in paths if p is not False})
        if "bf16_stem_vcat_subpixel" in ms:
            # the sub-pixel bf16 arm against the vcat arm of the same run: the new entry points and the skip half's launches, the `_src` calls
            # of the vcat arm they replace, bracketed by name; peak memory of one step per arm
            snames = ("u3d_subpixel2d_conv_fwd_bf16", "u3d_subpixel2d_conv_dgrad_bf16", "u3d_subpixel2d_conv_wgrad_bf16", "u3d_conv2d_bf16_res",
                      "u3d_conv2d_wgrad_bf16_strided", "u3d_conv2d_bf16", "u3d_conv2d_wgrad_bf16", "u3d_conv2d_bf16_src",
                      "u3d_conv2d_bf16_dgrad_src", "u3d_conv2d_wgrad_bf16_src", "u3d_gn_bwd_apply", "u3d_gn_bwd_apply_up")

            def snamed_step(path):
                prof = nat.EventProfiler(only=snames, prealloc=512)
                nat.profiler = prof
                step(*runs[path], x, target, loss_fn)
                torch.cuda.synchronize()
                nat.profiler = None
                return {k: {"calls": v["calls"], "ms": round(v["ms"], 3), "ms_per_call": round(v["ms"] / v["calls"], 4)}
                        for k, v in prof.summary().items()}

            def speak_bytes(path):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                step(*runs[path], x, target, loss_fn)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated(dev)

            vcb, spb = snamed_step("bf16_stem_vcat"), snamed_step("bf16_stem_vcat_subpixel")
            eng = runs["bf16_stem_vcat_subpixel"][0]._get_engine()
            taken = eng._subpixel_layers((1,) + tuple(hw))
            ratio = best["bf16_stem_vcat"] / best["bf16_stem_vcat_subpixel"]
            rec.update(bf16_subpixel_ms_per_step=[round(v, 3) for v in ms["bf16_stem_vcat_subpixel"]],
                       bf16_subpixel_images_per_s=round(batch * 1000.0 / best["bf16_stem_vcat_subpixel"], 2),
                       bf16_subpixel_speedup_over_vcat=round(ratio, 4),
                       bf16_subpixel_bar="more than 1.05x the native_2d_bf16_vcat arm of the same run",
                       bf16_subpixel_meets_bar=bool(ratio > 1.05),
                       bf16_subpixel_decoder_levels_taken=f"{len(taken)} of {len(eng.dec)}",
                       bf16_subpixel_vcat_arm_calls=vcb, bf16_subpixel_arm_calls=spb,
                       bf16_subpixel_peak_memory_bytes={p: speak_bytes(p) for p in ("bf16_stem_vcat", "bf16_stem_vcat_subpixel")})
        if not a.native_only:
            rec.update(stock_ms_per_step=[round(v, 3) for v in ms[False]], stock_images_per_s=round(batch * 1000.0 / best[False], 2),
                       native_speedup=round(best[False] / best[True], 3))
        print(json.dumps(rec), flush=True)
        del runs, x, target
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
