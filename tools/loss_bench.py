"""Stock against fused multi-class losses on an MI355X: forward + backward of the loss alone, timed with HIP events, and the
reference's multi-class training step (resources/3DUnet_multiclass: UNet3D f_maps [32, 64, 128, 256], 3 classes,
1x1x80x170x170) with each loss.

    python tools/loss_bench.py [--reps 20] [--no-step]
    python tools/loss_bench.py --options [--reps 20]

"stock" is the reference's formula on torch operators (what the loss runs without this library); "fused" is
u3d_softmax_ce_* / u3d_dice_*.  For the fused cross entropy the HBM time of its own bytes is printed too: logits and
target read twice (forward, backward), dlogits written once, at the 6.3 TB/s a float4 copy reaches on an MI355X, beside the
fused path's device time (HIP events around each native call: the kernels without the host time between launches).

`--options` times the regression losses and the factory's loss options (`skip_last_target`, `ignore_index` through
MaskingLossWrapper, a one-element `pos_weight`) at the shipped shapes: the denoising config's 1x1x128^3 patch and BASELINE
config 2's 2x1x64x128x128 logits with a 2-channel target.  "native" is the criterion as `install_fused` builds it; "before" is
the same criterion object with `losses._OPTIONS_NATIVE = False`: the wrappers' and regression losses' stock statements, and a
`.contiguous()` copy of the sliced target in front of the fused kernels, which is what ran before these paths existed.  The
native column's GB/s counts 8 B per element forward (input and target read) and 12 B backward (both read again, the gradient
written)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-3dunet_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch3dunet_amd import _native as nat  # noqa: E402
from pytorch3dunet_amd.unet3d import losses as L  # noqa: E402

HBM_BPS = 6.3e12
DEV = torch.device("cuda", 0)
SHAPES = {
    "multiclass 1x3x80x170x170": (1, 3, 80, 170, 170),
    "DSB2018 2-D 32x3x256x256 (D=1)": (32, 3, 1, 256, 256),
    "C=1024 1x1024x8x16x16": (1, 1024, 8, 16, 16),
}


def _stock_wce(x, t):
    return F.cross_entropy(x, t, weight=L.WeightedCrossEntropyLoss._class_weights(x), ignore_index=-100)


def losses():
    dice = L.DiceLoss(normalization="softmax")
    gdl = L.GeneralizedDiceLoss(normalization="softmax")
    return {
        # name: (target kind, stock, fused)
        "CrossEntropyLoss": ("label", lambda x, t: F.cross_entropy(x, t), L._upgrade(torch.nn.CrossEntropyLoss())),
        "WeightedCrossEntropyLoss": ("label", _stock_wce, L.WeightedCrossEntropyLoss(ignore_index=-100)),
        "DiceLoss(softmax)": ("onehot", lambda x, t: L._AbstractDiceLoss.forward(dice, x, t), dice),
        "GeneralizedDiceLoss(softmax)": ("onehot", lambda x, t: L._AbstractDiceLoss.forward(gdl, x, t), gdl),
    }


def time_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        fn()
        en.record()
        torch.cuda.synchronize()
        out.append(st.elapsed_time(en))
    return statistics.median(out)


def device_ms(fn, reps):
    """stream time of the fused entry points alone (HIP events around each native call, summed per rep): the kernels'
    time without the host's Python / autograd overhead between the launches"""
    fn()
    torch.cuda.synchronize()
    nat.profiler = prof = nat.EventProfiler()
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    return sum(d["ms"] for d in prof.summary().values()) / reps


def fwd_bwd(f, x, t):
    def run():
        x.grad = None
        f(x, t).backward()
    return run


def bench_losses(reps):
    for sname, shape in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(0)
        x = (2.0 * torch.randn(shape, device=DEV, generator=g)).requires_grad_(True)
        lab = torch.randint(0, shape[1], (shape[0],) + shape[2:], device=DEV, generator=g)
        oh = None
        for lname, (kind, stock, fused) in losses().items():
            if kind == "onehot" and oh is None:
                oh = F.one_hot(lab, shape[1]).movedim(-1, 1).float().contiguous()
            t = lab if kind == "label" else oh
            n0 = nat.launch_count
            fwd_bwd(fused, x, t)()
            assert nat.launch_count > n0, "fused path did not run"
            ms_s = time_ms(fwd_bwd(stock, x, t), reps)
            ms_f = time_ms(fwd_bwd(fused, x, t), reps)
            line = f"{sname:32s} {lname:30s} stock {ms_s:8.3f} ms  fused {ms_f:8.3f} ms  speed-up {ms_s / ms_f:5.2f}x"
            dev_ms = device_ms(fwd_bwd(fused, x, t), reps)
            line += f"  fused device {dev_ms:7.3f} ms"
            if lname == "CrossEntropyLoss":
                nbytes = 2 * (x.numel() * 4 + lab.numel() * 8) + x.numel() * 4
                hbm = nbytes / HBM_BPS * 1e3
                line += f"  own bytes {nbytes / 1e6:.1f} MB -> HBM time {hbm:.3f} ms, device/HBM {dev_ms / hbm:.2f}"
            print(line, flush=True)


def bench_step(reps):
    from pytorch3dunet_amd.unet3d.model import UNet3D

    torch.manual_seed(0)
    model = UNet3D(1, 3, final_sigmoid=False, f_maps=[32, 64, 128, 256], num_groups=8).to(DEV).train()
    x = torch.randn(1, 1, 80, 170, 170, device=DEV)
    lab = torch.randint(0, 3, (1, 80, 170, 170), device=DEV)
    oh = F.one_hot(lab, 3).movedim(-1, 1).float().contiguous()
    for lname, (kind, stock, fused) in losses().items():
        t = lab if kind == "label" else oh
        res = {}
        for which, f in (("stock", stock), ("fused", fused)):
            def step():
                model.zero_grad(set_to_none=True)
                _, logits = model(x, return_logits=True)
                f(logits, t).backward()
            res[which] = time_ms(step, reps)
        print(f"step UNet3D f[32,64,128,256] 1x1x80x170x170 {lname:30s} stock {res['stock']:8.2f} ms  fused "
              f"{res['fused']:8.2f} ms  saved {res['stock'] - res['fused']:6.2f} ms", flush=True)


class _Masking(torch.nn.Module):
    """the caller's masking wrapper in its stock form: a mask of the target, two full-size multiplies"""

    def __init__(self, loss, ignore_index):
        super().__init__()
        self.loss, self.ignore_index = loss, ignore_index

    def forward(self, input, target):
        mask = target.clone().ne_(self.ignore_index)
        return self.loss(input * mask, target * mask)


class _SkipLast(torch.nn.Module):
    def __init__(self, loss):
        super().__init__()
        self.loss = loss

    def forward(self, input, target):
        return self.loss(input, target[:, :-1, ...])


class _WeightedSmoothL1(torch.nn.SmoothL1Loss):
    """the caller's weighted SmoothL1 in its stock form: boolean-mask gather and scatter (a host synchronisation each)"""

    def __init__(self, threshold, initial_weight, apply_below_threshold=True):
        super().__init__(reduction="none")
        self.threshold, self.weight, self.apply_below_threshold = threshold, initial_weight, apply_below_threshold

    def forward(self, input, target):
        l1 = super().forward(input, target)
        mask = target < self.threshold if self.apply_below_threshold else target >= self.threshold
        l1[mask] = l1[mask] * self.weight
        return l1.mean()


def option_cases():
    masking, skip = L._masking_wrapper_class(_Masking), L._skip_last_wrapper_class(_SkipLast)
    wsl1 = L._weighted_smooth_l1_class(_WeightedSmoothL1)
    pw = L._upgrade(torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([2.5]))).to(DEV)
    reg, seg = (1, 1, 128, 128, 128), (2, 1, 64, 128, 128)
    # name: (logits shape, target channels, target kind, criterion)
    return {
        "MSELoss": (reg, 1, "real", L.MSELoss()),
        "L1Loss": (reg, 1, "real", L.L1Loss()),
        "SmoothL1Loss": (reg, 1, "real", L.SmoothL1Loss()),
        "WeightedSmoothL1Loss": (reg, 1, "real", wsl1(0.5, 3.0)),
        "SmoothL1Loss ignore_index": (reg, 1, "real", masking(L.SmoothL1Loss(), -1)),
        "BCEDiceLoss skip_last_target": (seg, 2, "binary", skip(L.BCEDiceLoss())),
        "BCEDiceLoss ignore_index": (seg, 1, "binary", masking(L.BCEDiceLoss(), -1)),
        "BCEDiceLoss ignore_index skip_last": (seg, 2, "binary", skip(masking(L.BCEDiceLoss(), -1))),
        "DiceLoss(softmax) ignore_index": ((1, 3, 80, 170, 170), 3, "binary", masking(L.DiceLoss(normalization="softmax"), -1)),
        "BCEWithLogitsLoss pos_weight": (seg, 1, "binary", pw),
        "BCEWithLogitsLoss pos_weight skip_last": (seg, 2, "binary", skip(pw)),
    }


def bench_options(reps):
    print(f"{'case':40s} {'logits':18s} {'before ms':>10s} {'native ms':>10s} {'speed-up':>9s} {'native GB/s':>12s} "
          f"{'native device ms':>17s}", flush=True)
    for name, (shape, tc, kind, crit) in option_cases().items():
        g = torch.Generator(device=DEV).manual_seed(0)
        x = (2.0 * torch.randn(shape, device=DEV, generator=g)).requires_grad_(True)
        tshape = (shape[0], tc) + shape[2:]
        u = torch.rand(tshape, device=DEV, generator=g)
        t = torch.round(u * 256) / 256 if kind == "real" else (u > 0.6).float()
        if "ignore_index" in name:
            t[torch.rand(tshape, device=DEV, generator=g) < 0.2] = -1.0
        run = fwd_bwd(crit, x, t)
        n0 = nat.launch_count
        run()
        assert nat.launch_count >= n0 + 2, "native path did not run"
        ms_n = time_ms(run, reps)
        dev_ms = device_ms(run, reps)
        L._OPTIONS_NATIVE = False
        try:
            ms_b = time_ms(run, reps)
        finally:
            L._OPTIONS_NATIVE = True
        gbs = 20.0 * x.numel() / (ms_n * 1e-3) / 1e9
        print(f"{name:40s} {'x'.join(map(str, shape)):18s} {ms_b:10.3f} {ms_n:10.3f} {ms_b / ms_n:8.2f}x {gbs:12.1f} {dev_ms:17.3f}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--options", action="store_true", help="the regression losses and the factory's loss options")
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} reps, HIP events; loss = forward + backward", flush=True)
    if a.options:
        bench_options(a.reps)
        return
    bench_losses(a.reps)
    if not a.no_step:
        bench_step(max(5, a.reps // 2))


if __name__ == "__main__":
    main()
