"""Generate tests/golden/l3_losses_reg.npz from the LIVE reference's losses.py (wolny/pytorch-3dunet 1.9.6 imported through
oracle/ref_import.py) on the CPU — run in the build container only, like make_losses_mc.py:

    python tests/golden/make_losses_reg.py

The regression losses and the factory's loss options (`ignore_index` on non-cross-entropy losses, `skip_last_target`,
`squeeze_channel`, a one-element `pos_weight`).  Each case stores the logits, the target, the loss the reference's own factory
(`get_loss_criterion`) builds for the case's config and the gradient of 1.7 * loss with respect to the logits.  `<case>/spec`
is the loss config as a dict literal.  Only arrays and that string go into the file."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from ref_import import import_reference  # noqa: E402

UPSTREAM = 1.7
S3 = (2, 3, 7, 9, 11)
S1 = (2, 1, 7, 9, 11)
IGN = {"ignore_index": -1}
SKIP = {"skip_last_target": True}
WSL1 = {"name": "WeightedSmoothL1Loss", "threshold": 0.5, "initial_weight": 3.0}
# name: (loss config, logits shape, target kind); the target has one channel more where the config skips the last one, and
# about 20 % of it is -1 where the config ignores -1
CASES = {
    "mse": ({"name": "MSELoss"}, S3, "real"),
    "l1": ({"name": "L1Loss"}, S3, "real"),
    "smooth_l1": ({"name": "SmoothL1Loss"}, S3, "real"),
    "wsl1_below": ({**WSL1, "apply_below_threshold": True}, S3, "real"),
    "wsl1_above": ({**WSL1, "apply_below_threshold": False}, S3, "real"),
    "smooth_l1_ign": ({"name": "SmoothL1Loss", **IGN}, S3, "real"),
    "mse_ign": ({"name": "MSELoss", **IGN}, S3, "real"),
    "bcedice_ign": ({"name": "BCEDiceLoss", **IGN}, S3, "binary"),
    "dice_sigmoid_ign": ({"name": "DiceLoss", **IGN}, S3, "binary"),
    "dice_softmax_ign": ({"name": "DiceLoss", "normalization": "softmax", **IGN}, S3, "onehot"),
    "gdl_ign": ({"name": "GeneralizedDiceLoss", **IGN}, S3, "binary"),
    "bcedice_skip": ({"name": "BCEDiceLoss", **SKIP}, S3, "binary"),
    "bce_skip": ({"name": "BCEWithLogitsLoss", **SKIP}, S3, "binary"),
    "smooth_l1_skip": ({"name": "SmoothL1Loss", **SKIP}, S3, "real"),
    "bcedice_ign_skip": ({"name": "BCEDiceLoss", **IGN, **SKIP}, S3, "binary"),
    "ce_skip_squeeze": ({"name": "CrossEntropyLoss", **SKIP, "squeeze_channel": True}, S3, "label2"),
    "bce_pw": ({"name": "BCEWithLogitsLoss", "pos_weight": [2.5]}, S3, "binary"),
    "bce_pw_skip": ({"name": "BCEWithLogitsLoss", "pos_weight": [2.5], **SKIP}, S3, "binary"),
    # the shipped shape of things: one output channel, a 2-channel target whose last channel is skipped
    "bcedice_skip_c1": ({"name": "BCEDiceLoss", **SKIP}, S1, "binary"),
    # exact ties: x == t pins sign(0) = 0, |x - t| == 1 the branch at beta
    "l1_ties": ({"name": "L1Loss"}, S3, "ties"),
    "smooth_l1_ties": ({"name": "SmoothL1Loss"}, S3, "ties"),
}


def make_inputs(spec, shape, kind, g):
    n, c = shape[0], shape[1]
    # inputs on a grid of fp32-exact values (logits in steps of 1/32, real targets in steps of 1/256): every branch of the
    # losses is decided by exact numbers, the threshold 0.5 is hit exactly now and then, and the arrays compress
    logits = torch.round(64.0 * torch.randn(shape, generator=g)) / 32
    tc = c + 1 if spec.get("skip_last_target") else c
    tshape = (n, tc) + tuple(shape[2:])
    if kind == "real":
        target = torch.randint(0, 257, tshape, generator=g).float() / 256
    elif kind == "binary":
        target = (torch.rand(tshape, generator=g) > 0.6).float()
    elif kind == "onehot":
        lab = torch.randint(0, tc, (n,) + tuple(shape[2:]), generator=g)
        target = torch.nn.functional.one_hot(lab, tc).movedim(-1, 1).float()
    elif kind == "label2":  # int64 (N, 2, *S): channel 0 holds the class labels, channel 1 is the one skipped
        target = torch.randint(0, c, (n, 2) + tuple(shape[2:]), generator=g)
    elif kind == "ties":  # multiples of 1/4 in [-2, 2]: differences of exactly 0 and exactly +-1 are frequent
        logits = torch.randint(-8, 9, shape, generator=g).float() / 4
        target = torch.randint(-8, 9, tshape, generator=g).float() / 4
    else:
        raise ValueError(kind)
    if spec.get("ignore_index") is not None:
        target = torch.where(torch.rand(tshape, generator=g) < 0.2, torch.full_like(target, spec["ignore_index"]), target)
    return logits, target


def main():
    import importlib

    import_reference()
    R = importlib.import_module("pytorch3dunet.unet3d.losses")
    g = torch.Generator().manual_seed(4242)
    out = {}
    for name, (spec, shape, kind) in CASES.items():
        logits, target = make_inputs(spec, shape, kind, g)
        crit = R.get_loss_criterion({"device": "cpu", "loss": dict(spec)})
        x = logits.clone().requires_grad_(True)
        val = crit(x, target)
        (UPSTREAM * val).backward()
        assert torch.isfinite(val) and torch.isfinite(x.grad).all(), name
        out[f"{name}/spec"] = np.array(repr(spec))
        out[f"{name}/logits"] = logits.numpy()
        out[f"{name}/target"] = target.numpy()
        out[f"{name}/loss"] = val.detach().numpy()
        out[f"{name}/dlogits"] = x.grad.numpy()
        print(f"{name}: {type(crit).__name__} loss={val.item():.6f}")
    path = os.path.join(HERE, "l3_losses_reg.npz")
    np.savez_compressed(path, **out)
    print(f"l3_losses_reg: {len(out)} arrays -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
