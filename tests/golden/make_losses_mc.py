"""Generate tests/golden/l2_losses_mc.npz from the LIVE reference's losses.py (wolny/pytorch-3dunet 1.9.6 imported through
oracle/ref_import.py) on the CPU — run in the build container only, like `make_golden.py --losses-only`:

    python tests/golden/make_losses_mc.py

Each case stores the logits, the target, the loss the reference's own factory (`get_loss_criterion`) builds for the case's
config and the gradient of 1.7 * loss with respect to the logits.  `<case>/spec` is the loss config as a dict literal."""
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
# name: (loss config, logits shape, target kind, ignored label or None)
CASES = {
    "ce": ({"name": "CrossEntropyLoss"}, S3, "label", None),
    "ce_w": ({"name": "CrossEntropyLoss", "weight": [0.2, 0.5, 1.3]}, S3, "label", None),
    "ce_ign": ({"name": "CrossEntropyLoss", "ignore_index": -1}, S3, "label", -1),
    "wce": ({"name": "WeightedCrossEntropyLoss"}, S3, "label", None),
    "wce_ign": ({"name": "WeightedCrossEntropyLoss", "ignore_index": 2}, S3, "label", 2),
    "dice_softmax": ({"name": "DiceLoss", "normalization": "softmax"}, S3, "onehot", None),
    "dice_none": ({"name": "DiceLoss", "normalization": "none"}, S3, "onehot", None),
    "dice_softmax_w": ({"name": "DiceLoss", "normalization": "softmax", "weight": [0.2, 0.3, 0.5]}, S3, "onehot", None),
    "gdl_sigmoid_c1": ({"name": "GeneralizedDiceLoss"}, (2, 1, 7, 9, 11), "binary", None),
    "gdl_sigmoid_c3": ({"name": "GeneralizedDiceLoss"}, S3, "binary", None),
    "gdl_softmax": ({"name": "GeneralizedDiceLoss", "normalization": "softmax"}, S3, "onehot", None),
    # a 2-D net's output after the trainer's unsqueeze back to D = 1 (trainer.py:354-365)
    "ce_2d": ({"name": "CrossEntropyLoss"}, (2, 4, 1, 13, 17), "label", None),
    # wide heads: the any-C channel-sums path (C > 16) and the 16-register one
    "ce_c64": ({"name": "CrossEntropyLoss"}, (1, 64, 3, 5, 7), "label", None),
    "dice_softmax_c64": ({"name": "DiceLoss", "normalization": "softmax"}, (1, 64, 3, 5, 7), "onehot", None),
    "gdl_softmax_c8": ({"name": "GeneralizedDiceLoss", "normalization": "softmax"}, (2, 8, 3, 5, 7), "onehot", None),
}


def main():
    import importlib

    import_reference()
    R = importlib.import_module("pytorch3dunet.unet3d.losses")
    g = torch.Generator().manual_seed(9191)
    out = {}
    for name, (spec, shape, kind, ignored) in CASES.items():
        c = shape[1]
        logits = 2.0 * torch.randn(shape, generator=g)
        labels = torch.randint(0, c, (shape[0],) + shape[2:], generator=g)
        if kind == "label":
            target = labels
            if ignored is not None:
                target = torch.where(torch.rand(labels.shape, generator=g) < 0.2, torch.full_like(labels, ignored), labels)
        elif kind == "onehot":
            target = torch.nn.functional.one_hot(labels, c).movedim(-1, 1).float()
        else:
            target = (torch.rand(shape, generator=g) > 0.6).float()
        crit = R.get_loss_criterion({"device": "cpu", "loss": dict(spec)})
        x = logits.clone().requires_grad_(True)
        val = crit(x, target)
        (UPSTREAM * val).backward()
        out[f"{name}/spec"] = np.array(repr(spec))
        out[f"{name}/logits"] = logits.numpy()
        out[f"{name}/target"] = target.numpy()
        out[f"{name}/loss"] = val.detach().numpy()
        out[f"{name}/dlogits"] = x.grad.numpy()
        print(f"{name}: {type(crit).__name__} loss={val.item():.6f}")
    path = os.path.join(HERE, "l2_losses_mc.npz")
    np.savez_compressed(path, **out)
    print(f"l2_losses_mc: {len(out)} arrays -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
