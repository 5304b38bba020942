"""Shared by test_losses_reg.py and test_gpu_losses_reg.py: the fixture tests/golden/l3_losses_reg.npz (make_losses_reg.py, written
from the live reference's factory) and a stand-in for the CALLER's `pytorch3dunet.unet3d.losses` that has the facts
`install_fused()` relies on, so the factory path can be tested where the reference checkout does not exist (the GPU box)."""
import os
import types

import numpy as np
import torch

from conftest import GOLDEN_DIR
from pytorch3dunet_amd.unet3d import losses as L

Z = np.load(os.path.join(GOLDEN_DIR, "l3_losses_reg.npz"))
CASES = sorted({k.split("/")[0] for k in Z.files})
UPSTREAM = 1.7  # make_losses_reg.py back-propagates 1.7 * loss

_CALLER_SOURCE = '''
import torch
from torch import nn
from torch.nn import L1Loss, MSELoss, SmoothL1Loss


class _Unfused(nn.Module):  # the caller's unfused classes: install_fused() must REPLACE them
    def __init__(self, *a, **k):
        super().__init__()


class BCEDiceLoss(_Unfused):
    pass


class DiceLoss(_Unfused):
    pass


class GeneralizedDiceLoss(_Unfused):
    pass


class WeightedCrossEntropyLoss(_Unfused):
    pass


class WeightedSmoothL1Loss(nn.SmoothL1Loss):
    def __init__(self, threshold, initial_weight, apply_below_threshold=True):
        super().__init__(reduction="none")
        self.threshold, self.weight, self.apply_below_threshold = threshold, initial_weight, apply_below_threshold

    def forward(self, input, target):
        each = super().forward(input, target)
        chosen = target < self.threshold if self.apply_below_threshold else target >= self.threshold
        return torch.where(chosen, each * self.weight, each).mean()


class MaskingLossWrapper(nn.Module):
    def __init__(self, loss, ignore_index):
        super().__init__()
        self.loss, self.ignore_index = loss, ignore_index

    def forward(self, input, target):
        keep = (target != self.ignore_index).to(target.dtype)
        return self.loss(input * keep, target * keep)


class SkipLastTargetChannelWrapper(nn.Module):
    def __init__(self, loss, squeeze_channel=False):
        super().__init__()
        self.loss, self.squeeze_channel = loss, squeeze_channel

    def forward(self, input, target):
        target = target[:, :-1, ...]
        return self.loss(input, target.squeeze(1) if self.squeeze_channel else target)


def _create_loss(name, cfg, weight, ignore_index, pos_weight):
    ce_ignore = -100 if ignore_index is None else ignore_index
    norm = cfg.get("normalization", "sigmoid")
    if name == "BCEWithLogitsLoss":
        return nn.BCEWithLogitsLoss(pos_weight=pos_weight)
    if name == "CrossEntropyLoss":
        return nn.CrossEntropyLoss(weight=weight, ignore_index=ce_ignore)
    if name == "WeightedSmoothL1Loss":
        return WeightedSmoothL1Loss(cfg["threshold"], cfg["initial_weight"], cfg.get("apply_below_threshold", True))
    makers = {"BCEDiceLoss": lambda: BCEDiceLoss(cfg.get("alpha", 1.0)),
              "WeightedCrossEntropyLoss": lambda: WeightedCrossEntropyLoss(ignore_index=ce_ignore),
              "GeneralizedDiceLoss": lambda: GeneralizedDiceLoss(normalization=norm),
              "DiceLoss": lambda: DiceLoss(weight=weight, normalization=norm),
              "MSELoss": lambda: MSELoss(), "SmoothL1Loss": lambda: SmoothL1Loss(), "L1Loss": lambda: L1Loss()}
    if name not in makers:
        raise RuntimeError(f"Unsupported loss function: '{name}'")
    return makers[name]()


def get_loss_criterion(config):
    cfg = config["loss"]
    name = cfg.pop("name")
    ignore_index = cfg.pop("ignore_index", None)
    skip_last = cfg.pop("skip_last_target", False)
    weight, pos_weight = cfg.pop("weight", None), cfg.pop("pos_weight", None)
    weight = None if weight is None else torch.tensor(weight).float()
    pos_weight = None if pos_weight is None else torch.tensor(pos_weight)
    loss = _create_loss(name, cfg, weight, ignore_index, pos_weight)
    if ignore_index is not None and name not in ("CrossEntropyLoss", "WeightedCrossEntropyLoss"):
        loss = MaskingLossWrapper(loss, ignore_index)
    if skip_last:
        loss = SkipLastTargetChannelWrapper(loss, cfg.get("squeeze_channel", False))
    return loss.to(config["device"])
'''


def caller_losses(fused=True):
    """a fresh stand-in for the caller's loss module, with the fused family installed unless fused=False"""
    mod = types.ModuleType("pytorch3dunet.unet3d.losses")
    exec(_CALLER_SOURCE, mod.__dict__)
    return L.install_fused(mod) if fused else mod


def spec_of(case):
    return eval(str(Z[f"{case}/spec"]))  # noqa: S307 - a dict literal make_losses_reg.py wrote


def criterion(mod, spec, device):
    return mod.get_loss_criterion({"device": device, "loss": dict(spec)})


def foreign_objects(crit):
    """the wrappers and losses of a criterion tree that are NOT classes of pytorch3dunet_amd.unet3d.losses (the nn.Sigmoid /
    nn.Softmax a Dice loss holds as its normalisation is neither a loss nor a wrapper)"""
    return [m for m in crit.modules()
            if type(m).__module__ != L.__name__ and type(m).__module__ != "torch.nn.modules.activation"]


def check_case(mod, case, device, tol_loss, tol_grad):
    """loss and gradient of the factory's criterion for a fixture case against the reference's recorded values"""
    crit = criterion(mod, spec_of(case), device)
    x = torch.from_numpy(Z[f"{case}/logits"]).to(device).requires_grad_(True)
    target = torch.from_numpy(Z[f"{case}/target"]).to(device)
    val = crit(x, target)
    (UPSTREAM * val).backward()
    ref_loss = float(Z[f"{case}/loss"])
    ref_grad = torch.from_numpy(Z[f"{case}/dlogits"])
    scale = ref_grad.abs().max().item()
    err = (x.grad.cpu() - ref_grad).abs().max().item()
    print(f"{case} on {device}: loss {val.item():.8f} ref {ref_loss:.8f}, gradient max err {err:.3e} of scale {scale:.3e}")
    assert abs(val.item() - ref_loss) <= tol_loss * max(1.0, abs(ref_loss)), (case, val.item(), ref_loss)
    assert err <= tol_grad * scale + 1e-12, (case, err, scale)
    return crit
