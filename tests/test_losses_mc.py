"""Multi-class losses (softmax / weighted cross entropy, softmax / no-normalisation Dice, generalized Dice) on the CPU: our
`pytorch3dunet_amd.unet3d.losses` torch branch against golden vectors of the LIVE reference's losses.py
(tests/golden/l2_losses_mc.npz, make_losses_mc.py), the install into a caller's loss module, and the routing between the
fused kernels and the torch branch.  The fused kernels themselves are tested by test_gpu_losses_mc.py."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR
from pytorch3dunet_amd.unet3d import losses as L

Z = np.load(os.path.join(GOLDEN_DIR, "l2_losses_mc.npz"))
CASES = sorted({k.split("/")[0] for k in Z.files})
UPSTREAM = 1.7  # make_losses_mc.py back-propagates 1.7 * loss


def build_loss(spec):
    """our class for a loss config, with the defaults of the reference's `_create_loss` (losses.py:310-345)"""
    spec = dict(spec)
    name = spec.pop("name")
    weight = spec.pop("weight", None)
    weight = None if weight is None else torch.tensor(weight).float()
    ignore_index = spec.pop("ignore_index", None)
    if name == "CrossEntropyLoss":
        return L._upgrade(torch.nn.CrossEntropyLoss(weight=weight, ignore_index=-100 if ignore_index is None else ignore_index))
    if name == "WeightedCrossEntropyLoss":
        return L.WeightedCrossEntropyLoss(ignore_index=-100 if ignore_index is None else ignore_index)
    if name == "DiceLoss":
        return L.DiceLoss(weight=weight, normalization=spec.get("normalization", "sigmoid"))
    if name == "GeneralizedDiceLoss":
        return L.GeneralizedDiceLoss(normalization=spec.get("normalization", "sigmoid"))
    raise ValueError(name)


def spec_of(case):
    return eval(str(Z[f"{case}/spec"]))  # noqa: S307 - a dict literal make_losses_mc.py wrote


def check_case(case, device, tol_loss, tol_grad):
    crit = build_loss(spec_of(case)).to(device)
    x = torch.from_numpy(Z[f"{case}/logits"]).to(device).requires_grad_(True)
    target = torch.from_numpy(Z[f"{case}/target"]).to(device)
    val = crit(x, target)
    (UPSTREAM * val).backward()
    ref_loss = float(Z[f"{case}/loss"])
    ref_grad = torch.from_numpy(Z[f"{case}/dlogits"])
    assert abs(val.item() - ref_loss) <= tol_loss * max(1.0, abs(ref_loss)), (case, val.item(), ref_loss)
    scale = ref_grad.abs().max().item()
    err = (x.grad.cpu() - ref_grad).abs().max().item()
    assert err <= tol_grad * scale + 1e-12, (case, err, scale)
    return val, x.grad


@pytest.mark.parametrize("case", CASES)
def test_mc_losses_cpu_match_reference_golden(case):
    check_case(case, "cpu", 1e-6, 2e-5)


def _fake_caller_losses(monkeypatch):
    """a stand-in for the CALLER's `pytorch3dunet.unet3d.losses` with the facts install_fused() relies on: a factory that
    resolves the loss classes from its module globals, builds nn.CrossEntropyLoss / nn.MSELoss from torch.nn, and wraps
    (reference losses.py:40-82,273-345)"""
    pkg = types.ModuleType("pytorch3dunet")
    sub = types.ModuleType("pytorch3dunet.unet3d")
    mod = types.ModuleType("pytorch3dunet.unet3d.losses")
    exec("""
import torch
from torch import nn


class WeightedCrossEntropyLoss(nn.Module):  # the caller's unfused classes: must be REPLACED
    def __init__(self, ignore_index=-1):
        super().__init__()
        self.ignore_index = ignore_index


class GeneralizedDiceLoss(nn.Module):
    def __init__(self, normalization="sigmoid", epsilon=1e-6):
        super().__init__()


class DiceLoss(nn.Module):
    def __init__(self, weight=None, normalization="sigmoid"):
        super().__init__()


class BCEDiceLoss(nn.Module):
    def __init__(self, alpha=1.0):
        super().__init__()


class SkipLastTargetChannelWrapper(nn.Module):
    def __init__(self, loss, squeeze_channel=False):
        super().__init__()
        self.loss = loss
        self.squeeze_channel = squeeze_channel

    def forward(self, input, target):
        target = target[:, :-1, ...]
        if self.squeeze_channel:
            target = torch.squeeze(target, dim=1)
        return self.loss(input, target)


def _create_loss(name, cfg, weight, ignore_index):
    if name == "CrossEntropyLoss":
        return nn.CrossEntropyLoss(weight=weight, ignore_index=-100 if ignore_index is None else ignore_index)
    if name == "WeightedCrossEntropyLoss":
        return WeightedCrossEntropyLoss(ignore_index=-100 if ignore_index is None else ignore_index)
    if name == "GeneralizedDiceLoss":
        return GeneralizedDiceLoss(normalization=cfg.get("normalization", "sigmoid"))
    if name == "DiceLoss":
        return DiceLoss(weight=weight, normalization=cfg.get("normalization", "sigmoid"))
    if name == "MSELoss":
        return nn.MSELoss()
    raise RuntimeError(f"Unsupported loss function: '{name}'")


def get_loss_criterion(config):
    cfg = dict(config["loss"])
    name = cfg.pop("name")
    weight = cfg.pop("weight", None)
    weight = None if weight is None else torch.tensor(weight).float()
    loss = _create_loss(name, cfg, weight, cfg.pop("ignore_index", None))
    if cfg.pop("skip_last_target", False):
        loss = SkipLastTargetChannelWrapper(loss, cfg.get("squeeze_channel", False))
    return loss
""", mod.__dict__)
    pkg.unet3d, sub.losses = sub, mod
    for k, v in (("pytorch3dunet", pkg), ("pytorch3dunet.unet3d", sub), ("pytorch3dunet.unet3d.losses", mod)):
        monkeypatch.setitem(sys.modules, k, v)
    return mod


def test_install_fused_covers_the_multiclass_losses(monkeypatch):
    mod = _fake_caller_losses(monkeypatch)
    unfused = (mod.WeightedCrossEntropyLoss, mod.GeneralizedDiceLoss)
    w = [0.5, 1.0, 2.0]
    ce = L.get_loss_criterion({"device": "cpu", "loss": {"name": "CrossEntropyLoss", "weight": w, "ignore_index": 7}})
    # nn.CrossEntropyLoss upgraded IN PLACE: same state, the weight buffer kept
    assert type(ce) is L.CrossEntropyLoss and ce.ignore_index == 7 and torch.equal(ce.weight, torch.tensor(w))
    assert list(dict(ce.named_buffers())) == ["weight"]
    wce = L.get_loss_criterion({"device": "cpu", "loss": {"name": "WeightedCrossEntropyLoss"}})
    assert type(wce) is L.WeightedCrossEntropyLoss and wce.ignore_index == -100
    gdl = L.get_loss_criterion({"device": "cpu", "loss": {"name": "GeneralizedDiceLoss", "normalization": "softmax"}})
    assert type(gdl) is L.GeneralizedDiceLoss and gdl.normalization_name == "softmax"
    assert mod.WeightedCrossEntropyLoss is L.WeightedCrossEntropyLoss and mod.GeneralizedDiceLoss is L.GeneralizedDiceLoss
    assert mod.WeightedCrossEntropyLoss is not unfused[0] and mod.GeneralizedDiceLoss is not unfused[1]
    d = L.get_loss_criterion({"device": "cpu", "loss": {"name": "DiceLoss", "normalization": "none"}})
    assert type(d) is L.DiceLoss and d.normalization_name == "none"
    assert type(L.get_loss_criterion({"device": "cpu", "loss": {"name": "MSELoss"}})) is torch.nn.MSELoss
    # the caller's wrapper stays the caller's and wraps the upgraded class
    wr = L.get_loss_criterion({"device": "cpu", "loss": {"name": "CrossEntropyLoss", "skip_last_target": True,
                                                         "squeeze_channel": True}})
    assert type(wr).__name__ == "SkipLastTargetChannelWrapper" and type(wr.loss) is L.CrossEntropyLoss
    x, t = torch.randn(2, 3, 4, 5), torch.randint(0, 3, (2, 2, 4, 5))
    assert torch.allclose(wr(x, t), F.cross_entropy(x, t[:, 0]))


class _FakeTensor:
    """only the attributes the routing predicates read — lets a HIP tensor be described without a GPU"""

    def __init__(self, shape, dtype, device="cuda:0"):
        self.shape = torch.Size(shape)
        self.dtype = dtype
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"

    def dim(self):
        return len(self.shape)

    def numel(self):
        return math.prod(self.shape)


def _routes_native(crit, x, t, monkeypatch):
    """True when crit(x, t) takes the fused path (the autograd function is replaced by a marker)"""
    hit = []
    monkeypatch.setattr(L._FusedSoftmaxCE, "apply", lambda *a: hit.append("ce") or torch.zeros(()))
    monkeypatch.setattr(L._FusedDice, "apply", lambda *a: hit.append("dice") or torch.zeros(()))
    try:
        crit(x, t)
    except Exception:  # the torch branch cannot run on a fake tensor: reaching it is the "not native" outcome
        pass
    return bool(hit)


def test_fallback_conditions_route_as_documented(monkeypatch):
    x = _FakeTensor((2, 3, 4, 5, 6), torch.float32)
    t = _FakeTensor((2, 4, 5, 6), torch.int64)
    assert L._ce_native_ok(x, t)
    ce = L._upgrade(torch.nn.CrossEntropyLoss())
    assert _routes_native(ce, x, t, monkeypatch)
    assert not _routes_native(L._upgrade(torch.nn.CrossEntropyLoss(label_smoothing=0.1)), x, t, monkeypatch)
    assert not _routes_native(L._upgrade(torch.nn.CrossEntropyLoss(reduction="sum")), x, t, monkeypatch)
    assert not _routes_native(ce, x, _FakeTensor((2, 4, 5, 6), torch.int32), monkeypatch)  # int32 target
    assert not _routes_native(ce, _FakeTensor(x.shape, torch.float32, "cpu"), _FakeTensor(t.shape, torch.int64, "cpu"),
                              monkeypatch)  # CPU tensors
    assert not _routes_native(ce, _FakeTensor(x.shape, torch.float64), t, monkeypatch)  # fp64 logits
    assert not _routes_native(ce, x, _FakeTensor((2, 1, 4, 5, 6), torch.int64), monkeypatch)  # (N, 1, *S) target
    assert not _routes_native(ce, _FakeTensor((1, 1025, 2, 2, 2), torch.float32), _FakeTensor((1, 2, 2, 2), torch.int64),
                              monkeypatch)  # C > 1024
    assert _routes_native(L.WeightedCrossEntropyLoss(ignore_index=-100), x, t, monkeypatch)
    assert not _routes_native(L.WeightedCrossEntropyLoss(), x, _FakeTensor((2, 4, 5, 6), torch.int32), monkeypatch)
    # Dice family: softmax / none and the generalized Dice on the new kernels; sigmoid DiceLoss stays on the BCE-Dice kernels
    tf = _FakeTensor(x.shape, torch.float32)
    assert _routes_native(L.DiceLoss(normalization="softmax"), x, tf, monkeypatch)
    assert _routes_native(L.DiceLoss(normalization="none"), x, tf, monkeypatch)
    assert _routes_native(L.GeneralizedDiceLoss(), x, tf, monkeypatch)
    assert not _routes_native(L.DiceLoss(normalization="sigmoid"), x, tf, monkeypatch)
    assert not _routes_native(L.GeneralizedDiceLoss(normalization="softmax"), x, _FakeTensor(x.shape, torch.int64), monkeypatch)
    assert not _routes_native(L.DiceLoss(normalization="softmax"), _FakeTensor(x.shape, torch.float32, "cpu"),
                              _FakeTensor(x.shape, torch.float32, "cpu"), monkeypatch)


def test_fallback_branches_compute_the_stock_values():
    """what the routed-away options compute on real CPU tensors: torch's own cross entropy"""
    torch.manual_seed(3)
    x, t = torch.randn(2, 4, 3, 5), torch.randint(0, 4, (2, 3, 5))
    for kw in ({"label_smoothing": 0.1}, {"reduction": "sum"}, {}):
        crit = L._upgrade(torch.nn.CrossEntropyLoss(**kw))
        assert torch.equal(crit(x, t), F.cross_entropy(x, t, **kw))


def test_mc_losses_match_live_reference():
    """our torch branch against the LIVE reference's classes on fresh inputs (skips where the reference is absent)"""
    from ref_import import import_reference, reference_available

    if not reference_available():
        pytest.skip("the reference checkout is not present")
    import importlib

    import_reference()
    R = importlib.import_module("pytorch3dunet.unet3d.losses")
    g = torch.Generator().manual_seed(77)
    x = 3.0 * torch.randn((2, 5, 4, 6, 7), generator=g)
    lab = torch.randint(0, 5, (2, 4, 6, 7), generator=g)
    oh = F.one_hot(lab, 5).movedim(-1, 1).float()
    pairs = [
        (R.WeightedCrossEntropyLoss(ignore_index=1), L.WeightedCrossEntropyLoss(ignore_index=1), lab),
        (R.GeneralizedDiceLoss(normalization="softmax"), L.GeneralizedDiceLoss(normalization="softmax"), oh),
        (R.GeneralizedDiceLoss(), L.GeneralizedDiceLoss(), oh),
        (R.DiceLoss(normalization="none"), L.DiceLoss(normalization="none"), oh),
        (R.DiceLoss(normalization="softmax"), L.DiceLoss(normalization="softmax"), oh),
    ]
    for ref, ours, tgt in pairs:
        xr, xo = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a, b = ref(xr, tgt), ours(xo, tgt)
        a.backward()
        b.backward()
        assert torch.equal(a, b) and torch.equal(xr.grad, xo.grad), type(ours).__name__
