"""-m gpu: the fused multi-class losses (u3d_softmax_ce_* / u3d_dice_*) against the live reference's golden vectors
(tests/golden/l2_losses_mc.npz), against float64 torch at the reference's multi-class training shape, at C = 1024 and odd
voxel counts, for bitwise run-to-run reproducibility, and inside a full native UNet3D step."""
import pytest
import torch
import torch.nn.functional as F

import unet3d_oracle as orc
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d import losses as L
from test_losses_mc import CASES, build_loss, check_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("case", CASES)
def test_fused_mc_losses_match_reference_golden(case):
    n0 = nat.launch_count
    check_case(case, "cuda", 1e-5, 1e-3)  # the tolerance of the BCE-Dice kernels' golden test
    assert nat.launch_count > n0, "fused loss kernels did not run"


def _inputs(shape, kind, seed, ignored=None):
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    x = 2.5 * torch.randn(shape, generator=g)
    lab = torch.randint(0, c, (shape[0],) + tuple(shape[2:]), generator=g)
    if ignored is not None:
        lab[torch.rand(lab.shape, generator=g) < 0.2] = ignored
    if kind == "label":
        return x, lab
    return x, F.one_hot(lab.clamp(min=0), c).movedim(-1, 1).float()


LOSSES = {
    "ce": ({"name": "CrossEntropyLoss"}, "label"),
    "ce_w": ({"name": "CrossEntropyLoss", "weight": "ramp"}, "label"),
    "wce": ({"name": "WeightedCrossEntropyLoss"}, "label"),
    "dice_softmax": ({"name": "DiceLoss", "normalization": "softmax"}, "onehot"),
    "dice_none": ({"name": "DiceLoss", "normalization": "none"}, "onehot"),
    "gdl_softmax": ({"name": "GeneralizedDiceLoss", "normalization": "softmax"}, "onehot"),
    "gdl_sigmoid": ({"name": "GeneralizedDiceLoss"}, "onehot"),
}


def _crit(name, c):
    spec = dict(LOSSES[name][0])
    if spec.get("weight") == "ramp":
        spec["weight"] = [0.5 + i / c for i in range(c)]
    return build_loss(spec)


def _vs_float64(name, shape, seed):
    x, t = _inputs(shape, LOSSES[name][1], seed)
    crit = _crit(name, shape[1])
    xr = x.double().requires_grad_(True)
    ref = crit.double()(xr, t if t.dtype == torch.int64 else t.double())
    ref.backward()
    n0 = nat.launch_count
    xd = x.to(DEV).requires_grad_(True)
    val = crit.float().to(DEV)(xd, t.to(DEV))
    val.backward()
    assert nat.launch_count > n0
    e_loss = abs(val.item() - ref.item())
    scale = xr.grad.abs().max().item()
    e_grad = (xd.grad.cpu().double() - xr.grad).abs().max().item()
    assert e_loss <= 1e-5 * max(1.0, abs(ref.item())), (name, shape, val.item(), ref.item())
    assert e_grad <= 1e-3 * scale, (name, shape, e_grad, scale)


@pytest.mark.parametrize("name", sorted(LOSSES))
def test_fused_vs_float64_multiclass_shape(name):
    """the reference's multi-class training patch: resources/3DUnet_multiclass, 3 classes at 80x170x170"""
    _vs_float64(name, (1, 3, 80, 170, 170), 11)


@pytest.mark.parametrize("name", ["ce", "ce_w", "wce", "dice_softmax", "gdl_softmax"])
def test_fused_vs_float64_c1024(name):
    _vs_float64(name, (1, 1024, 3, 5, 7), 12)


@pytest.mark.parametrize("name", sorted(LOSSES))
@pytest.mark.parametrize("shape", [(3, 5, 5, 7, 9), (2, 12, 3, 3, 5), (1, 2, 1, 1, 1)])
def test_fused_vs_float64_odd_voxel_counts(name, shape):
    _vs_float64(name, shape, 13)


def test_sigmoid_gdl_single_channel_vs_float64():
    x, t = _inputs((2, 1, 9, 11, 13), "label", 14)
    t = (torch.rand(x.shape, generator=torch.Generator().manual_seed(3)) > 0.7).float()
    crit = L.GeneralizedDiceLoss()
    xr = x.double().requires_grad_(True)
    ref = crit(xr, t.double())
    ref.backward()
    xd = x.to(DEV).requires_grad_(True)
    val = crit(xd, t.to(DEV))
    val.backward()
    assert abs(val.item() - ref.item()) <= 1e-5
    assert (xd.grad.cpu().double() - xr.grad).abs().max().item() <= 1e-3 * xr.grad.abs().max().item()


@pytest.mark.parametrize("name", ["ce", "wce", "dice_softmax", "gdl_softmax"])
def test_fused_losses_bitwise_reproducible(name):
    x, t = _inputs((1, 3, 80, 170, 170), LOSSES[name][1], 21)
    crit = _crit(name, 3).to(DEV)
    x, t = x.to(DEV), t.to(DEV)
    out = []
    for _ in range(2):
        xd = x.clone().requires_grad_(True)
        val = crit(xd, t)
        val.backward()
        out.append((val.detach().clone(), xd.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("name", ["ce", "wce", "dice_none", "gdl_softmax"])
def test_device_upstream_scalar(name):
    """a non-unit upstream gradient that stays on the device: no .item() between forward and backward"""
    x, t = _inputs((2, 3, 6, 7, 9), LOSSES[name][1], 31)
    crit = _crit(name, 3)
    s = torch.tensor(-2.75)
    xr = x.double().requires_grad_(True)
    (crit.double()(xr, t if t.dtype == torch.int64 else t.double()) * s.double()).backward()
    xd = x.to(DEV).requires_grad_(True)
    (crit.float().to(DEV)(xd, t.to(DEV)) * s.to(DEV)).backward()
    assert (xd.grad.cpu().double() - xr.grad).abs().max().item() <= 1e-3 * xr.grad.abs().max().item()


def test_ignore_index_all_ignored_is_nan_like_torch():
    x, t = _inputs((2, 3, 4, 5, 6), "label", 41)
    t[:] = -1
    for crit in (L._upgrade(torch.nn.CrossEntropyLoss(ignore_index=-1)), L.WeightedCrossEntropyLoss(ignore_index=-1)):
        ref = crit(x, t)
        assert torch.isnan(ref)
        n0 = nat.launch_count
        xd = x.to(DEV).requires_grad_(True)
        val = crit(xd, t.to(DEV))
        val.backward()
        assert nat.launch_count > n0 and torch.isnan(val.cpu())
        assert torch.count_nonzero(xd.grad).item() == 0  # zero gradient on ignored voxels


def test_ignore_index_partial_vs_float64():
    for ignored in (-1, 1):
        x, t = _inputs((2, 3, 5, 7, 9), "label", 42, ignored=ignored)
        for crit in (L._upgrade(torch.nn.CrossEntropyLoss(ignore_index=ignored, weight=torch.tensor([0.3, 1.0, 2.0]))),
                     L.WeightedCrossEntropyLoss(ignore_index=ignored)):
            xr = x.double().requires_grad_(True)
            ref = crit.double()(xr, t)
            ref.backward()
            xd = x.to(DEV).requires_grad_(True)
            val = crit.float().to(DEV)(xd, t.to(DEV))
            val.backward()
            assert abs(val.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
            assert (xd.grad.cpu().double() - xr.grad).abs().max().item() <= 1e-3 * xr.grad.abs().max().item()
            assert torch.count_nonzero(xd.grad.cpu().movedim(1, -1)[t == ignored]).item() == 0


def test_out_of_range_label_gives_nan_without_indexing():
    """a non-ignored label outside [0, C) is never used as an index: the loss is NaN, the other voxels' gradients intact"""
    x, t = _inputs((1, 3, 4, 4, 4), "label", 51)
    t[0, 1, 2, 3] = 3
    xd = x.to(DEV).requires_grad_(True)
    val = L._upgrade(torch.nn.CrossEntropyLoss())(xd, t.to(DEV))
    val.backward()
    assert torch.isnan(val.cpu())
    g = xd.grad.cpu()
    assert torch.isnan(g[0, :, 1, 2, 3]).all() and torch.isfinite(g[0, :, 0]).all()


def test_native_unet3d_step_with_fused_ce():
    """a full native UNet3D step (3-class softmax head) on the fused CE: the parameter gradients equal the same model's with
    torch's cross entropy taken on float64 CPU copies of the logits, within the model tests' 1e-3 gate"""
    from pytorch3dunet_amd.unet3d.model import UNet3D

    torch.manual_seed(0)
    model = UNet3D(2, 3, final_sigmoid=False, f_maps=[8, 16, 32], num_groups=4)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "groupnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    model = model.to(DEV).train()
    x = torch.randn(1, 2, 16, 20, 24, device=DEV)
    t = torch.randint(0, 3, (1, 16, 20, 24), device=DEV)
    crit = L._upgrade(torch.nn.CrossEntropyLoss())

    n0 = nat.launch_count
    _, logits = model(x, return_logits=True)
    n1 = nat.launch_count
    loss = crit(logits, t)
    assert nat.launch_count > n1 > n0
    model.zero_grad()
    loss.backward()
    ours = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters()}

    _, logits = model(x, return_logits=True)
    l64 = logits.detach().cpu().double().requires_grad_(True)
    ref = F.cross_entropy(l64, t.cpu())
    ref.backward()
    model.zero_grad()
    logits.backward(l64.grad.float().to(DEV))
    torch.cuda.synchronize()
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    worst = max((orc.rel_err(ours[k], p.grad.detach().cpu().double()), k) for k, p in model.named_parameters())
    assert worst[0] < 1e-3, worst
