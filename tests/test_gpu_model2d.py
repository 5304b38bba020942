"""UNet2D under `native_2d: true` on the MI355X: (N,C,H,W) in and out, every 3x3 convolution and pool on csrc/u3d_conv2d.hip, no
warning — against the float64 module tree on the CPU (whose fp32 form reproduces the live reference, tests/test_native2d.py) with the
bars of tests/test_gpu_model.py: logits / probs within 1e-4 of the range, the loss within 1e-4, the global gradient rel-L2 within
max(1e-3, 2x the fp32 module tree's own distance from float64)."""
import warnings

import pytest
import torch

import unet3d_oracle as orc
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from reference_records_2d import CASES, Run2D

pytestmark = pytest.mark.gpu
REL = 1e-4


def _loss(model, probs, logits, target):
    if model.final_activation is None:  # regression head: a smooth loss on the raw output
        return ((logits - target) ** 2).mean()
    return orc.bce_dice_loss(logits, target)


def _cpu_run(cfg, sd, x, target, dtype, train):
    m = get_model(dict(cfg)).to(dtype)
    m.load_state_dict(sd)
    m.train(train)
    probs, logits = m(x.to(dtype), return_logits=True)
    loss = _loss(m, probs, logits, target.to(dtype))
    loss.backward()
    return m, probs.detach(), logits.detach(), loss.item(), {k: p.grad.detach() for k, p in m.named_parameters()}


def _global_rel_l2(ga, gb, keys):
    a = torch.cat([ga[k].double().flatten() for k in keys])
    b = torch.cat([gb[k].double().flatten() for k in keys])
    return ((a - b).norm() / b.norm()).item()


def run_and_check(cfg, shape, seed=0, train=True, perturb=True, sd=None, x=None, target=None):
    torch.manual_seed(seed)
    model = get_model(dict(cfg, native_2d=True))
    assert model.native_supported, model._native_blockers
    if sd is None:
        with torch.no_grad():  # a trained-like net: the default norm init (gamma 1, beta 0) hides half of the gradient paths
            for k, p in model.named_parameters():
                if perturb and ("groupnorm" in k or "batchnorm" in k):
                    p.add_(0.2 * torch.randn_like(p))
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        x = torch.randn(shape)
        cout = cfg.get("out_channels", 1)
        target = (torch.rand((shape[0], cout) + tuple(shape[2:])) > 0.5).float()
    model.load_state_dict(sd)
    m64, p64, l64, loss64, g64 = _cpu_run(cfg, sd, x, target, torch.float64, train)
    _, _, _, _, g32 = _cpu_run(cfg, sd, x, target, torch.float32, train)
    model = model.to(DEV).train(train)
    n0 = nat.launch_count
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the native path raises no "not covered" warning
        probs, logits = model(x.to(DEV), return_logits=True)
        loss = _loss(model, probs, logits, target.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    assert nat.launch_count > n0, "native HIP path did not run"
    assert logits.shape == tuple(x.shape[:1]) + (cfg.get("out_channels", 1),) + tuple(x.shape[2:])
    e_l, e_p = orc.rel_err(logits.detach().cpu().double(), l64), orc.rel_err(probs.detach().cpu().double(), p64)
    assert e_l < REL and e_p < REL, (e_l, e_p)
    assert abs(loss.item() - loss64) < REL * max(1.0, abs(loss64)), (loss.item(), loss64)
    keys = list(g64)
    ours = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    e_ours, e_32 = _global_rel_l2(ours, g64, keys), _global_rel_l2(g32, g64, keys)
    print(f"{cfg.get('layer_order', 'gcr')} {tuple(shape)}: logits {e_l:.1e} probs {e_p:.1e} grad rel-L2 {e_ours:.1e} "
          f"(fp32 CPU {e_32:.1e}), {nat.launch_count - n0} launches")
    assert e_ours <= max(1e-3, 2.0 * e_32), (e_ours, e_32)
    return g32, g64


@pytest.mark.parametrize("case", list(CASES))
def test_unet2d_matches_reference_records(case):
    """seeded UNet2D runs of the live reference (tests/golden/r6_reference_unet2d.npz) at 2 x 1 x 67 x 45: floor pooling and
    n -> 2n + 1 decoder levels"""
    run = Run2D(case)
    g32, g64 = run_and_check(run.cfg, run.shape, sd=run.sd, x=run.x, target=run.target)
    m = get_model(dict(run.cfg, native_2d=True))
    m.load_state_dict(run.sd)
    m = m.to(DEV).train()
    probs, logits = m(run.x.to(DEV), return_logits=True)
    assert orc.rel_err(logits.detach().cpu(), run.logits) < 1e-4 and orc.rel_err(probs.detach().cpu(), run.probs) < 1e-4
    loss = orc.bce_dice_loss(logits, run.target.to(DEV))
    assert abs(loss.item() - run.loss) < 1e-4
    loss.backward()
    # per parameter against the recorded fp32 run: 5e-3, or 4x the fp32 module tree's own distance from float64 where that is larger —
    # the first norm weight's gradient is analytically ~0 at the default init (scale invariance), so every fp32 implementation lands
    # anywhere within its round-off there (0.17 of its range for the softmax case on the CPU); the global bar is in run_and_check
    bad = [(k, run.grad_rel_err(k, p.grad.cpu())) for k, p in m.named_parameters()
           if run.grad_rel_err(k, p.grad.cpu()) > max(5e-3, 4.0 * orc.rel_err(g32[k].double(), g64[k]))]
    assert not bad, bad
    sd = m.state_dict()
    for k, v in run.buffers.items():  # BatchNorm running statistics after the training forward
        assert torch.allclose(sd[k].cpu(), v, rtol=1e-4, atol=1e-6), k


@pytest.mark.parametrize("cfg,shape", [
    # resources/2DUnet_dsb2018/train_config.yml (bcr, f_maps [32, 64, 128]) and test_config.yml (gcr) at reduced batch
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="bcr", num_groups=8), (2, 1, 256, 256)),
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="gcr", num_groups=8), (2, 1, 256, 256)),
    # resources/2DUnet_confocal_boundary/train_config.yml: f_maps 32, 4 levels, gcr, patch 515 x 512
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=32, num_levels=4, layer_order="gcr", num_groups=8), (2, 1, 515, 512)),
])
def test_shipped_2d_configurations(cfg, shape):
    run_and_check(cfg, shape, seed=1)


@pytest.mark.parametrize("cfg,shape", [
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=8, num_levels=2, num_groups=4), (1, 1, 16, 16)),  # the warning test's model
    (dict(name="UNet2D", in_channels=2, out_channels=3, f_maps=[8, 16], num_groups=4, final_sigmoid=False), (3, 2, 32, 24)),  # batch 3
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32, 64], num_groups=4), (2, 1, 8, 8)),  # 1 x 1 bottom level
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4, is_segmentation=False), (2, 1, 20, 18)),
])
def test_unet2d_edge_cases(cfg, shape):
    run_and_check(cfg, shape, seed=2)


@pytest.mark.parametrize("order", ["cr", "gcl", "cgr", "bcr"])
def test_unet2d_layer_orders(order):
    cfg = dict(name="UNet2D", in_channels=1, out_channels=2, f_maps=[8, 16, 32], num_groups=4, layer_order=order, final_sigmoid=False)
    run_and_check(cfg, (2, 1, 35, 29), seed=3)


def test_unet2d_inference_and_batchnorm_running_statistics():
    """eval-mode / no_grad inference uses the running statistics; a training forward updates them as nn.BatchNorm2d does"""
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32], layer_order="bcr")
    torch.manual_seed(4)
    model = get_model(dict(cfg, native_2d=True))
    ref = get_model(dict(cfg)).double()
    ref.load_state_dict(model.state_dict())
    model = model.to(DEV)
    for step in range(2):  # two training forwards: running estimates move
        x = torch.randn(2, 1, 40, 36)
        model.train()
        ref.train()
        model(x.to(DEV))
        ref(x.double())
    torch.cuda.synchronize()
    sd, rsd = model.state_dict(), ref.state_dict()
    for k in rsd:
        if "running" in k or "num_batches" in k:
            assert torch.allclose(sd[k].cpu().double(), rsd[k].double(), rtol=1e-4, atol=1e-6), k
    model.eval()
    ref.eval()
    x = torch.randn(3, 1, 50, 44)
    n0 = nat.launch_count
    with torch.no_grad():
        probs, logits = model(x.to(DEV), return_logits=True)
    assert nat.launch_count > n0
    p64, l64 = ref(x.double(), return_logits=True)
    assert orc.rel_err(logits.cpu().double(), l64.detach()) < REL and orc.rel_err(probs.cpu().double(), p64.detach()) < REL


def test_unet2d_input_gradient():
    """a gradient w.r.t. the (N,C,H,W) input comes back in that layout"""
    cfg = dict(name="UNet2D", in_channels=3, out_channels=1, f_maps=[8, 16], num_groups=4)
    torch.manual_seed(5)
    model = get_model(dict(cfg, native_2d=True))
    ref = get_model(dict(cfg)).double()
    ref.load_state_dict(model.state_dict())
    x = torch.randn(2, 3, 24, 20)
    xg = x.to(DEV).requires_grad_(True)
    model.to(DEV)(xg).sum().backward()
    xr = x.double().requires_grad_(True)
    ref(xr).sum().backward()
    assert xg.grad.shape == x.shape and orc.rel_err(xg.grad.cpu().double(), xr.grad) < 1e-3
