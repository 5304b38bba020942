"""ResidualUNet2D under `native_2d_residual: true` on the MI355X: (N,C,H,W) in and out, the 3x3 convolutions on csrc/u3d_conv2d.hip (conv3
with the residual epilogue), the decoders' ConvTranspose2d on u3d_convtr2d_*, no warning — against the recorded live reference
(tests/golden/r7_reference_resunet2d.npz) and the float64 module tree on the CPU, with the bars of tests/test_gpu_model2d.py: logits /
probs within 1e-4 of the range, the loss within 1e-4, the global gradient rel-L2 within max(1e-3, 2x the fp32 module tree's own distance
from float64)."""
import contextlib
import warnings

import pytest
import torch

import unet3d_oracle as orc
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from reference_records_resunet2d import CASES, RunRes2D

pytestmark = pytest.mark.gpu
REL = 1e-4
NEW_ENTRY_POINTS = ("u3d_conv2d_res_reps", "u3d_convtr2d_fwd")
NEW_BWD_ENTRY_POINTS = ("u3d_convtr2d_dgrad", "u3d_convtr2d_wgrad")


@contextlib.contextmanager
def called_entry_points():
    """the names of the native entry points called inside the block (nat.call wrapped)"""
    names, orig = set(), nat.call

    def spy(name, *args, **kw):
        names.add(name)
        return orig(name, *args, **kw)

    nat.call = spy
    try:
        yield names
    finally:
        nat.call = orig


def _loss(model, probs, logits, target):
    if model.final_activation is None:
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


def run_and_check(cfg, shape, seed=0, perturb=True, sd=None, x=None, target=None):
    torch.manual_seed(seed)
    model = get_model(dict(cfg, native_2d_residual=True))
    assert model.native_supported and model.native_2d, model._native_blockers
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
    _, p64, l64, loss64, g64 = _cpu_run(cfg, sd, x, target, torch.float64, True)
    _, _, _, _, g32 = _cpu_run(cfg, sd, x, target, torch.float32, True)
    model = model.to(DEV).train()
    n0 = nat.launch_count
    with warnings.catch_warnings(), called_entry_points() as names:
        warnings.simplefilter("error")  # the native path raises no "not covered" warning
        probs, logits = model(x.to(DEV), return_logits=True)
        loss = _loss(model, probs, logits, target.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    assert nat.launch_count > n0, "native HIP path did not run"
    # (the residual rides in conv3's epilogue for pre-norm orders; post-norm and norm-free orders add it in the norm-apply pass)
    want = {"u3d_convtr2d_fwd"} | set(NEW_BWD_ENTRY_POINTS)
    if cfg.get("layer_order", "gcr")[0] in "gb":
        want.add("u3d_conv2d_res_reps")
    assert want <= names, names
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
def test_resunet2d_matches_reference_records(case):
    """seeded ResidualUNet2D runs of the live reference at 2 x 1 x 67 x 45: floor pooling, both resize ratios after the 2n - 1
    transposed convolutions, ELU after the add, BatchNorm, explicit deconv (concat joining) and a softmax head"""
    run = RunRes2D(case)
    g32, g64 = run_and_check(run.cfg, run.shape, sd=run.sd, x=run.x, target=run.target)
    m = get_model(dict(run.cfg, native_2d_residual=True))
    m.load_state_dict(run.sd)
    m = m.to(DEV).train()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        probs, logits = m(run.x.to(DEV), return_logits=True)
    assert orc.rel_err(logits.detach().cpu(), run.logits) < 1e-4 and orc.rel_err(probs.detach().cpu(), run.probs) < 1e-4
    loss = orc.bce_dice_loss(logits, run.target.to(DEV))
    assert abs(loss.item() - run.loss) < 1e-4
    loss.backward()
    # per parameter against the recorded fp32 run (the bar of tests/test_gpu_model2d.py)
    bad = [(k, run.grad_rel_err(k, p.grad.cpu())) for k, p in m.named_parameters()
           if run.grad_rel_err(k, p.grad.cpu()) > max(5e-3, 4.0 * orc.rel_err(g32[k].double(), g64[k]))]
    assert not bad, bad
    sd = m.state_dict()
    for k, v in run.buffers.items():  # BatchNorm running statistics after the training forward
        assert torch.allclose(sd[k].cpu(), v, rtol=1e-4, atol=1e-6), k


@pytest.mark.parametrize("order", ["gcr", "cge", "gcl", "bcr", "crg", "cr"])
def test_resunet2d_layer_orders(order):
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=2, f_maps=[8, 16, 32], num_groups=4, layer_order=order,
               final_sigmoid=False)
    run_and_check(cfg, (2, 1, 35, 29), seed=3)


def test_resunet2d_reference_defaults():
    """f_maps 64, 5 levels (64 .. 1024 channels, a 6 x 5 bottom level), one training step"""
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=64, num_groups=8, layer_order="gcr")
    run_and_check(cfg, (2, 1, 96, 80), seed=1)


def test_resunet2d_inference_and_batchnorm_running_statistics():
    """eval-mode / no_grad inference uses the running statistics; a training forward updates them as nn.BatchNorm2d does"""
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32], layer_order="bcr")
    torch.manual_seed(4)
    model = get_model(dict(cfg, native_2d_residual=True))
    ref = get_model(dict(cfg)).double()
    ref.load_state_dict(model.state_dict())
    model = model.to(DEV)
    for step in range(2):
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
    with warnings.catch_warnings(), called_entry_points() as names, torch.no_grad():
        warnings.simplefilter("error")
        probs, logits = model(x.to(DEV), return_logits=True)
    assert nat.launch_count > n0 and set(NEW_ENTRY_POINTS) <= names, names
    p64, l64 = ref(x.double(), return_logits=True)
    assert orc.rel_err(logits.cpu().double(), l64.detach()) < REL and orc.rel_err(probs.cpu().double(), p64.detach()) < REL


def test_resunet2d_input_gradient():
    """a gradient w.r.t. the (N,C,H,W) input comes back in that layout"""
    cfg = dict(name="ResidualUNet2D", in_channels=3, out_channels=1, f_maps=[8, 16], num_groups=4)
    torch.manual_seed(5)
    model = get_model(dict(cfg, native_2d_residual=True))
    ref = get_model(dict(cfg)).double()
    ref.load_state_dict(model.state_dict())
    x = torch.randn(2, 3, 24, 20)
    xg = x.to(DEV).requires_grad_(True)
    n0 = nat.launch_count
    with warnings.catch_warnings(), called_entry_points() as names:
        warnings.simplefilter("error")
        model.to(DEV)(xg).sum().backward()
    assert nat.launch_count > n0 and set(NEW_ENTRY_POINTS + NEW_BWD_ENTRY_POINTS) <= names, names
    xr = x.double().requires_grad_(True)
    ref(xr).sum().backward()
    assert xg.grad.shape == x.shape and orc.rel_err(xg.grad.cpu().double(), xr.grad) < 1e-3
