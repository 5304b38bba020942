"""-m gpu: UNet2D under `native_2d_bf16: true` on the MI355X — the 3x3 layers whose channel counts fit on the bf16 kernels of
csrc/u3d_conv2d_bf16.hip (the decoders' first convolutions on a materialised concat), the others on the fp32 2-D kernels, no warning —
against the float64 emulation with the same operand rounding restated (tests/bf16_emul_2d.py) and against the plain float64 run, with the
gates of tests/test_gpu_bf16.py::test_model_bf16_against_bf16_operand_oracle_and_fp32_oracle."""
import warnings

import pytest
import torch

import bf16_emul_2d as E
import unet3d_oracle as orc
from conftest import diag, loss_by_name
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model

pytestmark = pytest.mark.gpu

BF16_LOGITS_TOL = 3e-2  # the stated bf16 tolerances of tests/test_gpu_bf16.py: logits within 3 % of their range ...
BF16_GRAD_TOL = 0.15    # ... and the global relative L2 distance of all parameter gradients within 15 % of the plain run

CASES = [
    # floor pooling (35 -> 17 -> 8, 45 -> 22 -> 11) and n -> 2n + 1 decoder levels; 8 of the 10 layers on the bf16 kernels
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="gcr", num_groups=8), (2, 1, 35, 45)),
    # the shipped 2-D order: BatchNorm in front of the convolution
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="bcr"), (2, 1, 32, 32)),
    # several input / output channels, softmax head
    (dict(name="UNet2D", in_channels=2, out_channels=3, f_maps=[32, 64], final_sigmoid=False, num_groups=8), (1, 2, 24, 40)),
]


def _prep(cfg, shape, **extra):
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


def _step(model, x, target, loss_name):
    model = model.to(DEV).train()
    prof = nat.EventProfiler()
    nat.profiler = prof
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the native path raises no "not covered" warning
            probs, logits = model(x.to(DEV), return_logits=True)
            loss = loss_by_name(loss_name, probs, logits, target.to(DEV))
            model.zero_grad()
            loss.backward()
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return logits.detach().cpu(), loss.item(), grads, set(prof.summary())


@pytest.mark.parametrize("cfg,shape", CASES)
def test_unet2d_bf16_against_bf16_operand_emulation_and_plain_float64(cfg, shape):
    """(1) closer to the emulation of the same operand rounding than 0.75x the emulation's own distance from the plain float64 run, for
    the logits and for the global gradient rel-L2 (a network of bf16 layers is chaotic in the last bf16 bit, see the 3-D test);
    (2) within the stated bf16 tolerance of the plain run.  All five distances of every case go to conftest.diag.

    The bars are the 3-D test's, unchanged; the distances of the 2-D cases have not been recorded on an MI355X yet, so no
    measured worst is stated here — every run of this test records them through conftest.diag."""
    loss_name = "bce_dice" if cfg.get("final_sigmoid", True) else "probs_sum"
    model, sd, x, target = _prep(cfg, shape, native_2d_bf16=True)
    assert model.native_supported and model.compute_bf16, model._native_blockers
    l32, _, g32 = E.run(cfg, sd, x, target, loss_name, emulate=False)
    l16, _, g16 = E.run(cfg, sd, x, target, loss_name, emulate=True)
    logits, loss, grads, names = _step(model, x, target, loss_name)
    # routing: the bf16 family ran, the concat was written out, the ineligible first layers stayed on the fp32 2-D kernel
    assert "u3d_conv2d_bf16" in names and "u3d_conv2d_wgrad_bf16" in names, names
    assert "u3d_nearest_cat_fwd" in names, names
    assert "u3d_conv2d_ex_reps" in names and "u3d_conv2d_wgrad" in names, names
    keys = list(g32)
    cat = lambda d: torch.cat([d[k].flatten().double() for k in keys])  # noqa: E731
    ours, r16, r32 = cat(grads), cat(g16), cat(g32)
    e_l16, e_l32, e_l_or = orc.rel_err(logits.double(), l16), orc.rel_err(logits.double(), l32), orc.rel_err(l16, l32)
    e_g16 = ((ours - r16).norm() / r16.norm()).item()
    e_g32 = ((ours - r32).norm() / r32.norm()).item()
    e_or = ((r16 - r32).norm() / r32.norm()).item()
    rec = dict(test="bf16_model_2d", cfg=str(cfg), shape=str(shape), logits_vs_bf16_emulation=e_l16, logits_vs_plain=e_l32,
               grad_l2_vs_bf16_emulation=e_g16, grad_l2_vs_plain=e_g32, emulation_vs_plain_grad_l2=e_or, emulation_vs_plain_logits=e_l_or)
    diag(**rec)
    print(rec)
    assert e_l16 < 0.75 * e_l_or and e_g16 < 0.75 * e_or, rec
    assert e_l32 < BF16_LOGITS_TOL and e_g32 < BF16_GRAD_TOL, rec


def test_eval_forward_equals_the_training_forward():
    """a GroupNorm net computes the same logits in training mode and under eval() + torch.no_grad() (no tape, forward images only)"""
    cfg, shape = CASES[0]
    model, sd, x, target = _prep(cfg, shape, native_2d_bf16=True)
    model = model.to(DEV).train()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, l_train = model(x.to(DEV), return_logits=True)
        model.eval()
        with torch.no_grad():
            _, l_eval = model(x.to(DEV), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(l_train.detach().cpu(), l_eval.cpu())


def test_a_model_without_eligible_layers_is_unchanged_by_the_key():
    """f_maps = [8, 16]: no layer fits the bf16 kernels, every convolution stays on the fp32 2-D kernels — gradients bitwise equal to
    the native_2d run"""
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], layer_order="gcr", num_groups=4)
    shape = (2, 1, 35, 45)
    runs = []
    for extra in (dict(native_2d=True), dict(native_2d_bf16=True)):
        model, sd, x, target = _prep(cfg, shape, **extra)
        logits, loss, grads, names = _step(model, x, target, "bce_dice")
        assert "u3d_conv2d_ex_reps" in names and not any("bf16" in n for n in names), names
        runs.append((logits, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
