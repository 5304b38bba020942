"""-m gpu: ResidualUNet2D under `native_2d_residual_bf16: true` on the MI355X — conv2 / conv3 of every block whose width is a multiple of
32 on the bf16 kernels of csrc/u3d_conv2d_bf16.hip (conv3 of the pre-norm orders with the residual epilogue u3d_conv2d_bf16_res), the 1x1
convolutions, ConvTranspose2d, joining and the head on their fp32 kernels, no warning — against the float64 emulation with the same
operand rounding restated (tests/bf16_emul_res2d.py) and against the plain float64 run, with the two gates and the bars of
tests/test_gpu_model2d_bf16.py, taken from it unchanged."""
import warnings

import pytest
import torch

import bf16_emul_res2d as E
import test_gpu_model2d_bf16 as M2
import unet3d_oracle as orc
from conftest import diag, loss_by_name
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model

pytestmark = pytest.mark.gpu

BF16_LOGITS_TOL, BF16_GRAD_TOL = M2.BF16_LOGITS_TOL, M2.BF16_GRAD_TOL

_R = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, num_groups=8)
CASES = [
    # floor pooling (35 -> 17 -> 8, 45 -> 22 -> 11) and the 2n - 1 -> 2n + 1 resize after the transposed convolutions; ten bf16 layers
    (dict(_R, f_maps=[32, 64, 128], layer_order="gcr"), (2, 1, 35, 45)),
    # ELU after the add: the epilogue runs without ReLU and the in-place activation pass follows
    (dict(_R, f_maps=[32, 64], layer_order="gce"), (2, 1, 32, 32)),
    # explicit deconv: concat joining consumed by the block's 1x1 conv1; several input / output channels, softmax head
    (dict(_R, f_maps=[32, 64], upsample="deconv", in_channels=2, out_channels=3, final_sigmoid=False), (1, 2, 24, 40)),
    # post-norm: the residual is added in the norm-apply pass, conv3 takes the plain entry point
    (dict(_R, f_maps=[32, 64], layer_order="cge"), (2, 1, 32, 32)),
]
FP32_CONV_ENTRY_POINTS = {"u3d_conv2d_res_reps", "u3d_conv2d_ex_reps", "u3d_conv2d_wgrad"}


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
def test_resunet2d_bf16_against_bf16_operand_emulation_and_plain_float64(cfg, shape):
    """(1) closer to the emulation of the same operand rounding than 0.75x the emulation's own distance from the plain float64 run, for
    the logits and for the global gradient rel-L2; (2) within the stated bf16 tolerance of the plain run.  All five distances of every
    case go to conftest.diag.  The bars are the UNet2D test's, unchanged.  Measured worst on an MI355X: gate 1 at 0.47 of the
    emulation's own distance (gradients of the `gcr` case; logits 0.36, `cge`), gate 2 at 7.0e-2 for gradients (`deconv` case) and 6.1e-3
    for logits (`gcr`)."""
    loss_name = "bce_dice" if cfg.get("final_sigmoid", True) else "probs_sum"
    model, sd, x, target = M2._prep(cfg, shape, native_2d_residual_bf16=True)
    assert model.native_supported and model.compute_bf16 and model.native_2d_residual_bf16, model._native_blockers
    l32, _, g32 = E.run(cfg, sd, x, target, loss_name, emulate=False)
    l16, _, g16 = E.run(cfg, sd, x, target, loss_name, emulate=True)
    logits, loss, grads, names = _step(model, x, target, loss_name)
    # routing: every 3x3 layer of these nets fits, in all three directions; the transposed convolutions stay on their fp32 kernels
    pre_norm = cfg.get("layer_order", "gcr")[0] in "gb"
    assert {"u3d_conv2d_bf16", "u3d_conv2d_wgrad_bf16", "u3d_convtr2d_fwd", "u3d_convtr2d_dgrad", "u3d_convtr2d_wgrad"} <= names, names
    assert ("u3d_conv2d_bf16_res" in names) == pre_norm, names
    assert not (FP32_CONV_ENTRY_POINTS & names), names
    assert not any("_b16" in n or "_t8" in n for n in names), names  # fp32 activation storage, no 3-D space-to-depth branch
    keys = list(g32)
    cat = lambda d: torch.cat([d[k].flatten().double() for k in keys])  # noqa: E731
    ours, r16, r32 = cat(grads), cat(g16), cat(g32)
    e_l16, e_l32, e_l_or = orc.rel_err(logits.double(), l16), orc.rel_err(logits.double(), l32), orc.rel_err(l16, l32)
    e_g16 = ((ours - r16).norm() / r16.norm()).item()
    e_g32 = ((ours - r32).norm() / r32.norm()).item()
    e_or = ((r16 - r32).norm() / r32.norm()).item()
    rec = dict(test="bf16_resunet_2d", cfg=str(cfg), shape=str(shape), logits_vs_bf16_emulation=e_l16, logits_vs_plain=e_l32,
               grad_l2_vs_bf16_emulation=e_g16, grad_l2_vs_plain=e_g32, emulation_vs_plain_grad_l2=e_or, emulation_vs_plain_logits=e_l_or)
    diag(**rec)
    print(rec)
    assert e_l16 < 0.75 * e_l_or and e_g16 < 0.75 * e_or, rec
    assert e_l32 < BF16_LOGITS_TOL and e_g32 < BF16_GRAD_TOL, rec


def test_eval_forward_equals_the_training_forward():
    """a GroupNorm net computes the same logits in training mode and under eval() + torch.no_grad() (no tape, forward images only)"""
    cfg, shape = CASES[0]
    model, sd, x, target = M2._prep(cfg, shape, native_2d_residual_bf16=True)
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
    """f_maps = [8, 16]: no layer fits the bf16 kernels, every convolution stays on the fp32 2-D kernels — logits and every gradient
    bitwise equal to the native_2d_residual run, no bf16 entry point called"""
    cfg = dict(_R, f_maps=[8, 16], layer_order="gcr", num_groups=4)
    shape = (2, 1, 35, 45)
    runs = []
    for extra in (dict(native_2d_residual=True), dict(native_2d_residual_bf16=True)):
        model, sd, x, target = M2._prep(cfg, shape, **extra)
        logits, loss, grads, names = _step(model, x, target, "bce_dice")
        assert "u3d_conv2d_res_reps" in names and "u3d_conv2d_ex_reps" in names and not any("bf16" in n for n in names), names
        runs.append((logits, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_explicit_bf16_activation_storage_warns_and_matches_the_auto_run():
    """`activation_dtype: bf16` next to the key: the 2-D kernels have no bf16-storage forms — one warning when the executor is built,
    then the `auto` run bit for bit"""
    cfg, shape = CASES[1]
    model, sd, x, target = M2._prep(cfg, shape, native_2d_residual_bf16=True)
    auto = _step(model, x, target, "bce_dice")
    model, sd, x, target = M2._prep(cfg, shape, native_2d_residual_bf16=True, activation_dtype="bf16")
    with pytest.warns(UserWarning, match="activations stay fp32"):
        eng = model._get_engine()
    assert not eng.act_bf16
    explicit = _step(model, x, target, "bce_dice")  # (warnings are errors inside: the executor warned once, above)
    assert torch.equal(auto[0], explicit[0]) and auto[3] == explicit[3]
    assert all(torch.equal(auto[2][k], explicit[2][k]) for k in auto[2])
