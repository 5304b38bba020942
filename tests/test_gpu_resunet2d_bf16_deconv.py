"""-m gpu: ResidualUNet2D under `native_2d_residual_bf16_deconv: true` on the MI355X — the `native_2d_residual_bf16` path with the
decoders' ConvTranspose2d (both channel counts % 32) on u3d_convtr2d_fwd_bf16 / _dgrad_bf16 / _wgrad_bf16 — against the float64
emulation with the same operand rounding restated (tests/bf16_emul_res2d_deconv.py) and against the plain float64 run, with the two
gates and the bars of tests/test_gpu_resunet2d_bf16.py, taken from it unchanged."""
import pytest
import torch

import bf16_emul_res2d_deconv as E
import test_gpu_model2d_bf16 as M2
import test_gpu_resunet2d_bf16 as R2
import unet3d_oracle as orc
from conftest import diag

pytestmark = pytest.mark.gpu

BF16_LOGITS_TOL, BF16_GRAD_TOL = R2.BF16_LOGITS_TOL, R2.BF16_GRAD_TOL
KEY = dict(native_2d_residual_bf16_deconv=True)
_R = R2._R
CASES = [
    # two transposed convolutions (128 -> 64, 64 -> 32) between floor pooling and the 2n - 1 -> 2n + 1 resize; summation joining
    (dict(_R, f_maps=[32, 64, 128], layer_order="gcr"), (2, 1, 35, 45)),
    # explicit deconv: 64 -> 64 into the concat consumed by the block's 1x1 conv1; several input / output channels, softmax head
    (dict(_R, f_maps=[32, 64], upsample="deconv", in_channels=2, out_channels=3, final_sigmoid=False), (1, 2, 24, 40)),
]
BF16_DECONV = {"u3d_convtr2d_fwd_bf16", "u3d_convtr2d_dgrad_bf16", "u3d_convtr2d_wgrad_bf16"}
FP32_DECONV = {"u3d_convtr2d_fwd", "u3d_convtr2d_dgrad", "u3d_convtr2d_wgrad"}


@pytest.mark.parametrize("cfg,shape", CASES)
def test_resunet2d_bf16_deconv_against_bf16_operand_emulation_and_plain_float64(cfg, shape):
    """(0) the emulation alone is inside the bars of the plain run on these inputs; (1) the GPU result is closer to the emulation of the
    same operand rounding than 0.75x the emulation's own distance from the plain float64 run, for the logits and for the global gradient
    rel-L2; (2) it is within 3e-2 (logits) and 0.15 (gradient rel-L2) of the plain run.  All distances go to conftest.diag; the measured
    ones are in DESIGN.md §9."""
    loss_name = "bce_dice" if cfg.get("final_sigmoid", True) else "probs_sum"
    model, sd, x, target = M2._prep(cfg, shape, **KEY)
    assert model.native_supported and model.compute_bf16 and model.native_2d_residual_bf16_deconv, model._native_blockers
    assert len(E.eligible_convtr(model)) == len(cfg["f_maps"]) - 1
    l32, _, g32 = E.run(cfg, sd, x, target, loss_name, emulate=False)
    l16, _, g16 = E.run(cfg, sd, x, target, loss_name, emulate=True)
    logits, loss, grads, names = R2._step(model, x, target, loss_name)
    # routing: every 3x3 layer and every transposed convolution of these nets fits, in all three directions
    assert BF16_DECONV <= names and not (FP32_DECONV & names), names
    assert {"u3d_conv2d_bf16", "u3d_conv2d_wgrad_bf16"} <= names and not (R2.FP32_CONV_ENTRY_POINTS & names), names
    assert not any("_b16" in n or "_t8" in n for n in names), names  # fp32 activation storage, no 3-D space-to-depth branch
    keys = list(g32)
    cat = lambda d: torch.cat([d[k].flatten().double() for k in keys])  # noqa: E731
    ours, r16, r32 = cat(grads), cat(g16), cat(g32)
    e_l16, e_l32, e_l_or = orc.rel_err(logits.double(), l16), orc.rel_err(logits.double(), l32), orc.rel_err(l16, l32)
    e_g16 = ((ours - r16).norm() / r16.norm()).item()
    e_g32 = ((ours - r32).norm() / r32.norm()).item()
    e_or = ((r16 - r32).norm() / r32.norm()).item()
    rec = dict(test="bf16_resunet_2d_deconv", cfg=str(cfg), shape=str(shape), logits_vs_bf16_emulation=e_l16, logits_vs_plain=e_l32,
               grad_l2_vs_bf16_emulation=e_g16, grad_l2_vs_plain=e_g32, emulation_vs_plain_grad_l2=e_or, emulation_vs_plain_logits=e_l_or)
    diag(**rec)
    print(rec)
    assert e_l_or < BF16_LOGITS_TOL and e_or < BF16_GRAD_TOL, rec  # (0)
    assert e_l16 < 0.75 * e_l_or and e_g16 < 0.75 * e_or, rec
    assert e_l32 < BF16_LOGITS_TOL and e_g32 < BF16_GRAD_TOL, rec


def test_a_model_without_eligible_layers_is_unchanged_by_the_key():
    """f_maps = [8, 16]: neither a 3x3 layer nor the transposed convolution fits the bf16 kernels — logits and every gradient bitwise equal
    to the native_2d_residual_bf16 run, no bf16 entry point called"""
    cfg = dict(_R, f_maps=[8, 16], layer_order="gcr", num_groups=4)
    shape = (2, 1, 35, 45)
    runs = []
    for extra in (dict(native_2d_residual_bf16=True), KEY):
        model, sd, x, target = M2._prep(cfg, shape, **extra)
        logits, loss, grads, names = R2._step(model, x, target, "bce_dice")
        assert FP32_DECONV <= names and not any("bf16" in n for n in names), names
        runs.append((logits, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_an_eligible_model_differs_from_the_run_without_the_key():
    """f_maps = [32, 64]: the 64 -> 32 transposed convolution moves to the bf16 kernels — other entry points, other bits, and only within
    the operand rounding of the run without the key"""
    cfg, shape = dict(_R, f_maps=[32, 64], layer_order="gcr"), (1, 1, 24, 40)
    runs = []
    for extra in (dict(native_2d_residual_bf16=True), KEY):
        model, sd, x, target = M2._prep(cfg, shape, **extra)
        logits, loss, grads, names = R2._step(model, x, target, "bce_dice")
        runs.append((logits, grads, names))
    assert FP32_DECONV <= runs[0][2] and not (BF16_DECONV & runs[0][2]), runs[0][2]
    assert BF16_DECONV <= runs[1][2] and not (FP32_DECONV & runs[1][2]), runs[1][2]
    assert runs[0][2] - FP32_DECONV - {"u3d_pack_convtr2d"} == runs[1][2] - BF16_DECONV - {"u3d_pack_convtr2d_bf16"}  # the rest runs what it ran
    assert not torch.equal(runs[0][0], runs[1][0])
    assert orc.rel_err(runs[1][0].double(), runs[0][0].double()) < BF16_LOGITS_TOL
    kw = "decoders.0.upsampling.upsample.conv_transposed.weight"
    assert not torch.equal(runs[0][1][kw], runs[1][1][kw])
