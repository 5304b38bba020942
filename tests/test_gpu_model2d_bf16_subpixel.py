"""-m gpu: UNet2D under `native_2d_bf16_subpixel: true` on the MI355X — the decoders' first convolutions at exact-2x levels on the sub-pixel
bf16 kernels of csrc/u3d_conv2d_bf16.hip (no written-out concat), every other layer as under `native_2d_bf16` — against the float64
emulation with the same rounding points restated (tests/bf16_emul_2d_subpixel.py) and against the plain float64 run, with the gates of
tests/test_gpu_model2d_bf16.py.

The emulation's own distance from the plain run, measured on the CPU (logits / gradient rel-L2; tests/test_native2d_bf16_subpixel.py
asserts them inside the bars): 0.0072 / 0.0170 at (2, 1, 32, 40), 0.0079 / 0.0060 at (2, 1, 36, 42), 0.0041 / 0.0649 for the 'bcr' net and
0.0050 / 0.0839 for the softmax net.  A three-level 'gcr' net is deliberately not a gated case: ReLU decision flips alone put its emulation
at 0.14 - 0.18 of the 0.15 gradient bar."""
import warnings

import pytest
import torch

import bf16_emul_2d_subpixel as SE
import unet3d_oracle as orc
from conftest import diag
from gpu_utils import DEV
from test_gpu_model2d_bf16 import _step

pytestmark = pytest.mark.gpu
NEW = {"u3d_subpixel2d_conv_fwd_bf16", "u3d_subpixel2d_conv_dgrad_bf16", "u3d_subpixel2d_conv_wgrad_bf16"}
_REF = {}


def _reference(cfg, shape):
    """(plain, emulation) float64 runs of a case, computed once and shared by its variants (never modified)"""
    key = (str(cfg), shape)
    if key not in _REF:
        _, sd, x, target = SE.prep(cfg, shape)
        ln = SE.loss_name_of(cfg)
        _REF[key] = (SE.run(cfg, sd, x, target, ln, emulate=False), SE.run(cfg, sd, x, target, ln, emulate=True))
    return _REF[key]


@pytest.mark.parametrize("cfg,shape,extra", SE.MODEL_CASES)
def test_unet2d_bf16_subpixel_against_its_emulation_and_plain_float64(cfg, shape, extra):
    """(1) closer to the emulation of the same rounding points than 0.75x the emulation's own distance from the plain float64 run, for the
    logits and for the global gradient rel-L2; (2) within the stated bf16 tolerance of the plain run; (3) the routing, read off the
    recorded launch names.  All distances go to conftest.diag."""
    model, sd, x, target = SE.prep(cfg, shape, native_2d_bf16_subpixel=True, **extra)
    assert model.native_supported and model.compute_bf16 and model.native_2d_bf16_subpixel, model._native_blockers
    n_dec, n_sub = len(model.decoders), len(SE.eligible_subpixel(model, shape))
    assert n_sub >= 1
    plain, emul = _reference(cfg, shape)
    logits, loss, grads, names = _step(model, x, target, SE.loss_name_of(cfg))  # (raises on any warning)
    # routing: the three new entry points and the residual epilogue ran; a concat is written out only for a level outside the rule, and
    # only without the virtual concat, whose `_src` entry points then take it
    assert NEW <= names and "u3d_conv2d_bf16_res" in names and "u3d_conv2d_wgrad_bf16_strided" in names, names
    outside = n_sub < n_dec
    assert ("u3d_nearest_cat_fwd" in names) == (outside and not extra), names
    assert ("u3d_conv2d_bf16_src" in names) == (outside and bool(extra)), names
    ours = (logits, loss, grads)
    e_l16, e_g16 = SE.distances(ours, emul)
    e_l32, e_g32 = SE.distances(ours, plain)
    e_l_or, e_or = SE.distances(emul, plain)
    rec = dict(test="bf16_subpixel_model_2d", cfg=str(cfg), shape=str(shape), extra=str(extra), logits_vs_bf16_emulation=e_l16,
               logits_vs_plain=e_l32, grad_l2_vs_bf16_emulation=e_g16, grad_l2_vs_plain=e_g32, emulation_vs_plain_grad_l2=e_or,
               emulation_vs_plain_logits=e_l_or)
    diag(**rec)
    print(rec)
    assert e_l16 < 0.75 * e_l_or and e_g16 < 0.75 * e_or, rec
    assert e_l32 < SE.BF16_LOGITS_TOL and e_g32 < SE.BF16_GRAD_TOL, rec


def test_a_model_without_eligible_levels_is_unchanged_by_the_key():
    """(2, 1, 35, 45): every level upsamples n -> 2n + 1 on some axis — logits and gradients bitwise equal to `native_2d_bf16`"""
    cfg, shape = SE.MODEL_CASES[0][0], SE.NO_ELIGIBLE_SHAPE
    runs = []
    for extra in (dict(native_2d_bf16=True), dict(native_2d_bf16_subpixel=True)):
        model, sd, x, target = SE.prep(cfg, shape, **extra)
        assert not SE.eligible_subpixel(model, shape)
        logits, loss, grads, names = _step(model, x, target, "bce_dice")
        assert not (NEW & names) and "u3d_nearest_cat_fwd" in names, names
        runs.append((logits, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_eval_forward_equals_the_training_forward():
    cfg, shape, _ = SE.MODEL_CASES[0]
    model, sd, x, target = SE.prep(cfg, shape, native_2d_bf16_subpixel=True)
    model = model.to(DEV).train()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, l_train = model(x.to(DEV), return_logits=True)
        model.eval()
        with torch.no_grad():
            _, l_eval = model(x.to(DEV), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(l_train.detach().cpu(), l_eval.cpu())
    assert orc.rel_err(l_eval.cpu().double(), _reference(cfg, shape)[1][0]) < SE.BF16_LOGITS_TOL
