"""-m gpu: UNet3D under `bf16_subpixel: true` on the MI355X — the decoders' first convolutions at exact-2x levels on the sub-pixel bf16
kernels of csrc/u3d_subpix_bf16.hip (no written-out concat), every other layer as under `compute_dtype: bf16` — against the float64
emulation with the same rounding points restated (tests/bf16_emul_3d_subpixel.py) and against the plain float64 run, with the bars of
tests/test_gpu_bf16.py (logits 3e-2 of their range, global gradient rel-L2 0.15).

The emulation's own distance from the plain run, measured on the CPU (logits / gradient rel-L2; tests/test_bf16_subpixel3d.py asserts
them inside 2/3 of the bars): 0.0149 / 0.0733 at (2, 1, 16, 32, 32), 0.0114 / 0.0818 at (2, 1, 16, 32, 26), 0.0053 / 0.0869 for the 'bcr'
net and 0.0071 / 0.0878 for the softmax net."""
import warnings

import pytest
import torch

import bf16_emul_3d_subpixel as SE
import unet3d_oracle as orc
from conftest import diag
from gpu_utils import DEV
from test_gpu_model2d_bf16 import _step

pytestmark = pytest.mark.gpu
NEW = {"u3d_subpixel_conv_fwd_bf16", "u3d_subpixel_conv_dgrad_bf16", "u3d_subpixel_conv_wgrad_bf16"}
_REF = {}


def _reference(cfg, shape):
    """(plain, emulation) float64 runs of a case, computed once and shared by its variants (never modified)"""
    key = (str(cfg), shape)
    if key not in _REF:
        _, sd, x, target = SE.prep(cfg, shape)
        ln = SE.loss_name_of(cfg)
        _REF[key] = (SE.run(cfg, sd, x, target, ln, emulate=False), SE.run(cfg, sd, x, target, ln, emulate=True))
    return _REF[key]


@pytest.mark.parametrize("cfg,shape", SE.MODEL_CASES)
def test_unet3d_bf16_subpixel_against_its_emulation_and_plain_float64(cfg, shape):
    """(1) closer to the emulation of the same rounding points than 0.75x the emulation's own distance from the plain float64 run, for the
    logits and for the global gradient rel-L2; (2) within the stated bf16 tolerance of the plain run; (3) the routing, read off the
    recorded launch names.  All distances go to conftest.diag."""
    model, sd, x, target = SE.prep(cfg, shape, bf16_subpixel=True)
    assert model.native_supported and model.compute_bf16 and model.bf16_subpixel, model._native_blockers
    n_dec, n_sub = len(model.decoders), len(SE.eligible_subpixel(model, shape))
    assert n_sub >= 1
    plain, emul = _reference(cfg, shape)
    logits, loss, grads, names = _step(model, x, target, SE.loss_name_of(cfg))  # (raises on any warning)
    # routing: the three new entry points, the skip half's epilogue launch and its strided weight gradient ran; a concat is written out
    # if and only if some level is outside the rule
    assert NEW <= names and "u3d_conv3d_bf16_ex" in names and "u3d_conv3d_wgrad_bf16_strided" in names, names
    assert ("u3d_nearest_cat_fwd" in names) == (n_sub < n_dec), names
    ours = (logits, loss, grads)
    e_l16, e_g16 = SE.distances(ours, emul)
    e_l32, e_g32 = SE.distances(ours, plain)
    e_l_or, e_or = SE.distances(emul, plain)
    rec = dict(test="bf16_subpixel_model_3d", cfg=str(cfg), shape=str(shape), logits_vs_bf16_emulation=e_l16, logits_vs_plain=e_l32,
               grad_l2_vs_bf16_emulation=e_g16, grad_l2_vs_plain=e_g32, emulation_vs_plain_grad_l2=e_or, emulation_vs_plain_logits=e_l_or)
    diag(**rec)
    print(rec)
    assert e_l16 < 0.75 * e_l_or and e_g16 < 0.75 * e_or, rec
    assert e_l32 < SE.BF16_LOGITS_TOL and e_g32 < SE.BF16_GRAD_TOL, rec


@pytest.mark.parametrize("cfg,shape", [(SE.MODEL_CASES[0][0], SE.NO_ELIGIBLE_SHAPE), (SE.NET_OUTSIDE_CHANNEL_RULE, (1, 1, 16, 16, 16))],
                         ids=["no_exact_2x_level", "no_level_inside_the_channel_rule"])
def test_a_model_without_eligible_levels_is_unchanged_by_the_key(cfg, shape):
    """every level upsamples n -> 2n + 1 on some axis, or no level lies inside the channel rule: logits and every gradient bitwise equal
    to plain `compute_dtype: bf16`"""
    runs = []
    for extra in (dict(compute_dtype="bf16"), dict(bf16_subpixel=True)):
        model, sd, x, target = SE.prep(cfg, shape, **extra)
        assert not SE.eligible_subpixel(model, shape)
        logits, loss, grads, names = _step(model, x, target, "bce_dice")
        assert not (NEW & names), names
        runs.append((logits, grads, names))
    assert runs[0][2] == runs[1][2]  # the same entry points ran
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_eval_forward_equals_the_training_forward():
    cfg, shape = SE.MODEL_CASES[0]
    model, sd, x, target = SE.prep(cfg, shape, bf16_subpixel=True)
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


def test_checkpointed_encoders_give_the_same_gradients():
    """`checkpoint_encoders: true` next to the key: the decoders are not recomputed, the recomputed encoder blocks are bit-identical"""
    cfg, shape = SE.MODEL_CASES[0]
    runs = []
    for extra in (dict(bf16_subpixel=True), dict(bf16_subpixel=True, checkpoint_encoders=True)):
        model, sd, x, target = SE.prep(cfg, shape, **extra)
        logits, loss, grads, names = _step(model, x, target, "bce_dice")
        assert NEW <= names, names
        runs.append((logits, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_hip_graph_is_refused_at_construction():
    """the decision of DESIGN.md §9 for `hip_graph: true` next to the key: a ValueError, before anything touches the device"""
    from pytorch3dunet_amd.unet3d.model import get_model

    with pytest.raises(ValueError, match="hip_graph is not available with bf16_subpixel"):
        get_model(dict(SE.MODEL_CASES[0][0], bf16_subpixel=True, hip_graph=True))
