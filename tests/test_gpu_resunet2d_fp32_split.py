"""-m gpu: ResidualUNet2D under `native_2d_residual_fp32_split: true` on the MI355X.  conv2 / conv3 of every block whose width is a multiple
of 32 run forward, data gradient and weight gradient on the six-product kernels of csrc/u3d_conv2d_f32s.h (conv3 of the pre-norm orders
with the residual epilogue u3d_conv2d_f32s_res); the 1x1 convolutions, ConvTranspose2d, joining, pooling and the head stay fp32.  The claim
is fp32 grade, so the bars are those of `native_2d_residual` (tests/test_gpu_resunet2d.py), restated: one training step against the float64
module tree — logits / probs within 1e-4 of the range, the loss within 1e-4, the global gradient rel-L2 within max(1e-3, 2x the fp32 CPU
run's own distance from float64) —, no warning.  On top of them: an EventProfiler sees each entry point as often as the restated rule of
tests/f32s_emul_res2d.py says, and the logits agree with a `native_2d_residual` model on the same weights and input within 2e-5 of their
range (the bar of tests/test_gpu_model2d_fp32_split.py)."""
import warnings

import pytest
import torch

import f32s_emul_res2d as FR
import unet3d_oracle as orc
from conftest import diag
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from test_gpu_resunet2d import _cpu_run, _global_rel_l2, _loss

pytestmark = pytest.mark.gpu
KEY = FR.KEY
REL = 1e-4
FP32_CONV = ("u3d_conv2d_res_reps", "u3d_conv2d_ex_reps", "u3d_conv2d_wgrad")
CONVTR = ("u3d_convtr2d_fwd", "u3d_convtr2d_dgrad", "u3d_convtr2d_wgrad")

_R = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, num_groups=8)
CASES = {
    # floor pooling (35 -> 17 -> 8, 45 -> 22 -> 11) and the 2n - 1 -> 2n + 1 resize after the transposed convolutions
    "gcr_3levels": (dict(_R, f_maps=[32, 64, 128], layer_order="gcr"), (2, 1, 35, 45)),
    # ELU after the add: the epilogue runs without ReLU and the in-place activation pass follows
    "gce": (dict(_R, f_maps=[32, 64], layer_order="gce"), (2, 1, 32, 32)),
    # explicit deconv: concat joining consumed by the block's 1x1 conv1; several input / output channels, softmax head
    "deconv_softmax": (dict(_R, f_maps=[32, 64], upsample="deconv", in_channels=2, out_channels=3, final_sigmoid=False), (1, 2, 24, 40)),
    # post-norm: the residual is added in the norm-apply pass, `_res` is never called
    "cge_post_norm": (dict(_R, f_maps=[32, 64], layer_order="cge"), (2, 1, 32, 32)),
    # the 16-channel blocks keep u3d_conv2d_res_reps / u3d_conv2d_ex_reps next to the routed ones
    "gcr_mixed": (dict(_R, f_maps=[16, 32, 64], layer_order="gcr"), (2, 1, 35, 45)),
}


def _prep(cfg, shape, seed):
    """a trained-like net (the default norm init hides half of the gradient paths): (state dict, input, target)"""
    torch.manual_seed(seed)
    model = get_model(dict(cfg))
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "groupnorm" in k or "batchnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.randn(shape)
    target = (torch.rand((shape[0], cfg["out_channels"]) + tuple(shape[2:])) > 0.5).float()
    return sd, x, target


def _step(cfg, sd, x, target):
    """one training step on the GPU, profiled, warnings as errors: (logits, probs, loss, grads, {entry point: calls})"""
    model = get_model(dict(cfg))
    assert model.native_supported and model.native_2d_residual, model._native_blockers
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    prof = nat.EventProfiler()
    nat.profiler = prof
    n0 = nat.launch_count
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the native path raises no "not covered" warning
            probs, logits = model(x.to(DEV), return_logits=True)
            loss = _loss(model, probs, logits, target.to(DEV))
            loss.backward()
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    assert nat.launch_count > n0, "native HIP path did not run"
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return logits.detach().cpu(), probs.detach().cpu(), loss.item(), grads, {k: v["calls"] for k, v in prof.summary().items()}


@pytest.mark.parametrize("case", list(CASES))
def test_resunet2d_fp32_split_holds_the_fp32_bars_and_routes_every_layer_of_the_rule(case):
    cfg, shape = CASES[case]
    keyed = dict(cfg, **{KEY: True})
    model = get_model(dict(keyed))
    assert model.native_supported and model.compute_split and model._get_engine().split2d, model._native_blockers
    routed = FR.routed(model)
    n_res = sum(r for _, _, r in routed)
    assert routed and n_res == (len(routed) // 2 if FR.pre_norm(cfg.get("layer_order", "gcr")) else 0)
    sd, x, target = _prep(cfg, shape, seed=21)
    _, p64, l64, loss64, g64 = _cpu_run(cfg, sd, x, target, torch.float64, True)
    _, _, _, _, g32 = _cpu_run(cfg, sd, x, target, torch.float32, True)
    logits, probs, loss, grads, calls = _step(keyed, sd, x, target)
    # ---- the bars of native_2d_residual
    assert logits.shape == tuple(x.shape[:1]) + (cfg["out_channels"],) + tuple(x.shape[2:])
    e_l, e_p = orc.rel_err(logits.double(), l64), orc.rel_err(probs.double(), p64)
    keys = list(g64)
    e_ours, e_32 = _global_rel_l2(grads, g64, keys), _global_rel_l2(g32, g64, keys)
    # ---- the same weights and input under plain native_2d_residual
    l_f32, _, _, _, calls_f32 = _step(dict(cfg, native_2d_residual=True), sd, x, target)
    e_vs = orc.rel_err(logits, l_f32)
    rec = dict(test="resunet2d_fp32_split", case=case, shape=list(shape), routed=len(routed), with_residual=n_res, logits_rel=e_l, probs_rel=e_p,
               loss_abs=abs(loss - loss64), grad_l2=e_ours, grad_l2_fp32_cpu=e_32, logits_vs_native_2d_residual=e_vs)
    diag(**rec)
    print(rec)
    assert e_l < REL and e_p < REL, rec
    assert abs(loss - loss64) < REL * max(1.0, abs(loss64)), rec
    assert e_ours <= max(1e-3, 2.0 * e_32), rec
    assert e_vs < 2e-5, rec
    # ---- routing against the restated rule
    assert calls.get("u3d_conv2d_f32s_res", 0) == n_res, calls
    assert calls.get("u3d_conv2d_f32s", 0) == len(routed) - n_res, calls
    assert calls.get("u3d_conv2d_f32s_dgrad", 0) == len(routed) and calls.get("u3d_conv2d_wgrad_f32s", 0) == len(routed), calls
    assert all(calls.get(n, 0) > 0 for n in CONVTR), calls  # the transposed convolutions stay where they were
    if len(routed) == len(FR.conv3x3(model)):
        assert not any(n in calls for n in FP32_CONV), calls
    else:  # (the 16-wide blocks: conv2 plain, conv3 with the fp32 residual epilogue, the fp32 weight gradient)
        n_fp32 = len(FR.conv3x3(model)) - len(routed)
        assert calls.get("u3d_conv2d_res_reps", 0) == n_fp32 // 2 and calls.get("u3d_conv2d_wgrad", 0) == n_fp32, calls
        assert calls.get("u3d_conv2d_ex_reps", 0) >= n_fp32 // 2, calls  # (conv2 forward + the fp32 data gradients)
    assert not any("f32s" in n for n in calls_f32), calls_f32


def test_a_model_without_routed_layers_is_unchanged_by_the_key():
    """f_maps = [8, 16]: no block is % 32 wide, every convolution stays on the fp32 2-D kernels — logits and every gradient bitwise
    equal to the native_2d_residual run, no six-product entry point called"""
    cfg = dict(_R, f_maps=[8, 16], layer_order="gcr", num_groups=4)
    shape = (2, 1, 35, 45)
    assert FR.routed(get_model(dict(cfg, **{KEY: True}))) == []
    sd, x, target = _prep(cfg, shape, seed=22)
    runs = []
    for extra in (dict(native_2d_residual=True), {KEY: True}):
        logits, _, _, grads, calls = _step(dict(cfg, **extra), sd, x, target)
        assert "u3d_conv2d_res_reps" in calls and "u3d_conv2d_ex_reps" in calls and not any("f32s" in n for n in calls), calls
        runs.append((logits, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_eval_forward_equals_the_training_forward():
    """a GroupNorm net computes the same logits in training mode and under eval() + torch.no_grad() (no tape, forward images only)"""
    cfg, shape = CASES["gcr_3levels"]
    sd, x, _ = _prep(cfg, shape, seed=23)
    model = get_model(dict(cfg, **{KEY: True}))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, l_train = model(x.to(DEV), return_logits=True)
        model.eval()
        with torch.no_grad():
            _, l_eval = model(x.to(DEV), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(l_train.detach().cpu(), l_eval.cpu())
