"""UNet2D under `native_2d_subpixel: true` on the MI355X: the upsampled half of every exact-2x decoder level on the sub-pixel kernels of
csrc/u3d_subpix2d.hip — against the float64 module tree on the CPU with the bars of tests/test_gpu_model2d.py (logits / probs within
1e-4 of the range, the loss within 1e-4, the global gradient rel-L2 within max(1e-3, 2x the fp32 module tree's own distance from
float64)), and which entry points ran (nat.EventProfiler)."""
import warnings

import pytest
import torch

import unet3d_oracle as orc
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from test_gpu_model2d import REL, _cpu_run, _global_rel_l2, _loss

pytestmark = pytest.mark.gpu
NEW = ("u3d_subpixel2d_conv_fwd", "u3d_subpixel2d_conv_dgrad_reps", "u3d_subpixel2d_conv_wgrad")
SMALL = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32], num_groups=4)


def _seeded(cfg, shape, seed, **keys):
    torch.manual_seed(seed)
    model = get_model(dict(cfg, **keys))
    assert model.native_supported, model._native_blockers
    with torch.no_grad():  # a trained-like net: the default norm init (gamma 1, beta 0) hides half of the gradient paths
        for k, p in model.named_parameters():
            if "groupnorm" in k or "batchnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.randn(shape)
    target = (torch.rand((shape[0], cfg.get("out_channels", 1)) + tuple(shape[2:])) > 0.5).float()
    return model, sd, x, target


def _gpu_step(model, x, target):
    """one training step; returns (logits, probs, loss, grads, {entry point: calls})"""
    model = model.to(DEV).train()
    prof = nat.EventProfiler()
    nat.profiler = prof
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the native path raises no "not covered" warning
            probs, logits = model(x.to(DEV), return_logits=True)
            loss = _loss(model, probs, logits, target.to(DEV))
            model.zero_grad()
            loss.backward()
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return logits.detach().cpu(), probs.detach().cpu(), loss.item(), grads, {k: v["calls"] for k, v in prof.summary().items()}


def run_and_check(cfg, shape, seed=0, **keys):
    """tests/test_gpu_model2d.py::run_and_check with the model built under native_2d_subpixel (+ `keys`); returns the call counts"""
    model, sd, x, target = _seeded(cfg, shape, seed, native_2d_subpixel=True, **keys)
    _, p64, l64, loss64, g64 = _cpu_run(cfg, sd, x, target, torch.float64, True)
    _, _, _, _, g32 = _cpu_run(cfg, sd, x, target, torch.float32, True)
    logits, probs, loss, ours, calls = _gpu_step(model, x, target)
    assert logits.shape == tuple(x.shape[:1]) + (cfg.get("out_channels", 1),) + tuple(x.shape[2:])
    e_l, e_p = orc.rel_err(logits.double(), l64), orc.rel_err(probs.double(), p64)
    keys_ = list(g64)
    e_ours, e_32 = _global_rel_l2(ours, g64, keys_), _global_rel_l2(g32, g64, keys_)
    print(f"{cfg.get('layer_order', 'gcr')} {tuple(shape)}: logits {e_l:.1e} probs {e_p:.1e} loss {loss:.6f} / {loss64:.6f} grad rel-L2 "
          f"{e_ours:.1e} (fp32 CPU {e_32:.1e}), sub-pixel calls {[calls.get(k, 0) for k in NEW]}")
    assert e_l < REL and e_p < REL, (e_l, e_p)
    assert abs(loss - loss64) < REL * max(1.0, abs(loss64)), (loss, loss64)
    assert e_ours <= max(1e-3, 2.0 * e_32), (e_ours, e_32)
    return calls


def test_both_decoder_levels_eligible():
    calls = run_and_check(SMALL, (2, 1, 36, 40), seed=1)
    assert all(calls.get(k) == 2 for k in NEW), calls  # once per decoder level
    assert "u3d_gn_bwd_apply_up" not in calls, calls


def test_exact_and_odd_levels_mixed_in_one_net():
    calls = run_and_check(SMALL, (2, 1, 34, 40), seed=2)  # 8 -> 17 is n -> 2n + 1 (virtual concat), 17 -> 34 exact (sub-pixel)
    assert all(calls.get(k) == 1 for k in NEW), calls
    assert calls.get("u3d_gn_bwd_apply_up") == 1, calls


@pytest.mark.parametrize("order", ["gcr", "bcr"])
def test_dsb2018_configuration(order):
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order=order, num_groups=8)
    calls = run_and_check(cfg, (2, 1, 64, 64), seed=3)
    assert all(calls.get(k) == 2 for k in NEW), calls


@pytest.mark.parametrize("order", ["cr", "gcl", "cgr"])
def test_layer_orders(order):
    calls = run_and_check(dict(SMALL, out_channels=2, layer_order=order, final_sigmoid=False), (2, 1, 36, 40), seed=4)
    assert all(calls.get(k) == 2 for k in NEW), calls


def test_next_to_the_stem():
    calls = run_and_check(SMALL, (2, 1, 36, 40), seed=5, native_2d_stem=True)
    assert all(calls.get(k) == 2 for k in NEW) and calls.get("u3d_conv2d_small_cin_fwd_reps") == 2, calls  # (1 -> 4 and 4 -> 8)


def test_two_inputs_three_classes():
    calls = run_and_check(dict(SMALL, in_channels=2, out_channels=3, final_sigmoid=False), (2, 2, 36, 40), seed=6)
    assert all(calls.get(k) == 2 for k in NEW), calls


def test_eval_mode_forward():
    model, sd, x, _ = _seeded(SMALL, (2, 1, 36, 40), 7, native_2d_subpixel=True)
    ref = get_model(dict(SMALL)).double()
    ref.load_state_dict(sd)
    ref.eval()
    model = model.to(DEV).eval()
    prof = nat.EventProfiler()
    nat.profiler = prof
    try:
        with torch.no_grad():
            probs = model(x.to(DEV))
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    calls = {k: v["calls"] for k, v in prof.summary().items()}
    assert calls.get("u3d_subpixel2d_conv_fwd") == 2 and "u3d_subpixel2d_conv_wgrad" not in calls, calls
    with torch.no_grad():
        p64 = ref(x.double())
    assert orc.rel_err(probs.cpu().double(), p64) < REL


def test_no_eligible_level_is_bit_identical_to_native_2d():
    shape = (2, 1, 35, 29)  # 8 -> 17 -> 35 and 7 -> 14 -> 29: n -> 2n + 1 on both levels
    out = []
    for keys in (dict(native_2d=True), dict(native_2d_subpixel=True)):
        model, _, x, target = _seeded(SMALL, shape, 8, **keys)
        out.append(_gpu_step(model, x, target))
    (l0, _, _, g0, c0), (l1, _, _, g1, c1) = out
    assert not any(k in c1 for k in NEW), c1
    assert c0 == c1
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
