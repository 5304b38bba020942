"""-m gpu: UNet2D under `native_2d_fp32_split: true` on the MI355X.  The 3x3 layers `_split2d` routes run forward, data gradient and weight
gradient on the six-product kernels of csrc/u3d_conv2d_f32s.h; the claim is fp32 grade, so the comparison and the bars are those of
`native_2d`, unchanged (tests/test_gpu_model2d.py::run_and_check: logits / probs within 1e-4 of the range, the loss within 1e-4, the global
gradient rel-L2 within max(1e-3, 2x the fp32 module tree's own distance from float64).  On top of them: an EventProfiler sees each of
the three new entry points once per routed layer (the restated rule of tests/f32s_emul_2d.py), and the logits agree with a `native_2d`
model on the same weights within 2e-5 of their range (the 3-D mode's bar in tests/test_gpu_f32s.py).

None of the recorded reference cases (tests/reference_records_2d.py, f_maps [8, 16, 32]) has a layer inside the rule — their widest
single-source layer is 16 -> 32: the recorded `gcr` case runs with the key to show that it changes nothing there; the routed layers are
covered by the seeded cases against the float64 module tree."""
import pytest
import torch

import f32s_emul_2d as FE2
import unet3d_oracle as orc
from conftest import diag
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from reference_records_2d import Run2D
from test_gpu_model2d import run_and_check

pytestmark = pytest.mark.gpu
KEY = "native_2d_fp32_split"
NEW = ("u3d_conv2d_f32s", "u3d_conv2d_f32s_dgrad", "u3d_conv2d_wgrad_f32s")

CASES = {
    "gcr_plus1": (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="gcr", num_groups=8), (2, 1, 37, 45), {}),
    "bcr_3levels": (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="bcr"), (1, 1, 40, 56), {}),
    "cgr_post_norm": (dict(name="UNet2D", in_channels=1, out_channels=2, f_maps=[32, 64], layer_order="cgr", num_groups=8,
                           final_sigmoid=False), (1, 1, 24, 40), {}),
    "gcr_stem": (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="gcr", num_groups=8), (2, 1, 37, 45),
                 dict(native_2d_stem=True)),
}


def _profiled(fn):
    prof = nat.EventProfiler()
    nat.profiler = prof
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    return out, {k: v["calls"] for k, v in prof.summary().items()}


def _logits(cfg, sd, x):
    m = get_model(dict(cfg))
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    with torch.no_grad():
        _, logits = m(x.to(DEV), return_logits=True)
    torch.cuda.synchronize()
    return logits.cpu()


@pytest.mark.parametrize("case", list(CASES))
def test_unet2d_fp32_split_holds_the_native_2d_bars_and_routes_every_layer_of_the_rule(case):
    cfg, shape, extra = CASES[case]
    keyed = dict(cfg, **{KEY: True}, **extra)
    model = get_model(dict(keyed))
    assert model.native_supported and model.compute_split and model._get_engine().split2d
    routed = FE2.routed(model)
    assert routed
    # one training step against the float64 module tree, profiled (the forward of a training step, its data and weight gradients)
    _, calls = _profiled(lambda: run_and_check(keyed, shape, seed=11))
    for name in NEW:
        assert calls.get(name, 0) == len(routed), (name, calls.get(name, 0), len(routed))
    if extra.get("native_2d_stem"):
        assert calls.get("u3d_conv2d_small_cin_fwd_reps", 0) == 1  # the first layer on the small-Cin kernels
        assert ("encoders.0.basic_module.SingleConv2.conv.weight", 16, 0, 32) not in routed  # 16 -> 32 stays on the fp32 conv2d kernels
    # the same weights and input under plain native_2d: fp32-grade agreement of the logits
    torch.manual_seed(12)
    sd = {k: v.detach().clone() for k, v in get_model(dict(cfg)).state_dict().items()}
    x = torch.randn(shape)
    l_key, l_f32 = _logits(keyed, sd, x), _logits(dict(cfg, native_2d=True, **extra), sd, x)
    err = orc.rel_err(l_key, l_f32)
    diag(test="unet2d_fp32_split_vs_native_2d", case=case, shape=list(shape), routed=len(routed), logits_rel=err)
    assert err < 2e-5, err


def test_a_recorded_reference_case_is_unchanged_by_the_key():
    """`gcr` of tests/reference_records_2d.py (f_maps [8, 16, 32]): no layer lies inside the rule, so every launch is that of native_2d"""
    run = Run2D("gcr")
    keyed = dict(run.cfg, **{KEY: True})
    assert FE2.routed(get_model(dict(keyed))) == []
    _, calls = _profiled(lambda: run_and_check(keyed, run.shape, sd=run.sd, x=run.x, target=run.target))
    assert not any(n in calls for n in NEW + ("u3d_pack_weights2d_f32s",))
    l_key, l_f32 = _logits(keyed, run.sd, run.x), _logits(dict(run.cfg, native_2d=True), run.sd, run.x)
    assert torch.equal(l_key, l_f32)
    assert orc.rel_err(l_key, run.logits) < 1e-4
