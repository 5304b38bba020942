"""UNet2D under `native_2d_subpixel_plus: true` on the MI355X: the decoder levels that upsample n -> 2n + 1 along H and / or W on the
windowed sub-pixel kernels of csrc/u3d_subpix2d.hip + the box launches of csrc/u3d_conv2d.hip on the 2-pixel slab — against the float64
module tree on the CPU with the bars of tests/test_gpu_model2d.py (through tests/test_gpu_model2d_subpixel.py::run_and_check), which
entry points ran (nat.EventProfiler), and bit-identity with `native_2d_subpixel` where every level is an exact 2x."""
import pytest
import torch

import unet3d_oracle as orc
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from test_gpu_model2d import REL
from test_gpu_model2d_subpixel import NEW, SMALL, _gpu_step, _seeded, run_and_check

pytestmark = pytest.mark.gpu
WIN = ("u3d_subpixel2d_conv_fwd_win", "u3d_subpixel2d_conv_dgrad_win", "u3d_subpixel2d_conv_wgrad_win")


def _counts(calls, names):
    return [calls.get(k, 0) for k in names]


def test_both_levels_odd():
    # 8 x 7 -> 17 x 14 shifts H only, 17 x 14 -> 35 x 29 both axes
    calls = run_and_check(SMALL, (2, 1, 35, 29), seed=1, native_2d_subpixel_plus=True)
    assert _counts(calls, WIN) == [2, 2, 2] and _counts(calls, NEW) == [0, 0, 0], calls
    assert "u3d_gn_bwd_apply_up" not in calls, calls
    assert calls.get("u3d_gn_bwd_apply_children2d") == 2 and calls.get("u3d_chan_stats_children2d") == 2, calls
    # slab launches: (1 + 2) boxes forward, the same for the data gradient (+ one child-sum each) and for the weight gradient
    assert calls.get("u3d_conv2d_box") == 6 and calls.get("u3d_nearest_childsum_add2d") == 3 and calls.get("u3d_conv2d_wgrad_box") == 3, calls


def test_one_odd_and_one_exact_level():
    calls = run_and_check(SMALL, (2, 1, 34, 40), seed=2, native_2d_subpixel_plus=True)  # 8 -> 17 is n -> 2n + 1, 17 -> 34 exact
    assert _counts(calls, WIN) == [1, 1, 1] and _counts(calls, NEW) == [1, 1, 1], calls
    assert "u3d_gn_bwd_apply_up" not in calls, calls


def test_the_confocal_pattern():
    calls = run_and_check(SMALL, (2, 1, 67, 64), seed=3, native_2d_subpixel_plus=True)  # H 16 -> 33 -> 67 odd at both levels, W exact
    assert _counts(calls, WIN) == [2, 2, 2] and _counts(calls, NEW) == [0, 0, 0], calls


@pytest.mark.parametrize("order", ["bcr", "cr", "cgl", "cgr"])
def test_layer_orders(order):
    calls = run_and_check(dict(SMALL, out_channels=2, layer_order=order, final_sigmoid=False), (2, 1, 35, 29), seed=4,
                          native_2d_subpixel_plus=True)
    assert _counts(calls, WIN) == [2, 2, 2], calls


def test_next_to_the_stem():
    calls = run_and_check(SMALL, (2, 1, 35, 29), seed=5, native_2d_subpixel_plus=True, native_2d_stem=True)
    assert _counts(calls, WIN) == [2, 2, 2] and calls.get("u3d_conv2d_small_cin_fwd_reps") == 2, calls


def test_eval_mode_forward():
    model, sd, x, _ = _seeded(SMALL, (2, 1, 35, 29), 7, native_2d_subpixel_plus=True)
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
    assert calls.get("u3d_subpixel2d_conv_fwd_win") == 2 and calls.get("u3d_conv2d_box") == 3, calls
    assert not any(k in calls for k in WIN[1:] + ("u3d_conv2d_wgrad_box", "u3d_nearest_childsum_add2d")), calls
    with torch.no_grad():
        p64 = ref(x.double())
    assert orc.rel_err(probs.cpu().double(), p64) < REL


def test_all_exact_levels_are_bit_identical_to_native_2d_subpixel():
    out = []
    for keys in (dict(native_2d_subpixel=True), dict(native_2d_subpixel_plus=True)):
        model, _, x, target = _seeded(SMALL, (2, 1, 36, 40), 8, **keys)
        out.append(_gpu_step(model, x, target))
    (l0, _, _, g0, c0), (l1, _, _, g1, c1) = out
    assert not any(k in c1 for k in WIN), c1
    assert c0 == c1
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
