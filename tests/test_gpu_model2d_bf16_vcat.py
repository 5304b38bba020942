"""-m gpu: UNet2D under `native_2d_bf16_vcat: true` on the MI355X — the decoders' first convolutions read cat(skip, nearest(low)) inside
the bf16 kernels (the `_src` entry points of csrc/u3d_conv2d_bf16.hip) instead of a concat written out by u3d_nearest_cat_fwd.  The
arithmetic is the parent mode's (`native_2d_bf16`): the same bf16 values are staged in the same order, the statistics are f64 sums of the
same fp32 partials.  So the new mode is held to the parent mode itself (bit-equal whenever the parent is bit-equal to itself run to run,
else within 10x the parent's own run-to-run distance — room for another atomic order, nothing more), to the two model gates of
test_gpu_model2d_bf16.py against the unchanged emulation tests/bf16_emul_2d.py, to its routing (a recording wrapper around nat.call) and
to the memory it promises: the concats stop existing."""
import os
import warnings
from collections import Counter
from contextlib import contextmanager

import pytest
import torch

import bf16_emul_2d as E
import unet3d_oracle as orc
from conftest import diag, loss_by_name
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from test_gpu_model2d_bf16 import BF16_GRAD_TOL, BF16_LOGITS_TOL, _prep

pytestmark = pytest.mark.gpu

CASES = [
    # 35 -> 17 -> 8, 45 -> 22 -> 11: both decoder levels upsample n -> 2n + 1; halves 64 | 128 and 32 | 64
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="gcr", num_groups=8), (2, 1, 35, 45)),
    # BatchNorm in front of the convolution, exact 2x, one decoder
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="bcr"), (2, 1, 32, 32)),
]
SRC_CALLS = ("u3d_conv2d_bf16_src", "u3d_conv2d_bf16_dgrad_src", "u3d_conv2d_wgrad_bf16_src")
PARENT = dict(native_2d_bf16=True)
NEW = dict(native_2d_bf16_vcat=True)
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r17_unet2d_vcat_model_distances.txt")


@contextmanager
def recorded_calls():
    """counts every entry point issued through nat.call (the executors look `call` up on the module at call time)"""
    counts = Counter()
    real = nat.call

    def call(name, *args, **kw):
        counts[name] += 1
        return real(name, *args, **kw)

    nat.call = call
    try:
        yield counts
    finally:
        nat.call = real


def _step(cfg, sd, x, target, loss_name, **extra):
    """one training step of a fresh model on the given state; (logits, grads, call counts)"""
    model = get_model(dict(cfg, **extra))
    model.load_state_dict(sd)
    assert model.native_supported and model.compute_bf16, model._native_blockers
    model = model.to(DEV).train()
    with recorded_calls() as counts, warnings.catch_warnings():
        warnings.simplefilter("error")  # the native path raises no "not covered" warning
        probs, logits = model(x.to(DEV), return_logits=True)
        loss = loss_by_name(loss_name, probs, logits, target.to(DEV))
        model.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return logits.detach().cpu(), grads, counts


def _flat(grads, keys):
    return torch.cat([grads[k].flatten().double() for k in keys])


def _dist(a, b, keys):
    """(logits rel-L2, gradient rel-L2) of run a from run b"""
    la, lb = a[0].double(), b[0].double()
    ga, gb = _flat(a[1], keys), _flat(b[1], keys)
    return ((la - lb).norm() / lb.norm()).item(), ((ga - gb).norm() / gb.norm()).item()


def _bit_equal(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("cfg,shape", CASES)
def test_unet2d_bf16_vcat_against_the_parent_mode_and_the_emulation(cfg, shape):
    loss_name = "bce_dice"
    _, sd, x, target = _prep(cfg, shape, **PARENT)
    p1 = _step(cfg, sd, x, target, loss_name, **PARENT)
    p2 = _step(cfg, sd, x, target, loss_name, **PARENT)
    new = _step(cfg, sd, x, target, loss_name, **NEW)
    keys = list(new[1])
    n_dec = len(cfg["f_maps"]) - 1

    # ---- routing: the parent writes every concat out; the new mode none, one call of each `_src` entry point per decoder
    for run in (p1, p2):
        assert run[2]["u3d_nearest_cat_fwd"] == n_dec and not any(run[2][n] for n in SRC_CALLS), run[2]
    assert new[2]["u3d_nearest_cat_fwd"] == 0, new[2]
    assert all(new[2][n] == n_dec for n in SRC_CALLS), new[2]
    # (every other entry point is issued as often as before; the single-source bf16 calls lose the decoders' first convolutions)
    assert new[2]["u3d_conv2d_bf16"] == p1[2]["u3d_conv2d_bf16"] - 2 * n_dec, (new[2], p1[2])
    assert new[2]["u3d_conv2d_wgrad_bf16"] == p1[2]["u3d_conv2d_wgrad_bf16"] - n_dec, (new[2], p1[2])

    # ---- against the parent mode
    parent_same = _bit_equal(p1, p2)
    d_parent, d_new = _dist(p2, p1, keys), _dist(new, p1, keys)
    rec = dict(test="bf16_vcat_model_2d", cfg=str(cfg), shape=str(shape), parent_bit_equal=parent_same, new_bit_equal=_bit_equal(new, p1),
               parent_logits=d_parent[0], parent_grad_l2=d_parent[1], new_logits=d_new[0], new_grad_l2=d_new[1])
    diag(**rec)
    print(rec)
    if parent_same:
        assert _bit_equal(new, p1), rec
    else:
        with open(PROFILE, "a") as f:  # the measured distances, for the record
            f.write(repr(rec) + "\n")
        assert d_new[0] <= 10.0 * d_parent[0] and d_new[1] <= 10.0 * d_parent[1], rec

    # ---- the two model gates of test_gpu_model2d_bf16.py (the emulation is unchanged: the arithmetic is the same)
    l32, _, g32 = E.run(cfg, sd, x, target, loss_name, emulate=False)
    l16, _, g16 = E.run(cfg, sd, x, target, loss_name, emulate=True)
    gk = list(g32)
    ours, r16, r32 = _flat(new[1], gk), _flat(g16, gk), _flat(g32, gk)
    logits = new[0].double()
    e_l16, e_l32, e_l_or = orc.rel_err(logits, l16), orc.rel_err(logits, l32), orc.rel_err(l16, l32)
    e_g16 = ((ours - r16).norm() / r16.norm()).item()
    e_g32 = ((ours - r32).norm() / r32.norm()).item()
    e_or = ((r16 - r32).norm() / r32.norm()).item()
    gates = dict(test="bf16_vcat_model_2d_gates", cfg=str(cfg), logits_vs_bf16_emulation=e_l16, logits_vs_plain=e_l32,
                 grad_l2_vs_bf16_emulation=e_g16, grad_l2_vs_plain=e_g32, emulation_vs_plain_grad_l2=e_or, emulation_vs_plain_logits=e_l_or)
    diag(**gates)
    print(gates)
    assert e_l16 < 0.75 * e_l_or and e_g16 < 0.75 * e_or, gates
    assert e_l32 < BF16_LOGITS_TOL and e_g32 < BF16_GRAD_TOL, gates


def test_inference_takes_the_same_route():
    """eval() + no_grad (no tape): no concat is written, the forward `_src` entry point runs once per decoder, logits as in training"""
    cfg, shape = CASES[0]
    _, sd, x, target = _prep(cfg, shape, **PARENT)
    model = get_model(dict(cfg, **NEW))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    _, l_train = model(x.to(DEV), return_logits=True)
    model.eval()
    with recorded_calls() as counts, torch.no_grad():
        _, l_eval = model(x.to(DEV), return_logits=True)
    torch.cuda.synchronize()
    assert counts["u3d_nearest_cat_fwd"] == 0 and counts["u3d_conv2d_bf16_src"] == 2, counts
    assert torch.equal(l_train.detach().cpu(), l_eval.cpu())


def test_16_channel_halves_keep_the_written_out_concat():
    """f_maps [16, 32] under the key + `native_2d_stem`: the decoder's halves (16 | 32) are outside the % 32 envelope of the `_src` entry
    points — the concat is written out and the `_c16` single-source layer runs, exactly as without the key"""
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[16, 32], layer_order="gcr", num_groups=8)
    shape = (2, 1, 35, 45)
    _, sd, x, target = _prep(cfg, shape, native_2d_bf16=True, native_2d_stem=True)
    old = _step(cfg, sd, x, target, "bce_dice", native_2d_bf16=True, native_2d_stem=True)
    new = _step(cfg, sd, x, target, "bce_dice", native_2d_bf16_vcat=True, native_2d_stem=True)
    for run in (old, new):
        assert run[2]["u3d_nearest_cat_fwd"] == 1 and not any(run[2][n] for n in SRC_CALLS), run[2]
    assert old[2] == new[2]


def _peak_of_a_step(cfg, sd, x, target, **extra):
    model = get_model(dict(cfg, **extra))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    xd, td = x.to(DEV), target.to(DEV)
    peaks = []
    for _ in range(2):  # (the first step builds the weight images and the cached tables)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        probs, logits = model(xd, return_logits=True)
        loss = loss_by_name("bce_dice", probs, logits, td)
        model.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV) - base)
        del probs, logits, loss
    return peaks[-1]


def test_peak_memory_drops_by_the_largest_concat():
    """f_maps [32, 64, 128] at 4 x 1 x 128 x 128: the 96-channel concat of the top decoder (4 * 128 * 128 * 96 floats) is held from the
    forward to the decoder's backward in the parent mode and does not exist in the new one"""
    cfg = CASES[0][0]
    shape = (4, 1, 128, 128)
    _, sd, x, target = _prep(cfg, shape, **PARENT)
    parent = _peak_of_a_step(cfg, sd, x, target, **PARENT)
    new = _peak_of_a_step(cfg, sd, x, target, **NEW)
    largest = 4 * 128 * 128 * 96 * 4
    rec = dict(test="bf16_vcat_peak_memory", parent_bytes=parent, new_bytes=new, saved=parent - new, largest_concat=largest)
    diag(**rec)
    print(rec)
    assert parent - new >= largest, rec
