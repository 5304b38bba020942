"""CPU self-tests of the teacher-forced bf16 gate (tests/teacher.py).  The fake native run is the same emulation in float32, its
per-layer tensors captured at the forcing sites: the gate passes on it, planted errors fail it naming the layer, and the same errors
pass the global bars of tests/test_gpu_bf16.py / test_gpu_b16.py (the gap the gate closes)."""
import pytest
import torch

import decided as dcd
import teacher as T
import unet3d_oracle as orc
from conftest import diag, loss_by_name
from pytorch3dunet_amd.unet3d.model import get_model

UNET = dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=32, num_levels=3, num_groups=8)
RES = dict(name="ResidualUNet3D", in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8)
RESSE = dict(name="ResidualUNetSE3D", in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8)
DEEP = dict(name="ResidualUNet3D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], num_groups=8)
SHAPE = (1, 1, 8, 16, 16)


def _loss(p, lg, t):
    return loss_by_name("bce_dice", p, lg, t)


def _seeded(cfg, shape=SHAPE, seed=5):
    torch.manual_seed(seed)
    model = get_model(dict(cfg))
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "groupnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.randn(shape)
    t = (torch.rand((shape[0], cfg["out_channels"]) + tuple(shape[2:])) > 0.5).float()
    return sd, x, t


def _gate(cfg, sd, x, t, storage, recs, dec, grads, logits):
    return T.gate(cfg, sd, x, t, _loss, recs, dec, grads, storage, native_logits=logits)


# (UNet3D only without storage: bf16 activation storage is a residual-net mode, and the oracle restates it there only)
CASES = [(UNET, False), (RES, False), (RES, True), (RESSE, False), (RESSE, True)]


@pytest.mark.parametrize("cfg,storage", CASES, ids=["unet3d", "res", "res-storage", "resse", "resse-storage"])
def test_gate_passes_on_the_fake_native_run(cfg, storage):
    sd, x, t = _seeded(cfg)
    recs, dec, grads, logits = T.capture(cfg, sd, x, t, _loss, storage)
    rep, fails = _gate(cfg, sd, x, t, storage, recs, dec, grads, logits)
    assert not fails, fails
    convs = [k for k in sd if k.endswith(".conv.weight") and ("SingleConv" in k or ".conv2." in k or ".conv3." in k)]
    for k in convs:  # every conv was forced and checked on all four quantities
        p = k[: -len(".conv.weight")]
        assert {f"{p}:{q}" for q in ("affine", "y", "dz", "dg")} <= set(rep.figures), p
    if storage:
        worst = rep.worst("frac")
        assert worst[1] < T.B16_LINK_FRAC, worst
    diag(test="teacher_fake_native", cfg=str(cfg), storage=storage, worst_rel=rep.worst("slice"), worst_frac=rep.worst("frac"),
         worst_param=rep.worst("grad_rel"))


def test_fake_emulation_follows_the_oracle():
    """unforced, the teacher's graph is the oracle's bf16 emulation: same logits and gradients up to bf16 operand flips"""
    for cfg, storage in ((UNET, False), (RESSE, True)):
        sd, x, t = _seeded(cfg)
        _, _, grads, logits = T.capture(cfg, sd, x, t, _loss, storage, dtype=torch.float64)
        with T.bf16_modes(storage):
            sd64 = {k: v.double() for k, v in sd.items()}
            _, lo, _, go = orc.forward_backward(sd64, x.double(), t.double(), 8, True, True, "bce_dice")
        assert orc.rel_err(logits.double(), lo) < 2e-2
        a = torch.cat([grads[k].flatten().double() for k in go])
        b = torch.cat([go[k].flatten() for k in go])
        assert ((a - b).norm() / b.norm()).item() < 2e-2


def test_forcing_is_what_removes_the_chaos():
    """the same float32 run WITHOUT forcing, compared layer by layer with an unforced float64 run, breaks the per-layer bars: the
    bars are not loose, the forcing is what makes them hold"""
    sd, x, t = _seeded(DEEP, (1, 1, 16, 16, 16))
    out = {}
    for storage in (False, True):
        r32, _, _, _ = T.capture(DEEP, sd, x, t, _loss, storage)
        r64, _, _, _ = T.capture(DEEP, sd, x, t, _loss, storage, dtype=torch.float64)
        figs = T.compare_records(r32, r64, storage)
        bad = [k for k, _, b in figs if b]
        key = "ulp" if storage else "slice"
        worst = max((f[key] for _, f, _ in figs if key in f), default=0.0)
        out[storage] = (len(bad), worst)
        diag(test="teacher_unforced_chaos", storage=storage, failing_sites=len(bad), sites=len(figs), worst=worst)
    # without storage the fp32-vs-fp64 operand flips reach far beyond F32_REL; with storage the stored tensors differ in many ulps
    assert out[False][0] > 0 and out[False][1] > 10 * T.F32_REL, out
    assert out[True][0] > 0, out


def _planted(cfg, storage, plant=None, post=None):
    sd, x, t = _seeded(cfg)
    recs, dec, grads, logits = T.capture(cfg, sd, x, t, _loss, storage, plant=plant)
    if post is not None:
        post(grads)
    _, fails = _gate(cfg, sd, x, t, storage, recs, dec, grads, logits)
    return fails, (sd, x, t, grads, logits)


def _scale_channel(name, ch, f):
    def post(g):
        c = ch if ch is not None else int(g[name].flatten(1).abs().amax(1).argmax())  # (None: the channel holding the largest entry)
        g[name][c] *= f
    return post


PLANTS = {
    # one output channel of a mid-level conv's weight gradient x (1 + 1e-2)
    "wgrad_channel": (DEEP, False, None, _scale_channel("encoders.1.basic_module.conv3.conv.weight", None, 1.01),
                      "encoders.1.basic_module.conv3.conv.weight"),
    # the last D-plane's contribution dropped from one layer's data gradient
    "dgrad_last_plane": (DEEP, False, {("encoders.1.basic_module.conv2", "drop_last_dg"): True}, None, "encoders.1.basic_module.conv2: dg"),
    # truncation in place of round-to-nearest-even on one layer's dz operand
    "trunc_dz": (DEEP, False, {("decoders.0.basic_module.conv3", "trunc_dz"): True}, None, "decoders.0.basic_module.conv3: dg"),
    # one decoder GroupNorm beta gradient x 1.01
    "dec_gn_beta": (DEEP, False, None, _scale_channel("decoders.1.basic_module.conv2.groupnorm.bias", slice(None), 1.01),
                    "decoders.1.basic_module.conv2.groupnorm.bias"),
    # a transposed-conv weight gradient with one tap wrong
    "convtr_tap": (DEEP, False, None, lambda g: g["decoders.0.upsampling.upsample.conv_transposed.weight"][:, :, 2, 1, 0].mul_(1.01),
                   "decoders.0.upsampling.upsample.conv_transposed.weight"),
    # under storage: one stored gradient (a decoder block's residual, the joined tensor) rounded per consumer and then again
    "double_rounding": (DEEP, True, {("decoders.0.basic_module", "r_split_round"): True}, None, "encoders.1.basic_module.conv3: dz"),
}


@pytest.mark.parametrize("name", list(PLANTS))
def test_planted_error_fails_the_gate_naming_the_layer(name):
    cfg, storage, plant, post, where = PLANTS[name]
    fails, _ = _planted(cfg, storage, plant, post)
    diag(test="teacher_planted", plant=name, failures=fails[:6])
    assert fails, name
    assert any(f.startswith(where) or f.startswith(f"param {where}") for f in fails), (where, fails)


def global_bars_pass(cfg, sd, x, t, grads, logits, storage):
    """the model-level bars of test_gpu_bf16.py (no storage) / test_gpu_b16.py (storage) on a native step's (logits, grads)"""
    G, fs = cfg["num_groups"], cfg.get("final_sigmoid", True)
    _, l32, _, g32 = orc.forward_backward(sd, x, t, G, fs, True, "bce_dice")
    with T.bf16_modes(storage):
        _, lem, _, gem = orc.forward_backward(sd, x, t, G, fs, True, "bce_dice")
    keys = list(g32)
    cat = lambda d: torch.cat([d[k].flatten().double() for k in keys])  # noqa: E731
    ours, em, ref = cat(grads), cat(gem), cat(g32)
    e_l16, e_l32, e_l_or = orc.rel_err(logits, lem), orc.rel_err(logits, l32), orc.rel_err(lem, l32)
    e_g16 = ((ours - em).norm() / em.norm()).item()
    e_g32 = ((ours - ref).norm() / ref.norm()).item()
    e_or = ((em - ref).norm() / ref.norm()).item()
    if not storage:
        return e_l16 < 0.75 * e_l_or and e_g16 < 0.75 * e_or and e_l32 < 3e-2 and e_g32 < 0.15
    return (e_l16 < 0.75 * e_l_or and e_g16 < e_or and e_l32 < 1.25 * e_l_or + 1e-3 and e_g32 < 1.15 * e_or + 1e-3)


@pytest.mark.parametrize("name", ["wgrad_channel", "dec_gn_beta", "convtr_tap"])
def test_planted_errors_pass_the_global_bars(name):
    """the gap: these errors pass the model-level bars the bf16 modes had before the teacher-forced gate"""
    cfg, storage, plant, post, _ = PLANTS[name]
    fails, (sd, x, t, grads, logits) = _planted(cfg, storage, plant, post)
    assert fails
    assert global_bars_pass(cfg, sd, x, t, grads, logits, storage), name


def test_records_must_be_used_exactly_once_and_be_complete():
    sd, x, t = _seeded(RES)
    recs, dec, grads, logits = T.capture(RES, sd, x, t, _loss, False)
    extra = dict(recs)
    extra["decoders.7.basic_module.conv2"] = dict(recs["decoders.0.basic_module.conv2"])
    with pytest.raises(AssertionError, match="not used exactly once"):
        _gate(RES, sd, x, t, False, extra, dec, grads, logits)
    missing = {k: dict(v) for k, v in recs.items()}
    del missing["encoders.1.basic_module.conv3"]["dz"]
    with pytest.raises(KeyError, match="encoders.1.basic_module.conv3:dz"):
        _gate(RES, sd, x, t, False, missing, dec, grads, logits)
    skipped = {k: dict(v) for k, v in recs.items()}
    del skipped["encoders.0.basic_module.conv2"]["dg"]
    skipped["encoders.0.basic_module.conv2"]["dg_skip"] = "no input gradient"
    rep, fails = _gate(RES, sd, x, t, False, skipped, dec, grads, logits)
    assert not fails and rep.skipped == {"encoders.0.basic_module.conv2:dg": "no input gradient"}


def test_tape_names_map_through_the_decided_harness():
    mods = dict(dcd.build_model(RESSE, _seeded(RESSE)[0]).named_modules())
    assert dcd.record_module(mods, "dec0.c3") == ("decoders.0.basic_module", "decoders.0.basic_module.conv3")
    with pytest.raises(AssertionError):
        dcd.record_module(mods, "enc5.c2")
    with pytest.raises(AssertionError):
        dcd.record_module(mods, "enc0.c1")
