"""-m gpu: the decision-consistent float64 gate (tests/decided.py) for every native mode beyond the 3-D 'gcr' models of
tests/test_gpu_model.py::test_gradients_match_decision_consistent_fp64_oracle — UNet2D (`native_2d`), ResidualUNet2D
(`native_2d_residual`), the 3-D non-'gcr' orders and `upsample: deconv`, and `compute_dtype: fp32_split`.

One native training step runs with its activation tape captured; the product's CPU module tree then repeats the step in float64 with
the step's own ReLU / LeakyReLU masks and max-pool arg-maxes imposed.  Nothing but smooth arithmetic separates the two, so:
logits / probs and the loss within 1e-4, EVERY parameter gradient and the input gradient within 1e-4 of their own range (the first
norm's weight: 1e-3, see decided.FIRST_NORM_REL), BatchNorm running statistics within 1e-5.  The loose bars of the per-mode tests
absorb decision flips and stay as they are; this gate sees a single wrong bias, slope or statistic.

Debug mode turns the side-stream weight gradient off (_engine_conv.py `_wgrad_family`), so the same step runs a second time without
the tape and must be bitwise equal: the gate then holds for the production schedule too."""
import pytest
import torch

import decided as dcd
from conftest import Golden, diag, loss_by_name
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model

pytestmark = pytest.mark.gpu
REL = 1e-4
BUF_REL = 1e-5


def _loss_name(cfg):
    if not cfg.get("is_segmentation", True):
        return "mse"
    return "bce_dice" if cfg.get("final_sigmoid", True) else "probs_sum"


def _seeded(cfg, shape, seed, perturb=True):
    """(sd, x, target) of a seeded net; norms perturbed: the default init (gamma 1, beta 0) hides half of the gradient paths"""
    torch.manual_seed(seed)
    model = get_model(dict(cfg))
    with torch.no_grad():
        for k, p in model.named_parameters():
            if perturb and ("groupnorm" in k or "batchnorm" in k):
                p.add_(0.2 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.randn(shape)
    target = (torch.rand((shape[0], cfg["out_channels"]) + tuple(shape[2:])) > 0.5).float()
    return sd, x, target


def _native_step(model, x, target, loss_name, tape):
    """one native step with x.requires_grad; with `tape`: eng.debug on and the tape's decisions returned"""
    eng = model._get_engine()
    eng.debug = {} if tape else None
    xg = x.to(DEV).requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    n0 = nat.launch_count
    try:
        probs, logits = model(xg, return_logits=True)
        dec = dcd.decisions_from_tape(model, eng.debug["tape"]) if tape else None
        loss = loss_by_name(loss_name, probs, logits, target.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        eng.debug = None
    assert nat.launch_count > n0, "native HIP path did not run"
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return probs.detach().cpu(), logits.detach().cpu(), loss.item(), xg.grad.detach().cpu().clone(), grads, dec


def gate(mode, cfg, shape=None, seed=0, sd=None, x=None, target=None, native_keys=None, loss_name=None, check=None):
    """run the decided gate on one configuration; `native_keys` switch the native mode on (added to cfg for the GPU model only)"""
    if sd is None:
        sd, x, target = _seeded(cfg, shape, seed)
    loss_name = loss_name or _loss_name(cfg)
    model = get_model(dict(cfg, **(native_keys or {})))
    model.load_state_dict(sd)
    assert model.native_supported, model._native_blockers
    if check is not None:
        check(model)
    model = model.to(DEV).train()
    probs, logits, loss, dx, grads, dec = _native_step(model, x, target, loss_name, tape=True)
    buffers = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    # the production schedule (no tape, side-stream weight gradients where configured): bitwise the same step
    _, logits2, loss2, dx2, grads2, _ = _native_step(model, x, target, loss_name, tape=False)
    assert torch.equal(logits2, logits) and loss2 == loss and torch.equal(dx2, dx), "step without the tape differs"
    diff = [k for k in grads if not torch.equal(grads[k], grads2[k])]
    assert not diff, f"gradients of the step without the tape differ: {diff[:4]}"

    ref = dcd.decided_step(cfg, sd, x, target, lambda p, lg, t: loss_by_name(loss_name, p, lg, t), dec)
    e_logits, e_probs = dcd.rel_err(logits, ref.logits), dcd.rel_err(probs, ref.probs)
    e_loss = abs(loss - ref.loss) / max(1.0, abs(ref.loss))
    e_dx = dcd.rel_err(dx, ref.dx)
    first = dcd.first_norm_weight(ref.grads)
    errs = {k: dcd.rel_err(grads[k], ref.grads[k]) for k in ref.grads}
    worst = max(((k, e) for k, e in errs.items() if k != first), key=lambda t: t[1])
    e_buf = max((dcd.rel_err(buffers[k], ref.buffers[k]) for k in ref.buffers if "running_" in k), default=0.0)
    for k in ref.buffers:
        if "num_batches" in k:
            assert int(buffers[k]) == int(ref.buffers[k]), k
    rec = dict(test="decided_gate", mode=mode, cfg=str(cfg), shape=list(x.shape), logits_rel=e_logits, probs_rel=e_probs, loss_rel=e_loss,
               dx_rel=e_dx, worst_param=worst[0], worst_grad_rel=worst[1], first_norm=first,
               first_norm_rel=errs.get(first), buffers_rel=e_buf, decisions=len(dec))
    diag(**rec)
    print(rec)
    assert e_logits < REL and e_probs < REL and e_loss < REL, (e_logits, e_probs, e_loss)
    fails = dcd.gate_failures(grads, ref.grads, first)
    assert not fails, fails
    assert e_dx < dcd.GRAD_REL, e_dx
    assert set(buffers) == set(ref.buffers) and e_buf < BUF_REL, e_buf
    return rec


# ---- UNet2D, native_2d: the configurations of tests/test_gpu_model2d.py ------------------------------------------------------------
_N2D = dict(native_2d=True)


@pytest.mark.parametrize("cfg,shape", [
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=8, num_levels=2, num_groups=4), (1, 1, 16, 16)),
    (dict(name="UNet2D", in_channels=2, out_channels=3, f_maps=[8, 16], num_groups=4, final_sigmoid=False), (3, 2, 32, 24)),
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32, 64], num_groups=4), (2, 1, 8, 8)),
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4, is_segmentation=False), (2, 1, 20, 18)),
])
def test_unet2d_edge_cases_decided(cfg, shape):
    gate("native_2d", cfg, shape, seed=2, native_keys=_N2D)


@pytest.mark.parametrize("order", ["cr", "gcl", "cgr", "bcr"])
def test_unet2d_layer_orders_decided(order):
    cfg = dict(name="UNet2D", in_channels=1, out_channels=2, f_maps=[8, 16, 32], num_groups=4, layer_order=order, final_sigmoid=False)
    gate("native_2d", cfg, (2, 1, 35, 29), seed=3, native_keys=_N2D)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg,shape", [
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="bcr", num_groups=8), (2, 1, 256, 256)),
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=32, num_levels=4, layer_order="gcr", num_groups=8), (2, 1, 515, 512)),
], ids=["dsb2018-bcr", "confocal-gcr"])
def test_shipped_2d_configurations_decided(cfg, shape):
    gate("native_2d", cfg, shape, seed=1, native_keys=_N2D)


# ---- ResidualUNet2D, native_2d_residual: the cases of tests/reference_records_resunet2d.py, rebuilt from their seeds --------------------
@pytest.mark.parametrize("case", ["gcr", "cge", "bcr", "deconv", "softmax"])
def test_resunet2d_cases_decided(case):
    from reference_records_resunet2d import CASES, SHAPE

    seed, cfg = CASES[case]
    gate("native_2d_residual", cfg, SHAPE, seed=seed, native_keys=dict(native_2d_residual=True),
         check=lambda m: m.native_2d or pytest.fail("not on the 2-D path"))


# ---- 3-D orders beyond 'gcr' (tests/test_gpu_orders.py's shapes) -----------------------------------------------------------------------
_U3 = dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=16, num_levels=3, num_groups=8)
_R3 = dict(name="ResidualUNet3D", in_channels=2, out_channels=2, f_maps=[8, 16, 32], num_groups=4, final_sigmoid=False)


@pytest.mark.parametrize("order", ["cgr", "cgl", "cge", "crg", "bcr", "cbr", "crb", "cbl", "cr", "cl", "c"])
@pytest.mark.parametrize("cfg,shape", [(_U3, (2, 1, 16, 32, 32)), (_R3, (2, 2, 10, 12, 14))], ids=["UNet3D", "ResidualUNet3D"])
def test_3d_orders_decided(order, cfg, shape, monkeypatch):
    monkeypatch.setenv("U3D_STRICT", "1")  # no stock-operator fallback
    gate("3d_orders", dict(cfg, layer_order=order), shape, seed=31)


@pytest.mark.parametrize("order", ["gcr", "gce", "cgl"])
@pytest.mark.parametrize("cfg,shape", [
    (dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=16, num_levels=3, num_groups=8), (1, 1, 16, 32, 32)),
    (dict(name="UNet3D", in_channels=2, out_channels=2, f_maps=[8, 16, 32], num_groups=4, final_sigmoid=False), (2, 2, 9, 13, 11)),
])
def test_3d_deconv_doubleconv_decided(order, cfg, shape, monkeypatch):
    monkeypatch.setenv("U3D_STRICT", "1")
    gate("3d_deconv", dict(cfg, layer_order=order, upsample="deconv"), shape, seed=37,
         check=lambda m: any("conv_transposed" in k for k in m.state_dict()) or pytest.fail("no transposed convolution"))


# ---- compute_dtype: fp32_split (tests/test_gpu_f32s.py's models and the channel-ladder goldens) ----------------------------------------
_SPLIT = dict(compute_dtype="fp32_split")


def _is_split(m):
    assert m.compute_split


@pytest.mark.parametrize("cfg,shape", [
    (dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=32, num_groups=8), (2, 1, 16, 32, 32)),
    (dict(name="ResidualUNet3D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], num_groups=8), (1, 1, 16, 24, 24)),
    (dict(name="ResidualUNetSE3D", in_channels=3, out_channels=2, f_maps=[32, 64, 128], num_groups=8, final_sigmoid=False), (1, 3, 12, 16, 20)),
])
def test_split_models_decided(cfg, shape, monkeypatch):
    monkeypatch.setenv("U3D_STRICT", "1")
    gate("fp32_split", cfg, shape, seed=7, native_keys=_SPLIT, check=_is_split)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name", ["g10_resunet3d_f64_ladder", "g11_resunetse3d_in3_ladder"])
def test_split_channel_ladder_goldens_decided(name):
    """config 4's / 5's channel ladders (64 ... 1024 channels): the decided gate runs unconditionally, not only when the direct band of
    tests/test_gpu_f32s.py fails"""
    g = Golden(name)
    x, target = g.inputs()
    sd = {k: v.detach().clone() for k, v in g.build_model().state_dict().items()}
    gate("fp32_split", g.cfg, sd=sd, x=x, target=target, native_keys=_SPLIT, loss_name=g.loss_name, check=_is_split)
