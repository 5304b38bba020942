"""-m gpu: the teacher-forced float64 gate (tests/teacher.py) of the bf16 modes — `compute_dtype: bf16` (bf16 MFMA operands, fp32
tensors in HBM; the nets of tests/test_gpu_bf16.py) and `activation_dtype: bf16` (bf16 storage; the nets of tests/test_gpu_b16.py and
BASELINE config 4's channel ladder).

One native step runs with `eng.debug` on: its tape and the backward's dz / dg clones become per-layer records, its ReLU masks and pool
arg-maxes come from decided.decisions_from_tape.  The float64 restatement of the same bf16 arithmetic is then fed the native tensors
at every layer, so each layer's output, GroupNorm table, dz, dg, residual and SE output, and every parameter gradient, must match to
accumulation order (bars: tests/teacher.py).  A second step without the debug records must give bitwise-equal gradients."""
import time

import pytest
import torch

import decided as dcd
import teacher as T
from conftest import Golden, diag, loss_by_name
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d.model import get_model
from test_gpu_bf16 import MODEL_CASES

pytestmark = pytest.mark.gpu

B16_KERNELS = {"u3d_conv3d_bf16_ex_b16", "u3d_conv3d_wgrad_bf16_b16_job", "u3d_convtr3d_dgrad_t8_b16_ex", "u3d_convtr3d_wgrad_t8_b16",
               "u3d_maxpool2_bwd_merge_b16", "u3d_nearest_add_fwd_t8_b16", "u3d_nearest_sum_bwd_t8_b16", "u3d_gn_bwd_apply_b16",
               "u3d_conv1x1_head_fwd_b16", "u3d_conv1x1_head_bwd_b16"}


def _seeded(cfg, shape, seed):
    """as tests/test_gpu_bf16.py::_prep: norms perturbed (the default init hides half of the gradient paths)"""
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


def _native_step(model, x, t, loss_fn, debug):
    eng = model._get_engine()
    eng.debug = {} if debug else None
    for p in model.parameters():
        p.grad = None
    prof = nat.EventProfiler()
    nat.profiler = prof
    try:
        probs, logits = model(x.to(DEV), return_logits=True)
        recs = names = dec = None
        if debug:
            tape = eng.debug["tape"]
            dec = dcd.decisions_from_tape(model, tape)
            recs, names = T.native_records(model, tape)
        loss = loss_fn(probs, logits, t.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        if debug:
            T.attach_gradients(recs, names, eng.debug)
    finally:
        eng.debug = None
        nat.profiler = None
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return logits.detach().cpu(), grads, recs, dec, set(prof.summary())


def teacher_gate(mode, cfg, sd, x, t, loss_name, storage, kernels):
    keys = dict(compute_dtype="bf16", activation_dtype="bf16" if storage else "fp32")
    model = get_model(dict(cfg, **keys))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    eng = model._get_engine()
    assert eng.bf16 and eng.act_bf16 == storage, (eng.bf16, getattr(eng, "act_bf16", None))
    loss_fn = lambda p, lg, tt: loss_by_name(loss_name, p, lg, tt)  # noqa: E731
    logits, grads, recs, dec, names = _native_step(model, x, t, loss_fn, True)
    assert kernels <= names, sorted(kernels - names)
    # the production schedule (no debug records): bitwise the same step
    logits2, grads2, _, _, _ = _native_step(model, x, t, loss_fn, False)
    assert torch.equal(logits, logits2), "logits of the step without debug records differ"
    diff = [k for k in grads if not torch.equal(grads[k], grads2[k])]
    assert not diff, f"gradients of the step without debug records differ: {diff[:4]}"
    del model
    recs = T.strip_dtypes(recs, storage)
    t0 = time.time()
    rep, fails = T.gate(cfg, sd, x, t, loss_fn, recs, dec, grads, storage, native_logits=logits)
    cpu_s = time.time() - t0
    figs = rep.figures
    worst = {q: max(((k, f[m]) for k, f in figs.items() if k.endswith(":" + q) and m in f), key=lambda v: v[1], default=(None, 0.0))
             for q, m in (("y", "ulp" if storage else "slice"), ("dg", "ulp" if storage else "slice"),
                          ("affine", "slice"), ("logits", "slice"))}
    dz = [(k, f) for k, f in figs.items() if k.endswith(":dz")]
    m = "ulp" if storage else "slice"
    worst["dz_conv2"] = max(((k, f[m]) for k, f in dz if not k.endswith(".conv3:dz")), key=lambda v: v[1], default=(None, 0.0))
    worst["dz_conv3"] = max(((k, f[m]) for k, f in dz if k.endswith(".conv3:dz")), key=lambda v: v[1], default=(None, 0.0))
    if storage:
        worst["r_out"] = max(((k, f["ulp"]) for k, f in figs.items() if k.endswith((":r", ":out"))), key=lambda v: v[1], default=(None, 0.0))
        worst["frac"] = rep.worst("frac")
        link = lambda k: k.endswith(".conv3:dz") or (k.startswith("decoders.") and k.endswith(":r"))  # noqa: E731
        worst["frac_direct"] = max(((k, f["frac"]) for k, f in figs.items() if "frac" in f and not link(k)), key=lambda v: v[1])
        worst["beyond_ulp"] = rep.worst("beyond_ulp")
    first = dcd.first_norm_weight(rep.grads)
    pr = {k[6:]: f["grad_rel"] for k, f in figs.items() if k.startswith("param:")}
    behind = {k: e for k, e in pr.items() if T.behind_unforced_rounding(k, storage)}
    rest = {k: e for k, e in pr.items() if k not in behind and k != first}
    worst["param"] = max(rest.items(), key=lambda v: v[1])
    worst["param_behind"] = max(behind.items(), key=lambda v: v[1]) if behind else (None, 0.0)
    worst["first_norm"] = (first, pr.get(first))
    rec = dict(test="bf16_teacher_gate", mode=mode, cfg=str(cfg), shape=list(x.shape), cpu_seconds=round(cpu_s, 1),
               skipped=rep.skipped, worst=worst, failures=fails[:12])
    diag(**rec)
    print(rec)
    assert not fails, fails
    return rec


@pytest.mark.parametrize("cfg,shape", MODEL_CASES, ids=["resunet3d", "resunet3d-ragged", "unet3d"])
def test_bf16_operand_models_teacher_forced(cfg, shape):
    loss_name = "bce_dice" if cfg.get("final_sigmoid", True) else "probs_sum"
    sd, x, t = _seeded(cfg, shape, 99)
    kernels = {"u3d_conv3d_bf16_ex", "u3d_conv3d_wgrad_bf16_job"}
    teacher_gate("bf16", cfg, sd, x, t, loss_name, False, kernels)


@pytest.mark.parametrize("net", ["ResidualUNet3D", "ResidualUNetSE3D"])
def test_bf16_storage_models_teacher_forced(net):
    cfg = dict(name=net, in_channels=1, out_channels=1, f_maps=[64, 128, 256], num_groups=8, final_sigmoid=True)
    sd, x, t = _seeded(cfg, (1, 1, 16, 32, 32), 21)
    kernels = B16_KERNELS | ({"u3d_se_apply_fwd_b16", "u3d_se_bwd_reduce_b16", "u3d_se_bwd_apply_b16"} if net == "ResidualUNetSE3D" else set())
    teacher_gate("bf16_storage", cfg, sd, x, t, "bce_dice", True, kernels)


@pytest.mark.timeout(1200)
def test_config4_ladder_golden_teacher_forced():
    """BASELINE config 4's channel ladder (ResidualUNet3D f_maps=64, 64 ... 1024 channels) at the fixture's 1x1x32x64x64 under bf16
    compute + bf16 storage (the float64 side: 13 s on the GPU box)."""
    g = Golden("g10_resunet3d_f64_ladder")
    x, t = g.inputs()
    sd = {k: v.detach().clone() for k, v in g.build_model().state_dict().items()}
    teacher_gate("bf16_storage", g.cfg, sd, x, t, g.loss_name, True, B16_KERNELS)
