"""-m gpu: the split weight gradient (`fp32_split_wgrad: true`; csrc/u3d_wgrad_f32s.hip, u3d_conv3d_wgrad_f32s of the extension library):
both operands split exactly into three bf16 values, six partial products on the bf16 MFMA, fp32 accumulation.  The claim under test is
FP32-GRADE accuracy.  The truth is a float64 conv3d weight gradient on the CPU of the SAME fp32 operands (affine applied in fp32 as
addcmul, as tests/test_gpu_f32s.py does); the yardstick is u3d_conv3d_wgrad (fp32 MFMA) on the same operands in the same test.

Bounds: relative L2 error below 2.5x the fp32 kernel's own (the factor of test_conv3d_f32s_forward_is_fp32_grade) and below 1e-2 of the
error of u3d_conv3d_wgrad_bf16 (bf16 operands err at 2^-9 against 2^-24: 1e-2 separates the grades with room on both sides).  Drift:
|mean signed error| / rms error over all dw entries at most max(0.1, 3x the fp32 kernel's) — an uncancelled round-down drift of the
accumulation gives a figure near 1, independent errors about 1 / sqrt(27 * 32 * 32) = 0.006."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import f32s_emul as FE
import gpu_utils as U
from conftest import diag
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import VSrc, _p, _stream

pytestmark = pytest.mark.gpu


def _ext():
    return nat.get_ext_lib()


def wgrad_f32s(xd, dzd, Cin, Cout, affine=None, ws_floats=None, dw=None, stride=None):
    """u3d_conv3d_wgrad_f32s on NDHWC device tensors; returns (dw, workspace floats used)"""
    N, D, H, W, _ = xd.shape
    need = _ext().u3d_wgrad_f32s_workspace_floats(N, D, H, W, Cin, Cout)
    assert need > 0 and need % (27 * Cin * Cout) == 0
    n = need if ws_floats is None else ws_floats
    ws = torch.empty(n, dtype=torch.float32, device=U.DEV)
    stride = Cin if stride is None else stride
    if dw is None:
        dw = torch.empty((Cout, stride, 3, 3, 3), dtype=torch.float32, device=U.DEV)
    nat.call("u3d_conv3d_wgrad_f32s", 0, _stream(U.DEV), _p(xd), _p(affine), _p(dzd), _p(dw), stride, N, D, H, W, Cin, Cout, _p(ws), n)
    torch.cuda.synchronize()
    return dw, n


def wgrad_bf16(xd, dzd, Cin, Cout, affine=None):
    N, D, H, W, _ = xd.shape
    n = nat.get_lib().u3d_wgrad_bf16_workspace_floats(N, D, H, W, Cin, Cout)
    ws = torch.empty(max(n, 4), dtype=torch.float32, device=U.DEV)
    dw = torch.empty((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=U.DEV)
    nat.call("u3d_conv3d_wgrad_bf16", 0, _stream(U.DEV), _p(xd), _p(affine), _p(dzd), _p(dw), N, D, H, W, Cin, Cout, _p(ws), ws.numel())
    torch.cuda.synchronize()
    return dw


def truth_f64(g32, dz):
    """float64 weight gradient of conv3d(g, w, padding=1) for the output gradient dz, on the CPU"""
    K, C = dz.shape[1], g32.shape[1]
    w = torch.zeros(K, C, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(g32.double(), w, None, padding=1).backward(dz.double())
    return w.grad


def operands(shape, C, K, seed, with_affine, relu_like=False):
    N, D, H, W = shape
    torch.manual_seed(seed)
    x = torch.randn(N, C, D, H, W) * (1.0 + torch.rand(N, C, 1, 1, 1) * 3.0)  # channel scales differ, like pre-GroupNorm data
    dz = torch.randn(N, K, D, H, W) * (1.0 + torch.rand(N, K, 1, 1, 1) * 3.0)
    if relu_like:  # nonzero-mean operands
        x = x.clamp_min(0)
        dz = dz + 0.5
    aff = None
    g32 = x
    if with_affine:
        a = 1.0 + 0.3 * torch.randn(N, C)
        b = 0.2 * torch.randn(N, C)
        aff = torch.stack((a, b), dim=-1).contiguous().to(U.DEV)
        g32 = torch.addcmul(b.view(N, C, 1, 1, 1), x, a.view(N, C, 1, 1, 1))
    return x, dz, aff, g32


def rel_l2(dw, ref):
    return ((dw.detach().cpu().double() - ref).norm() / ref.norm()).item()


_CASES = {}


def _case(shape, C, K, with_affine, relu_like=False):
    """operands, float64 truth and the fp32 kernel's result of one case: computed once, shared, left unchanged"""
    key = (shape, C, K, with_affine, relu_like)
    if key not in _CASES:
        x, dz, aff, g32 = operands(shape, C, K, 11, with_affine, relu_like)
        xd, dzd = U.ndhwc(x), U.ndhwc(dz)
        ref = truth_f64(g32, dz)
        dw32 = U.wgrad(VSrc(xd), dzd, K, affine=aff)
        torch.cuda.synchronize()
        _CASES[key] = (xd, dzd, aff, ref, dw32.cpu())
    return _CASES[key]


GRADE_SHAPES = [
    ((2, 9, 13, 17), 32, 32),    # ragged on every axis
    ((1, 8, 16, 16), 64, 96),    # Cout % 64 == 32
    ((1, 5, 10, 10), 128, 64),   # more (ci, co) pairs than tiles
]


@pytest.mark.parametrize("with_affine", [False, True])
@pytest.mark.parametrize("shape,C,K", GRADE_SHAPES)
def test_wgrad_f32s_is_fp32_grade(shape, C, K, with_affine):
    xd, dzd, aff, ref, dw32 = _case(shape, C, K, with_affine)
    dw, _ = wgrad_f32s(xd, dzd, C, K, aff)
    dwb = wgrad_bf16(xd, dzd, C, K, aff)
    e_new, e_f32, e_b16 = rel_l2(dw, ref), rel_l2(dw32, ref), rel_l2(dwb, ref)
    diag(test="wgrad_f32s_grade", shape=list(shape), C=C, K=K, affine=with_affine, l2_split=e_new, l2_f32mfma=e_f32, l2_bf16=e_b16)
    assert e_new < 2.5 * e_f32, (e_new, e_f32)
    assert e_new < 1e-2 * e_b16, (e_new, e_b16)


def _drift(dw, ref):
    err = dw.detach().cpu().double() - ref
    return (err.mean().abs() / err.pow(2).mean().sqrt()).item()


def test_wgrad_f32s_accumulation_does_not_drift():
    shape, C, K = (1, 24, 48, 48), 32, 32
    xd, dzd, aff, ref, dw32 = _case(shape, C, K, False, relu_like=True)
    dw, _ = wgrad_f32s(xd, dzd, C, K, aff)
    d_new, d_f32 = _drift(dw, ref), _drift(dw32, ref)
    diag(test="wgrad_f32s_drift", shape=list(shape), C=C, K=K, drift_split=d_new, drift_f32mfma=d_f32, l2_split=rel_l2(dw, ref),
         l2_f32mfma=rel_l2(dw32, ref))
    assert d_new <= max(0.1, 3.0 * d_f32), (d_new, d_f32)


def test_wgrad_f32s_same_workspace_same_bits_and_one_slot_is_fp32_grade():
    shape, C, K = GRADE_SHAPES[0]
    xd, dzd, aff, ref, dw32 = _case(shape, C, K, True)
    dw1, n = wgrad_f32s(xd, dzd, C, K, aff)
    dw2, _ = wgrad_f32s(xd, dzd, C, K, aff)
    assert torch.equal(dw1, dw2)
    slot = 27 * C * K
    assert n > slot  # the plan splits
    one, _ = wgrad_f32s(xd, dzd, C, K, aff, ws_floats=slot)
    e_one, e_f32 = rel_l2(one, ref), rel_l2(dw32, ref)
    diag(test="wgrad_f32s_one_slot", shape=list(shape), C=C, K=K, l2_one_slot=e_one, l2_f32mfma=e_f32, slots_planned=n // slot)
    assert e_one < 2.5 * e_f32, (e_one, e_f32)
    two, _ = wgrad_f32s(xd, dzd, C, K, aff, ws_floats=2 * slot + 5)  # as many splits as it holds
    assert rel_l2(two, ref) < 2.5 * e_f32


def test_wgrad_f32s_strided_write_touches_only_its_slice():
    shape, C, K = GRADE_SHAPES[0]
    xd, dzd, aff, ref, _ = _case(shape, C, K, True)
    plain, _ = wgrad_f32s(xd, dzd, C, K, aff)
    again, _ = wgrad_f32s(xd, dzd, C, K, aff, stride=C)
    assert torch.equal(plain, again)
    Ct, c0 = C + 64, 32  # a (K, Ct, 27) gradient; the slice starts at channel c0
    poison = 12345.0
    wide = torch.full((K, Ct, 27), poison, dtype=torch.float32, device=U.DEV)
    wgrad_f32s(xd, dzd, C, K, aff, dw=wide.view(-1)[c0 * 27:], stride=Ct)
    wide = wide.cpu()
    assert torch.equal(wide[:, c0:c0 + C], plain.cpu().view(K, C, 27))
    assert (wide[:, :c0] == poison).all() and (wide[:, c0 + C:] == poison).all()


def test_wgrad_f32s_refusals_launch_nothing():
    N, D, H, W = 1, 4, 8, 8
    lib, core = _ext(), nat.get_lib()
    x = torch.randn(N, D, H, W, 64, device=U.DEV)
    dz = torch.randn(N, D, H, W, 64, device=U.DEV)
    ws = torch.empty(27 * 64 * 64 * 4, device=U.DEV)
    poison = 777.0
    dw = torch.full((64 * 64 * 27,), poison, device=U.DEV)
    st = _stream(U.DEV)

    def refused(x_, dz_, Cin, Cout, stride, ws_, n, what):
        rc = lib.u3d_conv3d_wgrad_f32s(0, st, x_, None, dz_, _p(dw), stride, N, D, H, W, Cin, Cout, ws_, n)
        torch.cuda.synchronize()
        assert rc == nat.U3D_EINVAL, what
        assert b"u3d_conv3d_wgrad_f32s" in core.u3d_last_error(), what
        assert (dw == poison).all(), what

    refused(_p(x), _p(dz), 16, 32, 16, _p(ws), ws.numel(), "Cin outside the envelope")
    refused(_p(x), _p(dz), 32, 48, 32, _p(ws), ws.numel(), "Cout outside the envelope")
    refused(_p(x), _p(dz), 0, 32, 32, _p(ws), ws.numel(), "no channels")
    refused(_p(x), _p(dz), 32, 32, 32, _p(ws), 27 * 32 * 32 - 1, "less than one slot")
    refused(_p(x), _p(dz), 32, 32, 32, None, 0, "no workspace")
    refused(_p(x), _p(dz), 32, 32, 16, _p(ws), ws.numel(), "stride below Cin")
    refused(ctypes.c_void_p(x.data_ptr() + 4), _p(dz), 32, 32, 32, _p(ws), ws.numel(), "unaligned x")
    refused(None, _p(dz), 32, 32, 32, _p(ws), ws.numel(), "no x")
    assert lib.u3d_wgrad_f32s_workspace_floats(N, D, H, W, 16, 32) == 0 and lib.u3d_wgrad_f32s_workspace_floats(N, D, H, W, 32, 32) > 0


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
MODEL_CASES = [
    ("UNet3D", dict(in_channels=1, out_channels=1, f_maps=32, num_groups=8), (2, 1, 16, 32, 32)),
    ("ResidualUNet3D", dict(in_channels=1, out_channels=1, f_maps=[32, 64, 128], num_groups=8), (1, 1, 16, 24, 24)),
]


def _run_arm(model, x, target):
    from conftest import loss_by_name

    model = model.to(U.DEV).train()
    prof = nat.EventProfiler()
    nat.profiler = prof
    try:
        probs, logits = model(x.to(U.DEV), return_logits=True)
        loss = loss_by_name("bce_dice", probs, logits, target.to(U.DEV))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    return logits.detach().cpu(), grads, prof.summary()


@pytest.mark.parametrize("cls,cfg,shape", MODEL_CASES)
def test_models_with_the_key_route_the_weight_gradients_and_hold_the_fp32_tolerances(cls, cfg, shape, monkeypatch):
    import unet3d_oracle as orc
    from pytorch3dunet_amd.unet3d import model as M

    monkeypatch.setenv("U3D_STRICT", "1")
    torch.manual_seed(7)
    parent = getattr(M, cls)(compute_dtype="fp32_split", **cfg)
    keyed = getattr(M, cls)(fp32_split_wgrad=True, **cfg)
    sd = {k: v.detach().clone() for k, v in parent.state_dict().items()}
    keyed.load_state_dict(sd)
    assert keyed.compute_split and keyed.fp32_split_wgrad and keyed.native_supported and not parent.fp32_split_wgrad
    x = torch.randn(shape)
    target = (torch.rand((shape[0], cfg["out_channels"]) + shape[2:]) > 0.5).float()
    G = cfg["num_groups"]
    _, _, _, g32 = orc.forward_backward(sd, x, target, G, True, True, "bce_dice")
    _, _, _, g64 = orc.forward_backward({k: v.double() for k, v in sd.items()}, x.double(), target.double(), G, True, True, "bce_dice")
    routed = FE.routed(keyed, shape[2:])
    assert routed
    l_par, g_par, s_par = _run_arm(parent, x, target)
    l_key, g_key, s_key = _run_arm(keyed, x, target)
    assert s_par.get("u3d_conv3d_wgrad_f32s", {"calls": 0})["calls"] == 0
    assert s_key.get("u3d_conv3d_wgrad_f32s", {"calls": 0})["calls"] == len(routed)
    assert torch.equal(l_par, l_key)  # the forward is untouched
    keys = list(g32)
    cat = lambda g: torch.cat([g[k].double().flatten() for k in keys])  # noqa: E731
    r64 = cat(g64)
    e_key, e_par, e_ref = (((cat(g) - r64).norm() / r64.norm()).item() for g in (g_key, g_par, g32))
    worst = max((((g_key[n].double() - g_par[n].double()).norm() / g_par[n].double().norm()).item(), n) for n, _, _, _ in routed)
    diag(test="wgrad_f32s_model", cls=cls, shape=list(shape), routed=len(routed), key_vs_fp64=e_key, parent_vs_fp64=e_par, ref32_vs_fp64=e_ref,
         worst_routed_vs_parent=worst[0], worst_routed=worst[1])
    assert e_key <= max(1e-3, 3.0 * e_ref), (e_key, e_ref)
    assert worst[0] <= 1e-4, worst
