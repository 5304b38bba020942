"""The kernels ResidualUNet2D adds under `native_2d_residual: true`, through the C-ABI: the residual epilogue of the 3x3 conv2d
(u3d_conv2d_res_reps, split-K included) and ConvTranspose2d(k=3, s=2, p=1) forward, data gradient (with and without the ReLU mask) and
weight gradient (u3d_convtr2d_*) — against float64 F.conv2d / F.conv_transpose2d and autograd on the CPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import VSrc, _p, _stream

pytestmark = pytest.mark.gpu
TOL = 1e-4  # max-abs error relative to the float64 result's range


def nhwc(x):  # (N,C,H,W) cpu -> (N,1,H,W,C) gpu
    return x.permute(0, 2, 3, 1).contiguous().unsqueeze(1).to(DEV)


def nchw(y):  # (N,1,H,W,C) gpu -> (N,C,H,W) cpu
    return y.squeeze(1).permute(0, 3, 1, 2).contiguous().cpu()


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def pack2d(w):
    Cout, Cin = w.shape[:2]
    out = torch.empty(nat.get_lib().u3d_packed_weight2d_floats(Cin, Cout, 0), dtype=torch.float32, device=DEV)
    wd = w.float().contiguous().to(DEV)
    nat.call("u3d_pack_weights2d", 0, _stream(DEV), _p(wd), Cout, Cin, 0, _p(out))
    return out


def conv2d_res(x, w, res, relu, aff=None):
    """one u3d_conv2d_res_reps call: x (N,Cin,H,W), res (N,Cout,H,W) cpu -> output (N,Cout,H,W), statistics (N,Cout,2), split-K size"""
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    src = VSrc(nhwc(x))
    wp = pack2d(w)
    y = torch.empty((N, 1, H, W, Cout), dtype=torch.float32, device=DEV)
    r = nhwc(res)
    st = torch.zeros(N * Cout * 2, dtype=torch.float64, device=DEV)
    need = nat.get_lib().u3d_conv2d_workspace_floats(N, H, W, Cin, Cout)
    ws = torch.empty(need, dtype=torch.float32, device=DEV) if need > 0 else None
    s = src.struct(aff.to(DEV) if aff is not None else None)
    nat.call("u3d_conv2d_res_reps", 0, _stream(DEV), ctypes.byref(s), _p(wp), _p(y), N, H, W, Cout, relu, _p(st), None, None, _p(ws),
             need, 1, _p(r))
    return nchw(y), st.view(N, Cout, 2).cpu(), need


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 7, 9, 3, 5), (2, 67, 45, 8, 8), (1, 1, 1, 5, 64), (2, 33, 22, 16, 16),
                                            (1, 64, 64, 64, 64)])
@pytest.mark.parametrize("relu", [0, 1])
def test_conv2d_residual_epilogue(N, H, W, Cin, Cout, relu):
    g = torch.Generator().manual_seed(N + H + Cin + Cout + relu)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    res = torch.randn(N, Cout, H, W, generator=g)
    aff = torch.stack((0.5 + torch.rand(N, Cin, generator=g), 0.3 * torch.randn(N, Cin, generator=g)), -1).contiguous()
    xa = x.double() * aff[..., 0].double()[:, :, None, None] + aff[..., 1].double()[:, :, None, None]
    ref = F.conv2d(xa, w.double(), padding=1) + res.double()
    if relu:
        ref = ref.clamp_min(0)
    y, st, _ = conv2d_res(x, w, res, relu, aff)
    assert rel(y, ref) < TOL
    s_ref = torch.stack((ref.sum((2, 3)), (ref * ref).sum((2, 3))), -1)  # sums of the written values
    assert rel(st, s_ref) < 1e-5


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(1, 8, 8, 256, 128), (2, 16, 16, 128, 64)])
@pytest.mark.parametrize("relu", [0, 1])
def test_conv2d_residual_split_k(N, H, W, Cin, Cout, relu):
    g = torch.Generator().manual_seed(9 + relu)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    res = torch.randn(N, Cout, H, W, generator=g)
    ref = F.conv2d(x.double(), w.double(), padding=1) + res.double()
    if relu:
        ref = ref.clamp_min(0)
    y, st, need = conv2d_res(x, w, res, relu)
    assert need > 0  # the split-K reduction adds the residual
    assert rel(y, ref) < TOL
    assert rel(st, torch.stack((ref.sum((2, 3)), (ref * ref).sum((2, 3))), -1)) < 1e-5


def test_conv2d_residual_refuses_gx():
    x = nhwc(torch.randn(1, 4, 5, 5))
    wp = pack2d(torch.randn(4, 4, 3, 3))
    y = torch.empty_like(x)
    gst = torch.zeros(8, dtype=torch.float64, device=DEV)
    s, sg = VSrc(x).struct(), VSrc(x).struct()
    with pytest.raises(Exception, match="residual"):
        nat.call("u3d_conv2d_res_reps", 0, _stream(DEV), ctypes.byref(s), _p(wp), _p(y), 1, 5, 5, 4, 0, None, ctypes.byref(sg), _p(gst),
                 None, 0, 1, _p(x))


# ---- ConvTranspose2d(k=3, stride=2, padding=1, bias=False) ----------------------------------------------------------------------
def pack_tr(w, mode):
    Cin, Cout = w.shape[:2]
    out = torch.empty(nat.get_lib().u3d_convtr2d_packed_floats(Cin, Cout), dtype=torch.float32, device=DEV)
    wd = w.float().contiguous().to(DEV)  # (kept alive across the call: a temporary's memory may be handed out again at once)
    nat.call("u3d_pack_convtr2d", 0, _stream(DEV), _p(wd), Cin, Cout, mode, _p(out))
    return out


def check_convtr(N, H1, W1, Cin, Cout, seed, tol=TOL):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H1, W1, generator=g)
    x_low = torch.where(torch.rand(N, Cin, H1, W1, generator=g) > 0.3, x.abs() + 0.1, torch.zeros(()))  # a post-ReLU tensor
    w = torch.randn(Cin, Cout, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    Ht, Wt = 2 * H1 - 1, 2 * W1 - 1
    # forward
    t = torch.empty((N, 1, Ht, Wt, Cout), dtype=torch.float32, device=DEV)
    xd, xld, wp0, wp1 = nhwc(x), nhwc(x_low), pack_tr(w, 0), pack_tr(w, 1)
    nat.call("u3d_convtr2d_fwd", 0, _stream(DEV), _p(xd), _p(wp0), _p(t), N, H1, W1, Cin, Cout)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    ref = F.conv_transpose2d(xr, wr, stride=2, padding=1)
    assert ref.shape == (N, Cout, Ht, Wt)
    assert rel(nchw(t), ref.detach()) < tol
    # autograd: dx (unmasked and masked by x_low > 0) and dw
    dt = torch.randn(N, Cout, Ht, Wt, generator=g)
    ref.backward(dt.double())
    dtd = nhwc(dt)
    dx = torch.empty((N, 1, H1, W1, Cin), dtype=torch.float32, device=DEV)
    nat.call("u3d_convtr2d_dgrad", 0, _stream(DEV), _p(dtd), _p(wp1), None, _p(dx), N, H1, W1, Cin, Cout)
    assert rel(nchw(dx), xr.grad) < tol
    nat.call("u3d_convtr2d_dgrad", 0, _stream(DEV), _p(dtd), _p(wp1), _p(xld), _p(dx), N, H1, W1, Cin, Cout)
    assert rel(nchw(dx), xr.grad * (x_low > 0)) < tol
    nws = nat.get_lib().u3d_convtr2d_wgrad_workspace_doubles(Cin, Cout)
    ws = torch.full((nws,), 7.0, dtype=torch.float64, device=DEV)  # (the call zeroes its own scratch)
    dw = torch.empty((Cin, Cout, 3, 3), dtype=torch.float32, device=DEV)
    nat.call("u3d_convtr2d_wgrad", 0, _stream(DEV), _p(xd), _p(dtd), _p(dw), N, H1, W1, Cin, Cout, 0, _p(ws), nws)
    assert rel(dw.cpu(), wr.grad) < tol
    nat.call("u3d_convtr2d_wgrad", 0, _stream(DEV), _p(xd), _p(dtd), _p(dw), N, H1, W1, Cin, Cout, 1, _p(ws), nws)  # accumulate
    assert rel(dw.cpu(), 2 * wr.grad) < tol


@pytest.mark.parametrize("Cin", [1, 3, 5, 64])
@pytest.mark.parametrize("Cout", [1, 3, 5, 64])
def test_convtr2d_channels_and_odd_sizes(Cin, Cout):
    for i, (H1, W1) in enumerate([(1, 1), (1, 6), (5, 1), (7, 4), (16, 11)]):
        check_convtr(2, H1, W1, Cin, Cout, seed=1000 * Cin + 10 * Cout + i)


@pytest.mark.parametrize("N,H1,W1,Cin,Cout", [(2, 16, 16, 1024, 512), (1, 33, 22, 16, 8), (3, 16, 16, 128, 64), (1, 128, 128, 64, 32)])
def test_convtr2d_decoder_shapes(N, H1, W1, Cin, Cout):
    """the bottom of the reference-default U (1024 -> 512 on 16 x 16: few row tiles, K = 1024 per tap) and wider grids"""
    check_convtr(N, H1, W1, Cin, Cout, seed=N + H1 + Cin)


def test_convtr2d_refuses_bad_sizes():
    lib = nat.get_lib()
    assert lib.u3d_convtr2d_packed_floats(0, 4) == 0
    with pytest.raises(Exception, match="2\\^31"):
        x = torch.empty(4, device=DEV)
        nat.call("u3d_convtr2d_fwd", 0, _stream(DEV), _p(x), _p(x), _p(x), 1, 40000, 40000, 1, 1)  # (rejected before any launch)
