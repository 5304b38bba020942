"""The sub-pixel decoder kernels of csrc/u3d_subpix2d.hip through the C-ABI (`native_2d_subpixel`): forward, low-res data gradient and
weight gradient of the upsampled half of a decoder's first Conv2d, alone and together with the skip half on the kernels of
csrc/u3d_conv2d.hip — against float64 F.conv2d / conv2d_input / conv2d_weight over the nearest-upsampled tensor on the CPU, with the
bars of tests/test_gpu_conv2d.py (TOL for tensors, 1e-5 for the f64 sums)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import VSrc, _p, _stream
from test_gpu_conv2d import TOL, affine_table, apply_affine, nchw, nhwc, rel

pytestmark = pytest.mark.gpu
SHAPES = [(2, 1, 1, 4, 4),        # all border
          (2, 1, 3, 8, 24),
          (2, 9, 23, 12, 20),     # ragged tiles, channel counts off the chunk
          (1, 17, 16, 64, 40),    # one row past a tile
          (1, 8, 8, 256, 128)]    # fewer blocks than CUs (no split-K form: the workspace is not used)
C0 = 4  # skip channels in front of the packed slice of the (Cout, C0 + C1, 3, 3) weight


def up2(x):
    return F.interpolate(x, size=(2 * x.shape[2], 2 * x.shape[3]), mode="nearest")


def childsum(d):
    N, C, H, W = d.shape
    return d.view(N, C, H // 2, 2, W // 2, 2).sum((3, 5))


@functools.lru_cache(maxsize=None)
def case(N, H1, W1, C1, Cout):
    """inputs and float64 references of one shape, computed once and shared (never modified) by the tests below"""
    g = torch.Generator().manual_seed(1000 * H1 + 10 * W1 + C1)
    Ct = C0 + C1
    low = torch.randn(N, C1, H1, W1, generator=g)
    w = torch.randn(Cout, Ct, 3, 3, generator=g) / (3.0 * Ct ** 0.5)
    aff = affine_table(N, Ct, g)
    dz = torch.randn(N, Cout, 2 * H1, 2 * W1, generator=g)
    w1 = w[:, C0:].double()
    la = apply_affine(low.double(), aff[:, C0:])
    dup = torch.nn.grad.conv2d_input((N, C1, 2 * H1, 2 * W1), w1, dz.double(), padding=1)
    dlow = childsum(dup)
    return dict(low=low, w=w, aff=aff, dz=dz,
                y_aff=F.conv2d(up2(la), w1, padding=1), y_plain=F.conv2d(up2(low.double()), w1, padding=1), dlow=dlow,
                gst=torch.stack((dlow.sum((2, 3)), (dlow * low.double()).sum((2, 3))), -1),
                dw=torch.nn.grad.conv2d_weight(up2(la), w1.shape, dz.double(), padding=1))


def pack_up(w_d, Cout, Ct, c_off, C1, dgrad):
    lib = nat.get_lib()
    n = lib.u3d_subpixel2d_dgrad_packed_floats(Cout, C1) if dgrad else lib.u3d_subpixel2d_packed_floats(C1, Cout)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    nat.call("u3d_pack_subpixel2d_dgrad_weights" if dgrad else "u3d_pack_subpixel2d_weights", 0, _stream(DEV), _p(w_d), Cout, Ct, c_off, C1,
             _p(out))
    return out


def up_fwd(low_d, aff_d, w_d, N, H1, W1, c_off, C1, Cout):
    """u3d_subpixel2d_conv_fwd on channels [c_off, c_off + C1) of the weight; aff_d: the (N, Ct, 2) table of the whole layer or None"""
    Ct = w_d.shape[1]
    wp = pack_up(w_d, Cout, Ct, c_off, C1, 0)
    out = torch.full((N, 1, 2 * H1, 2 * W1, Cout), float("nan"), dtype=torch.float32, device=DEV)
    rows = aff_d.view(-1)[2 * c_off:] if aff_d is not None else None
    nat.call("u3d_subpixel2d_conv_fwd", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(wp), _p(out), N, H1, W1, C1, Cout, None, 0)
    return out


def up_dgrad(dz_d, low_d, w_d, N, H1, W1, c_off, C1, Cout, reps):
    wp = pack_up(w_d, Cout, w_d.shape[1], c_off, C1, 1)
    dlow = torch.full((N, 1, H1, W1, C1), float("nan"), dtype=torch.float32, device=DEV)
    gst = torch.zeros(reps * N * C1 * 2, dtype=torch.float64, device=DEV)
    nat.call("u3d_subpixel2d_conv_dgrad_reps", 0, _stream(DEV), _p(dz_d), _p(wp), _p(low_d), _p(dlow), _p(gst), N, H1, W1, C1, Cout, reps)
    return dlow, gst


def up_wgrad(low_d, aff_d, dz_d, dw_buf, N, H1, W1, c_off, C1, Cout):
    """u3d_subpixel2d_conv_wgrad into channels [c_off, c_off + C1) of dw_buf (Cout, Ct, 3, 3)"""
    Ct = dw_buf.shape[1]
    need = nat.get_lib().u3d_subpixel2d_wgrad_workspace_floats(N, H1, W1, C1, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    rows = aff_d.view(-1)[2 * c_off:] if aff_d is not None else None
    nat.call("u3d_subpixel2d_conv_wgrad", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(dz_d), _p(dw_buf.view(-1)[c_off * 9:]), Ct, N, H1,
             W1, C1, Cout, _p(ws), need)


@pytest.mark.parametrize("N,H1,W1,C1,Cout", SHAPES)
def test_forward(N, H1, W1, C1, Cout):
    c = case(N, H1, W1, C1, Cout)
    low_d, w_d = nhwc(c["low"]), c["w"].contiguous().to(DEV)
    # a per-sample affine with b != 0: the border shows whether padding stayed exactly 0 after it
    y = up_fwd(low_d, c["aff"].to(DEV), w_d, N, H1, W1, C0, C1, Cout)
    e = rel(nchw(y), c["y_aff"])
    print(f"fwd affine {e:.2e}")
    assert e < TOL
    y = up_fwd(low_d, None, w_d, N, H1, W1, C0, C1, Cout)
    e = rel(nchw(y), c["y_plain"])
    print(f"fwd plain {e:.2e}")
    assert e < TOL


def test_forward_padding_stays_zero_after_affine():
    N, H1, W1, C1, Cout = 1, 3, 5, 16, 4
    low = torch.zeros(N, C1, H1, W1)
    aff = torch.stack((torch.ones(N, C1), torch.full((N, C1), 3.0)), -1).contiguous()
    w = torch.ones(Cout, C1, 3, 3)
    y = up_fwd(nhwc(low), aff.to(DEV), w.to(DEV), N, H1, W1, 0, C1, Cout)
    ref = F.conv2d(torch.full((N, C1, 2 * H1, 2 * W1), 3.0, dtype=torch.float64), w.double(), padding=1)
    assert torch.equal(nchw(y).double(), ref)


@pytest.mark.parametrize("N,H1,W1,C1,Cout", SHAPES)
def test_data_gradient_and_its_sums(N, H1, W1, C1, Cout):
    c = case(N, H1, W1, C1, Cout)
    low_d, w_d, dz_d = nhwc(c["low"]), c["w"].contiguous().to(DEV), nhwc(c["dz"])
    dlow1, g1 = up_dgrad(dz_d, low_d, w_d, N, H1, W1, C0, C1, Cout, 1)
    e, es = rel(nchw(dlow1), c["dlow"]), rel(g1.view(N, C1, 2).cpu(), c["gst"])
    print(f"dgrad {e:.2e} sums {es:.2e}")
    assert e < TOL and es < 1e-5
    dlow8, g8 = up_dgrad(dz_d, low_d, w_d, N, H1, W1, C0, C1, Cout, 8)
    assert torch.equal(dlow1, dlow8)
    assert rel(g8.view(8, -1).sum(0).cpu(), g1.cpu()) < 1e-12  # the replica rows sum to the one-table result


@pytest.mark.parametrize("N,H1,W1,C1,Cout", SHAPES)
def test_weight_gradient_slice_is_deterministic(N, H1, W1, C1, Cout):
    c = case(N, H1, W1, C1, Cout)
    low_d, dz_d, aff_d = nhwc(c["low"]), nhwc(c["dz"]), c["aff"].to(DEV)
    Ct = C0 + C1 + 4  # (channels on both sides of the slice)
    aff_w = torch.zeros(N, Ct, 2, device=DEV)
    aff_w[:, C0:C0 + C1] = aff_d[:, C0:]
    bufs = []
    for _ in range(2):
        dw = torch.full((Cout, Ct, 3, 3), 7.5, dtype=torch.float32, device=DEV)
        up_wgrad(low_d, aff_w, dz_d, dw, N, H1, W1, C0, C1, Cout)
        bufs.append(dw)
    a = bufs[0].cpu()
    e = rel(a[:, C0:C0 + C1], c["dw"])
    print(f"wgrad {e:.2e}")
    assert e < TOL
    assert torch.all(a[:, :C0] == 7.5) and torch.all(a[:, C0 + C1:] == 7.5)  # the other channels are untouched
    assert torch.equal(bufs[0], bufs[1])  # bitwise


@pytest.mark.parametrize("hs,ws,hl,wl,C0_,C1", [(16, 16, 8, 8, 16, 32), (18, 46, 9, 23, 8, 12)])
def test_composition_with_the_skip_half(hs, ws, hl, wl, C0_, C1):
    """the pair (sub-pixel upsampled half, skip half on the conv2d kernels) reproduces the references of
    test_gpu_conv2d.py::test_conv2d_virtual_concat: y with ReLU, the full dw, the GroupNorm-backward sums of both halves"""
    g = torch.Generator().manual_seed(hs * 100 + C1)
    N, Cout = 2, 24
    skip = torch.randn(N, C0_, hs, ws, generator=g)
    low = torch.randn(N, C1, hl, wl, generator=g)
    cat = torch.cat((skip, F.interpolate(low, size=(hs, ws), mode="nearest")), dim=1)
    Ct = C0_ + C1
    w = torch.randn(Cout, Ct, 3, 3, generator=g) / (3.0 * Ct ** 0.5)
    aff = affine_table(N, Ct, g)
    ca = apply_affine(cat.double(), aff)
    dz = torch.randn(N, Cout, hs, ws, generator=g)
    y_ref = F.conv2d(ca, w.double(), padding=1).clamp_min(0)
    dg_ref = torch.nn.grad.conv2d_input(ca.shape, w.double(), dz.double(), padding=1)
    g_ref = torch.stack((dg_ref.sum((2, 3)), (dg_ref * cat.double()).sum((2, 3))), -1)
    dw_ref = torch.nn.grad.conv2d_weight(ca, w.shape, dz.double(), padding=1)
    lib = nat.get_lib()
    skip_d, low_d, w_d, aff_d, dz_d = nhwc(skip), nhwc(low), w.contiguous().to(DEV), aff.to(DEV), nhwc(dz)
    a0 = aff_d[:, :C0_].contiguous()

    def pack_skip(mode):
        out = torch.empty(lib.u3d_packed_weight2d_floats(C0_, Cout, mode), dtype=torch.float32, device=DEV)
        nat.call("u3d_pack_weights2d_slice", 0, _stream(DEV), _p(w_d), Cout, C0_, mode, Ct, 0, _p(out))
        return out

    # forward: partial sums of the upsampled half, then the skip half adds them before ReLU / statistics
    part = up_fwd(low_d, aff_d, w_d, N, hl, wl, C0_, C1, Cout)
    y = torch.empty((N, 1, hs, ws, Cout), dtype=torch.float32, device=DEV)
    st = torch.zeros(N * Cout * 2, dtype=torch.float64, device=DEV)
    s0 = VSrc(skip_d).struct(a0)
    need = lib.u3d_conv2d_workspace_floats(N, hs, ws, C0_, Cout)
    kws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    wp0, wp1 = pack_skip(0), pack_skip(1)
    nat.call("u3d_conv2d_res_reps", 0, _stream(DEV), ctypes.byref(s0), _p(wp0), _p(y), N, hs, ws, Cout, 1, _p(st), None, None,
             _p(kws) if need else None, need, 1, _p(part))
    assert rel(nchw(y), y_ref) < TOL
    assert rel(st.view(N, Cout, 2).cpu(), torch.stack((y_ref.sum((2, 3)), (y_ref * y_ref).sum((2, 3))), -1)) < 1e-5
    # data gradient: skip half at full resolution (mode-1 image of its channels), upsampled half at low resolution
    dg0 = torch.empty((N, 1, hs, ws, C0_), dtype=torch.float32, device=DEV)
    gst0 = torch.zeros(N * C0_ * 2, dtype=torch.float64, device=DEV)
    s_dz, s_x0 = VSrc(dz_d).struct(), VSrc(skip_d).struct()
    need = lib.u3d_conv2d_workspace_floats(N, hs, ws, Cout, C0_)
    kws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_ex_reps", 0, _stream(DEV), ctypes.byref(s_dz), _p(wp1), _p(dg0), N, hs, ws, C0_, 0, None,
             ctypes.byref(s_x0), _p(gst0), _p(kws) if need else None, need, 1)
    dlow, gst1 = up_dgrad(dz_d, low_d, w_d, N, hl, wl, C0_, C1, Cout, 1)
    assert rel(nchw(dg0), dg_ref[:, :C0_]) < TOL
    assert rel(nchw(dlow), childsum(dg_ref[:, C0_:])) < TOL
    gst = torch.cat((gst0.view(N, C0_, 2), gst1.view(N, C1, 2)), dim=1).cpu()
    assert rel(gst, g_ref) < 1e-5
    # weight gradient: the two channel slices of one (Cout, Ct, 3, 3) buffer
    dw = torch.full((Cout, Ct, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    up_wgrad(low_d, aff_d, dz_d, dw, N, hl, wl, C0_, C1, Cout)
    need = lib.u3d_wgrad2d_workspace_floats(N, hs, ws, C0_, Cout)
    ws_ = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_wgrad_strided", 0, _stream(DEV), ctypes.byref(s0), _p(dz_d), _p(dw), Ct, N, hs, ws, Cout, _p(ws_), need)
    assert rel(dw.cpu(), dw_ref) < TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 40, 37, 16, 32), (1, 5, 6, 8, 4), (4, 96, 80, 48, 40)])
def test_strided_skip_weight_gradient_equals_the_plain_one_bitwise(N, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(N + H + Cin)
    x, dz = nhwc(torch.randn(N, Cin, H, W, generator=g)), nhwc(torch.randn(N, Cout, H, W, generator=g))
    aff = affine_table(N, Cin, g).to(DEV)
    need = nat.get_lib().u3d_wgrad2d_workspace_floats(N, H, W, Cin, Cout)
    ws_ = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    s = VSrc(x).struct(aff)
    a = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=DEV)
    b = torch.empty_like(a)
    nat.call("u3d_conv2d_wgrad", 0, _stream(DEV), ctypes.byref(s), _p(dz), _p(a), N, H, W, Cout, _p(ws_), need)
    nat.call("u3d_conv2d_wgrad_strided", 0, _stream(DEV), ctypes.byref(s), _p(dz), _p(b), Cin, N, H, W, Cout, _p(ws_), need)
    assert torch.equal(a, b)
