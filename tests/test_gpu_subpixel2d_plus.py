"""Decoder levels of a 2-D net that upsample n -> 2n + 1 (`native_2d_subpixel_plus`) through the C-ABI: the windowed sub-pixel kernels of
csrc/u3d_subpix2d.hip (u3d_subpixel2d_conv_fwd_win / _dgrad_win / _wgrad_win), the box launches of csrc/u3d_conv2d.hip on the 2-pixel
slab (u3d_conv2d_box, u3d_conv2d_wgrad_box) and the 2-D forms of the three low-res helpers — against float64 F.conv2d / conv2d_input /
conv2d_weight over F.interpolate(low, size=(2 * H1 + py, 2 * W1 + px), mode="nearest") on the CPU, the data gradient summed over each
low-res cell's children through the nearest index map.  Bars of tests/test_gpu_conv2d.py: TOL for tensors, 1e-5 for the f64 sums."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd._engine_base import slab_boxes
from pytorch3dunet_amd.engine import VSrc, _p, _stream
from test_gpu_conv2d import TOL, affine_table, apply_affine, nchw, nhwc, rel

pytestmark = pytest.mark.gpu
PLUS = [(1, 0), (0, 1), (1, 1)]
SHAPES = [(2, 1, 1, 4, 4),        # output 3 x 3 at most: the slab is most of it
          (2, 1, 5, 8, 24),       # one axis of length 1
          (2, 3, 1, 8, 24),
          (2, 9, 23, 12, 20),     # ragged tiles, channel counts off the 16-channel chunk
          (1, 17, 16, 64, 40)]    # one row past the 16 x 8 forward tile and the 8 x 8 gradient tiles
C0 = 4  # skip channels in front of the packed slice of the (Cout, C0 + C1, 3, 3) weight
I4 = ctypes.c_int * 4


def upn(x, py, px):
    return F.interpolate(x, size=(2 * x.shape[2] + py, 2 * x.shape[3] + px), mode="nearest")


def nearest_map(n_in, n_out):
    """the source index of every output of F.interpolate(mode='nearest') along one axis, taken from the operator itself"""
    return F.interpolate(torch.arange(n_in, dtype=torch.float64).view(1, 1, n_in), size=n_out, mode="nearest").view(-1).long()


def childsum(d, H1, W1):
    """backward of the nearest upsampling: every full-res pixel added to the low-res cell it was copied from"""
    N, C, H, W = d.shape
    rows = torch.zeros(N, C, H1, W, dtype=d.dtype).index_add_(2, nearest_map(H1, H), d)
    return torch.zeros(N, C, H1, W1, dtype=d.dtype).index_add_(3, nearest_map(W1, W), rows)


@functools.lru_cache(maxsize=None)
def case(N, H1, W1, C1, Cout, py, px):
    """inputs and float64 references of one shape, computed once and shared (never modified) by the tests below"""
    g = torch.Generator().manual_seed(1000 * H1 + 10 * W1 + C1 + 7 * py + 3 * px)
    Ct = C0 + C1
    H, W = 2 * H1 + py, 2 * W1 + px
    low = torch.randn(N, C1, H1, W1, generator=g)
    w = torch.randn(Cout, Ct, 3, 3, generator=g) / (3.0 * Ct ** 0.5)
    aff = affine_table(N, Ct, g)
    dz = torch.randn(N, Cout, H, W, generator=g)
    w1 = w[:, C0:].double()
    la = apply_affine(low.double(), aff[:, C0:])
    dlow = childsum(torch.nn.grad.conv2d_input((N, C1, H, W), w1, dz.double(), padding=1), H1, W1)
    return dict(low=low, w=w, aff=aff, dz=dz,
                y_aff=F.conv2d(upn(la, py, px), w1, padding=1), y_plain=F.conv2d(upn(low.double(), py, px), w1, padding=1), dlow=dlow,
                gst=torch.stack((dlow.sum((2, 3)), (dlow * low.double()).sum((2, 3))), -1),
                dw=torch.nn.grad.conv2d_weight(upn(la, py, px), w1.shape, dz.double(), padding=1))


def pack_up(w_d, Cout, Ct, c_off, C1, dgrad):
    lib = nat.get_lib()
    n = lib.u3d_subpixel2d_dgrad_packed_floats(Cout, C1) if dgrad else lib.u3d_subpixel2d_packed_floats(C1, Cout)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    nat.call("u3d_pack_subpixel2d_dgrad_weights" if dgrad else "u3d_pack_subpixel2d_weights", 0, _stream(DEV), _p(w_d), Cout, Ct, c_off, C1,
             _p(out))
    return out


def pack_slice(w_d, Cout, Ct, c_off, Cin, mode):
    out = torch.empty(nat.get_lib().u3d_packed_weight2d_floats(Cin, Cout, mode), dtype=torch.float32, device=DEV)
    nat.call("u3d_pack_weights2d_slice", 0, _stream(DEV), _p(w_d), Cout, Cin, mode, Ct, c_off, _p(out))
    return out


def up_src(low_d, N, H, W, aff_c):
    """the upsampled half alone as a source (C0 = 0) with the compact (N, C1, 2) affine rows; returns (struct, what it points at)"""
    dummy = torch.zeros((N, 1, H, W, 4), dtype=torch.float32, device=DEV)
    v = VSrc(dummy, low_d)
    return v.up_only_struct(aff_c), (v, dummy, aff_c)


def plus_fwd(low_d, aff_d, w_d, N, H1, W1, c_off, C1, Cout, py, px):
    """window launch + slab boxes on channels [c_off, c_off + C1) of the weight; aff_d: the (N, Ct, 2) table of the whole layer or None"""
    Ct = w_d.shape[1]
    H, W = 2 * H1 + py, 2 * W1 + px
    out = torch.full((N, 1, H, W, Cout), float("nan"), dtype=torch.float32, device=DEV)
    rows = aff_d.view(-1)[2 * c_off:] if aff_d is not None else None
    wpu = pack_up(w_d, Cout, Ct, c_off, C1, 0)
    nat.call("u3d_subpixel2d_conv_fwd_win", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(wpu), _p(out), N, H1, W1, C1, Cout,
             I4(H, W, py, px))
    s_up, keep = up_src(low_d, N, H, W, aff_d[:, c_off:c_off + C1].contiguous() if aff_d is not None else None)
    wp = pack_slice(w_d, Cout, Ct, c_off, C1, 0)
    for b in slab_boxes((1, H, W), (0, py, px), 2):
        nat.call("u3d_conv2d_box", 0, _stream(DEV), ctypes.byref(s_up), _p(wp), _p(out), N, H, W, Cout, I4(b[1], b[2], b[4], b[5]), None, None)
    torch.cuda.synchronize()
    return out


def plus_dgrad(dz_d, low_d, w_d, N, H1, W1, c_off, C1, Cout, py, px, reps):
    """window + slab (a scratch the size of each box) + child-sum"""
    Ct = w_d.shape[1]
    H, W = 2 * H1 + py, 2 * W1 + px
    dlow = torch.full((N, 1, H1, W1, C1), float("nan"), dtype=torch.float32, device=DEV)
    gst = torch.zeros(reps * N * C1 * 2, dtype=torch.float64, device=DEV)
    wpu = pack_up(w_d, Cout, Ct, c_off, C1, 1)
    nat.call("u3d_subpixel2d_conv_dgrad_win", 0, _stream(DEV), _p(dz_d), _p(wpu), _p(low_d), _p(dlow), _p(gst), N, H1, W1, C1, Cout, reps,
             (ctypes.c_int * 6)(H, W, py, px, py, px))
    s_dz = VSrc(dz_d).struct()
    wp = pack_slice(w_d, Cout, Ct, c_off, C1, 1)
    mask = (ctypes.c_int * 2)(2 * py, 2 * px)
    for b in slab_boxes((1, H, W), (0, py, px), 3):
        y0, x0, y1, x1 = b[1], b[2], b[4], b[5]
        dv = torch.full((N, y1 - y0, x1 - x0, C1), float("nan"), dtype=torch.float32, device=DEV)
        nat.call("u3d_conv2d_box", 0, _stream(DEV), ctypes.byref(s_dz), _p(wp), _p(dv), N, H, W, C1, I4(y0, x0, y1, x1), mask,
                 I4(y1 - y0, x1 - x0, y0, x0))
        nat.call("u3d_nearest_childsum_add2d", 0, _stream(DEV), _p(dv), _p(low_d), _p(dlow), _p(gst), N, H1, W1, C1, py, px,
                 I4(y0, x0, y1, x1))
    torch.cuda.synchronize()
    return dlow, gst


def plus_wgrad(low_d, aff_d, dz_d, dw_buf, N, H1, W1, c_off, C1, Cout, py, px):
    """window + slab boxes into channels [c_off, c_off + C1) of dw_buf (Cout, Ct, 3, 3); aff_d: (N, Ct, 2) of dw_buf's channels"""
    Ct = dw_buf.shape[1]
    H, W = 2 * H1 + py, 2 * W1 + px
    lib = nat.get_lib()
    need = lib.u3d_subpixel2d_wgrad_workspace_floats(N, H1, W1, C1, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    nat.call("u3d_subpixel2d_conv_wgrad_win", 0, _stream(DEV), _p(low_d), _p(aff_d.view(-1)[2 * c_off:]), Ct * 2, _p(dz_d),
             _p(dw_buf.view(-1)[c_off * 9:]), Ct, N, H1, W1, C1, Cout, _p(ws), need, (ctypes.c_int * 6)(H, W, py, px, py, px))
    s_up, keep = up_src(low_d, N, H, W, aff_d[:, c_off:c_off + C1].contiguous())
    for b in slab_boxes((1, H, W), (0, py, px), 2):
        need = lib.u3d_wgrad2d_workspace_floats(N, b[4] - b[1], b[5] - b[2], C1, Cout)
        ws2 = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
        tmp = torch.full((Cout, C1, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
        nat.call("u3d_conv2d_wgrad_box", 0, _stream(DEV), ctypes.byref(s_up), _p(dz_d), _p(tmp), N, H, W, Cout, _p(ws2), need,
                 I4(b[1], b[2], b[4], b[5]))
        dw_buf[:, c_off:c_off + C1] += tmp
    torch.cuda.synchronize()


@pytest.mark.parametrize("py,px", PLUS)
@pytest.mark.parametrize("N,H1,W1,C1,Cout", SHAPES)
def test_forward(N, H1, W1, C1, Cout, py, px):
    c = case(N, H1, W1, C1, Cout, py, px)
    low_d, w_d = nhwc(c["low"]), c["w"].contiguous().to(DEV)
    # a per-sample affine with b != 0: the border shows whether padding stayed exactly 0 after it
    y = plus_fwd(low_d, c["aff"].to(DEV), w_d, N, H1, W1, C0, C1, Cout, py, px)
    e = rel(nchw(y), c["y_aff"])
    print(f"fwd affine {e:.2e}")
    assert e < TOL
    y = plus_fwd(low_d, None, w_d, N, H1, W1, C0, C1, Cout, py, px)
    e = rel(nchw(y), c["y_plain"])
    print(f"fwd plain {e:.2e}")
    assert e < TOL


@pytest.mark.parametrize("py,px", PLUS)
@pytest.mark.parametrize("N,H1,W1,C1,Cout", SHAPES)
def test_data_gradient_and_its_sums(N, H1, W1, C1, Cout, py, px):
    c = case(N, H1, W1, C1, Cout, py, px)
    low_d, w_d, dz_d = nhwc(c["low"]), c["w"].contiguous().to(DEV), nhwc(c["dz"])
    dlow1, g1 = plus_dgrad(dz_d, low_d, w_d, N, H1, W1, C0, C1, Cout, py, px, 1)
    e, es = rel(nchw(dlow1), c["dlow"]), rel(g1.view(N, C1, 2).cpu(), c["gst"])
    print(f"dgrad {e:.2e} sums {es:.2e}")
    assert e < TOL and es < 1e-5
    dlow8, g8 = plus_dgrad(dz_d, low_d, w_d, N, H1, W1, C0, C1, Cout, py, px, 8)
    assert torch.equal(dlow1, dlow8)
    assert rel(g8.view(8, N, C1, 2).sum(0).cpu(), c["gst"]) < 1e-5  # the replica rows sum to the same table


@pytest.mark.parametrize("py,px", PLUS)
@pytest.mark.parametrize("N,H1,W1,C1,Cout", SHAPES)
def test_weight_gradient_slice_is_deterministic(N, H1, W1, C1, Cout, py, px):
    c = case(N, H1, W1, C1, Cout, py, px)
    low_d, dz_d, aff_d = nhwc(c["low"]), nhwc(c["dz"]), c["aff"].to(DEV)
    Ct = C0 + C1 + 4  # (channels on both sides of the slice)
    aff_w = torch.zeros(N, Ct, 2, device=DEV)
    aff_w[:, C0:C0 + C1] = aff_d[:, C0:]
    bufs = []
    for _ in range(2):
        dw = torch.full((Cout, Ct, 3, 3), 7.5, dtype=torch.float32, device=DEV)
        plus_wgrad(low_d, aff_w, dz_d, dw, N, H1, W1, C0, C1, Cout, py, px)
        bufs.append(dw)
    a = bufs[0].cpu()
    e = rel(a[:, C0:C0 + C1], c["dw"])
    print(f"wgrad {e:.2e}")
    assert e < TOL
    assert torch.all(a[:, :C0] == 7.5) and torch.all(a[:, C0 + C1:] == 7.5)  # the other channels are untouched
    assert torch.equal(bufs[0], bufs[1])  # bitwise


@pytest.mark.parametrize("hs,ws,hl,wl,C0_,C1", [(17, 16, 8, 8, 16, 32), (19, 47, 9, 23, 8, 12)])
def test_composition_with_the_skip_half(hs, ws, hl, wl, C0_, C1):
    """the pair (windowed sub-pixel upsampled half + slab, skip half on the conv2d kernels) reproduces the references of
    test_gpu_conv2d.py::test_conv2d_virtual_concat: y with ReLU, the full dw, the GroupNorm-backward sums of both halves"""
    py, px = hs - 2 * hl, ws - 2 * wl
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
    # forward: partial sums of the upsampled half, then the skip half adds them before ReLU / statistics
    part = plus_fwd(low_d, aff_d, w_d, N, hl, wl, C0_, C1, Cout, py, px)
    y = torch.empty((N, 1, hs, ws, Cout), dtype=torch.float32, device=DEV)
    st = torch.zeros(N * Cout * 2, dtype=torch.float64, device=DEV)
    s0 = VSrc(skip_d).struct(a0)
    need = lib.u3d_conv2d_workspace_floats(N, hs, ws, C0_, Cout)
    kws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    wp0, wp1 = pack_slice(w_d, Cout, Ct, 0, C0_, 0), pack_slice(w_d, Cout, Ct, 0, C0_, 1)
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
    dlow, gst1 = plus_dgrad(dz_d, low_d, w_d, N, hl, wl, C0_, C1, Cout, py, px, 1)
    assert rel(nchw(dg0), dg_ref[:, :C0_]) < TOL
    assert rel(nchw(dlow), childsum(dg_ref[:, C0_:], hl, wl)) < TOL
    gst = torch.cat((gst0.view(N, C0_, 2), gst1.view(N, C1, 2)), dim=1).cpu()
    assert rel(gst, g_ref) < 1e-5
    # weight gradient: the two channel slices of one (Cout, Ct, 3, 3) buffer
    dw = torch.full((Cout, Ct, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    plus_wgrad(low_d, aff_d, dz_d, dw, N, hl, wl, C0_, C1, Cout, py, px)
    need = lib.u3d_wgrad2d_workspace_floats(N, hs, ws, C0_, Cout)
    ws_ = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_wgrad_strided", 0, _stream(DEV), ctypes.byref(s0), _p(dz_d), _p(dw), Ct, N, hs, ws, Cout, _p(ws_), need)
    assert rel(dw.cpu(), dw_ref) < TOL


def test_window_of_zeros_is_the_exact_2x_entry_point_bitwise():
    N, H1, W1, C1, Cout = 2, 9, 23, 12, 20
    g = torch.Generator().manual_seed(77)
    Ct = C0 + C1
    low_d = nhwc(torch.randn(N, C1, H1, W1, generator=g))
    w_d = (torch.randn(Cout, Ct, 3, 3, generator=g) / (3.0 * Ct ** 0.5)).to(DEV)
    aff_d = affine_table(N, Ct, g).to(DEV)
    dz_d = nhwc(torch.randn(N, Cout, 2 * H1, 2 * W1, generator=g))
    rows = aff_d.view(-1)[2 * C0:]
    lib = nat.get_lib()
    H, W = 2 * H1, 2 * W1
    # forward
    wp = pack_up(w_d, Cout, Ct, C0, C1, 0)
    ya = torch.full((N, 1, H, W, Cout), float("nan"), dtype=torch.float32, device=DEV)
    yb = torch.full_like(ya, float("nan"))
    nat.call("u3d_subpixel2d_conv_fwd", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(wp), _p(ya), N, H1, W1, C1, Cout, None, 0)
    nat.call("u3d_subpixel2d_conv_fwd_win", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(wp), _p(yb), N, H1, W1, C1, Cout, I4(H, W, 0, 0))
    assert not torch.isnan(ya).any() and torch.equal(ya, yb)
    # data gradient (one replica row: the f64 atomics of several blocks per channel are added in no fixed order)
    wpd = pack_up(w_d, Cout, Ct, C0, C1, 1)
    da = torch.full((N, 1, H1, W1, C1), float("nan"), dtype=torch.float32, device=DEV)
    db = torch.full_like(da, float("nan"))
    ga = torch.zeros(N * C1 * 2, dtype=torch.float64, device=DEV)
    gb = torch.zeros_like(ga)
    nat.call("u3d_subpixel2d_conv_dgrad_reps", 0, _stream(DEV), _p(dz_d), _p(wpd), _p(low_d), _p(da), _p(ga), N, H1, W1, C1, Cout, 1)
    nat.call("u3d_subpixel2d_conv_dgrad_win", 0, _stream(DEV), _p(dz_d), _p(wpd), _p(low_d), _p(db), _p(gb), N, H1, W1, C1, Cout, 1,
             (ctypes.c_int * 6)(H, W, 0, 0, 0, 0))
    assert not torch.isnan(da).any() and torch.equal(da, db)
    assert rel(gb.cpu(), ga.cpu()) < 1e-12
    # weight gradient
    need = lib.u3d_subpixel2d_wgrad_workspace_floats(N, H1, W1, C1, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    wa = torch.full((Cout, Ct, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    wb = torch.full_like(wa, float("nan"))
    nat.call("u3d_subpixel2d_conv_wgrad", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(dz_d), _p(wa.view(-1)[C0 * 9:]), Ct, N, H1, W1, C1,
             Cout, _p(ws), need)
    nat.call("u3d_subpixel2d_conv_wgrad_win", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(dz_d), _p(wb.view(-1)[C0 * 9:]), Ct, N, H1, W1,
             C1, Cout, _p(ws), need, (ctypes.c_int * 6)(H, W, 0, 0, 0, 0))
    torch.cuda.synchronize()
    assert not torch.isnan(wa[:, C0:]).any() and torch.equal(wa[:, C0:], wb[:, C0:])


@pytest.mark.parametrize("N,H,W,Cin,Cout,box", [(2, 5, 6, 8, 4, (0, 0, 2, 6)),        # rows [0, 2)
                                                (1, 35, 29, 12, 20, (2, 0, 35, 2))])  # columns [0, 2) from row 2
def test_box_kernels_alone(N, H, W, Cin, Cout, box):
    g = torch.Generator().manual_seed(H * 10 + Cin)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    aff = affine_table(N, Cin, g)
    dz = torch.randn(N, Cout, H, W, generator=g)
    xa = apply_affine(x.double(), aff)
    y0, x0, y1, x1 = box
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[y0:y1, x0:x1] = True
    x_d, w_d, aff_d, dz_d = nhwc(x), w.contiguous().to(DEV), aff.to(DEV), nhwc(dz)
    s = VSrc(x_d).struct(aff_d)
    # forward: the box region is the convolution, everything else is untouched
    out = torch.full((N, 1, H, W, Cout), float("nan"), dtype=torch.float32, device=DEV)
    wp = pack_slice(w_d, Cout, Cin, 0, Cin, 0)
    nat.call("u3d_conv2d_box", 0, _stream(DEV), ctypes.byref(s), _p(wp), _p(out), N, H, W, Cout, I4(*box), None, None)
    y = nchw(out)
    y_ref = F.conv2d(xa, w.double(), padding=1)
    assert rel(y[:, :, inside], y_ref[:, :, inside]) < TOL
    assert torch.isnan(y[:, :, ~inside]).all()
    # ... into a scratch the size of the box
    small = torch.full((N, y1 - y0, x1 - x0, Cout), float("nan"), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_box", 0, _stream(DEV), ctypes.byref(s), _p(wp), _p(small), N, H, W, Cout, I4(*box), None,
             I4(y1 - y0, x1 - x0, y0, x0))
    assert torch.equal(small.cpu(), out[:, 0, y0:y1, x0:x1].cpu())
    # weight gradient: the sum over the box's dz pixels
    need = nat.get_lib().u3d_wgrad2d_workspace_floats(N, y1 - y0, x1 - x0, Cin, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_wgrad_box", 0, _stream(DEV), ctypes.byref(s), _p(dz_d), _p(dw), N, H, W, Cout, _p(ws), need, I4(*box))
    dw_ref = torch.nn.grad.conv2d_weight(xa, w.shape, dz.double() * inside, padding=1)
    assert rel(dw.cpu(), dw_ref) < TOL


def test_low_res_helpers_2d_form():
    """children = (2 + [y == 0]) (2 + [x == 0]) — one along the z axis a 2-D tensor does not have — against a direct f64 evaluation"""
    N, H1, W1, C = 2, 3, 5, 8
    ey = ex = 1
    H, W = 2 * H1 + ey, 2 * W1 + ex
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H1, W1, generator=g)
    cnt = ((2.0 + (torch.arange(H1) == 0).double()).view(H1, 1) * (2.0 + (torch.arange(W1) == 0).double()).view(1, W1))
    x_d = nhwc(x)
    # u3d_chan_stats_children2d
    st = torch.zeros(N * C * 2, dtype=torch.float64, device=DEV)
    nat.call("u3d_chan_stats_children2d", 0, _stream(DEV), _p(x_d), N, H1, W1, C, ey, ex, _p(st))
    ref = torch.stack(((cnt * x.double()).sum((2, 3)), (cnt * x.double() ** 2).sum((2, 3))), -1)
    assert rel(st.view(N, C, 2).cpu(), ref) < 1e-5
    up = upn(x.double(), ey, ex)  # (the same sums over the upsampled image itself)
    assert rel(ref, torch.stack((up.sum((2, 3)), (up * up).sum((2, 3))), -1)) < 1e-12
    # u3d_gn_bwd_apply_children2d on channels [4, 12) of a 16-channel coefficient table, with the ReLU mask
    Ctot, coff = 16, 4
    dlow = torch.randn(N, C, H1, W1, generator=g)
    coef = torch.randn(N, 3, Ctot, generator=g)
    out = torch.full((N, 1, H1, W1, C), float("nan"), dtype=torch.float32, device=DEV)
    dlow_d, coef_d = nhwc(dlow), coef.to(DEV)  # (held: _p keeps only the pointer)
    nat.call("u3d_gn_bwd_apply_children2d", 0, _stream(DEV), _p(dlow_d), _p(x_d), _p(coef_d), Ctot, coff, N, H1, W1, C, ey, ex, 1, _p(out))
    p, q, r = (coef[:, k, coff:coff + C].double()[:, :, None, None] for k in range(3))
    ref = (p * dlow.double() + cnt * (q * x.double() + r)) * (x > 0)
    assert rel(nchw(out), ref) < TOL
    # u3d_nearest_childsum_add2d over the two boxes the slab's data gradient reaches
    dv = torch.randn(N, C, H, W, generator=g)
    d0 = torch.randn(N, C, H1, W1, generator=g)
    d_d = nhwc(d0)
    gst = torch.zeros(N * C * 2, dtype=torch.float64, device=DEV)
    covered = torch.zeros(H, W, dtype=torch.bool)
    for b in slab_boxes((1, H, W), (0, ey, ex), 3):
        y0, x0, y1, x1 = b[1], b[2], b[4], b[5]
        covered[y0:y1, x0:x1] = True
        dv_d = dv[:, :, y0:y1, x0:x1].permute(0, 2, 3, 1).contiguous().to(DEV)
        nat.call("u3d_nearest_childsum_add2d", 0, _stream(DEV), _p(dv_d), _p(x_d), _p(d_d), _p(gst), N, H1, W1, C, ey, ex, I4(y0, x0, y1, x1))
    torch.cuda.synchronize()
    add = childsum(dv.double() * covered, H1, W1)
    assert rel(nchw(d_d), d0.double() + add) < TOL
    assert rel(gst.view(N, C, 2).cpu(), torch.stack((add.sum((2, 3)), (add * x.double()).sum((2, 3))), -1)) < 1e-5
