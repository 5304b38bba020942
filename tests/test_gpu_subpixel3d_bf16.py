"""-m gpu: the sub-pixel bf16 decoder kernels of csrc/u3d_subpix_bf16.hip through the C-ABI (`bf16_subpixel`): forward, low-res data
gradient and weight gradient of the upsampled half of a decoder's first Conv3d on v_mfma_f32_32x32x16_bf16, the two slice helpers of the
skip half (csrc/u3d_bf16.hip), and the composition of both halves — against float64 on the CPU over the SAME bf16-rounded operands
(tests/bf16_emul_3d_subpixel.py: pre-summed taps added in fp32 and rounded once, activations / dz rounded once after the fp32 affine).

Bars: the project's own from tests/test_gpu_conv2d_bf16.py, relative to the result's range — identical operands 1e-4, a random affine
1e-3, against the un-rounded operands 2e-2 (the emulation itself was checked against that bar on the CPU at these shapes: at most 4.1e-3);
gstats against float64 sums of the written dlow 1e-6 of the table's maximum."""
import functools

import pytest
import torch
import torch.nn.functional as F

import bf16_emul_3d_subpixel as SE
from gpu_utils import DEV, ncdhw, ndhwc
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import _p, _stream
from test_gpu_conv2d_bf16 import TOL_AFF, TOL_EXACT, TOL_SAME, r16, rel

pytestmark = pytest.mark.gpu
TOL_GSTATS = 1e-6
U3D_EINVAL = -1  # include/u3d.h

# (N, D1, H1, W1, C1, Cout); tiles: forward / data gradient 4 x 4 x 8 low-res voxels, weight gradient 2 x 4 x 16
SHAPES = [(2, 1, 1, 1, 32, 32),      # all border
          (1, 2, 3, 5, 32, 64),      # below a tile
          (1, 5, 9, 11, 96, 32),     # ragged on all axes, six chunks
          (1, 3, 17, 9, 32, 96),     # odd n-tile count
          (1, 3, 5, 17, 64, 64)]     # several blocks in every kernel; weight gradient: 8 tiles, more than one slot
MULTI_SLOT = SHAPES[-1]
C0 = 32  # skip channels in front of the packed slice of the (Cout, C0 + C1, 3, 3, 3) weight


def up2(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def childsum(d):
    N, C, D, H, W = d.shape
    return d.view(N, C, D // 2, 2, H // 2, 2, W // 2, 2).sum((3, 5, 7))


def border(t):
    m = torch.zeros(t.shape[-3:], dtype=torch.bool)
    m[:2] = m[-2:] = True
    m[:, :2] = m[:, -2:] = True
    m[:, :, :2] = m[:, :, -2:] = True
    return t[..., m]


@functools.lru_cache(maxsize=None)
def case(N, D1, H1, W1, C1, Cout):
    """inputs and float64 references of one shape, computed once and shared (never modified) by the tests below"""
    g = torch.Generator().manual_seed(3000 + 1000 * D1 + 100 * H1 + 10 * W1 + C1 + Cout)
    Ct = C0 + C1
    low = torch.randn(N, C1, D1, H1, W1, generator=g)
    w = torch.randn(Cout, Ct, 3, 3, 3, generator=g) / (5.0 * Ct ** 0.5)
    dz = torch.randn(N, Cout, 2 * D1, 2 * H1, 2 * W1, generator=g)
    a = 1.0 + 0.3 * torch.randn(N, Ct, generator=g)
    b = 0.5 + 0.2 * torch.randn(N, Ct, generator=g)  # a clearly nonzero offset: padding must not pick it up
    aff = torch.stack((a, b), dim=-1).contiguous()
    ga = low * a[:, C0:].view(N, C1, 1, 1, 1) + b[:, C0:].view(N, C1, 1, 1, 1)  # the affine in fp32, as the kernel applies it
    w1 = w[:, C0:]
    kf, kd = SE.presum_fwd(w1), SE.presum_dgrad(w1)
    up = up2(ga.double())
    return dict(low=low, w=w, dz=dz, aff=aff,
                y_same=SE.up_forward(r16(low), kf), y_aff=SE.up_forward(r16(ga), kf),
                y_exact=F.conv3d(up, w1.double(), padding=1),
                dlow=SE.up_dgrad(r16(dz), kd),
                dlow_exact=childsum(torch.nn.grad.conv3d_input(up.shape, w1.double(), dz.double(), padding=1)),
                dw_same=SE.up_wgrad(r16(low), r16(dz)), dw_aff=SE.up_wgrad(r16(ga), r16(dz)),
                dw_exact=torch.nn.grad.conv3d_weight(up, w1.shape, dz.double(), padding=1))


def pack_up(w_d, c_off, C1, dgrad):
    Cout, Ct = w_d.shape[:2]
    n = nat.get_lib().u3d_subpixel_bf16_packed_elems(C1, Cout, dgrad)
    assert n == 64 * C1 * Cout
    out = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    nat.call("u3d_pack_subpixel_weights_bf16", 0, _stream(DEV), _p(w_d), Cout, Ct, c_off, C1, dgrad, _p(out))
    return out


def up_fwd(low_d, aff_d, w_d, c_off, C1):
    """u3d_subpixel_conv_fwd_bf16 on channels [c_off, c_off + C1) of the weight; aff_d: the (N, Ct, 2) table of the whole layer or None"""
    N, D1, H1, W1, _ = low_d.shape
    Cout, Ct = w_d.shape[:2]
    out = torch.full((N, 2 * D1, 2 * H1, 2 * W1, Cout), float("nan"), dtype=torch.float32, device=DEV)
    rows = aff_d.view(-1)[2 * c_off:] if aff_d is not None else None
    nat.call("u3d_subpixel_conv_fwd_bf16", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(pack_up(w_d, c_off, C1, 0)), _p(out), N, D1, H1,
             W1, C1, Cout)
    return out


def up_dgrad(dz_d, low_d, w_d, c_off, C1, reps):
    N, D1, H1, W1, _ = low_d.shape
    Cout = w_d.shape[0]
    dlow = torch.full((N, D1, H1, W1, C1), float("nan"), dtype=torch.float32, device=DEV)
    gst = torch.zeros((reps, N, C1, 2), dtype=torch.float64, device=DEV)
    nat.call("u3d_subpixel_conv_dgrad_bf16", 0, _stream(DEV), _p(dz_d), _p(pack_up(w_d, c_off, C1, 1)), _p(low_d), _p(dlow), _p(gst), N, D1,
             H1, W1, C1, Cout, reps)
    return dlow, gst


def up_wgrad(low_d, aff_d, dz_d, dw_buf, c_off, C1):
    """u3d_subpixel_conv_wgrad_bf16 into channels [c_off, c_off + C1) of dw_buf (Cout, Ct, 3, 3, 3); returns the workspace floats"""
    N, D1, H1, W1, _ = low_d.shape
    Cout, Ct = dw_buf.shape[:2]
    need = nat.get_lib().u3d_subpixel_wgrad_bf16_workspace_floats(N, D1, H1, W1, C1, Cout)
    assert need >= 64 * C1 * Cout and need % (64 * C1 * Cout) == 0
    ws = torch.full((need,), float("nan"), dtype=torch.float32, device=DEV)
    rows = aff_d.view(-1)[2 * c_off:] if aff_d is not None else None
    nat.call("u3d_subpixel_conv_wgrad_bf16", 0, _stream(DEV), _p(low_d), _p(rows), Ct * 2, _p(dz_d), _p(dw_buf.view(-1)[c_off * 27:]), Ct, N,
             D1, H1, W1, C1, Cout, _p(ws), need)
    return need


@pytest.mark.parametrize("N,D1,H1,W1,C1,Cout", SHAPES)
def test_forward(N, D1, H1, W1, C1, Cout):
    c = case(N, D1, H1, W1, C1, Cout)
    low_d, w_d = ndhwc(c["low"]), c["w"].contiguous().to(DEV)
    y = ncdhw(up_fwd(low_d, None, w_d, C0, C1)).double()
    e_same = rel(y, c["y_same"])
    # a per-sample affine with b = 0.5: the border shows whether padding stayed exactly 0 after it
    y = ncdhw(up_fwd(low_d, c["aff"].to(DEV), w_d, C0, C1)).double()
    scale = c["y_aff"].abs().max().item()
    e_aff = rel(y, c["y_aff"])
    e_border = (border(y) - border(c["y_aff"])).abs().max().item() / scale
    e_exact = (y - c["y_exact"]).abs().max().item() / scale
    print(dict(test="subpixel3d_bf16_fwd", shape=(N, D1, H1, W1, C1, Cout), same=e_same, aff=e_aff, border=e_border, exact=e_exact))
    assert e_same < TOL_SAME
    assert e_aff < TOL_AFF and e_border < TOL_AFF
    assert e_exact < TOL_EXACT


def test_forward_padding_stays_zero_after_affine():
    N, D1, H1, W1, C1, Cout = 1, 2, 3, 5, 32, 32
    low = torch.zeros(N, C1, D1, H1, W1)
    aff = torch.stack((torch.ones(N, C1), torch.full((N, C1), 0.5)), -1).contiguous()
    w = torch.ones(Cout, C1, 3, 3, 3)
    y = up_fwd(ndhwc(low), aff.to(DEV), w.to(DEV), 0, C1)
    ref = F.conv3d(torch.full((N, C1, 2 * D1, 2 * H1, 2 * W1), 0.5, dtype=torch.float64), w.double(), padding=1)  # (small integers x 0.5: exact)
    assert torch.equal(ncdhw(y).double(), ref)


@pytest.mark.parametrize("N,D1,H1,W1,C1,Cout", SHAPES)
def test_data_gradient_and_its_sums(N, D1, H1, W1, C1, Cout):
    c = case(N, D1, H1, W1, C1, Cout)
    low_d, w_d, dz_d = ndhwc(c["low"]), c["w"].contiguous().to(DEV), ndhwc(c["dz"])
    dlow1, g1 = up_dgrad(dz_d, low_d, w_d, C0, C1, 1)
    dlow3, g3 = up_dgrad(dz_d, low_d, w_d, C0, C1, 3)
    d = ncdhw(dlow1).double()
    e_same, e_exact = rel(d, c["dlow"]), (d - c["dlow_exact"]).abs().max().item() / c["dlow_exact"].abs().max().item()
    gref = torch.stack((d.sum((2, 3, 4)), (d * c["low"].double()).sum((2, 3, 4))), -1)
    e_g1, e_g3 = rel(g1[0].cpu(), gref), rel(g3.sum(0).cpu(), gref)
    print(dict(test="subpixel3d_bf16_dgrad", shape=(N, D1, H1, W1, C1, Cout), same=e_same, exact=e_exact, gstats=e_g1, gstats_reps3=e_g3))
    assert torch.equal(dlow1, dlow3)
    assert e_same < TOL_SAME and e_exact < TOL_EXACT
    assert e_g1 < TOL_GSTATS and e_g3 < TOL_GSTATS


@pytest.mark.parametrize("N,D1,H1,W1,C1,Cout", SHAPES)
def test_weight_gradient(N, D1, H1, W1, C1, Cout):
    c = case(N, D1, H1, W1, C1, Cout)
    low_d, dz_d, aff_d = ndhwc(c["low"]), ndhwc(c["dz"]), c["aff"].to(DEV)
    Ct = C0 + C1
    runs = []
    for aff in (None, aff_d, aff_d):
        dw = torch.full((Cout, Ct, 3, 3, 3), float("nan"), dtype=torch.float32, device=DEV)  # outputs pre-filled with NaN
        dw[:, :C0] = 7.25  # the sentinel outside the channel slice
        need = up_wgrad(low_d, aff, dz_d, dw, C0, C1)
        runs.append(dw.cpu())
    if (N, D1, H1, W1, C1, Cout) == MULTI_SLOT:
        assert need > 64 * C1 * Cout  # more than one block slot is added by the fold kernel
    e_same, e_aff = rel(runs[0][:, C0:], c["dw_same"]), rel(runs[1][:, C0:], c["dw_aff"])
    e_exact = rel(runs[1][:, C0:], c["dw_exact"])
    print(dict(test="subpixel3d_bf16_wgrad", shape=(N, D1, H1, W1, C1, Cout), slots=need // (64 * C1 * Cout), same=e_same, aff=e_aff,
               exact=e_exact))
    assert e_same < TOL_SAME and e_aff < TOL_AFF and e_exact < TOL_EXACT
    assert torch.equal(runs[1], runs[2])  # bitwise repeatable
    assert all(bool((r[:, :C0] == 7.25).all()) for r in runs)  # channels outside the slice are untouched


def test_slice_helpers_equal_the_plain_entry_points():
    """c_off = 0, stride = Cin: the image of u3d_pack_weights_bf16 and the dw of u3d_conv3d_wgrad_bf16 bit for bit"""
    lib = nat.get_lib()
    g = torch.Generator().manual_seed(5)
    N, D, H, W, Cin, Cout = 1, 5, 9, 19, 32, 64
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) / 10).to(DEV)
    for mode in (0, 1):
        n = lib.u3d_packed_weight_bf16_elems(Cin, Cout, mode)
        a = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        b = torch.ones(n, dtype=torch.bfloat16, device=DEV)  # (both write every element, the zero prefetch tail included)
        nat.call("u3d_pack_weights_bf16", 0, _stream(DEV), _p(w), Cout, Cin, mode, _p(a))
        nat.call("u3d_pack_weights_bf16_slice", 0, _stream(DEV), _p(w), Cout, Cin, mode, Cin, 0, _p(b))
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and bool((a != 0).any())
    x, dz = ndhwc(torch.randn(N, Cin, D, H, W, generator=g)), ndhwc(torch.randn(N, Cout, D, H, W, generator=g))
    need = lib.u3d_wgrad_bf16_workspace_floats(N, D, H, W, Cin, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    dwa = torch.zeros((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=DEV)
    dwb = torch.ones((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv3d_wgrad_bf16", 0, _stream(DEV), _p(x), None, _p(dz), _p(dwa), N, D, H, W, Cin, Cout, _p(ws), need)
    nat.call("u3d_conv3d_wgrad_bf16_strided", 0, _stream(DEV), _p(x), None, _p(dz), _p(dwb), Cin, N, D, H, W, Cin, Cout, _p(ws), need)
    assert torch.equal(dwa, dwb)
    # ... and a slice of a wider weight / gradient: the image of the slice's own weight, the same dw inside the slice, nothing outside
    wide = torch.randn(Cout, 32 + Cin, 3, 3, 3, generator=g).to(DEV)
    own = wide[:, 32:].contiguous()
    for mode in (0, 1):
        n = lib.u3d_packed_weight_bf16_elems(Cin, Cout, mode)
        a = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        b = torch.ones(n, dtype=torch.bfloat16, device=DEV)
        nat.call("u3d_pack_weights_bf16", 0, _stream(DEV), _p(own), Cout, Cin, mode, _p(a))
        nat.call("u3d_pack_weights_bf16_slice", 0, _stream(DEV), _p(wide), Cout, Cin, mode, 32 + Cin, 32, _p(b))
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    dwide = torch.full((Cout, 32 + Cin, 3, 3, 3), 7.25, dtype=torch.float32, device=DEV)
    nat.call("u3d_conv3d_wgrad_bf16_strided", 0, _stream(DEV), _p(x), None, _p(dz), _p(dwide.view(-1)[32 * 27:]), 32 + Cin, N, D, H, W, Cin,
             Cout, _p(ws), need)
    assert torch.equal(dwide[:, 32:], dwa) and bool((dwide[:, :32] == 7.25).all())


def test_both_halves_compose_to_the_emulated_layer():
    """C0 = 32 skip + C1 = 64 upsampled channels, 8 x 16 x 16 from 4 x 8 x 8: sub-pixel launch + u3d_conv3d_bf16_ex with residual = its out
    (forward), u3d_conv3d_bf16_ex on the sliced mode-1 image + sub-pixel data gradient, the two weight-gradient slices of one buffer —
    against the emulated full layer"""
    lib = nat.get_lib()
    g = torch.Generator().manual_seed(11)
    N, D1, H1, W1, c0, C1, Cout = 1, 4, 8, 8, 32, 64, 64
    D, H, W, Ct = 2 * D1, 2 * H1, 2 * W1, c0 + C1
    skip, low = torch.randn(N, c0, D, H, W, generator=g), torch.randn(N, C1, D1, H1, W1, generator=g)
    w = torch.randn(Cout, Ct, 3, 3, 3, generator=g) / (5.0 * Ct ** 0.5)
    dz = torch.randn(N, Cout, D, H, W, generator=g)
    x = torch.cat((skip, up2(low)), dim=1).double().requires_grad_(True)
    wd64 = w.double().requires_grad_(True)
    y_ref = SE.SubpixelBf16Conv3d.apply(x, wd64, c0, SE.r16)
    y_ref.backward(dz.double())
    dskip_ref, dlow_ref = x.grad[:, :c0], x.grad[:, c0:, ::2, ::2, ::2]
    skip_d, low_d, dz_d, w_d = ndhwc(skip), ndhwc(low), ndhwc(dz), w.contiguous().to(DEV)

    def pack_skip(mode):
        out = torch.zeros(lib.u3d_packed_weight_bf16_elems(c0, Cout, mode), dtype=torch.bfloat16, device=DEV)
        nat.call("u3d_pack_weights_bf16_slice", 0, _stream(DEV), _p(w_d), Cout, c0, mode, Ct, 0, _p(out))
        return out

    part = up_fwd(low_d, None, w_d, c0, C1)
    y = torch.empty((N, D, H, W, Cout), dtype=torch.float32, device=DEV)
    need = lib.u3d_conv3d_bf16_workspace_floats(N, D, H, W, c0, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv3d_bf16_ex", 0, _stream(DEV), _p(skip_d), None, _p(pack_skip(0)), _p(y), N, D, H, W, c0, Cout, 0, None, None, None,
             _p(part), _p(ws), need)
    dg0 = torch.empty((N, D, H, W, c0), dtype=torch.float32, device=DEV)
    gst0 = torch.zeros((N, c0, 2), dtype=torch.float64, device=DEV)
    need = lib.u3d_conv3d_bf16_workspace_floats(N, D, H, W, Cout, c0)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv3d_bf16_ex", 0, _stream(DEV), _p(dz_d), None, _p(pack_skip(1)), _p(dg0), N, D, H, W, Cout, c0, 0, None, _p(skip_d),
             _p(gst0), None, _p(ws), need)
    dlow, _ = up_dgrad(dz_d, low_d, w_d, c0, C1, 1)
    dw = torch.full((Cout, Ct, 3, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    up_wgrad(low_d, None, dz_d, dw, c0, C1)
    need = lib.u3d_wgrad_bf16_workspace_floats(N, D, H, W, c0, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv3d_wgrad_bf16_strided", 0, _stream(DEV), _p(skip_d), None, _p(dz_d), _p(dw), Ct, N, D, H, W, c0, Cout, _p(ws), need)
    torch.cuda.synchronize()
    errs = dict(fwd=rel(ncdhw(y), y_ref.detach()), dskip=rel(ncdhw(dg0), dskip_ref), dlow=rel(ncdhw(dlow), dlow_ref),
                dw=rel(dw.cpu(), wd64.grad))
    print(dict(test="subpixel3d_bf16_composition", **errs))
    assert all(e < TOL_SAME for e in errs.values()), errs


def test_envelope():
    lib = nat.get_lib()
    assert lib.u3d_subpixel_bf16_packed_elems(16, 32, 0) == 0 and lib.u3d_subpixel_bf16_packed_elems(32, 16, 1) == 0
    assert lib.u3d_subpixel_wgrad_bf16_workspace_floats(1, 2, 4, 4, 16, 32) == 0
    N, D1, H1, W1 = 1, 2, 4, 4
    buf = torch.zeros(1 << 18, dtype=torch.float32, device=DEV)
    img = torch.zeros(1 << 18, dtype=torch.bfloat16, device=DEV)
    dst = torch.zeros(1 << 18, dtype=torch.float32, device=DEV)
    gst = torch.zeros(256, dtype=torch.float64, device=DEV)
    n0 = dst.clone()
    for C1, Cout, off in ((16, 32, 0), (32, 16, 0), (32, 32, 1)):  # C1 = 16, Cout = 16, a misaligned pointer (4 bytes off)
        src = buf[off:]
        for name, args in (
                ("u3d_subpixel_conv_fwd_bf16", (_p(src), None, 0, _p(img), _p(dst), N, D1, H1, W1, C1, Cout)),
                ("u3d_subpixel_conv_dgrad_bf16", (_p(src), _p(img), _p(buf), _p(dst), _p(gst), N, D1, H1, W1, C1, Cout, 1)),
                ("u3d_subpixel_conv_wgrad_bf16", (_p(src), None, 0, _p(buf), _p(dst), C1, N, D1, H1, W1, C1, Cout, _p(buf), buf.numel()))):
            rc = getattr(lib, name)(0, _stream(DEV), *args)
            assert rc == U3D_EINVAL and lib.u3d_last_error(), (name, C1, Cout, off, rc)
        if not off:
            assert lib.u3d_pack_subpixel_weights_bf16(0, _stream(DEV), _p(buf), Cout, C1, 0, C1, 0, _p(img)) == U3D_EINVAL
            assert lib.u3d_pack_weights_bf16_slice(0, _stream(DEV), _p(buf), Cout, C1, 0, C1, 0, _p(dst)) == U3D_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(dst, n0)  # nothing was launched
