"""-m gpu: the 3x3 Conv2d kernels of `native_2d_fp32_split` (csrc/u3d_conv2d_f32s.h; u3d_conv2d_f32s, u3d_conv2d_f32s_dgrad,
u3d_conv2d_wgrad_f32s of the extension library) through the C-ABI.  The claim under test is FP32-GRADE accuracy: each new kernel and the
fp32 kernel it replaces (u3d_conv2d_ex_reps / u3d_conv2d_wgrad) are measured against a float64 convolution of the SAME fp32 operands
(per-channel scales, the affine applied in fp32 as addcmul, as tests/test_gpu_f32s.py does).

Bars: relative L2 of the new kernel <= 2.5x the fp32 kernel's (the margin of tests/test_gpu_f32s.py) and <= 1/100 of u3d_conv2d_bf16's /
u3d_conv2d_wgrad_bf16's on the same operands (bf16 operand rounding is ~2^-9, fp32 grade ~2^-23: a bf16 path cannot pass by accident).
Statistics tables: within 1e-5 of the table's largest entry from float64 sums of the stored output (fp32 partial sums over a 16 x 16
tile, then f64 atomics: the bar of tests/test_gpu_conv2d_bf16.py).  A virtual source equals the launch on its written-out concat bit for
bit (same plan, same staged values).

Measured on an MI355X (new / fp32 kernel): forward 0.82x, 1.39x, 0.83x; data gradient 1.67x; virtual forward 2.0 - 2.1x (the
closest to the bar), virtual weight gradient 1.36x; weight gradient 1.34x and 1.54x, one slot the same; drift cases: forward 4.6e-7 (bar
6.4e-6), one-slot weight gradient over 64 tiles 1.02x.  Against the bf16 kernels: below 1.6e-4 of their error everywhere."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv2d as C2
import test_gpu_conv2d_bf16 as C2B
from conftest import diag
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import VSrc, _p, _stream

pytestmark = pytest.mark.gpu
TOL_STATS = 1e-5


def _ext():
    return nat.get_ext_lib()


def nhwc(x):  # (N,C,H,W) cpu -> (N,H,W,C) gpu
    return x.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(y):  # (N,H,W,C) gpu -> (N,C,H,W) cpu
    return y.permute(0, 3, 1, 2).contiguous().cpu()


def rel_l2(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


def pack(w, mode):
    Cout, Cin = w.shape[:2]
    n = _ext().u3d_packed_weight2d_f32s_elems(Cin, Cout, mode)
    assert n > 0
    out = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    wd = w.float().contiguous().to(DEV)
    nat.call("u3d_pack_weights2d_f32s", 0, _stream(DEV), _p(wd), Cout, Cin, mode, _p(out))
    return out


def _src_args(x0, x1=None):
    """flat source arguments from (N,H,W,C) device tensors: a single tensor, or skip + low-res half with the nearest tables"""
    if x1 is None:
        return (_p(x0), None, None, None, x0.shape[-1], 0, 0, 0), None
    v = VSrc(x0.unsqueeze(1), x1.unsqueeze(1))
    return (_p(x0), _p(x1), _p(v.maps[1]), _p(v.maps[2]), v.C0, v.C1, v.H1, v.W1), v


def fwd(x0, w, x1=None, affine=None, relu=0, out_stats=None, reps=1):
    """u3d_conv2d_f32s on (N,H,W,C) device tensors; returns (N,H,W,Cout) on the device"""
    N, H, W, _ = x0.shape
    args, keep = _src_args(x0, x1)
    y = torch.empty((N, H, W, w.shape[0]), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_f32s", 0, _stream(DEV), *args, _p(affine), _p(pack(w, 0)), _p(y), N, H, W, w.shape[0], relu, _p(out_stats), reps)
    torch.cuda.synchronize()
    return y


def dgrad(dz, w, gx0=None, gx1=None, gstats=None, reps=1):
    """u3d_conv2d_f32s_dgrad of the layer with forward weight w (Cout, Cin, 3, 3); dz (N,H,W,Cout) on the device"""
    N, H, W, Cout = dz.shape
    Cin = w.shape[1]
    if gx0 is None:
        args, keep = (None, None, None, None, Cin, 0, 0, 0), None
    else:
        args, keep = _src_args(gx0, gx1)
    dg = torch.empty((N, H, W, Cin), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_f32s_dgrad", 0, _stream(DEV), _p(dz), _p(pack(w, 1)), _p(dg), N, H, W, Cout, *args, _p(gstats), reps)
    torch.cuda.synchronize()
    return dg


def wgrad(x0, dz, x1=None, affine=None, ws_floats=None):
    """u3d_conv2d_wgrad_f32s; returns (dw (Cout, Cin, 3, 3) on the device, workspace floats used)"""
    N, H, W, Cout = dz.shape
    args, keep = _src_args(x0, x1)
    Cin = args[4] + args[5]
    need = _ext().u3d_wgrad2d_f32s_workspace_floats(N, H, W, Cin, Cout)
    assert need > 0 and need % (9 * Cin * Cout) == 0
    n = need if ws_floats is None else ws_floats
    ws = torch.empty(n, dtype=torch.float32, device=DEV)
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    nat.call("u3d_conv2d_wgrad_f32s", 0, _stream(DEV), *args, _p(affine), _p(dz), _p(dw), N, H, W, Cout, _p(ws), n)
    torch.cuda.synchronize()
    return dw, n


def operands(N, H, W, C, K, seed, positive=False):
    """x, w, dz with per-channel scales, the affine table and the conv input g = fma(x, a, b) as the kernels form it in fp32"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g) * (1.0 + 3.0 * torch.rand(N, C, 1, 1, generator=g))
    w = torch.randn(K, C, 3, 3, generator=g) / (9 * C) ** 0.5
    dz = torch.randn(N, K, H, W, generator=g) * (1.0 + 3.0 * torch.rand(N, K, 1, 1, generator=g))
    a = 1.0 + 0.3 * torch.randn(N, C, generator=g)
    b = 0.2 * torch.randn(N, C, generator=g)
    if positive:
        x, w, dz, a, b = x.abs(), w.abs(), dz.abs(), a.abs(), b.abs()
    aff = torch.stack((a, b), dim=-1).contiguous()
    g32 = torch.addcmul(b.view(N, C, 1, 1), x, a.view(N, C, 1, 1))
    return x, w, dz, aff, g32


def stat_table(y, other):
    y = y.double()
    return torch.stack((y.sum(dim=(2, 3)), (y * other.double()).sum(dim=(2, 3))), dim=-1)


def check_stats(table, want, what):
    err = (table.cpu() - want).abs().max().item() / want.abs().max().item()
    assert err < TOL_STATS, (what, err)


# ---- forward -------------------------------------------------------------------------------------------------------------------------------
FWD_SHAPES = [
    (2, 21, 37, 16, 32),   # ragged, one chunk
    (1, 32, 48, 48, 96),   # three chunks, odd last chunk, three n-tiles
    (1, 1, 1, 32, 32),     # single pixel
]


@pytest.mark.parametrize("N,H,W,C,K", FWD_SHAPES)
def test_forward_is_fp32_grade_with_relu_and_statistics(N, H, W, C, K):
    x, w, _, aff, g32 = operands(N, H, W, C, K, 1)
    ref = F.conv2d(g32.double(), w.double(), None, padding=1).clamp_min(0)
    xd, affd = nhwc(x), aff.to(DEV)
    st1 = torch.zeros((1, N, K, 2), dtype=torch.float64, device=DEV)
    y = nchw(fwd(xd, w, affine=affd, relu=1, out_stats=st1, reps=1))
    st3 = torch.zeros((3, N, K, 2), dtype=torch.float64, device=DEV)
    y3 = nchw(fwd(xd, w, affine=affd, relu=1, out_stats=st3, reps=3))
    assert torch.equal(y, y3)
    y32, _ = C2.conv2d(VSrc(xd.unsqueeze(1)), w, K, relu=1, affine=affd)
    y32 = nchw(y32.squeeze(1))
    yb, _ = C2B.conv(x, w, affine=affd, relu=1)
    torch.cuda.synchronize()
    e_new, e_f32, e_b16 = rel_l2(y, ref), rel_l2(y32, ref), rel_l2(yb, ref)
    diag(test="conv2d_f32s_fwd", shape=[N, H, W], C=C, K=K, l2_split=e_new, l2_f32mfma=e_f32, l2_bf16=e_b16)
    assert e_new <= 2.5 * e_f32, (e_new, e_f32)
    assert e_new <= 1e-2 * e_b16, (e_new, e_b16)
    want = stat_table(y, y)
    check_stats(st1[0], want, "reps 1")
    check_stats(st3.sum(0), want, "reps 3")
    if N * ((H + 15) // 16) * ((W + 15) // 16) * (K // 32) >= 3:
        assert all(st3[r].abs().sum().item() > 0 for r in range(3))  # the blocks spread over the replica rows


def test_forward_accumulation_does_not_drift():
    """all operands positive, 16 chunks: L = 9 taps x 6 products x 16 chunks = 864 accumulations per output.  An uncancelled round-down
    drift of the bf16 MFMA's accumulation is estimated at L * 2^-25 relative; the bar is a quarter of that, or the general one"""
    N, H, W, C, K = 1, 16, 16, 256, 64
    x, w, _, aff, g32 = operands(N, H, W, C, K, 2, positive=True)
    ref = F.conv2d(g32.double(), w.double(), None, padding=1)
    xd, affd = nhwc(x), aff.to(DEV)
    y = nchw(fwd(xd, w, affine=affd))
    y32, _ = C2.conv2d(VSrc(xd.unsqueeze(1)), w, K, affine=affd)
    torch.cuda.synchronize()
    r_new, r_f32 = rel_l2(y, ref), rel_l2(nchw(y32.squeeze(1)), ref)
    signed = ((y.double() - ref).mean() / ref.abs().mean()).item()
    L = 9 * 6 * 16
    diag(test="conv2d_f32s_fwd_drift", shape=[N, H, W], C=C, K=K, l2_split=r_new, l2_f32mfma=r_f32, mean_signed=signed, bar=L * 2.0 ** -27)
    assert r_new <= max(2.5 * r_f32, L * 2.0 ** -27), (r_new, r_f32)


# ---- data gradient ---------------------------------------------------------------------------------------------------------------------------
def test_data_gradient_is_fp32_grade_with_gstats():
    N, H, W, C, K = 2, 21, 37, 32, 64  # a 32 -> 64 layer: contraction over 64, 32 produced channels
    x, w, dz, _, _ = operands(N, H, W, C, K, 3)
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w.double(), dz.double(), padding=1)
    dzd, xd = nhwc(dz), nhwc(x)
    gst = torch.zeros((2, N, C, 2), dtype=torch.float64, device=DEV)
    dg = nchw(dgrad(dzd, w, gx0=xd, gstats=gst, reps=2))
    plain = nchw(dgrad(dzd, w))  # gstats is optional
    assert torch.equal(dg, plain)
    dg32, _ = C2.conv2d(VSrc(dzd.unsqueeze(1)), w, C, mode=1)
    dgb, _ = C2B.conv(dz, w, mode=1)
    torch.cuda.synchronize()
    e_new, e_f32, e_b16 = rel_l2(dg, ref), rel_l2(nchw(dg32.squeeze(1)), ref), rel_l2(dgb, ref)
    diag(test="conv2d_f32s_dgrad", shape=[N, H, W], C=C, K=K, l2_split=e_new, l2_f32mfma=e_f32, l2_bf16=e_b16)
    assert e_new <= 2.5 * e_f32, (e_new, e_f32)
    assert e_new <= 1e-2 * e_b16, (e_new, e_b16)
    check_stats(gst.sum(0), stat_table(dg, x), "gstats")


# ---- virtual source ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(20, 36), (21, 37)])  # exact 2x, and n -> 2n + 1 through the general nearest tables
def test_a_virtual_source_equals_its_written_out_concat_bit_for_bit(H, W):
    N, C0, C1, K, H1, W1 = 2, 32, 64, 32, 10, 18
    g = torch.Generator().manual_seed(4)
    skip = torch.randn(N, C0, H, W, generator=g) * (1.0 + 3.0 * torch.rand(N, C0, 1, 1, generator=g))
    low = torch.randn(N, C1, H1, W1, generator=g) * (1.0 + 3.0 * torch.rand(N, C1, 1, 1, generator=g))
    w = torch.randn(K, C0 + C1, 3, 3, generator=g) / (9 * (C0 + C1)) ** 0.5
    dz = torch.randn(N, K, H, W, generator=g)
    aff = torch.stack((1.0 + 0.3 * torch.randn(N, C0 + C1, generator=g), 0.2 * torch.randn(N, C0 + C1, generator=g)), dim=-1).contiguous()
    cat = torch.cat((skip, F.interpolate(low, size=(H, W), mode="nearest")), dim=1)
    g32 = torch.addcmul(aff[..., 1].view(N, -1, 1, 1), cat, aff[..., 0].view(N, -1, 1, 1))
    sd, ld, cd, dzd, affd = nhwc(skip), nhwc(low), nhwc(cat), nhwc(dz), aff.to(DEV)
    # forward (ReLU + statistics)
    sv = torch.zeros((1, N, K, 2), dtype=torch.float64, device=DEV)
    sc = torch.zeros((1, N, K, 2), dtype=torch.float64, device=DEV)
    yv = fwd(sd, w, x1=ld, affine=affd, relu=1, out_stats=sv)
    yc = fwd(cd, w, affine=affd, relu=1, out_stats=sc)
    assert torch.equal(yv, yc)
    ref = F.conv2d(g32.double(), w.double(), None, padding=1).clamp_min(0)
    y32, _ = C2.conv2d(VSrc(cd.unsqueeze(1)), w, K, relu=1, affine=affd)
    torch.cuda.synchronize()
    e_new, e_f32 = rel_l2(nchw(yv), ref), rel_l2(nchw(y32.squeeze(1)), ref)
    diag(test="conv2d_f32s_virtual_fwd", shape=[N, H, W], C0=C0, C1=C1, K=K, l2_split=e_new, l2_f32mfma=e_f32)
    assert e_new <= 2.5 * e_f32, (e_new, e_f32)
    check_stats(sv[0], stat_table(nchw(yv), nchw(yv)), "virtual out_stats")
    # data gradient: dg of the full concat width, gstats against the virtual forward input
    gv = torch.zeros((1, N, C0 + C1, 2), dtype=torch.float64, device=DEV)
    gc = torch.zeros((1, N, C0 + C1, 2), dtype=torch.float64, device=DEV)
    dgv = dgrad(dzd, w, gx0=sd, gx1=ld, gstats=gv)
    dgc = dgrad(dzd, w, gx0=cd, gstats=gc)
    assert torch.equal(dgv, dgc)
    check_stats(gv[0], stat_table(nchw(dgv), cat), "virtual gstats")
    check_stats(gc[0], stat_table(nchw(dgc), cat), "concat gstats")
    # weight gradient
    dwv, n = wgrad(sd, dzd, x1=ld, affine=affd)
    dwc, m = wgrad(cd, dzd, affine=affd)
    assert n == m and torch.equal(dwv, dwc)
    dw_ref = torch.nn.grad.conv2d_weight(g32.double(), w.shape, dz.double(), padding=1)
    dw32 = C2.wgrad2d(VSrc(cd.unsqueeze(1)), dzd.unsqueeze(1), K, affine=affd)
    torch.cuda.synchronize()
    e_new, e_f32 = rel_l2(dwv.cpu(), dw_ref), rel_l2(dw32.cpu(), dw_ref)
    diag(test="conv2d_f32s_virtual_wgrad", shape=[N, H, W], C0=C0, C1=C1, K=K, l2_split=e_new, l2_f32mfma=e_f32)
    assert e_new <= 2.5 * e_f32, (e_new, e_f32)


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------------
_WCASES = {}


def _wcase(N, H, W, C, K, positive=False):
    """operands, float64 truth and the fp32 / bf16 kernels' results of one case: computed once, shared, left unchanged"""
    key = (N, H, W, C, K, positive)
    if key not in _WCASES:
        x, w, dz, aff, g32 = operands(N, H, W, C, K, 5, positive)
        ref = torch.nn.grad.conv2d_weight(g32.double(), w.shape, dz.double(), padding=1)
        xd, dzd, affd = nhwc(x), nhwc(dz), aff.to(DEV)
        dw32 = C2.wgrad2d(VSrc(xd.unsqueeze(1)), dzd.unsqueeze(1), K, affine=affd)
        dwb = C2B.wgrad(x, dz, affine=affd)
        torch.cuda.synchronize()
        _WCASES[key] = (xd, dzd, affd, ref, dw32.cpu(), dwb)
    return _WCASES[key]


@pytest.mark.parametrize("N,H,W,C,K", [(2, 21, 37, 32, 32), (1, 32, 48, 64, 96)])
def test_weight_gradient_is_fp32_grade_reproducible_and_holds_on_one_slot(N, H, W, C, K):
    xd, dzd, affd, ref, dw32, dwb = _wcase(N, H, W, C, K)
    dw1, n = wgrad(xd, dzd, affine=affd)
    dw2, _ = wgrad(xd, dzd, affine=affd)
    assert torch.equal(dw1, dw2)  # the same workspace size gives the same bits
    slot = 9 * C * K
    one, _ = wgrad(xd, dzd, affine=affd, ws_floats=slot)
    two, _ = wgrad(xd, dzd, affine=affd, ws_floats=2 * slot + 5)  # as many splits as it holds
    e_new, e_one, e_two, e_f32, e_b16 = (rel_l2(t.cpu(), ref) for t in (dw1, one, two, dw32, dwb))
    diag(test="conv2d_f32s_wgrad", shape=[N, H, W], C=C, K=K, slots_planned=n // slot, l2_split=e_new, l2_one_slot=e_one, l2_two_slots=e_two,
         l2_f32mfma=e_f32, l2_bf16=e_b16)
    assert e_new <= 2.5 * e_f32 and e_one <= 2.5 * e_f32 and e_two <= 2.5 * e_f32, (e_new, e_one, e_two, e_f32)
    assert e_new <= 1e-2 * e_b16, (e_new, e_b16)


def test_weight_gradient_does_not_drift_over_64_tiles_in_one_chain():
    """one slot at (1, 128, 128) with positive operands: one block per (co, ci) cell walks all 64 tiles"""
    N, H, W, C, K = 1, 128, 128, 32, 32
    xd, dzd, affd, ref, dw32, _ = _wcase(N, H, W, C, K, positive=True)
    one, _ = wgrad(xd, dzd, affine=affd, ws_floats=9 * C * K)
    e_one, e_f32 = rel_l2(one.cpu(), ref), rel_l2(dw32, ref)
    signed = ((one.cpu().double() - ref).mean() / ref.abs().mean()).item()
    diag(test="conv2d_f32s_wgrad_drift", shape=[N, H, W], C=C, K=K, l2_one_slot=e_one, l2_f32mfma=e_f32, mean_signed=signed)
    assert e_one <= 2.5 * e_f32, (e_one, e_f32)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_einval_and_launch_nothing():
    N, H, W = 1, 8, 8
    lib, core, st = _ext(), nat.get_lib(), _stream(DEV)
    x = torch.randn(N, H, W, 64, device=DEV)
    low = torch.randn(N, 4, 4, 64, device=DEV)
    v = VSrc(x[..., :16].contiguous().unsqueeze(1), low.unsqueeze(1))
    ymap, xmap = _p(v.maps[1]), _p(v.maps[2])
    img = torch.zeros(27 * 64 * 64, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(9 * 64 * 64 * 4, device=DEV)
    poison = 777.0
    out = torch.full((N * H * W * 64 + 9 * 64 * 64,), poison, device=DEV)
    off4 = lambda t: ctypes.c_void_p(t.data_ptr() + 4)  # noqa: E731

    def refused(rc, who, what):
        torch.cuda.synchronize()
        assert rc == nat.U3D_EINVAL, what
        assert who in core.u3d_last_error(), what
        assert (out == poison).all(), what

    def f(p0, C0, Cout, p1=None, ym=None, xm=None, C1=0, H1=0, W1=0):
        return lib.u3d_conv2d_f32s(0, st, p0, p1, ym, xm, C0, C1, H1, W1, None, _p(img), _p(out), N, H, W, Cout, 0, None, 1)

    def d(dz, Cout, C0, C1=0):
        return lib.u3d_conv2d_f32s_dgrad(0, st, dz, _p(img), _p(out), N, H, W, Cout, None, None, None, None, C0, C1, 0, 0, None, 1)

    def wg(p0, C0, Cout, n, p1=None, ym=None, xm=None, C1=0, H1=0, W1=0, wsp=None):
        return lib.u3d_conv2d_wgrad_f32s(0, st, p0, p1, ym, xm, C0, C1, H1, W1, None, _p(x), _p(out), N, H, W, Cout,
                                         _p(ws) if wsp is None else wsp, n)

    refused(f(_p(x), 24, 32), b"u3d_conv2d_f32s", "Cin = 24")
    refused(f(_p(x), 32, 48), b"u3d_conv2d_f32s", "produced = 48")
    refused(f(_p(x), 16, 32, _p(low), ymap, xmap, 32, 4, 4), b"u3d_conv2d_f32s", "C0 = 16 virtual")
    refused(f(off4(x), 32, 32), b"u3d_conv2d_f32s", "a pointer 4 bytes off")
    refused(d(_p(x), 24, 32), b"u3d_conv2d_f32s_dgrad", "contraction = 24")
    refused(d(_p(x), 32, 48), b"u3d_conv2d_f32s_dgrad", "produced = 48")
    refused(d(_p(x), 32, 16, 32), b"u3d_conv2d_f32s_dgrad", "C0 = 16 virtual")
    refused(d(off4(x), 32, 32), b"u3d_conv2d_f32s_dgrad", "a pointer 4 bytes off")
    refused(wg(_p(x), 24, 32, ws.numel()), b"u3d_conv2d_wgrad_f32s", "Cin = 24")
    refused(wg(_p(x), 32, 48, ws.numel()), b"u3d_conv2d_wgrad_f32s", "Cout = 48")
    refused(wg(_p(x), 16, 32, ws.numel(), _p(low), ymap, xmap, 48, 4, 4), b"u3d_conv2d_wgrad_f32s", "C0 = 16 virtual")
    refused(wg(off4(x), 32, 32, ws.numel()), b"u3d_conv2d_wgrad_f32s", "a pointer 4 bytes off")
    refused(wg(_p(x), 32, 32, 9 * 32 * 32 // 2), b"u3d_conv2d_wgrad_f32s", "half a slot of workspace")
    refused(wg(_p(x), 32, 32, ws.numel(), wsp=ctypes.c_void_p(0)), b"u3d_conv2d_wgrad_f32s", "no workspace")
    rc = lib.u3d_pack_weights2d_f32s(0, st, _p(x), 48, 32, 0, _p(out))
    refused(rc, b"u3d_pack_weights2d_f32s", "pack: produced = 48")
