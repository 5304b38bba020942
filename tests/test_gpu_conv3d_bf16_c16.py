"""-m gpu: the entry points of the extension library libu3d_ext_hip.so (csrc/u3d_c16_bf16.hip, include/u3d_ext.h) through the C-ABI: the
bf16 3x3x3 forward, data gradient and weight gradient of a UNet3D's 16-channel layers (`bf16_stem`) — half n-tiles in the image, masked
epilogue stores and statistics, zero-staged channel octets and masked partial sums in the weight gradient.

Reference and bars are those of tests/test_gpu_conv2d_bf16.py (TOL_SAME, TOL_AFF, TOL_EXACT), relative to the result's range: float64
F.conv3d / autograd on the CPU with the SAME operand rounding restated, 1e-4 with an identity affine (accumulation order only), 1e-3 with
a random affine (a clearly non-zero offset: padding must not pick it up), 2e-2 against the exact operands; the statistics tables 1e-6 of
the table's maximum against float64 sums of the written output.

Shapes (N, D, H, W) against the 4 x 8 x 8 forward tile and the 2 x 4 x 16 weight-gradient tile: all border; below a tile; ragged on all
axes; one plane group with a 2 + 1 / 1 + 1 tile split; several blocks in every kernel (45 forward tiles, 75 weight-gradient tiles: more
than one split, asserted through the workspace size).  Outputs are pre-filled with NaN in front of a guard band."""
from functools import cached_property

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import _p, _stream

pytestmark = pytest.mark.gpu
TOL_SAME = 1e-4   # identical operands: fp32 accumulation order only
TOL_AFF = 1e-3    # operands after a random fp32 affine
TOL_EXACT = 2e-2  # against the un-rounded operands
TOL_STATS = 1e-6  # a statistics table against float64 sums of the written output, relative to the table's maximum
GUARD = 1024
GUARD_VALUE = -12345.0

SHAPES = [(2, 1, 1, 1), (1, 2, 3, 5), (1, 5, 9, 11), (1, 3, 17, 9), (1, 9, 17, 33)]
MULTI_SPLIT_SHAPE = SHAPES[-1]
PAIRS = [(16, 32), (32, 16), (16, 16), (48, 16), (16, 48), (80, 48)]  # (Cin, Cout) of the LAYER
CASES = [(s, p) for s in SHAPES for p in PAIRS]


def ext():
    return nat.get_ext_lib()


def r16(t):
    return t.float().to(torch.bfloat16).double()


def ndhwc(x):
    return x.float().permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def ncdhw(y):
    return y.permute(0, 4, 1, 2, 3).contiguous().cpu()


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def guarded(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), GUARD_VALUE, dtype=torch.float32, device=DEV)
    view = buf[:n].view(shape)
    view.fill_(float("nan"))
    return view, buf


def check_guard(view, buf, what):
    assert torch.isfinite(view).all().item(), f"{what}: not every element was written"
    assert (buf[view.numel():] == GUARD_VALUE).all().item(), f"{what}: the guard band was touched"


def pack(w, mode):
    Cout, Cin = w.shape[:2]
    n = ext().u3d_packed_weight_bf16_c16_elems(Cin, Cout, mode)
    assert n > 0
    buf = torch.full((n + GUARD,), 3.0, dtype=torch.bfloat16, device=DEV)
    buf[:n] = float("nan")
    wd = w.float().contiguous().to(DEV)
    nat.call("u3d_pack_weights_bf16_c16", 0, _stream(DEV), _p(wd), Cout, Cin, mode, _p(buf))
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:n].float()).all() and (buf[n:] == 3.0).all()
    return buf[:n]


def conv(x, w, mode=0, affine=None, relu=0, out_stats=None, gx=None, gstats=None):
    """one launch on x (N,C,D,H,W) cpu; mode 1: x is dz and w the forward weight.  Returns (N,K,D,H,W) cpu"""
    N, C, D, H, W = x.shape
    K = w.shape[0] if mode == 0 else w.shape[1]
    wp, xd = pack(w, mode), ndhwc(x)
    y, ybuf = guarded((N, D, H, W, K))
    assert ext().u3d_conv3d_bf16_c16_workspace_floats(N, D, H, W, C, K) == 0
    nat.call("u3d_conv3d_bf16_c16", 0, _stream(DEV), _p(xd), _p(affine), _p(wp), _p(y), N, D, H, W, C, K, relu, _p(out_stats), _p(gx),
             _p(gstats), None, 0)
    torch.cuda.synchronize()
    check_guard(y, ybuf, "out")
    return ncdhw(y)


def wgrad(x, dz, affine=None, slots=None):
    N, C, D, H, W = x.shape
    K = dz.shape[1]
    need = ext().u3d_wgrad_bf16_c16_workspace_floats(N, D, H, W, C, K)
    assert need > 0 and need % (27 * C * K) == 0
    if slots is not None:
        need = slots * 27 * C * K
    ws = torch.full((need + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ws[need:] = GUARD_VALUE
    dw, dwbuf = guarded((K, C, 3, 3, 3))
    xd, dzd = ndhwc(x), ndhwc(dz)
    nat.call("u3d_conv3d_wgrad_bf16_c16", 0, _stream(DEV), _p(xd), _p(affine), _p(dzd), _p(dw), N, D, H, W, C, K, _p(ws), need)
    torch.cuda.synchronize()
    check_guard(dw, dwbuf, "dw")
    assert (ws[need:] == GUARD_VALUE).all().item(), "the workspace's guard band was touched"
    return dw.cpu()


class Case:
    """inputs and float64 references of one layer shape, each computed once, when first asked for, and shared by the tests"""

    def __init__(self, shape, pair):
        (N, D, H, W), (Cin, Cout) = shape, pair
        g = torch.Generator().manual_seed(3000 + 7 * D * H * W + 3 * Cin + Cout)
        self.x = torch.randn(N, Cin, D, H, W, generator=g)
        self.w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (5.2 * Cin ** 0.5)
        self.dz = torch.randn(N, Cout, D, H, W, generator=g)
        a = 1.0 + 0.3 * torch.randn(N, Cin, generator=g)
        b = 0.5 + 0.2 * torch.randn(N, Cin, generator=g)  # a clearly nonzero offset: padding must not pick it up
        self.aff = torch.stack((a, b), dim=-1).contiguous()
        # the affine in fp32 with ONE rounding, as the kernel's fmaf applies it (a float64 product of two fp32 values is exact)
        self.g = (self.x.double() * a.double().view(N, Cin, 1, 1, 1) + b.double().view(N, Cin, 1, 1, 1)).float()

    @cached_property
    def fwd_same(self):
        return F.conv3d(r16(self.x), r16(self.w), padding=1)

    @cached_property
    def fwd_aff(self):
        return F.conv3d(r16(self.g), r16(self.w), padding=1)

    @cached_property
    def fwd_exact(self):
        return F.conv3d(self.g.double(), self.w.double(), padding=1)

    @cached_property
    def dg(self):
        return torch.nn.grad.conv3d_input(self.x.shape, r16(self.w), r16(self.dz), padding=1)

    @cached_property
    def dg_exact(self):
        return torch.nn.grad.conv3d_input(self.x.shape, self.w.double(), self.dz.double(), padding=1)

    @cached_property
    def dw_same(self):
        return torch.nn.grad.conv3d_weight(r16(self.x), self.w.shape, r16(self.dz), padding=1)

    @cached_property
    def dw_aff(self):
        return torch.nn.grad.conv3d_weight(r16(self.g), self.w.shape, r16(self.dz), padding=1)

    @cached_property
    def dw_exact(self):
        return torch.nn.grad.conv3d_weight(self.g.double(), self.w.shape, self.dz.double(), padding=1)


_CASES = {}


def case(shape, pair) -> Case:
    if (shape, pair) not in _CASES:
        _CASES[(shape, pair)] = Case(shape, pair)
    return _CASES[(shape, pair)]


def stat_table(y, other):
    y = y.double()
    return torch.stack((y.sum(dim=(2, 3, 4)), (y * other.double()).sum(dim=(2, 3, 4))), dim=-1)


@pytest.mark.parametrize("shape,pair", CASES)
def test_forward(shape, pair):
    c = case(shape, pair)
    N, (Cin, Cout) = shape[0], pair
    # identity: accumulation order only; an identity affine table changes no bit
    y = conv(c.x, c.w)
    e_same = rel(y, c.fwd_same)
    ida = torch.tensor([1.0, 0.0]).repeat(N, Cin, 1).contiguous().to(DEV)
    assert torch.equal(y, conv(c.x, c.w, affine=ida))
    # affine, ReLU, out_stats
    st = torch.zeros((N, Cout, 2), dtype=torch.float64, device=DEV)
    ya = conv(c.x, c.w, affine=c.aff.to(DEV), relu=1, out_stats=st)
    scale = c.fwd_aff.abs().max().item()
    e_aff = (ya.double() - c.fwd_aff.clamp_min(0)).abs().max().item() / scale
    e_exact = (ya.double() - c.fwd_exact.clamp_min(0)).abs().max().item() / scale
    e_stats = rel(st.cpu(), stat_table(ya, ya))
    print(dict(test="conv3d_bf16_c16_fwd", shape=shape, pair=pair, same=e_same, aff=e_aff, exact=e_exact, stats=e_stats))
    assert e_same < TOL_SAME and e_aff < TOL_AFF and e_exact < TOL_EXACT and e_stats < TOL_STATS
    assert (ya >= 0).all()
    # without ReLU and statistics: the pre-activation; with ReLU and no table: the same output bits
    yn = conv(c.x, c.w, affine=c.aff.to(DEV))
    assert rel(yn, c.fwd_aff) < TOL_AFF and torch.equal(yn.clamp_min(0), ya)
    assert torch.equal(ya, conv(c.x, c.w, affine=c.aff.to(DEV), relu=1))


@pytest.mark.parametrize("shape,pair", CASES)
def test_data_gradient_with_groupnorm_sums(shape, pair):
    c = case(shape, pair)
    N, (Cin, Cout) = shape[0], pair
    gst = torch.zeros((N, Cin, 2), dtype=torch.float64, device=DEV)
    xd = ndhwc(c.x)
    dg = conv(c.dz, c.w, mode=1, gx=xd, gstats=gst)  # the launch contracts over the layer's Cout and produces its Cin
    scale = c.dg.abs().max().item()
    e = (dg.double() - c.dg).abs().max().item() / scale
    e_exact = (dg.double() - c.dg_exact).abs().max().item() / scale
    e_stats = rel(gst.cpu(), stat_table(dg, c.x))
    print(dict(test="conv3d_bf16_c16_dgrad", shape=shape, pair=pair, err=e, exact=e_exact, stats=e_stats))
    assert e < TOL_SAME and e_exact < TOL_EXACT and e_stats < TOL_STATS
    assert torch.equal(dg, conv(c.dz, c.w, mode=1))  # gstats = NULL: the same output


@pytest.mark.parametrize("use_aff", [False, True])
@pytest.mark.parametrize("shape,pair", CASES)
def test_weight_gradient(shape, pair, use_aff):
    c = case(shape, pair)
    aff = c.aff.to(DEV) if use_aff else None
    ref = c.dw_aff if use_aff else c.dw_same
    dw = wgrad(c.x, c.dz, aff)
    scale = ref.abs().max().item()
    e = (dw.double() - ref).abs().max().item() / scale
    e_exact = (dw.double() - (c.dw_exact if use_aff else ref)).abs().max().item() / scale
    print(dict(test="conv3d_bf16_c16_wgrad", shape=shape, pair=pair, affine=use_aff, err=e, exact=e_exact))
    assert e < (TOL_AFF if use_aff else TOL_SAME) and e_exact < TOL_EXACT
    assert torch.equal(dw, wgrad(c.x, c.dz, aff))  # fixed-order reduction: the same inputs give a bitwise-identical dw


@pytest.mark.parametrize("pair", PAIRS)
def test_weight_gradient_plan_has_several_splits_and_runs_on_fewer_slots(pair):
    N, D, H, W = MULTI_SPLIT_SHAPE
    Cin, Cout = pair
    need = ext().u3d_wgrad_bf16_c16_workspace_floats(N, D, H, W, Cin, Cout)
    assert need // (27 * Cin * Cout) > 1, "the multi-split shape runs on one split"
    c = case(MULTI_SPLIT_SHAPE, pair)
    for slots in (1, 3):  # a smaller workspace: as many splits as it holds (another summation order: the accumulation-order bar)
        assert rel(wgrad(c.x, c.dz, slots=slots), c.dw_same) < TOL_SAME


def test_host_only_envelope_queries():
    lib = ext()
    assert lib.u3d_ext_version() == nat.U3D_EXT_VERSION
    for Cin, Cout, ok in [(16, 32, 1), (32, 16, 1), (16, 16, 1), (48, 16, 1), (80, 48, 1), (32, 32, 1), (8, 16, 0), (16, 24, 0), (0, 16, 0),
                          (16, -16, 0)]:
        assert lib.u3d_conv3d_bf16_c16_supported(Cin, Cout) == ok
        for mode in (0, 1):
            K, Nn = (Cin, Cout) if mode == 0 else (Cout, Cin)
            want = (K // 16) * 27 * ((Nn + 31) // 32) * 512 if ok else 0
            assert lib.u3d_packed_weight_bf16_c16_elems(Cin, Cout, mode) == want
        assert (lib.u3d_wgrad_bf16_c16_workspace_floats(1, 4, 4, 4, Cin, Cout) > 0) == bool(ok)
    assert lib.u3d_packed_weight_bf16_c16_elems(16, 32, 2) == 0
    assert lib.u3d_wgrad_bf16_c16_workspace_floats(0, 4, 4, 4, 16, 32) == 0


def _last_error():
    msg = nat.get_lib().u3d_last_error()
    return msg.decode() if msg else ""


def test_refusals_return_einval_set_the_last_error_and_launch_nothing():
    N, D, H, W = 1, 3, 4, 5
    lib = ext()
    st = _stream(DEV)

    def tensors(Cin, Cout):
        return (torch.randn(N, D, H, W, Cin + 4, device=DEV), torch.randn(N, D, H, W, Cout, device=DEV),
                torch.randn(Cout, Cin, 3, 3, 3, device=DEV), torch.full((1 << 16,), 7.0, dtype=torch.bfloat16, device=DEV),
                torch.full((N, D, H, W, Cout), 7.0, device=DEV), torch.full((Cout, Cin, 3, 3, 3), 7.0, device=DEV),
                torch.full((1 << 16,), 7.0, device=DEV))

    for Cin, Cout in [(8, 16), (16, 24)]:  # outside the envelope
        x, dz, w, img, y, dw, ws = tensors(Cin, Cout)
        rcs = [lib.u3d_pack_weights_bf16_c16(0, st, _p(w), Cout, Cin, 0, _p(img)),
               lib.u3d_conv3d_bf16_c16(0, st, _p(x), None, _p(img), _p(y), N, D, H, W, Cin, Cout, 0, None, None, None, None, 0),
               lib.u3d_conv3d_wgrad_bf16_c16(0, st, _p(x), None, _p(dz), _p(dw), N, D, H, W, Cin, Cout, _p(ws), ws.numel())]
        assert rcs == [nat.U3D_EINVAL] * 3 and "u3d_conv3d_wgrad_bf16_c16" in _last_error()
        with pytest.raises(nat.U3DError, match="16-channel bf16 envelope"):
            nat.call("u3d_conv3d_bf16_c16", 0, st, _p(x), None, _p(img), _p(y), N, D, H, W, Cin, Cout, 0, None, None, None, None, 0)
        torch.cuda.synchronize()
        assert (img == 7.0).all() and (y == 7.0).all() and (dw == 7.0).all() and (ws == 7.0).all()
    Cin, Cout = 16, 32
    x, dz, w, img, y, dw, ws = tensors(Cin, Cout)
    # a misaligned pointer
    assert lib.u3d_conv3d_bf16_c16(0, st, x.data_ptr() + 4, None, _p(img), _p(y), N, D, H, W, Cin, Cout, 0, None, None, None, None,
                                   0) == nat.U3D_EINVAL
    assert "aligned" in _last_error()
    assert lib.u3d_conv3d_wgrad_bf16_c16(0, st, x.data_ptr() + 4, None, _p(dz), _p(dw), N, D, H, W, Cin, Cout, _p(ws),
                                         ws.numel()) == nat.U3D_EINVAL
    assert "aligned" in _last_error()
    # a workspace smaller than one slot
    assert lib.u3d_conv3d_wgrad_bf16_c16(0, st, _p(x), None, _p(dz), _p(dw), N, D, H, W, Cin, Cout, _p(ws),
                                         27 * Cin * Cout - 1) == nat.U3D_EINVAL
    assert "workspace too small" in _last_error()
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (dw == 7.0).all() and (ws == 7.0).all()
