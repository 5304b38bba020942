"""-m gpu: the `_c16` entry points of csrc/u3d_conv2d_bf16.hip through the C-ABI (`native_2d_stem` next to `native_2d_bf16`): the bf16
Conv2d 3x3 forward, data gradient and weight gradient for layers whose channel counts are multiples of 16 — half n-tiles in the image,
masked epilogue stores and statistics, zero-staged channel octets and masked dw stores in the weight gradient.

Reference and bars are those of tests/test_gpu_conv2d_bf16.py, unchanged: float64 F.conv2d / autograd on the CPU with the SAME operand
rounding restated, 1e-4 of the result's range with an identity affine (accumulation order only), 1e-3 with a random affine, 2e-2 against
the exact operands; statistics tables 1e-5 of the table's maximum against float64 sums of the written output.

Every plan is asserted through u3d_conv2d_bf16_c16_variant / u3d_conv2d_wgrad_bf16_c16_variant (`_c16` keeps the split-K plan: each
shape runs with and without the workspace).  Outputs are pre-filled with NaN in front of a guard band: a store at co >= Cout of the last
pixel lands there, one of any other pixel in its neighbour's record."""
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
TOL_STATS = 1e-5  # a statistics table against float64 sums of the written output, relative to the table's maximum
GUARD = 1024
GUARD_VALUE = -12345.0

# LAYERS (N, H, W, Cin, Cout); the forward launch is (Cin -> Cout), the data gradient's contracts over Cout and produces Cin
SHAPES = [
    (2, 19, 21, 32, 16),   # half an n-tile produced, ragged 2 x 2 tiles, two K chunks
    (1, 16, 16, 16, 16),   # one tile, one chunk, half an n-tile in both directions
    (1, 35, 45, 48, 80),   # three chunks, 2.5 n-tiles (data gradient: five chunks, 1.5 n-tiles)
    (1, 33, 17, 32, 48),   # 1.5 n-tiles
]
PRODUCTION_SHAPE = (1, 250, 245, 32, 16)  # 256 ragged tiles: the plan of a full-resolution stem layer — one n-tile per block, unsplit
# (forward ksplit with a workspace, data-gradient ksplit with a workspace) on the 256 CUs of an MI355X: blocks < CUs split the chunks
KSPLIT = {SHAPES[0]: (2, 1), SHAPES[1]: (1, 1), SHAPES[2]: (3, 5), SHAPES[3]: (2, 3), PRODUCTION_SHAPE: (1, 1)}
WGRAD_MULTI_TILE_SHAPE = (1, 520, 523, 16, 32)  # 33 x 33 = 1089 ragged tiles on one channel cell: 2 tiles per block


def r16(t):
    return t.float().to(torch.bfloat16).double()


def nhwc(x):
    return x.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(y):
    return y.permute(0, 3, 1, 2).contiguous().cpu()


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


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


def fwd_variant(N, H, W, Cin, Cout, use_ws, sfx="_c16"):
    v = getattr(nat.get_lib(), f"u3d_conv2d_bf16{sfx}_variant")(N, H, W, Cin, Cout, 1 if use_ws else 0)
    assert v > 0, (v, (N, H, W, Cin, Cout))
    return v & 255, v >> 8


def wgrad_variant(N, H, W, Cin, Cout, sfx="_c16"):
    v = getattr(nat.get_lib(), f"u3d_conv2d_wgrad_bf16{sfx}_variant")(N, H, W, Cin, Cout)
    assert v > 0, (v, (N, H, W, Cin, Cout))
    return v >> 16, v & 0xFFFF


def pack(w, mode, sfx="_c16"):
    Cout, Cin = w.shape[:2]
    n = getattr(nat.get_lib(), f"u3d_packed_weight2d_bf16{sfx}_elems")(Cin, Cout, mode)
    assert n > 0
    buf = torch.full((n + GUARD,), 3.0, dtype=torch.bfloat16, device=DEV)
    buf[:n] = float("nan")
    wd = w.float().contiguous().to(DEV)
    nat.call("u3d_pack_weights2d_bf16" + sfx, 0, _stream(DEV), _p(wd), Cout, Cin, mode, _p(buf))
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:n].float()).all() and (buf[n:] == 3.0).all()
    return buf[:n]


def conv(x, w, mode=0, affine=None, relu=0, out_stats=None, gx=None, gstats=None, reps=1, use_ws=True, sfx="_c16"):
    """one launch on x (N,C,H,W) cpu; mode 1: x is dz and w the forward weight.  Returns (N,K,H,W) cpu"""
    N, C, H, W = x.shape
    K = w.shape[0] if mode == 0 else w.shape[1]
    wp, xd = pack(w, mode, sfx), nhwc(x)
    y, ybuf = guarded((N, H, W, K))
    need = getattr(nat.get_lib(), f"u3d_conv2d_bf16{sfx}_workspace_floats")(N, H, W, C, K) if use_ws else 0
    ws = torch.empty(need, dtype=torch.float32, device=DEV) if need > 0 else None
    nat.call("u3d_conv2d_bf16" + sfx, 0, _stream(DEV), _p(xd), _p(affine), _p(wp), _p(y), N, H, W, C, K, relu, _p(out_stats), _p(gx),
             _p(gstats), _p(ws), need, reps)
    torch.cuda.synchronize()
    check_guard(y, ybuf, "out")
    return nchw(y)


def wgrad(x, dz, affine=None, sfx="_c16"):
    N, C, H, W = x.shape
    K = dz.shape[1]
    need = getattr(nat.get_lib(), f"u3d_wgrad2d_bf16{sfx}_workspace_floats")(N, H, W, C, K)
    ws = torch.full((need + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ws[need:] = GUARD_VALUE
    dw, dwbuf = guarded((K, C, 3, 3))
    xd, dzd = nhwc(x), nhwc(dz)
    nat.call("u3d_conv2d_wgrad_bf16" + sfx, 0, _stream(DEV), _p(xd), _p(affine), _p(dzd), _p(dw), N, H, W, C, K, _p(ws), need)
    torch.cuda.synchronize()
    check_guard(dw, dwbuf, "dw")
    assert (ws[need:] == GUARD_VALUE).all().item(), "the workspace's guard band was touched"
    return dw.cpu()


class Case:
    """inputs and float64 references of one layer shape, each computed once, when first asked for, and shared by the tests"""

    def __init__(self, shape):
        N, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(2000 + H * W + Cin + Cout)
        self.shape = shape
        self.x = torch.randn(N, Cin, H, W, generator=g)
        self.w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
        self.dz = torch.randn(N, Cout, H, W, generator=g)
        a = 1.0 + 0.3 * torch.randn(N, Cin, generator=g)
        b = 0.5 + 0.2 * torch.randn(N, Cin, generator=g)  # a clearly nonzero offset: padding must not pick it up
        self.aff = torch.stack((a, b), dim=-1).contiguous()
        self.g = self.x * a.view(N, Cin, 1, 1) + b.view(N, Cin, 1, 1)  # the affine in fp32, as the kernel applies it

    @cached_property
    def fwd_same(self):
        return F.conv2d(r16(self.x), r16(self.w), padding=1)

    @cached_property
    def fwd_aff(self):
        return F.conv2d(r16(self.g), r16(self.w), padding=1)

    @cached_property
    def fwd_exact(self):
        return F.conv2d(self.g.double(), self.w.double(), padding=1)

    @cached_property
    def dg(self):
        return torch.nn.grad.conv2d_input(self.x.shape, r16(self.w), r16(self.dz), padding=1)

    @cached_property
    def dg_exact(self):
        return torch.nn.grad.conv2d_input(self.x.shape, self.w.double(), self.dz.double(), padding=1)

    @cached_property
    def dw_same(self):
        return torch.nn.grad.conv2d_weight(r16(self.x), self.w.shape, r16(self.dz), padding=1)

    @cached_property
    def dw_aff(self):
        return torch.nn.grad.conv2d_weight(r16(self.g), self.w.shape, r16(self.dz), padding=1)

    @cached_property
    def dw_exact(self):
        return torch.nn.grad.conv2d_weight(self.g.double(), self.w.shape, self.dz.double(), padding=1)


_CASES = {}


def case(shape) -> Case:
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


def _border(t):
    m = torch.zeros(t.shape[-2:], dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return t[..., m]


def stat_table(y, other):
    y = y.double()
    return torch.stack((y.sum(dim=(2, 3)), (y * other.double()).sum(dim=(2, 3))), dim=-1)


def check_forward(shape, use_ws):
    """affine, ReLU, out_stats and the border of one forward launch; returns its plan (n-tiles per block, ksplit)"""
    c = case(shape)
    N, H, W, Cin, Cout = shape
    var = fwd_variant(N, H, W, Cin, Cout, use_ws)
    st = torch.zeros((N, Cout, 2), dtype=torch.float64, device=DEV)
    y = conv(c.x, c.w, affine=c.aff.to(DEV), relu=1, out_stats=st, use_ws=use_ws)
    ref = c.fwd_aff.clamp_min(0)
    scale = c.fwd_aff.abs().max().item()
    e = (y.double() - ref).abs().max().item() / scale
    e_border = (_border(y.double()) - _border(ref)).abs().max().item() / scale
    e_exact = (y.double() - c.fwd_exact.clamp_min(0)).abs().max().item() / scale
    e_stats = rel(st.cpu(), stat_table(y, y))
    print(dict(test="conv2d_bf16_c16_fwd", shape=shape, nt=var[0], ksplit=var[1], err=e, border=e_border, exact=e_exact, stats=e_stats))
    assert e < TOL_AFF and e_border < TOL_AFF and e_exact < TOL_EXACT and e_stats < TOL_STATS
    y2 = conv(c.x, c.w, affine=c.aff.to(DEV), relu=1, use_ws=use_ws)  # out_stats = NULL: the same output
    assert torch.equal(y, y2)
    return var


def check_data_gradient(shape, use_ws):
    """gx / gstats of one data-gradient launch of the LAYER `shape`; returns its plan"""
    c = case(shape)
    N, H, W, Cin, Cout = shape
    var = fwd_variant(N, H, W, Cout, Cin, use_ws)  # the launch contracts over the layer's Cout
    gst = torch.zeros((N, Cin, 2), dtype=torch.float64, device=DEV)
    xd = nhwc(c.x)
    dg = conv(c.dz, c.w, mode=1, gx=xd, gstats=gst, use_ws=use_ws)
    scale = c.dg.abs().max().item()
    e = (dg.double() - c.dg).abs().max().item() / scale
    e_exact = (dg.double() - c.dg_exact).abs().max().item() / scale
    e_stats = rel(gst.cpu(), stat_table(dg, c.x))
    print(dict(test="conv2d_bf16_c16_dgrad", shape=shape, nt=var[0], ksplit=var[1], err=e, exact=e_exact, stats=e_stats))
    assert e < TOL_SAME and e_exact < TOL_EXACT and e_stats < TOL_STATS
    return var


def check_weight_gradient(shape, use_aff, exact=True):
    c = case(shape)
    var = wgrad_variant(*shape)
    aff = c.aff.to(DEV) if use_aff else None
    ref = c.dw_aff if use_aff else c.dw_same
    dw = wgrad(c.x, c.dz, aff)
    scale = ref.abs().max().item()
    e = (dw.double() - ref).abs().max().item() / scale
    print(dict(test="conv2d_bf16_c16_wgrad", shape=shape, tps=var[0], nsplit=var[1], affine=use_aff, err=e))
    assert e < (TOL_AFF if use_aff else TOL_SAME)
    if use_aff and exact:
        assert (dw.double() - c.dw_exact).abs().max().item() < TOL_EXACT * scale
    assert torch.equal(dw, wgrad(c.x, c.dz, aff))  # fixed-order reduction: the same inputs give a bitwise-identical dw
    return var


@pytest.mark.parametrize("use_ws", [True, False])
@pytest.mark.parametrize("shape", SHAPES + [PRODUCTION_SHAPE])
def test_forward_affine_relu_stats_and_zero_padding(shape, use_ws):
    try:
        nt, ksplit = check_forward(shape, use_ws)
    finally:
        if shape == PRODUCTION_SHAPE and not use_ws:
            _CASES.pop(shape, None)
    assert nt == 1 and ksplit == (KSPLIT[shape][0] if use_ws else 1), f"nt {nt}, ksplit {ksplit} on {cus()} CUs"


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_identity_affine_matches_to_accumulation_order(shape):
    c = case(shape)
    y = conv(c.x, c.w)
    e = rel(y, c.fwd_same)
    print(dict(test="conv2d_bf16_c16_fwd_same", shape=shape, err=e))
    assert e < TOL_SAME
    N, Cin = shape[0], shape[3]
    ida = torch.tensor([1.0, 0.0]).repeat(N, Cin, 1).contiguous().to(DEV)
    assert torch.equal(y, conv(c.x, c.w, affine=ida))


PRODUCTION_DGRAD_SHAPE = (1, 250, 245, 16, 32)  # the layer 16 -> 32: its data gradient is the 32 -> 16 launch of PRODUCTION_SHAPE


@pytest.mark.parametrize("use_ws", [True, False])
@pytest.mark.parametrize("shape", SHAPES + [PRODUCTION_DGRAD_SHAPE])
def test_data_gradient_with_groupnorm_sums(shape, use_ws):
    try:
        nt, ksplit = check_data_gradient(shape, use_ws)
    finally:
        if shape == PRODUCTION_DGRAD_SHAPE and not use_ws:
            _CASES.pop(shape, None)
    want = KSPLIT[shape][1] if shape in KSPLIT else 1
    assert nt == 1 and ksplit == (want if use_ws else 1), f"nt {nt}, ksplit {ksplit} on {cus()} CUs"


@pytest.mark.parametrize("reps", [1, 4])
def test_replica_rows_sum_to_the_one_row_table(reps):
    shape = SHAPES[0]
    c = case(shape)
    N, H, W, Cin, Cout = shape
    t1 = torch.zeros((1, N, Cout, 2), dtype=torch.float64, device=DEV)
    tr = torch.zeros((reps, N, Cout, 2), dtype=torch.float64, device=DEV)
    y1 = conv(c.x, c.w, relu=1, out_stats=t1, reps=1, use_ws=False)
    y2 = conv(c.x, c.w, relu=1, out_stats=tr, reps=reps, use_ws=False)
    assert torch.equal(y1, y2)
    assert rel(tr.sum(0).cpu(), t1[0].cpu()) < 1e-12
    assert rel(t1[0].cpu(), stat_table(y1, y1)) < TOL_STATS


@pytest.mark.parametrize("use_aff", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(1, 16, 16, 16, 32)])
def test_weight_gradient(shape, use_aff):
    tps, nsplit = check_weight_gradient(shape, use_aff)
    assert tps == 1, f"tps {tps}, nsplit {nsplit} on {cus()} CUs"


@pytest.mark.parametrize("use_aff", [False, True])
def test_weight_gradient_multi_tile_blocks(use_aff):
    try:
        tps, nsplit = check_weight_gradient(WGRAD_MULTI_TILE_SHAPE, use_aff, exact=False)
    finally:
        if use_aff:
            _CASES.pop(WGRAD_MULTI_TILE_SHAPE, None)
    assert tps >= 2 and nsplit > 1, f"tps {tps}, nsplit {nsplit} on {cus()} CUs"


@pytest.mark.parametrize("shape", [(2, 17, 19, 32, 32), (1, 8, 8, 64, 32)])
def test_inside_the_old_envelope_the_c16_entry_points_equal_the_old_ones_bit_for_bit(shape):
    c = case(shape)
    N, H, W, Cin, Cout = shape
    for mode in (0, 1):
        assert torch.equal(pack(c.w, mode, "_c16").view(torch.int16), pack(c.w, mode, "").view(torch.int16))
    aff = c.aff.to(DEV)
    for use_ws in (True, False):
        assert fwd_variant(N, H, W, Cin, Cout, use_ws, "_c16") == fwd_variant(N, H, W, Cin, Cout, use_ws, "")
        outs = []
        for sfx in ("_c16", ""):
            st = torch.zeros((N, Cout, 2), dtype=torch.float64, device=DEV)
            gst = torch.zeros((N, Cin, 2), dtype=torch.float64, device=DEV)
            y = conv(c.x, c.w, affine=aff, relu=1, out_stats=st, use_ws=use_ws, sfx=sfx)
            dg = conv(c.dz, c.w, mode=1, gx=nhwc(c.x), gstats=gst, use_ws=use_ws, sfx=sfx)
            outs.append((y, dg))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert wgrad_variant(*shape, "_c16") == wgrad_variant(*shape, "")
    assert torch.equal(wgrad(c.x, c.dz, aff, "_c16"), wgrad(c.x, c.dz, aff, ""))


@pytest.mark.parametrize("Cin,Cout", [(20, 32), (32, 8)])
def test_channel_counts_outside_the_envelope_are_refused(Cin, Cout):
    N, H, W = 1, 6, 7
    x = torch.randn(N, H, W, Cin, device=DEV)
    dz = torch.randn(N, H, W, Cout, device=DEV)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV)
    img = torch.full((4096,), 7.0, dtype=torch.bfloat16, device=DEV)
    y = torch.full((N, H, W, Cout), 7.0, device=DEV)
    dw = torch.full((Cout, Cin, 3, 3), 7.0, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    with pytest.raises(nat.U3DError):
        nat.call("u3d_pack_weights2d_bf16_c16", 0, _stream(DEV), _p(w), Cout, Cin, 0, _p(img))
    with pytest.raises(nat.U3DError):
        nat.call("u3d_conv2d_bf16_c16", 0, _stream(DEV), _p(x), None, _p(img), _p(y), N, H, W, Cin, Cout, 0, None, None, None, _p(ws),
                 ws.numel(), 1)
    with pytest.raises(nat.U3DError):
        nat.call("u3d_conv2d_wgrad_bf16_c16", 0, _stream(DEV), _p(x), None, _p(dz), _p(dw), N, H, W, Cin, Cout, _p(ws), ws.numel())
    torch.cuda.synchronize()
    assert (img == 7.0).all() and (y == 7.0).all() and (dw == 7.0).all()  # nothing was launched
