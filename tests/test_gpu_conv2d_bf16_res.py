"""-m gpu: u3d_conv2d_bf16_res through the C-ABI — out = [relu](conv2d(bf16(a*x + b), bf16(w)) + residual), the epilogue of conv3 of a
ResNetBlock under `native_2d_residual_bf16` (csrc/u3d_conv2d_bf16.hip) — on both launch plans: the unsplit kernel's fused epilogue (one and
two n-tiles per block) and the split-K launch, whose reduction kernel owns residual, ReLU and statistics.

Reference: float64 conv2d of the bf16-rounded operands (the activation after the fp32 affine) plus the residual in float64, then ReLU.
Bars: those of tests/test_gpu_conv2d_bf16.py, imported — 1e-4 of the output range with an identity affine, 1e-3 with a random one, the
statistics tables at 1e-5 of their maximum against float64 sums of the written output.  The residual is one exact fp32 add onto the fp32
accumulator and earns no margin of its own.  Which plan a shape runs is asserted through u3d_conv2d_bf16_variant (the plan does not depend
on the residual)."""
from functools import cached_property

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv2d_bf16 as K
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import _p, _stream

pytestmark = pytest.mark.gpu
TOL_SAME, TOL_AFF, TOL_STATS = K.TOL_SAME, K.TOL_AFF, K.TOL_STATS

# (N, H, W, Cin, Cout)
NT1_SHAPES = [(2, 35, 45, 32, 32), (2, 35, 45, 64, 64)]      # 18 ragged tiles: one n-tile per block, unsplit without a workspace
NT2_SHAPES = [(2, 250, 245, 64, 64), (2, 250, 245, 32, 96)]  # 512 ragged tiles: the 64-channel block; 96: a zero fragment in the last block
SPLIT_SHAPES = [(1, 9, 11, 128, 128), (2, 16, 16, 128, 128)]  # 1 and 2 tiles, 8 chunks: split-K whenever a workspace is passed
GUARD = 4096  # floats behind the output and the residual: a store or a load past Cout of the last pixel lands here


class Case:
    """inputs and float64 references of one shape, computed once when first asked for and shared (never modified)"""

    def __init__(self, shape):
        N, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(7000 + H * W + Cin + 3 * Cout)
        self.shape = shape
        self.x = torch.randn(N, Cin, H, W, generator=g)
        self.w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
        self.res = torch.randn(N, Cout, H, W, generator=g)  # of the convolution's own size: neither term hides the other
        a = 1.0 + 0.3 * torch.randn(N, Cin, generator=g)
        b = 0.5 + 0.2 * torch.randn(N, Cin, generator=g)
        self.aff = torch.stack((a, b), dim=-1).contiguous()
        self.g = self.x * a.view(N, Cin, 1, 1) + b.view(N, Cin, 1, 1)  # the affine in fp32, as the kernel applies it

    @cached_property
    def conv_same(self):  # identity affine, before the residual
        return F.conv2d(K.r16(self.x), K.r16(self.w), padding=1)

    @cached_property
    def conv_aff(self):
        return F.conv2d(K.r16(self.g), K.r16(self.w), padding=1)

    def ref(self, affine: bool, relu: bool):
        y = (self.conv_aff if affine else self.conv_same) + self.res.double()
        return y.clamp_min(0) if relu else y


_CASES = {}


def case(shape) -> Case:
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


def conv_res(c: Case, affine=False, relu=1, reps=1, use_ws=True, stats=True, residual="own", entry="u3d_conv2d_bf16_res"):
    """one launch on the case's tensors; output and residual sit in front of guard bands.  Returns ((N,Cout,H,W) cpu, summed (N,Cout,2)
    table or None, the raw replica rows, workspace floats)"""
    N, H, W, Cin, Cout = c.shape
    wp, xd = K.pack(c.w, 0), K.nhwc(c.x)
    n_out = N * H * W * Cout
    ybuf = torch.full((n_out + GUARD,), 7.0, dtype=torch.float32, device=DEV)
    rbuf = torch.full((n_out + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    if isinstance(residual, str):
        rbuf[:n_out] = K.nhwc(c.res).flatten()
    else:
        rbuf[:n_out] = residual
    need = nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, Cin, Cout) if use_ws else 0
    ws = torch.empty(need, dtype=torch.float32, device=DEV) if need > 0 else None
    st = torch.zeros((reps, N, Cout, 2), dtype=torch.float64, device=DEV) if stats else None
    aff = c.aff.to(DEV) if affine else None
    args = [0, _stream(DEV), _p(xd), _p(aff), _p(wp), _p(ybuf), N, H, W, Cin, Cout, relu, _p(st), None, None, _p(ws), need, reps]
    if entry == "u3d_conv2d_bf16_res":
        args.append(_p(rbuf))
    nat.call(entry, *args)
    torch.cuda.synchronize()
    assert (ybuf[n_out:] == 7.0).all(), "a store past the output"
    y = K.nchw(ybuf[:n_out].view(N, H, W, Cout))
    rows = st.cpu() if stats else None
    return y, (rows.sum(0) if stats else None), rows, need


def check(shape, affine, relu, reps, use_ws):
    """one launch against float64 and its statistics against the written output; returns (output, (n-tiles per block, ksplit))"""
    c = case(shape)
    var = K.fwd_variant(*shape, use_ws)
    y, s, rows, need = conv_res(c, affine=affine, relu=relu, reps=reps, use_ws=use_ws)
    assert torch.isfinite(y).all()  # (the guard behind the residual is NaN: a load past Cout that reaches an output shows here)
    assert (need > 0) == (var[1] > 1)
    ref = c.ref(affine, bool(relu))
    scale = c.ref(affine, False).abs().max().item()
    e = (y.double() - ref).abs().max().item() / scale
    table = torch.stack((y.double().sum(dim=(2, 3)), (y.double() ** 2).sum(dim=(2, 3))), dim=-1)
    e_stats = K.rel(s, table)
    print(dict(test="conv2d_bf16_res", shape=shape, nt=var[0], ksplit=var[1], affine=affine, relu=relu, reps=reps, err=e, stats=e_stats))
    assert e < (TOL_AFF if affine else TOL_SAME)
    assert e_stats < TOL_STATS
    if var[1] > 1:  # the reduction kernel writes replica row 0
        assert rows[1:].abs().sum() == 0
    return y, var


@pytest.mark.parametrize("reps", [1, 2])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", NT1_SHAPES)
def test_unsplit_one_n_tile_fused_epilogue(shape, relu, reps):
    """conv2d_bf16_kernel<1>, no workspace: residual, ReLU and the statistics (replica rows) in the fused epilogue on ragged tiles"""
    for affine in (False, True):
        _, (nt, ksplit) = check(shape, affine, relu, reps, use_ws=False)
        assert nt == 1 and ksplit == 1, f"nt {nt}, ksplit {ksplit} on {K.cus()} CUs"


@pytest.mark.parametrize("shape", NT2_SHAPES)
def test_unsplit_64_channel_block(shape):
    """conv2d_bf16_kernel<2>: both n-tiles add their residual columns; with three n-tiles the zero fragment of the last block neither reads
    the residual nor writes the output past Cout (guard bands, and every value checked)"""
    try:
        for affine, relu in ((False, 0), (True, 1)):
            _, (nt, ksplit) = check(shape, affine, relu, 2, use_ws=True)
            assert nt == 2 and ksplit == 1, f"nt {nt}, ksplit {ksplit} on {K.cus()} CUs"
    finally:
        _CASES.pop(shape, None)  # (~100 MB of references that no other test uses)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", SPLIT_SHAPES)
def test_split_k_reduction_owns_residual_relu_and_statistics(shape, relu):
    for affine in (False, True):
        _, (nt, ksplit) = check(shape, affine, relu, 2, use_ws=True)
        assert ksplit > 1, f"nt {nt}, ksplit {ksplit} on {K.cus()} CUs"


@pytest.mark.parametrize("shape", SPLIT_SHAPES)
def test_unsplit_and_split_k_agree(shape):
    """the same layer without the scratch runs the fused epilogue: the two plans differ in the order of the fp32 sums only"""
    c = case(shape)
    assert K.fwd_variant(*shape, True)[1] > 1 and K.fwd_variant(*shape, False)[1] == 1, f"{K.cus()} CUs"
    y_split, s_split, _, _ = conv_res(c, relu=1, use_ws=True)
    y_one, s_one, _, _ = conv_res(c, relu=1, use_ws=False)
    scale = c.ref(False, False).abs().max().item()
    e = (y_split.double() - y_one.double()).abs().max().item() / scale
    print(dict(test="conv2d_bf16_res_split_vs_unsplit", shape=shape, err=e))
    assert e < TOL_SAME
    assert K.rel(s_split, s_one) < 1e-4  # (sums of outputs that agree to TOL_SAME)


@pytest.mark.parametrize("shape,use_ws", [(NT1_SHAPES[0], False), (SPLIT_SHAPES[1], True)])
def test_two_calls_are_bitwise_equal(shape, use_ws):
    c = case(shape)
    a = conv_res(c, affine=True, relu=1, use_ws=use_ws)[0]
    b = conv_res(c, affine=True, relu=1, use_ws=use_ws)[0]
    assert torch.equal(a, b)


@pytest.mark.parametrize("shape,use_ws", [(NT1_SHAPES[1], False), (SPLIT_SHAPES[0], True)])
def test_zero_residual_is_the_plain_entry_point_bit_for_bit(shape, use_ws):
    """the existing entry point is unchanged by the new epilogue: adding an exact zero (ReLU off) gives u3d_conv2d_bf16's own output, and its
    statistics (signed zeros compare equal)"""
    c = case(shape)
    y0, s0, _, _ = conv_res(c, affine=True, relu=0, use_ws=use_ws, entry="u3d_conv2d_bf16")
    y1, s1, _, _ = conv_res(c, affine=True, relu=0, use_ws=use_ws, residual=0.0)
    assert torch.equal(y0, y1)
    assert torch.equal(s0, s1) or K.rel(s1, s0) < 1e-12  # (f64 atomics: the blocks' order is not fixed)
    # ... and the plain entry point still matches float64 without the residual
    assert K.rel(y0, c.conv_aff) < TOL_AFF


def test_bad_arguments_are_refused_without_a_launch():
    N, H, W, Cin, Cout = shape = NT1_SHAPES[0]
    c = case(shape)
    wp, xd, rd = K.pack(c.w, 0), K.nhwc(c.x), K.nhwc(c.res)
    y = torch.full((N, H, W, Cout), 7.0, device=DEV)
    gst = torch.zeros((N, Cout, 2), dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    tail = (_p(ws), ws.numel(), 1)  # every refusal below is U3D_EINVAL (-1)
    head = (0, _stream(DEV), _p(xd), None, _p(wp), _p(y), N, H, W)
    with pytest.raises(nat.U3DError, match="code -1:"):  # residual together with gx / gstats
        nat.call("u3d_conv2d_bf16_res", *head, Cin, Cout, 1, None, _p(rd), _p(gst), *tail, _p(rd))
    with pytest.raises(nat.U3DError, match="code -1:"):  # gstats alone
        nat.call("u3d_conv2d_bf16_res", *head, Cin, Cout, 1, None, None, _p(gst), *tail, _p(rd))
    with pytest.raises(nat.U3DError, match="code -1:"):  # no residual
        nat.call("u3d_conv2d_bf16_res", *head, Cin, Cout, 1, None, None, None, *tail, None)
    with pytest.raises(nat.U3DError, match="code -1:"):  # outside the envelope
        nat.call("u3d_conv2d_bf16_res", *head, 20, Cout, 1, None, None, None, *tail, _p(rd))
    with pytest.raises(nat.U3DError, match="code -1:"):  # a residual that is not 16-byte aligned
        nat.call("u3d_conv2d_bf16_res", *head, Cin, Cout, 1, None, None, None, *tail, _p(rd.flatten()[1:]))
    assert nat.get_lib().u3d_last_error()
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (gst == 0).all()  # nothing was launched
