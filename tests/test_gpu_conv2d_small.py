"""-m gpu: the small-Cin 2-D kernels of csrc/u3d_conv2d.hip through the C-ABI (`native_2d_stem`): u3d_conv2d_small_cin_fwd_reps and
u3d_conv2d_small_cin_bwd, the 2-D twins of the first-layer kernels of csrc/u3d_smallc.hip — against float64 F.conv2d and its autograd on
the CPU.

Bars: those tests/test_gpu_kernels.py::test_small_cin_first_layer_kernels holds the 3-D twins to — forward at that file's TOL (2e-5 of the
result's range), statistics 1e-5, dw 1e-4, (sum dg, sum dg * x) 1e-4.

Which plan a shape runs is asserted through the host-only u3d_conv2d_small_cin_fwd_variant / _bwd_variant queries: SHAPES are the smallest
that can go wrong (ragged tiles, odd channel counts, the direct and the matrix-pipe forward, one and two row tiles of 16 channels, one
and several partials), PLAN_SHAPES add what only a larger grid reaches: a block that walks several tiles.  Every output is pre-filled
with NaN in front of a guard band, the workspace too."""
from functools import cached_property

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV, relerr
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import _p, _stream

pytestmark = pytest.mark.gpu
TOL = 2e-5        # tests/test_gpu_kernels.py
TOL_STATS = 1e-5
TOL_DW = 1e-4
TOL_GSTATS = 1e-4
GUARD = 1024      # floats behind every output
GUARD_VALUE = -12345.0

# (N, H, W, Cin, Cout)
SHAPES = [
    (2, 19, 21, 1, 16),   # the first layer of the default net: ragged 2 x 2 tiles, matrix pipe, one row tile
    (1, 16, 16, 3, 32),   # exactly one tile: two row tiles, ONE partial in the backward reduction
    (1, 35, 45, 2, 8),    # 3 x 3 ragged tiles, half a row tile
    (1, 5, 3, 4, 12),     # smaller than a tile, Cin = 4
    (1, 7, 5, 1, 6),      # Cout % 4 != 0: the direct forward kernel
]
# 23 x 23 = 529 tiles per sample, two samples: more than the 256 (forward) / 512 (backward) blocks a sample gets
PLAN_SHAPES = [
    (2, 368, 368, 1, 16),  # the production plan: several tiles per block, matrix pipe
    (2, 368, 368, 2, 6),   # ... on the direct forward kernel
    (2, 368, 368, 4, 32),  # ... with two row tiles
]
FWD_PLANS = {SHAPES[0]: 1, SHAPES[1]: 1, SHAPES[2]: 1, SHAPES[3]: 1, SHAPES[4]: 0, PLAN_SHAPES[0]: 3, PLAN_SHAPES[1]: 2, PLAN_SHAPES[2]: 3}
BWD_PLANS = {SHAPES[0]: 4, SHAPES[1]: 1, SHAPES[2]: 4, SHAPES[3]: 0, SHAPES[4]: 0, PLAN_SHAPES[0]: 6, PLAN_SHAPES[1]: 6, PLAN_SHAPES[2]: 7}


def nhwc(x):  # (N,C,H,W) cpu -> (N,H,W,C) gpu
    return x.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(y):  # (N,H,W,C) gpu -> (N,C,H,W) cpu
    return y.permute(0, 3, 1, 2).contiguous().cpu()


def guarded(shape, dtype=torch.float32):
    """(view of `shape` filled with NaN, whole buffer with a guard band behind the view)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), GUARD_VALUE, dtype=dtype, device=DEV)
    view = buf[:n].view(shape)
    view.fill_(float("nan"))
    return view, buf


def check_guard(view, buf, what):
    assert torch.isfinite(view).all().item(), f"{what}: not every element was written"
    assert (buf[view.numel():] == GUARD_VALUE).all().item(), f"{what}: the guard band was touched"


class Case:
    """inputs and float64 references of one shape, computed once, when first asked for, and shared by the tests (never modified)"""

    def __init__(self, shape):
        N, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(77 + H * W + 17 * Cin + Cout)
        self.shape = shape
        self.x = torch.randn(N, Cin, H, W, generator=g)
        self.w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        self.dz = torch.randn(N, Cout, H, W, generator=g)
        a = 1.0 + 0.3 * torch.randn(N, Cin, generator=g)
        b = 0.5 + 0.2 * torch.randn(N, Cin, generator=g)  # a clearly nonzero offset: padding must not pick it up
        self.aff = torch.stack((a, b), dim=-1).contiguous()

    def _run(self, use_aff):
        N, H, W, Cin, Cout = self.shape
        xl = self.x.double()
        wl = self.w.double().requires_grad_(True)
        a, b = (self.aff[..., 0].double(), self.aff[..., 1].double()) if use_aff else (torch.ones(N, Cin).double(), torch.zeros(N, Cin).double())
        g = (xl * a.view(N, Cin, 1, 1) + b.view(N, Cin, 1, 1)).requires_grad_(True)
        z = F.conv2d(g, wl, None, padding=1)
        z.backward(self.dz.double())
        dg = g.grad
        gst = torch.stack((dg.sum(dim=(2, 3)), (dg * xl).sum(dim=(2, 3))), dim=-1)
        return z.detach(), wl.grad, gst

    @cached_property
    def with_affine(self):  # (z, dw, gstats)
        return self._run(True)

    @cached_property
    def plain(self):
        return self._run(False)


_CASES = {}


def case(shape) -> Case:
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


def forward(c: Case, use_aff, relu, reps=1, stats=True):
    """one forward launch; returns ((N,Cout,H,W) cpu, (reps,N,Cout,2) cpu or None)"""
    N, H, W, Cin, Cout = c.shape
    y, ybuf = guarded((N, H, W, Cout))
    st = torch.zeros((reps, N, Cout, 2), dtype=torch.float64, device=DEV) if stats else None
    xd, ad, wd = nhwc(c.x), (c.aff.to(DEV) if use_aff else None), c.w.contiguous().to(DEV)
    nat.call("u3d_conv2d_small_cin_fwd_reps", 0, _stream(DEV), _p(xd), _p(ad), _p(wd), _p(y), N, H, W, Cin, Cout, relu, _p(st), reps)
    torch.cuda.synchronize()
    check_guard(y, ybuf, "out")
    return nchw(y), (st.cpu() if stats else None)


def backward(c: Case, use_aff, gstats=True):
    """one backward launch; returns (dw cpu, (N,Cin,2) cpu or None)"""
    N, H, W, Cin, Cout = c.shape
    need = nat.get_lib().u3d_small_cin2d_bwd_workspace_floats(N, H, W, Cin, Cout)
    assert need > 0
    ws = torch.full((need + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ws[need:] = GUARD_VALUE
    dw, dwbuf = guarded((Cout, Cin, 3, 3))
    gst = torch.zeros((N, Cin, 2), dtype=torch.float64, device=DEV) if gstats else None
    xd, dzd, ad, wd = nhwc(c.x), nhwc(c.dz), (c.aff.to(DEV) if use_aff else None), c.w.contiguous().to(DEV)
    nat.call("u3d_conv2d_small_cin_bwd", 0, _stream(DEV), _p(xd), _p(ad), _p(dzd), _p(wd), _p(dw), _p(gst), N, H, W, Cin, Cout, _p(ws), need)
    torch.cuda.synchronize()
    check_guard(dw, dwbuf, "dw")
    assert (ws[need:] == GUARD_VALUE).all().item(), "the workspace's guard band was touched"
    return dw.cpu(), (gst.cpu() if gstats else None)


def check_forward(shape, use_aff, relu):
    c = case(shape)
    z = (c.with_affine if use_aff else c.plain)[0]
    ref = z.clamp_min(0) if relu else z
    y, st = forward(c, use_aff, relu)
    e = relerr(y, ref)
    s_ref = torch.stack((ref.sum(dim=(2, 3)), (ref * ref).sum(dim=(2, 3))), dim=-1)
    e_stats = relerr(st[0], s_ref)
    print(dict(test="conv2d_small_fwd", shape=shape, affine=use_aff, relu=relu, err=e, stats=e_stats))
    assert e < TOL
    assert e_stats < TOL_STATS
    return y


def check_backward(shape, use_aff):
    c = case(shape)
    _, dw_ref, g_ref = c.with_affine if use_aff else c.plain
    dw, gst = backward(c, use_aff)
    e_dw, e_g = relerr(dw, dw_ref), relerr(gst, g_ref)
    print(dict(test="conv2d_small_bwd", shape=shape, affine=use_aff, dw=e_dw, gstats=e_g))
    assert e_dw < TOL_DW
    assert e_g < TOL_GSTATS
    return dw


@pytest.mark.parametrize("shape", SHAPES + PLAN_SHAPES)
def test_every_shape_runs_the_plan_it_is_here_for(shape):
    lib = nat.get_lib()
    assert lib.u3d_conv2d_small_cin_fwd_variant(*shape) == FWD_PLANS[shape]
    assert lib.u3d_conv2d_small_cin_bwd_variant(*shape) == BWD_PLANS[shape]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_aff", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward(shape, use_aff, relu):
    check_forward(shape, use_aff, relu)


@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_forward_several_tiles_per_block(shape):
    try:
        check_forward(shape, True, 1)
    finally:
        if shape != PLAN_SHAPES[0]:
            _CASES.pop(shape, None)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_without_statistics_writes_the_same_output(shape):
    c = case(shape)
    y, _ = forward(c, True, 1)
    y2, _ = forward(c, True, 1, stats=False)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4], PLAN_SHAPES[0]])
def test_replica_rows_sum_to_the_one_row_table(shape):
    c = case(shape)
    y1, one = forward(c, True, 1, reps=1)
    y2, many = forward(c, True, 1, reps=4)
    assert torch.equal(y1, y2)
    if shape == PLAN_SHAPES[0]:
        assert (many.abs().sum(dim=(1, 2, 3)) > 0).all()  # 256 blocks per sample: every replica row took some
    assert relerr(many.sum(0), one[0]) < 1e-12


@pytest.mark.parametrize("use_aff", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_dw_and_groupnorm_sums(shape, use_aff):
    check_backward(shape, use_aff)


@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_backward_several_tiles_per_block(shape):
    try:
        check_backward(shape, True)
    finally:
        if shape != PLAN_SHAPES[0]:
            _CASES.pop(shape, None)


@pytest.mark.parametrize("shape", SHAPES + PLAN_SHAPES[:1])
def test_backward_is_bitwise_reproducible_and_gstats_is_optional(shape):
    c = case(shape)
    dw1, _ = backward(c, True)
    dw2, _ = backward(c, True)
    dw3, _ = backward(c, True, gstats=False)
    assert torch.equal(dw1, dw2) and torch.equal(dw1, dw3)


@pytest.mark.parametrize("Cin,Cout", [(5, 16), (1, 33), (0, 8)])
def test_channel_counts_outside_the_envelope_are_refused(Cin, Cout):
    lib = nat.get_lib()
    N, H, W = 1, 6, 7
    assert lib.u3d_conv2d_small_cin_fwd_variant(N, H, W, Cin, Cout) == -1
    assert lib.u3d_conv2d_small_cin_bwd_variant(N, H, W, Cin, Cout) == -1
    assert lib.u3d_small_cin2d_bwd_workspace_floats(N, H, W, Cin, Cout) == 0
    x = torch.randn(N, H, W, max(Cin, 1), device=DEV)
    dz = torch.randn(N, H, W, Cout, device=DEV)
    w = torch.randn(Cout, max(Cin, 1), 3, 3, device=DEV)
    y = torch.full((N, H, W, Cout), 7.0, device=DEV)
    dw = torch.full((Cout, max(Cin, 1), 3, 3), 7.0, device=DEV)
    ws = torch.full((1 << 16,), 7.0, device=DEV)
    with pytest.raises(nat.U3DError):
        nat.call("u3d_conv2d_small_cin_fwd_reps", 0, _stream(DEV), _p(x), None, _p(w), _p(y), N, H, W, Cin, Cout, 0, None, 1)
    with pytest.raises(nat.U3DError):
        nat.call("u3d_conv2d_small_cin_bwd", 0, _stream(DEV), _p(x), None, _p(dz), _p(w), _p(dw), None, N, H, W, Cin, Cout, _p(ws), ws.numel())
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (dw == 7.0).all() and (ws == 7.0).all()  # nothing was launched


def test_a_short_workspace_is_refused():
    N, H, W, Cin, Cout = SHAPES[0]
    need = nat.get_lib().u3d_small_cin2d_bwd_workspace_floats(N, H, W, Cin, Cout)
    x, dz = torch.randn(N, H, W, Cin, device=DEV), torch.randn(N, H, W, Cout, device=DEV)
    w, dw = torch.randn(Cout, Cin, 3, 3, device=DEV), torch.full((Cout, Cin, 3, 3), 7.0, device=DEV)
    ws = torch.full((need,), 7.0, device=DEV)
    with pytest.raises(nat.U3DError):
        nat.call("u3d_conv2d_small_cin_bwd", 0, _stream(DEV), _p(x), None, _p(dz), _p(w), _p(dw), None, N, H, W, Cin, Cout, _p(ws), need - 1)
    torch.cuda.synchronize()
    assert (dw == 7.0).all() and (ws == 7.0).all()
