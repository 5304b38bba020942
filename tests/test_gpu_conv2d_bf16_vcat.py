"""-m gpu: the `_src` entry points of csrc/u3d_conv2d_bf16.hip through the C-ABI (`native_2d_bf16_vcat`): the first convolution of a
UNet2D decoder reads torch.cat((skip, nearest(low)), dim=1) through two base pointers instead of a written-out copy — forward, data
gradient (gx is the virtual tensor) and weight gradient.

Every result is held against TWO references:
  1. float64 F.conv2d / autograd on the CPU on the concatenated tensor, the operand rounding restated as in test_gpu_conv2d_bf16.py, with
     that file's bars (1e-4 identical operands, 1e-3 with a random affine, 2e-2 against exact operands, 1e-5 statistics tables);
  2. the existing single-source entry point on the concat written by u3d_nearest_cat_fwd, same plan: out, dg and dw BIT-EQUAL (both routes
     stage the same bf16 values in the same order), statistics tables within the 1e-5 bar (f64 atomics in another order).
The two halves and every output sit inside larger buffers whose guard words (both sides) hold a NaN pattern: a NaN in a result or a changed
guard word fails the test.

Split-K: on a 256-CU device the (1, 8, 8, C0 + C1 = 256, 128) grid splits into 16 runs of ONE chunk each, so on it no choice of C0 puts the
source boundary inside a run; it is kept as the split-K case on a small grid (boundary between two runs, and the reduction kernel reading
the virtual gx), and SPLIT_INSIDE_SHAPE adds the grid where the plan gives runs of three chunks and the boundary (chunk 2) falls inside
the first run — asserted from the variant query on the current device."""
import ctypes
from functools import cached_property

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import _p, _stream
from test_gpu_conv2d_bf16 import (TOL_AFF, TOL_EXACT, TOL_SAME, TOL_STATS, cus, fwd_variant, nchw, nhwc, pack, r16, rel, stat_table,
                                  wgrad_variant)

pytestmark = pytest.mark.gpu
U3D_EINVAL = -1  # include/u3d.h

# (N, H, W, C0, C1, H1, W1, Cout): the smallest shapes at which each thing can go wrong
SHAPES = [
    (1, 4, 5, 32, 32, 2, 2, 32),       # smaller than one tile, 2n + 1 in x
    (2, 17, 19, 32, 64, 8, 9, 64),     # ragged 2 x 2 tiles, 2n + 1 in both axes, the source switch after chunk 2 of 6
    (1, 33, 45, 64, 32, 16, 22, 32),   # C0 > C1
    (1, 16, 16, 32, 96, 8, 8, 96),     # exact 2x, three n-tiles
    (1, 20, 20, 32, 32, 7, 9, 32),     # a general nearest map, neither 2x nor 2n + 1
    (1, 8, 8, 32, 224, 4, 4, 128),     # split-K on a small grid (C0 + C1 = 256)
]
SPLIT_SHAPE = SHAPES[-1]
SPLIT_INSIDE_SHAPE = (1, 64, 96, 32, 224, 32, 48, 128)  # 24 tiles x 4 n-tiles: runs of 3 chunks on 256 CUs, boundary inside run 0
# production variants (what a full-resolution level runs), asserted through the variant queries
NT2_FWD_SHAPE = (2, 251, 245, 32, 32, 125, 122, 64)     # 512 tiles: the 64-channel block in the forward
NT2_DGRAD_SHAPE = (1, 251, 245, 32, 64, 125, 122, 32)   # data gradient produces 96 channels: block 0 = channels 0 .. 63 straddles C0 = 32
WGRAD_MULTI_TILE_SHAPE = (1, 139, 157, 32, 64, 69, 78, 128)  # 90 tiles, 12 channel cells: two tiles per block, the same 32 | 64 split

GUARD = 64                 # floats on each side of a guarded tensor (256 bytes: the payload keeps its 16-byte alignment)
GUARD_BITS = 0x7FC0DEAD    # a quiet NaN with a recognisable payload


class Guarded:
    """a float32 device tensor inside a larger buffer whose every other word is GUARD_BITS (a NaN); `fill` = None leaves the payload NaN
    too (an output: every element the kernel does not write shows)"""

    def __init__(self, shape, fill=None):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(GUARD_BITS)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        bits = self.buf.view(torch.int32)
        assert (bits[:GUARD] == GUARD_BITS).all() and (bits[-GUARD:] == GUARD_BITS).all(), f"{what}: a guard word changed"
        assert not torch.isnan(self.t).any(), f"{what}: NaN in the result"
        return self.t


def nearest_map(n_in, n_out):
    """ATen's own nearest index map (the 1-D operator on an index ramp)"""
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in)
    return F.interpolate(ramp, size=n_out, mode="nearest").view(-1).to(torch.int64)


class VCase:
    """inputs and float64 references of one shape, each computed once, when first asked for, and shared by the tests (never modified)"""

    def __init__(self, shape):
        N, H, W, C0, C1, H1, W1, Cout = shape
        Ct = C0 + C1
        g = torch.Generator().manual_seed(2000 + H * W + 7 * C0 + C1 + Cout)
        self.shape = shape
        self.skip = torch.randn(N, C0, H, W, generator=g)
        self.low = torch.randn(N, C1, H1, W1, generator=g)
        self.ymap, self.xmap = nearest_map(H1, H), nearest_map(W1, W)
        self.x = torch.cat((self.skip, self.low[:, :, self.ymap, :][:, :, :, self.xmap]), dim=1)  # the concat, never on the device
        self.w = torch.randn(Cout, Ct, 3, 3, generator=g) / (3.0 * Ct ** 0.5)
        self.dz = torch.randn(N, Cout, H, W, generator=g)
        a = 1.0 + 0.3 * torch.randn(N, Ct, generator=g)
        b = 0.5 + 0.2 * torch.randn(N, Ct, generator=g)  # a clearly nonzero offset: padding must not pick it up
        self.aff = torch.stack((a, b), dim=-1).contiguous()
        self.g = self.x * a.view(N, Ct, 1, 1) + b.view(N, Ct, 1, 1)

    @cached_property
    def dev(self):
        """device side: the guarded halves, the maps, the affine, dz, the images"""
        d = {}
        d["p0"], d["p1"] = Guarded(nhwc(self.skip).shape, nhwc(self.skip)), Guarded(nhwc(self.low).shape, nhwc(self.low))
        d["ymap"], d["xmap"] = self.ymap.to(torch.int32).to(DEV), self.xmap.to(torch.int32).to(DEV)
        d["zmap"] = torch.zeros(1, dtype=torch.int32, device=DEV)
        d["aff"], d["dz"] = self.aff.to(DEV), nhwc(self.dz)
        d["wp0"], d["wp1"] = pack(self.w, 0), pack(self.w, 1)
        return d

    @cached_property
    def cat(self):
        """the concat as the parent mode writes it (u3d_nearest_cat_fwd), guarded"""
        N, H, W, C0, C1, H1, W1, _ = self.shape
        d = self.dev
        out = Guarded((N, H, W, C0 + C1))
        nat.call("u3d_nearest_cat_fwd", 0, _stream(DEV), _p(d["p0"].t), _p(d["p1"].t), _p(d["zmap"]), _p(d["ymap"]), _p(d["xmap"]), N, 1,
                 H, W, 1, H1, W1, C0, C1, _p(out.t))
        torch.cuda.synchronize()
        assert torch.equal(nchw(out.check("cat")), self.x)
        return out

    def src(self, affine=None, p0=None, p1=None, C0=None, C1=None):
        _, _, _, c0, c1, H1, W1, _ = self.shape
        d = self.dev
        s = nat.U3DSrc()
        s.p0 = (d["p0"].t if p0 is None else p0).data_ptr()
        s.p1 = (d["p1"].t if p1 is None else p1).data_ptr()
        s.zmap, s.ymap, s.xmap = d["zmap"].data_ptr(), d["ymap"].data_ptr(), d["xmap"].data_ptr()
        s.affine = affine.data_ptr() if affine is not None else None
        s.C0, s.C1 = c0 if C0 is None else C0, c1 if C1 is None else C1
        s.D1, s.H1, s.W1 = 1, H1, W1
        return s

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
        xin = r16(self.x).requires_grad_(True)
        F.conv2d(xin, r16(self.w), padding=1).backward(r16(self.dz))
        return xin.grad

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


def case(shape) -> VCase:
    if shape not in _CASES:
        _CASES[shape] = VCase(shape)
    return _CASES[shape]


def _ws(need):
    return torch.empty(need, dtype=torch.float32, device=DEV) if need > 0 else None


def forward_both(c, use_aff, relu, use_ws, reps=1):
    """the `_src` forward and the single-source one on the written-out concat, same plan; ((y, stats), (y, stats)) device tensors"""
    N, H, W, C0, C1, _, _, Cout = c.shape
    Ct = C0 + C1
    d = c.dev
    aff = d["aff"] if use_aff else None
    need = nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, Ct, Cout) if use_ws else 0
    ws = _ws(need)
    y_v, y_s = Guarded((N, H, W, Cout)), Guarded((N, H, W, Cout))
    st_v = torch.zeros((reps, N, Cout, 2), dtype=torch.float64, device=DEV)
    st_s = torch.zeros_like(st_v)
    s = c.src(aff)
    nat.call("u3d_conv2d_bf16_src", 0, _stream(DEV), ctypes.byref(s), _p(d["wp0"]), _p(y_v.t), N, H, W, Cout, relu, _p(st_v), _p(ws), need,
             reps)
    nat.call("u3d_conv2d_bf16", 0, _stream(DEV), _p(c.cat.t), _p(aff), _p(d["wp0"]), _p(y_s.t), N, H, W, Ct, Cout, relu, _p(st_s), None, None,
             _p(ws), need, reps)
    torch.cuda.synchronize()
    d["p0"].check("p0"), d["p1"].check("p1")
    return (y_v.check("out (_src)"), st_v.sum(0)), (y_s.check("out"), st_s.sum(0))


def check_forward(shape, use_ws):
    """random affine, ReLU and out_stats of one forward launch; returns the plan it ran as (n-tiles per block, ksplit)"""
    c = case(shape)
    N, H, W, C0, C1, _, _, Cout = shape
    var = fwd_variant(N, H, W, C0 + C1, Cout, use_ws)
    (yv, sv), (ys, ss) = forward_both(c, True, 1, use_ws)
    y = nchw(yv).double()
    ref = c.fwd_aff.clamp_min(0)
    scale = c.fwd_aff.abs().max().item()
    e = (y - ref).abs().max().item() / scale
    e_exact = (y - c.fwd_exact.clamp_min(0)).abs().max().item() / scale
    e_stats = rel(sv.cpu(), stat_table(y, y))
    e_routes = rel(sv, ss)
    print(dict(test="conv2d_bf16_src_fwd", shape=shape, nt=var[0], ksplit=var[1], err=e, exact=e_exact, stats=e_stats, stats_routes=e_routes,
               bit_equal=torch.equal(yv, ys)))
    assert e < TOL_AFF and e_exact < TOL_EXACT
    assert e_stats < TOL_STATS and e_routes < TOL_STATS
    assert torch.equal(yv, ys)  # the written-out route stages the same bf16 values in the same order
    return var


def check_forward_identity(shape, use_ws):
    c = case(shape)
    (yv, sv), (ys, ss) = forward_both(c, False, 0, use_ws)
    e = rel(nchw(yv), c.fwd_same)
    print(dict(test="conv2d_bf16_src_fwd_same", shape=shape, err=e, bit_equal=torch.equal(yv, ys)))
    assert e < TOL_SAME
    assert torch.equal(yv, ys)
    assert rel(sv, ss) < TOL_STATS


def check_data_gradient(shape, use_ws, reps=1):
    """dg and the gx / gstats sums of one data-gradient launch of the LAYER `shape`; returns (n-tiles per block, ksplit)"""
    c = case(shape)
    N, H, W, C0, C1, _, _, Cout = shape
    Ct = C0 + C1
    d = c.dev
    var = fwd_variant(N, H, W, Cout, Ct, use_ws)  # the launch contracts over the layer's Cout
    need = nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, Cout, Ct) if use_ws else 0
    ws = _ws(need)
    dg_v, dg_s = Guarded((N, H, W, Ct)), Guarded((N, H, W, Ct))
    g_v = torch.zeros((reps, N, Ct, 2), dtype=torch.float64, device=DEV)
    g_s = torch.zeros_like(g_v)
    s = c.src()
    nat.call("u3d_conv2d_bf16_dgrad_src", 0, _stream(DEV), _p(d["dz"]), _p(d["wp1"]), _p(dg_v.t), N, H, W, Cout, ctypes.byref(s), _p(g_v),
             _p(ws), need, reps)
    nat.call("u3d_conv2d_bf16", 0, _stream(DEV), _p(d["dz"]), None, _p(d["wp1"]), _p(dg_s.t), N, H, W, Cout, Ct, 0, None, _p(c.cat.t), _p(g_s),
             _p(ws), need, reps)
    torch.cuda.synchronize()
    d["p0"].check("p0"), d["p1"].check("p1")
    dv, ds = dg_v.check("dg (_src)"), dg_s.check("dg")
    dg = nchw(dv).double()
    scale = c.dg.abs().max().item()
    e = (dg - c.dg).abs().max().item() / scale
    e_exact = (dg - c.dg_exact).abs().max().item() / scale
    sv = g_v.sum(0)
    e_stats = rel(sv.cpu(), stat_table(dg, c.x))
    e_routes = rel(sv, g_s.sum(0))
    print(dict(test="conv2d_bf16_src_dgrad", shape=shape, nt=var[0], ksplit=var[1], err=e, exact=e_exact, stats=e_stats,
               stats_routes=e_routes, bit_equal=torch.equal(dv, ds)))
    assert e < TOL_SAME and e_exact < TOL_EXACT
    assert e_stats < TOL_STATS and e_routes < TOL_STATS
    assert torch.equal(dv, ds)
    return var


def check_weight_gradient(shape, use_aff, exact=True):
    """dw of one launch against float64 and bit-equal to the single-source route; returns (tiles per block, nsplit)"""
    c = case(shape)
    N, H, W, C0, C1, _, _, Cout = shape
    Ct = C0 + C1
    d = c.dev
    var = wgrad_variant(N, H, W, Ct, Cout)
    aff = d["aff"] if use_aff else None
    need = nat.get_lib().u3d_wgrad2d_bf16_workspace_floats(N, H, W, Ct, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    dw_v, dw_s = Guarded((Cout, Ct, 3, 3)), Guarded((Cout, Ct, 3, 3))
    s = c.src(aff)
    nat.call("u3d_conv2d_wgrad_bf16_src", 0, _stream(DEV), ctypes.byref(s), _p(d["dz"]), _p(dw_v.t), N, H, W, Cout, _p(ws), need)
    nat.call("u3d_conv2d_wgrad_bf16", 0, _stream(DEV), _p(c.cat.t), _p(aff), _p(d["dz"]), _p(dw_s.t), N, H, W, Ct, Cout, _p(ws), need)
    torch.cuda.synchronize()
    d["p0"].check("p0"), d["p1"].check("p1")
    dv, ds = dw_v.check("dw (_src)"), dw_s.check("dw")
    ref = c.dw_aff if use_aff else c.dw_same
    scale = ref.abs().max().item()
    e = (dv.cpu().double() - ref).abs().max().item() / scale
    print(dict(test="conv2d_bf16_src_wgrad", shape=shape, tps=var[0], nsplit=var[1], affine=use_aff, err=e, bit_equal=torch.equal(dv, ds)))
    assert e < (TOL_AFF if use_aff else TOL_SAME)
    if use_aff and exact:
        assert (dv.cpu().double() - c.dw_exact).abs().max().item() < TOL_EXACT * scale
    assert torch.equal(dv, ds)
    return var


@pytest.mark.parametrize("use_ws", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_affine_relu_stats(shape, use_ws):
    """with the workspace these small grids split the channel reduction; without it the main kernel's fused epilogue runs"""
    nt, ksplit = check_forward(shape, use_ws)
    assert use_ws or ksplit == 1


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_identity_affine(shape):
    check_forward_identity(shape, use_ws=True)


@pytest.mark.parametrize("use_ws", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_data_gradient_with_virtual_gx(shape, use_ws):
    """use_ws: the split-K reduction kernel reads the virtual gx; without: the main kernel's epilogue does"""
    nt, ksplit = check_data_gradient(shape, use_ws)
    assert use_ws or ksplit == 1


@pytest.mark.parametrize("use_aff", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient(shape, use_aff):
    check_weight_gradient(shape, use_aff)


def _runs_with_boundary_inside(nchunks, ksplit, boundary):
    """every run length the plan may have for this ksplit (ksplit = ceil(nchunks / cps)) puts chunk `boundary` strictly inside a run"""
    cands = [cps for cps in range(1, nchunks + 1) if -(-nchunks // cps) == ksplit]
    return bool(cands) and all(boundary % cps != 0 for cps in cands)


def test_split_k_small_grid():
    """(1, 8, 8, 256 -> 128): forward and data gradient split the channel reduction; the reduction kernel of the data gradient reads the
    virtual gx.  Where the plan of the current device gives runs of more than one chunk, the boundary (chunk 2) must not sit on a run's
    edge; with one-chunk runs (256 CUs) no C0 can put it inside — SPLIT_INSIDE_SHAPE covers that"""
    N, H, W, C0, C1, _, _, Cout = SPLIT_SHAPE
    assert nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, C0 + C1, Cout) > 0
    nt, ksplit = fwd_variant(N, H, W, C0 + C1, Cout, True)
    assert ksplit > 1, f"ksplit {ksplit} on {cus()} CUs"
    nchunks = (C0 + C1) // 16
    if ksplit < nchunks:
        assert _runs_with_boundary_inside(nchunks, ksplit, C0 // 16), f"ksplit {ksplit} on {cus()} CUs"
    assert fwd_variant(N, H, W, Cout, C0 + C1, True)[1] > 1
    for reps in (1, 2):
        check_data_gradient(SPLIT_SHAPE, True, reps=reps)


def test_split_k_source_boundary_inside_one_run():
    N, H, W, C0, C1, _, _, Cout = SPLIT_INSIDE_SHAPE
    nt, ksplit = fwd_variant(N, H, W, C0 + C1, Cout, True)
    assert ksplit > 1 and _runs_with_boundary_inside((C0 + C1) // 16, ksplit, C0 // 16), f"nt {nt}, ksplit {ksplit} on {cus()} CUs"
    try:
        assert check_forward(SPLIT_INSIDE_SHAPE, True) == (nt, ksplit)
        check_forward_identity(SPLIT_INSIDE_SHAPE, True)
    finally:
        _CASES.pop(SPLIT_INSIDE_SHAPE, None)


def _poisoned(shape):
    return torch.full(shape, 7.0, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("what", ["C0=16", "C1=48", "C1=0", "misaligned"])
def test_outside_the_envelope_is_refused_without_a_launch(what):
    c = case(SHAPES[1])  # (2, 17, 19, 32 + 64 -> 64)
    N, H, W, C0, C1, _, _, Cout = c.shape
    d = c.dev
    lib = nat.get_lib()
    kw = {}
    if what == "C0=16":
        kw = dict(C0=16, C1=48)   # (16 + 48 = 64 -> 64 is inside the single-source envelope: only the halves are refused)
    elif what == "C1=48":
        kw = dict(C0=32, C1=48)   # (a concat of 80: outside the % 32 rule too)
    elif what == "C1=0":
        kw = dict(C0=96, C1=0)
    else:
        kw = dict(p1=d["p1"].buf[GUARD + 1:])  # 4 bytes off a 16-byte boundary
    s = c.src(**kw)
    Ct = s.C0 + s.C1
    ws = torch.empty(1 << 20, dtype=torch.float32, device=DEV)
    y, dg, dw = _poisoned((N, H, W, Cout)), _poisoned((N, H, W, max(Ct, 96))), _poisoned((Cout, max(Ct, 96), 3, 3))
    gst = torch.zeros((N, max(Ct, 96), 2), dtype=torch.float64, device=DEV)
    rc = [lib.u3d_conv2d_bf16_src(0, _stream(DEV), ctypes.byref(s), _p(d["wp0"]), _p(y), N, H, W, Cout, 0, None, _p(ws), ws.numel(), 1),
          lib.u3d_conv2d_bf16_dgrad_src(0, _stream(DEV), _p(d["dz"]), _p(d["wp1"]), _p(dg), N, H, W, Cout, ctypes.byref(s), _p(gst), _p(ws),
                                        ws.numel(), 1),
          lib.u3d_conv2d_wgrad_bf16_src(0, _stream(DEV), ctypes.byref(s), _p(d["dz"]), _p(dw), N, H, W, Cout, _p(ws), ws.numel())]
    torch.cuda.synchronize()
    assert rc == [U3D_EINVAL] * 3, rc
    assert (y == 7.0).all() and (dg == 7.0).all() and (dw == 7.0).all() and (gst == 0).all()  # nothing was launched


# ---- production variants: what a full-resolution UNet2D decoder level runs --------------------------------------------------------------
def test_forward_64_channel_block():
    """conv2d_bf16_kernel<2, 1>: both n-tiles of a block over chunks from both sources"""
    try:
        nt, ksplit = check_forward(NT2_FWD_SHAPE, use_ws=True)
    finally:
        _CASES.pop(NT2_FWD_SHAPE, None)
    assert nt == 2 and ksplit == 1, f"nt {nt}, ksplit {ksplit} on {cus()} CUs"


def test_data_gradient_64_channel_block_straddles_the_sources():
    """conv2d_bf16_kernel<2, 2> with C0 = 32, C1 = 64: the first block's two n-tiles read gx from different sources"""
    try:
        nt, ksplit = check_data_gradient(NT2_DGRAD_SHAPE, use_ws=True)
    finally:
        _CASES.pop(NT2_DGRAD_SHAPE, None)
    assert nt == 2 and ksplit == 1, f"nt {nt}, ksplit {ksplit} on {cus()} CUs"


@pytest.mark.parametrize("use_aff", [False, True])
def test_weight_gradient_multi_tile_blocks(use_aff):
    """more than one tile per block with the 32 | 64 split: channel block 0 stages from the skip, blocks 1 and 2 through the maps"""
    tps, nsplit = check_weight_gradient(WGRAD_MULTI_TILE_SHAPE, use_aff, exact=False)
    assert tps >= 2, f"tps {tps}, nsplit {nsplit} on {cus()} CUs"
