"""-m gpu: the bf16-operand ConvTranspose2d kernels (csrc/u3d_conv2d_bf16.hip, u3d_convtr2d_*_bf16) through the C-ABI — the sub-pixel
forward, the stride-2 data gradient and the weight gradient on v_mfma_f32_32x32x16_bf16, their launch plans and the envelope — against
float64 F.conv_transpose2d and its autograd gradients on the CPU with the same operand rounding restated (bf16, nearest even).

Bars (the 2-D bf16 family's own, tests/test_gpu_conv2d_bf16.py): the operands match bit for bit and only the accumulation order differs —
1e-4 of the output range against the rounded-operand reference (there is no affine here); 2e-2 against the exact operands; split against
single-split weight gradient 1e-4.  Against the fp32 u3d_convtr2d_* result the kernels must be no closer than the operand rounding allows
and never bit-equal: the bf16 path ran.

Every output is pre-filled with NaN in front of a guard band: it must come back fully finite (every element written) with the band
untouched.  The launch plans are asserted, not assumed (u3d_convtr2d_dgrad_bf16_variant, u3d_convtr2d_wgrad_bf16_variant)."""
from functools import cached_property

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import _p, _stream

pytestmark = pytest.mark.gpu
TOL_SAME = 1e-4   # identical operands: fp32 accumulation order only
TOL_EXACT = 2e-2  # against the un-rounded operands
GUARD = 1024      # floats behind every output
GUARD_VALUE = -12345.0

# (N, H1, W1, Cin, Cout): the smallest shapes at which each thing can go wrong
SHAPES = [
    (1, 1, 1, 32, 32),     # the output is 1 x 1: three parity classes are empty
    (2, 1, 5, 32, 64),     # one row: the odd-row classes are empty
    (2, 5, 1, 64, 32),     # one column
    (1, 16, 16, 32, 32),   # an exact tile: the forward's halo (and the last odd row / column) lies outside the image
    (2, 17, 19, 64, 32),   # ragged 2 x 2 tiles: the halo comes from the neighbouring tile
    (1, 33, 18, 96, 64),   # an odd third 32-channel group (six 16-channel chunks; data gradient: 32 channels per block)
    (1, 4, 4, 256, 128),   # a long reduction on a tiny grid (the launchers have no split-K plan: the one plan runs)
]
MULTI_SPLIT_SHAPE = (2, 40, 37, 32, 32)  # 30 weight-gradient tiles, one channel cell


def r16(t):
    return t.float().to(torch.bfloat16).double()


def nhwc(x):  # (N,C,H,W) cpu -> (N,H,W,C) gpu
    return x.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(y):  # (N,H,W,C) gpu -> (N,C,H,W) cpu
    return y.permute(0, 3, 1, 2).contiguous().cpu()


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def guarded(shape):
    """(view of `shape` filled with NaN, whole buffer with a guard band behind the view)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), GUARD_VALUE, dtype=torch.float32, device=DEV)
    buf[:n] = float("nan")
    return buf[:n].view(shape), buf


def check_written(view, buf, what):
    assert torch.isfinite(view).all().item(), f"{what}: an element was not written"
    assert (buf[view.numel():] == GUARD_VALUE).all().item(), f"{what}: the guard band was touched"


def pack(w, mode, bf16=True):
    Cin, Cout = w.shape[:2]
    lib = nat.get_lib()
    wd = w.float().contiguous().to(DEV)
    if bf16:
        n = lib.u3d_packed_convtr2d_bf16_elems(Cin, Cout, mode)
        assert n == 9 * Cin * Cout
        out = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        nat.call("u3d_pack_convtr2d_bf16", 0, _stream(DEV), _p(wd), Cin, Cout, mode, _p(out))
    else:
        out = torch.empty(lib.u3d_convtr2d_packed_floats(Cin, Cout), dtype=torch.float32, device=DEV)
        nat.call("u3d_pack_convtr2d", 0, _stream(DEV), _p(wd), Cin, Cout, mode, _p(out))
    return out


def dgrad_variant(N, H1, W1, Cin, Cout):
    v = nat.get_lib().u3d_convtr2d_dgrad_bf16_variant(N, H1, W1, Cin, Cout)
    assert v > 0, (v, (N, H1, W1, Cin, Cout))
    return v


def wgrad_variant(N, H1, W1, Cin, Cout, ws_floats=-1):
    """(tiles per block, nsplit) of the u3d_convtr2d_wgrad_bf16 launch with a workspace of ws_floats (-1: the full one)"""
    v = nat.get_lib().u3d_convtr2d_wgrad_bf16_variant(N, H1, W1, Cin, Cout, ws_floats)
    assert v > 0, (v, (N, H1, W1, Cin, Cout))
    return v >> 16, v & 0xFFFF


def fwd(c, bf16=True):
    N, H1, W1, Cin, Cout = c.shape
    t, buf = guarded((N, 2 * H1 - 1, 2 * W1 - 1, Cout))
    xd, wp = nhwc(c.x), pack(c.w, 0, bf16)
    nat.call("u3d_convtr2d_fwd_bf16" if bf16 else "u3d_convtr2d_fwd", 0, _stream(DEV), _p(xd), _p(wp), _p(t), N, H1, W1, Cin, Cout)
    torch.cuda.synchronize()
    check_written(t, buf, "t")
    return nchw(t)


def dgrad(c, mask, bf16=True):
    N, H1, W1, Cin, Cout = c.shape
    dx, buf = guarded((N, H1, W1, Cin))
    dtd, wp = nhwc(c.dt), pack(c.w, 1, bf16)
    xl = nhwc(c.x_low) if mask else None
    nat.call("u3d_convtr2d_dgrad_bf16" if bf16 else "u3d_convtr2d_dgrad", 0, _stream(DEV), _p(dtd), _p(wp), _p(xl), _p(dx), N, H1, W1, Cin,
             Cout)
    torch.cuda.synchronize()
    check_written(dx, buf, "dx")
    return nchw(dx)


def wgrad(c, accumulate=0, ws_floats=None, start=None):
    """dw (Cin,Cout,3,3) cpu of one u3d_convtr2d_wgrad_bf16 call; start: the value dw holds before an accumulating call"""
    N, H1, W1, Cin, Cout = c.shape
    need = nat.get_lib().u3d_convtr2d_wgrad_bf16_workspace_floats(N, H1, W1, Cin, Cout) if ws_floats is None else ws_floats
    assert need >= 9 * Cin * Cout
    ws = torch.full((need + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ws[need:] = GUARD_VALUE
    dw, buf = guarded((Cin, Cout, 3, 3))
    if start is not None:
        dw.copy_(start.to(DEV))
    xd, dtd = nhwc(c.x), nhwc(c.dt)  # (named: a temporary would be freed, and its memory reused, before the call)
    nat.call("u3d_convtr2d_wgrad_bf16", 0, _stream(DEV), _p(xd), _p(dtd), _p(dw), N, H1, W1, Cin, Cout, accumulate, _p(ws), need)
    torch.cuda.synchronize()
    check_written(dw, buf, "dw")
    assert (ws[need:] == GUARD_VALUE).all().item(), "the workspace's guard band was touched"
    return dw.cpu()


def wgrad_f32(c):
    N, H1, W1, Cin, Cout = c.shape
    nws = nat.get_lib().u3d_convtr2d_wgrad_workspace_doubles(Cin, Cout)
    ws = torch.empty(nws, dtype=torch.float64, device=DEV)
    dw = torch.empty((Cin, Cout, 3, 3), dtype=torch.float32, device=DEV)
    xd, dtd = nhwc(c.x), nhwc(c.dt)
    nat.call("u3d_convtr2d_wgrad", 0, _stream(DEV), _p(xd), _p(dtd), _p(dw), N, H1, W1, Cin, Cout, 0, _p(ws), nws)
    torch.cuda.synchronize()
    return dw.cpu()


def _grads(x, w, dt):
    """float64 autograd gradients (dx, dw) of conv_transpose2d(x, w, stride=2, padding=1) for the output gradient dt"""
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv_transpose2d(xa, wa, stride=2, padding=1).backward(dt)
    return xa.grad, wa.grad


class Case:
    """inputs and float64 references of one shape, each computed once, when first asked for, and shared by the tests (never modified)"""

    def __init__(self, shape):
        N, H1, W1, Cin, Cout = shape
        g = torch.Generator().manual_seed(2000 + 7 * H1 + W1 + Cin + Cout)
        self.shape = shape
        self.x = torch.randn(N, Cin, H1, W1, generator=g)
        self.w = torch.randn(Cin, Cout, 3, 3, generator=g) / (1.5 * Cin ** 0.5)
        self.dt = torch.randn(N, Cout, 2 * H1 - 1, 2 * W1 - 1, generator=g)
        self.x_low = torch.randn(N, Cin, H1, W1, generator=g)  # the ReLU mask's tensor: about half of it <= 0
        self.x_low[0, 0, 0, 0] = 0.0                            # (0 itself is masked)

    @cached_property
    def fwd_same(self):
        return F.conv_transpose2d(r16(self.x), r16(self.w), stride=2, padding=1)

    @cached_property
    def fwd_exact(self):
        return F.conv_transpose2d(self.x.double(), self.w.double(), stride=2, padding=1)

    @cached_property
    def grads_same(self):  # every operand rounded: dx sees dt and w, dw sees x and dt
        return _grads(r16(self.x), r16(self.w), r16(self.dt))

    @property
    def dx_same(self):
        return self.grads_same[0]

    @property
    def dw_same(self):
        return self.grads_same[1]

    @cached_property
    def grads_exact(self):
        return _grads(self.x.double(), self.w.double(), self.dt.double())


_CASES = {}


def case(shape) -> Case:
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


def not_the_fp32_path(ours, f32, same, what):
    """against the fp32 kernels' result: not bit-equal, and no closer than the operand rounding allows — at least as far from it as a
    tenth of the rounded-operand reference's own distance from it"""
    assert not torch.equal(ours, f32), f"{what}: bit-equal to the fp32 path"
    assert rel(ours, f32) > 0.1 * rel(same, f32), (what, rel(ours, f32), rel(same, f32))


@pytest.mark.parametrize("shape", SHAPES)
def test_forward(shape):
    c = case(shape)
    t = fwd(c)
    assert t.shape == c.fwd_same.shape
    e, e_exact = rel(t, c.fwd_same), rel(t, c.fwd_exact)
    print(dict(test="convtr2d_bf16_fwd", shape=shape, err=e, exact=e_exact))
    assert e < TOL_SAME and e_exact < TOL_EXACT
    not_the_fp32_path(t, fwd(c, bf16=False), c.fwd_same, "t")
    assert torch.equal(t, fwd(c))  # one launch, no reduction across blocks: run-to-run identical


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mask", [False, True])
def test_data_gradient(shape, mask):
    c = case(shape)
    nt = dgrad_variant(*shape)
    assert nt == (2 if shape[3] % 64 == 0 else 1), f"nt {nt} on {cus()} CUs"  # both plans occur in SHAPES
    dx = dgrad(c, mask)
    keep = (c.x_low > 0) if mask else torch.ones_like(c.x_low, dtype=torch.bool)
    assert (dx[~keep] == 0).all().item()  # masked positions are exactly 0
    ref, ref_exact = c.dx_same * keep, c.grads_exact[0] * keep
    e, e_exact = rel(dx, ref), rel(dx, ref_exact)
    print(dict(test="convtr2d_bf16_dgrad", shape=shape, nt=nt, mask=mask, err=e, exact=e_exact))
    assert e < TOL_SAME and e_exact < TOL_EXACT
    not_the_fp32_path(dx, dgrad(c, mask, bf16=False), ref, "dx")


def test_both_data_gradient_plans_are_covered():
    assert {dgrad_variant(*s) for s in SHAPES} == {1, 2}, f"on {cus()} CUs"


@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient(shape):
    c = case(shape)
    tps, nsplit = wgrad_variant(*shape)
    dw = wgrad(c)
    e, e_exact = rel(dw, c.dw_same), rel(dw, c.grads_exact[1])
    print(dict(test="convtr2d_bf16_wgrad", shape=shape, tps=tps, nsplit=nsplit, err=e, exact=e_exact))
    assert e < TOL_SAME and e_exact < TOL_EXACT
    not_the_fp32_path(dw, wgrad_f32(c), c.dw_same, "dw")
    assert torch.equal(dw, wgrad(c))  # fixed-order sums: bitwise equal on a second call
    # accumulate: added to what dw held, in one rounding
    start = torch.full((shape[3], shape[4], 3, 3), 0.25)
    assert torch.equal(wgrad(c, accumulate=1, start=start), start + dw)


def test_weight_gradient_multi_split_against_single_split():
    """a workspace of one split runs every tile in one block per channel cell (tps = all tiles); the full workspace splits the tiles
    over blocks and adds the partial sums in split order — the same dw to fp32 round-off, each run-to-run identical"""
    shape = MULTI_SPLIT_SHAPE
    N, H1, W1, Cin, Cout = shape
    c = case(shape)
    one = 9 * Cin * Cout
    tiles = N * ((H1 + 7) // 8) * ((W1 + 15) // 16)
    tps, nsplit = wgrad_variant(*shape)
    assert nsplit > 1, f"tps {tps}, nsplit {nsplit} on {cus()} CUs"
    tps1, nsplit1 = wgrad_variant(*shape, ws_floats=one)
    assert (tps1, nsplit1) == (tiles, 1), f"tps {tps1}, nsplit {nsplit1} on {cus()} CUs"
    # an in-between workspace: several tiles per block AND several splits (both restaging under live accumulators and the reduction)
    tps3, nsplit3 = wgrad_variant(*shape, ws_floats=3 * one)
    assert tps3 == tiles // 3 and nsplit3 == 3, f"tps {tps3}, nsplit {nsplit3} on {cus()} CUs"
    multi, single, three = wgrad(c), wgrad(c, ws_floats=one), wgrad(c, ws_floats=3 * one)
    e_ms, e_3s = rel(multi, single), rel(three, single)
    print(dict(test="convtr2d_bf16_wgrad_split", shape=shape, nsplit=nsplit, multi_vs_single=e_ms, three_vs_single=e_3s,
               single=rel(single, c.dw_same)))
    assert e_ms < TOL_SAME and e_3s < TOL_SAME
    for dw in (multi, single, three):
        assert rel(dw, c.dw_same) < TOL_SAME and rel(dw, c.grads_exact[1]) < TOL_EXACT
    assert torch.equal(single, wgrad(c, ws_floats=one)) and torch.equal(three, wgrad(c, ws_floats=3 * one))


def test_weight_gradient_plans_on_the_test_shapes():
    """the small shapes take one tile per block; the multi-tile plan is pinned by the test above"""
    for s in SHAPES:
        tps, nsplit = wgrad_variant(*s)
        N, H1, W1 = s[:3]
        tiles = N * ((H1 + 7) // 8) * ((W1 + 15) // 16)
        assert (tps - 1) * nsplit < tiles <= tps * nsplit, f"{s}: tps {tps}, nsplit {nsplit} on {cus()} CUs"
    assert wgrad_variant(*SHAPES[0]) == (1, 1), f"on {cus()} CUs"


def test_bad_arguments_are_refused_without_a_launch():
    lib = nat.get_lib()
    x = torch.zeros(4096, dtype=torch.float32, device=DEV)
    out, buf = guarded((2048,))
    s = _stream(DEV)
    bad = [
        ("u3d_pack_convtr2d_bf16", (_p(x), 16, 32, 0, _p(out))),               # channels not % 32
        ("u3d_pack_convtr2d_bf16", (_p(x), 32, 32, 2, _p(out))),               # mode
        ("u3d_pack_convtr2d_bf16", (None, 32, 32, 0, _p(out))),
        ("u3d_convtr2d_fwd_bf16", (_p(x), _p(x), _p(out), 1, 1, 1, 32, 48)),
        ("u3d_convtr2d_fwd_bf16", (_p(x), _p(x), _p(out), 1, 1, 1, 16, 32)),
        ("u3d_convtr2d_fwd_bf16", (None, _p(x), _p(out), 1, 1, 1, 32, 32)),
        ("u3d_convtr2d_fwd_bf16", (_p(x), _p(x), None, 1, 1, 1, 32, 32)),
        ("u3d_convtr2d_fwd_bf16", (_p(x), _p(x), _p(out), 1, 0, 1, 32, 32)),
        ("u3d_convtr2d_fwd_bf16", (_p(x), _p(x), _p(out), 1, 40000, 40000, 32, 32)),  # the limits of u3d_convtr2d_*
        ("u3d_convtr2d_dgrad_bf16", (_p(x), _p(x), None, _p(out), 1, 1, 1, 48, 32)),
        ("u3d_convtr2d_dgrad_bf16", (_p(x), None, None, _p(out), 1, 1, 1, 32, 32)),
        ("u3d_convtr2d_dgrad_bf16", (_p(x), _p(x), None, None, 1, 1, 1, 32, 32)),
        ("u3d_convtr2d_wgrad_bf16", (_p(x), _p(x), _p(out), 1, 1, 1, 32, 40, 0, _p(x), 4096)),
        ("u3d_convtr2d_wgrad_bf16", (_p(x), _p(x), _p(out), 1, 1, 1, 32, 32, 0, None, 0)),
        ("u3d_convtr2d_wgrad_bf16", (_p(x), _p(x), _p(out), 1, 1, 1, 32, 32, 0, _p(x), 9 * 32 * 32 - 1)),  # a short workspace
        ("u3d_convtr2d_wgrad_bf16", (None, _p(x), _p(out), 1, 1, 1, 32, 32, 0, _p(x), 9 * 32 * 32)),
    ]
    for name, args in bad:
        with pytest.raises(RuntimeError):
            nat.call(name, 0, s, *args)
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item() and (buf[out.numel():] == GUARD_VALUE).all().item()  # nothing ran
    assert lib.u3d_convtr2d_bf16_supported(16, 32) == 0 and lib.u3d_packed_convtr2d_bf16_elems(16, 32, 0) == 0


# ---- production variants: what a decoder level of the default net runs ----------------------------------------------------------------
# 256 -> 512 on a 24 x 40 map: a 2 x 3 grid of ragged forward / data-gradient tiles, the data gradient's 64-channel block on it, and
# 9 weight-gradient tiles over 128 channel cells — on 256 CUs the FULL plan puts 2 tiles in a block (restaging both LDS images under
# live accumulators) and adds 5 splits
PRODUCTION_SHAPE = (1, 24, 40, 256, 512)


def test_production_shape_forward_and_data_gradient():
    c = case(PRODUCTION_SHAPE)
    t = fwd(c)
    e, e_exact = rel(t, c.fwd_same), rel(t, c.fwd_exact)
    nt = dgrad_variant(*PRODUCTION_SHAPE)
    assert nt == 2, f"nt {nt} on {cus()} CUs"
    dx = dgrad(c, True)
    keep = c.x_low > 0
    e_d, e_d_exact = rel(dx, c.dx_same * keep), rel(dx, c.grads_exact[0] * keep)
    print(dict(test="convtr2d_bf16_production", shape=PRODUCTION_SHAPE, fwd=e, fwd_exact=e_exact, dgrad=e_d, dgrad_exact=e_d_exact, nt=nt))
    assert e < TOL_SAME and e_exact < TOL_EXACT and e_d < TOL_SAME and e_d_exact < TOL_EXACT
    assert (dx[~keep] == 0).all().item()


def test_production_shape_weight_gradient_multi_tile_blocks_under_the_full_plan():
    c = case(PRODUCTION_SHAPE)
    tps, nsplit = wgrad_variant(*PRODUCTION_SHAPE)
    assert tps >= 2 and nsplit >= 2, f"tps {tps}, nsplit {nsplit} on {cus()} CUs"
    dw = wgrad(c)
    e, e_exact = rel(dw, c.dw_same), rel(dw, c.grads_exact[1])
    print(dict(test="convtr2d_bf16_wgrad_production", shape=PRODUCTION_SHAPE, tps=tps, nsplit=nsplit, err=e, exact=e_exact))
    assert e < TOL_SAME and e_exact < TOL_EXACT
    assert torch.equal(dw, wgrad(c))
