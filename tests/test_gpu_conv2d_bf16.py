"""-m gpu: the bf16-operand 2-D kernels of csrc/u3d_conv2d_bf16.hip through the C-ABI (`native_2d_bf16`): Conv2d 3x3 forward, data
gradient and weight gradient on v_mfma_f32_32x32x16_bf16, their statistics epilogues, split-K and the envelope — against float64
F.conv2d / autograd on the CPU with the SAME operand rounding restated (`.to(torch.bfloat16)`, the activation after the fp32 affine).

Bars (the project's own): with an identity affine the operands match bit for bit and only the accumulation order differs — 1e-4 of the
result's range, TOL of test_gpu_conv2d.py; with a random affine 1e-3 (test_gpu_bf16.py: the rare operand that rounds the other way after
a 1-ulp difference in the affine); 2e-2 against the exact fp32 operands.  Statistics tables: float64 sums of the kernel's own written
output, 1e-5 of the table's maximum (the fp32 2-D family's bar, test_gpu_conv2d.py).

The launch plans follow the grid size, so which kernel a shape runs is asserted, not assumed: u3d_conv2d_bf16_variant /
u3d_conv2d_wgrad_bf16_variant report the plan the launch takes.  SHAPES are small grids (one n-tile per block, split-K whenever a
workspace is passed, one tile per weight-gradient block); the tests from "production variants" on run what a full-resolution UNet2D level
runs: the unsplit kernel's fused epilogue, the 64-channel block and multi-tile weight-gradient blocks."""
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

# (N, H, W, Cin, Cout): the smallest shapes that exercise each way the kernels can go wrong
SHAPES = [
    (1, 4, 5, 32, 32),      # smaller than one tile
    (2, 17, 19, 32, 64),    # ragged 2 x 2 tiles, two 32-channel n-tiles (one per block: 8 tiles are too few for the 64-channel block)
    (1, 33, 45, 96, 32),    # three K chunks ... (six 16-channel ones)
    (1, 16, 16, 64, 96),    # three 32-channel n-tiles
    (1, 8, 8, 256, 128),    # split-K through the workspace
]
SPLIT_SHAPE = SHAPES[-1]


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


def fwd_variant(N, H, W, Cin, Cout, use_ws):
    """(n-tiles per block, ksplit) of the u3d_conv2d_bf16 launch on (N,H,W,Cin) -> Cout (a data gradient asks with the roles swapped)"""
    v = nat.get_lib().u3d_conv2d_bf16_variant(N, H, W, Cin, Cout, 1 if use_ws else 0)
    assert v > 0, (v, (N, H, W, Cin, Cout))
    return v & 255, v >> 8


def wgrad_variant(N, H, W, Cin, Cout):
    """(tiles per block, nsplit) of the u3d_conv2d_wgrad_bf16 launch"""
    v = nat.get_lib().u3d_conv2d_wgrad_bf16_variant(N, H, W, Cin, Cout)
    assert v > 0, (v, (N, H, W, Cin, Cout))
    return v >> 16, v & 0xFFFF


def pack(w, mode):
    Cout, Cin = w.shape[:2]
    n = nat.get_lib().u3d_packed_weight2d_bf16_elems(Cin, Cout, mode)
    assert n > 0
    out = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    wd = w.float().contiguous().to(DEV)
    nat.call("u3d_pack_weights2d_bf16", 0, _stream(DEV), _p(wd), Cout, Cin, mode, _p(out))
    return out


def conv(x, w, mode=0, affine=None, relu=0, out_stats=None, gx=None, gstats=None, reps=1, use_ws=True):
    """one u3d_conv2d_bf16 call on x (N,C,H,W) cpu; mode 1: x is dz and w the forward weight.  Returns ((N,K,H,W) cpu, workspace floats)"""
    N, C, H, W = x.shape
    K = w.shape[0] if mode == 0 else w.shape[1]
    wp, xd = pack(w, mode), nhwc(x)
    y = torch.empty((N, H, W, K), dtype=torch.float32, device=DEV)
    need = nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, C, K) if use_ws else 0
    ws = torch.empty(need, dtype=torch.float32, device=DEV) if need > 0 else None
    nat.call("u3d_conv2d_bf16", 0, _stream(DEV), _p(xd), _p(affine), _p(wp), _p(y), N, H, W, C, K, relu, _p(out_stats), _p(gx), _p(gstats),
             _p(ws), need, reps)
    torch.cuda.synchronize()
    return nchw(y), need


def wgrad(x, dz, affine=None):
    N, C, H, W = x.shape
    K = dz.shape[1]
    need = nat.get_lib().u3d_wgrad2d_bf16_workspace_floats(N, H, W, C, K)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    dw = torch.full((K, C, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    xd, dzd = nhwc(x), nhwc(dz)
    nat.call("u3d_conv2d_wgrad_bf16", 0, _stream(DEV), _p(xd), _p(affine), _p(dzd), _p(dw), N, H, W, C, K, _p(ws), need)
    torch.cuda.synchronize()
    return dw.cpu()


class Case:
    """inputs and float64 references of one shape, each computed once, when first asked for, and shared by the tests (never modified)"""

    def __init__(self, shape):
        N, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(1000 + H * W + Cin + Cout)
        self.shape = shape
        self.x = torch.randn(N, Cin, H, W, generator=g)
        self.w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
        self.dz = torch.randn(N, Cout, H, W, generator=g)
        a = 1.0 + 0.3 * torch.randn(N, Cin, generator=g)
        b = 0.5 + 0.2 * torch.randn(N, Cin, generator=g)  # a clearly nonzero offset: padding must not pick it up
        self.aff = torch.stack((a, b), dim=-1).contiguous()
        # the affine in fp32, as the kernel applies it (a product and a sum, or one fused multiply-add: 1 ulp apart at most)
        self.g = self.x * a.view(N, Cin, 1, 1) + b.view(N, Cin, 1, 1)

    @cached_property
    def fwd_same(self):  # identity affine
        return F.conv2d(r16(self.x), r16(self.w), padding=1)

    @cached_property
    def fwd_aff(self):
        return F.conv2d(r16(self.g), r16(self.w), padding=1)

    @cached_property
    def fwd_exact(self):
        return F.conv2d(self.g.double(), self.w.double(), padding=1)

    @cached_property
    def dg(self):  # mode-1 consistency: autograd of the mode-0 convolution on the rounded operands
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
    """float64 (sum y, sum y * other) per (sample, channel) of a written (N,C,H,W) output"""
    y = y.double()
    return torch.stack((y.sum(dim=(2, 3)), (y * other.double()).sum(dim=(2, 3))), dim=-1)


def check_forward(shape, use_ws):
    """affine, ReLU, out_stats and the border of one forward launch; returns the plan it ran as (n-tiles per block, ksplit)"""
    c = case(shape)
    N, H, W, Cin, Cout = shape
    var = fwd_variant(N, H, W, Cin, Cout, use_ws)
    st = torch.zeros((N, Cout, 2), dtype=torch.float64, device=DEV)
    y, _ = conv(c.x, c.w, affine=c.aff.to(DEV), relu=1, out_stats=st, use_ws=use_ws)
    ref = c.fwd_aff.clamp_min(0)
    scale = c.fwd_aff.abs().max().item()
    e = (y.double() - ref).abs().max().item() / scale
    e_border = (_border(y.double()) - _border(ref)).abs().max().item() / scale
    e_exact = (y.double() - c.fwd_exact.clamp_min(0)).abs().max().item() / scale
    s = st.cpu()
    e_stats = rel(s, stat_table(y, y))
    print(dict(test="conv2d_bf16_fwd", shape=shape, nt=var[0], ksplit=var[1], err=e, border=e_border, exact=e_exact, stats=e_stats))
    assert e < TOL_AFF
    assert e_border < TOL_AFF  # the offset b = 0.5 leaking into the padding would show here as ~b * |w| * taps, far above the bar
    assert e_exact < TOL_EXACT
    assert e_stats < TOL_STATS
    return var, s, y


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_affine_relu_stats_and_zero_padding(shape):
    N, H, W, Cin, Cout = shape
    _, s, y = check_forward(shape, use_ws=True)
    scale = case(shape).fwd_aff.abs().max().item()
    assert torch.allclose(s[..., 0], y.double().sum(dim=(2, 3)), rtol=1e-6, atol=1e-6 * H * W * scale)
    assert torch.allclose(s[..., 1], (y.double() ** 2).sum(dim=(2, 3)), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_identity_affine_matches_to_accumulation_order(shape):
    c = case(shape)
    y, _ = conv(c.x, c.w)
    e = rel(y, c.fwd_same)
    print(dict(test="conv2d_bf16_fwd_same", shape=shape, err=e))
    assert e < TOL_SAME
    # an explicit (1, 0) table is the same convolution
    N, Cin = shape[0], shape[3]
    ida = torch.tensor([1.0, 0.0]).repeat(N, Cin, 1).contiguous().to(DEV)
    y2, _ = conv(c.x, c.w, affine=ida)
    assert torch.equal(y, y2)


def check_data_gradient(shape, use_ws):
    """gx / gstats of one data-gradient launch of the LAYER `shape`; returns the plan it ran as (n-tiles per block, ksplit)"""
    c = case(shape)
    N, H, W, Cin, Cout = shape
    var = fwd_variant(N, H, W, Cout, Cin, use_ws)  # the launch contracts over the layer's Cout
    gst = torch.zeros((N, Cin, 2), dtype=torch.float64, device=DEV)
    xd = nhwc(c.x)
    dg, _ = conv(c.dz, c.w, mode=1, gx=xd, gstats=gst, use_ws=use_ws)
    scale = c.dg.abs().max().item()
    e = (dg.double() - c.dg).abs().max().item() / scale
    e_exact = (dg.double() - c.dg_exact).abs().max().item() / scale
    s = gst.cpu()
    e_stats = rel(s, stat_table(dg, c.x))
    print(dict(test="conv2d_bf16_dgrad", shape=shape, nt=var[0], ksplit=var[1], err=e, exact=e_exact, stats=e_stats))
    assert e < TOL_SAME and e_exact < TOL_EXACT
    assert e_stats < TOL_STATS
    return var, s, dg


@pytest.mark.parametrize("shape", SHAPES)
def test_data_gradient_with_groupnorm_sums(shape):
    """the mode-1 image on dz is the data gradient: equal to autograd of the mode-0 convolution on the rounded operands"""
    c = case(shape)
    N, H, W, Cin, Cout = shape
    _, s, dg = check_data_gradient(shape, use_ws=True)
    atol = 1e-6 * dg.abs().sum().item() / (N * Cin)
    assert torch.allclose(s[..., 0], dg.double().sum(dim=(2, 3)), rtol=1e-6, atol=atol)
    assert torch.allclose(s[..., 1], (dg.double() * c.x.double()).sum(dim=(2, 3)), rtol=1e-6, atol=atol)


def check_weight_gradient(shape, use_aff, exact=True):
    """dw of one launch (pre-filled with NaN) against float64, and bitwise equal on a second call; returns (tiles per block, nsplit)"""
    c = case(shape)
    var = wgrad_variant(*shape)
    aff = c.aff.to(DEV) if use_aff else None
    ref = c.dw_aff if use_aff else c.dw_same
    dw = wgrad(c.x, c.dz, aff)
    assert torch.isfinite(dw).all()
    scale = ref.abs().max().item()
    e = (dw.double() - ref).abs().max().item() / scale
    print(dict(test="conv2d_bf16_wgrad", shape=shape, tps=var[0], nsplit=var[1], affine=use_aff, err=e))
    assert e < (TOL_AFF if use_aff else TOL_SAME)
    if use_aff and exact:
        assert (dw.double() - c.dw_exact).abs().max().item() < TOL_EXACT * scale
    assert torch.equal(dw, wgrad(c.x, c.dz, aff))  # fixed-order reduction: the same inputs give a bitwise-identical dw
    return var


@pytest.mark.parametrize("use_aff", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient(shape, use_aff):
    check_weight_gradient(shape, use_aff)


@pytest.mark.parametrize("reps", [1, 2])
def test_split_k_through_the_workspace(reps):
    """fewer blocks than CUs: the channel reduction is split over blocks and added in a fixed order by the kernel that owns the
    epilogue — the results of the unsplit launch to round-off, run-to-run identical, the same statistics contract"""
    c = case(SPLIT_SHAPE)
    N, H, W, Cin, Cout = SPLIT_SHAPE
    assert nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, Cin, Cout) > 0
    ref = c.fwd_same.clamp_min(0)
    scale = c.fwd_same.abs().max().item()
    outs = []
    for use_ws in (True, True, False):
        st = torch.zeros((reps, N, Cout, 2), dtype=torch.float64, device=DEV)
        y, need = conv(c.x, c.w, relu=1, out_stats=st, reps=reps, use_ws=use_ws)
        assert (need > 0) == use_ws
        assert (y.double() - ref).abs().max().item() < TOL_SAME * scale
        s = st.sum(0).cpu()
        assert torch.allclose(s[..., 0], y.double().sum(dim=(2, 3)), rtol=1e-5, atol=1e-4)
        assert torch.allclose(s[..., 1], (y.double() ** 2).sum(dim=(2, 3)), rtol=1e-5, atol=1e-4)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    # the data gradient of the same layer splits too (contraction over 128 channels), with its GroupNorm-backward sums
    gst = torch.zeros((reps, N, Cin, 2), dtype=torch.float64, device=DEV)
    xd = nhwc(c.x)
    dg, need = conv(c.dz, c.w, mode=1, gx=xd, gstats=gst, reps=reps)
    assert need > 0 and rel(dg, c.dg) < TOL_SAME
    s = gst.sum(0).cpu()
    assert torch.allclose(s[..., 0], dg.double().sum(dim=(2, 3)), rtol=1e-5, atol=1e-4)
    assert torch.allclose(s[..., 1], (dg.double() * c.x.double()).sum(dim=(2, 3)), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("Cin,Cout", [(20, 32), (32, 8)])
def test_channel_counts_outside_the_envelope_are_refused(Cin, Cout):
    lib = nat.get_lib()
    assert lib.u3d_conv2d_bf16_supported(32, 32) == 1 and lib.u3d_conv2d_wgrad_bf16_supported(32, 64) == 1
    assert lib.u3d_conv2d_bf16_supported(16, 32) == 1 and lib.u3d_conv2d_wgrad_bf16_supported(16, 32) == 0
    assert lib.u3d_conv2d_bf16_supported(Cin, Cout) == 0 and lib.u3d_conv2d_wgrad_bf16_supported(Cin, Cout) == 0
    assert lib.u3d_packed_weight2d_bf16_elems(Cin, Cout, 0) == 0
    N, H, W = 1, 6, 7
    x = torch.randn(N, H, W, Cin, device=DEV)
    dz = torch.randn(N, H, W, Cout, device=DEV)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV)
    img = torch.full((4096,), 7.0, dtype=torch.bfloat16, device=DEV)
    y = torch.full((N, H, W, Cout), 7.0, device=DEV)
    dw = torch.full((Cout, Cin, 3, 3), 7.0, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    with pytest.raises(nat.U3DError):
        nat.call("u3d_pack_weights2d_bf16", 0, _stream(DEV), _p(w), Cout, Cin, 0, _p(img))
    with pytest.raises(nat.U3DError):
        nat.call("u3d_conv2d_bf16", 0, _stream(DEV), _p(x), None, _p(img), _p(y), N, H, W, Cin, Cout, 0, None, None, None, _p(ws),
                 ws.numel(), 1)
    with pytest.raises(nat.U3DError):
        nat.call("u3d_conv2d_wgrad_bf16", 0, _stream(DEV), _p(x), None, _p(dz), _p(dw), N, H, W, Cin, Cout, _p(ws), ws.numel())
    torch.cuda.synchronize()
    assert (img == 7.0).all() and (y == 7.0).all() and (dw == 7.0).all()  # nothing was launched


# ---- production variants: what a full-resolution UNet2D level runs ------------------------------------------------------------------
# A single 16-channel chunk cannot split even with a workspace: the engine's own situation on its 16 -> 32 layers
ONE_CHUNK_SHAPE = (2, 17, 19, 16, 32)
REPLICA_SHAPE = (2, 40, 37, 16, 32)  # the launch of test_conv2d_stat_replica_rows_sum_to_one_table: 18 blocks over the replica rows
# >= 2 * CUs tiles (256 CUs): the 64-channel block, unsplit.  250 x 245: the last tile row and column are ragged
NT2_FWD_SHAPES = [
    (2, 250, 245, 16, 64),  # 512 tiles, two n-tiles in one block
    (1, 250, 245, 32, 96),  # three n-tiles over two blocks: the second n-tile of the last block is the zero fragment, never written
]
NT2_DGRAD_SHAPE = (2, 250, 245, 64, 32)  # the layer 64 -> 32: its data gradient contracts over 32 channels and produces 64
WGRAD_MULTI_TILE_SHAPES = [
    (1, 139, 141, 128, 128),  # 81 ragged tiles, 16 channel cells: 2 tiles per block, 41 splits, the last block holds one tile
    (1, 70, 75, 256, 256),    # 25 tiles, 64 cells: 2 tiles per block, 13 splits
]


@pytest.mark.parametrize("shape", SHAPES + [ONE_CHUNK_SHAPE])
def test_forward_unsplit_fused_epilogue(shape):
    """no workspace: conv2d_bf16_kernel itself applies the ReLU and sums the statistics (c2b_flush_stats), on ragged and several tiles"""
    nt, ksplit = check_forward(shape, use_ws=False)[0]
    assert ksplit == 1, f"ksplit {ksplit} on {cus()} CUs"
    if shape == ONE_CHUNK_SHAPE:
        assert fwd_variant(*shape, use_ws=True)[1] == 1, f"a single chunk split on {cus()} CUs"


@pytest.mark.parametrize("shape", SHAPES)
def test_data_gradient_unsplit_fused_epilogue(shape):
    """no workspace: the gx / gstats sums of the main kernel's epilogue"""
    nt, ksplit = check_data_gradient(shape, use_ws=False)[0]
    assert ksplit == 1, f"ksplit {ksplit} on {cus()} CUs"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("reps", [2, 8])
def test_replica_rows_of_the_fused_epilogue_sum_to_one_table(reps, mode):
    """stat_reps > 1 in the main kernel: block b adds into row b % reps — the same output bit for bit, and rows that sum to the table of
    stat_reps = 1 (test_conv2d_stat_replica_rows_sum_to_one_table of the fp32 family); mode 1: the same launch as a data gradient"""
    N, H, W, C, K = REPLICA_SHAPE
    assert fwd_variant(N, H, W, C, K, use_ws=False)[1] == 1, f"split on {cus()} CUs"
    c = case(REPLICA_SHAPE if mode == 0 else (N, H, W, K, C))  # mode 1: the layer 32 -> 16, whose data gradient is the 16 -> 32 launch
    src, other = (c.x, None) if mode == 0 else (c.dz, nhwc(c.x))

    def run(r):
        t = torch.zeros((r, N, K, 2), dtype=torch.float64, device=DEV)
        if mode == 0:
            y, need = conv(src, c.w, relu=1, out_stats=t, reps=r, use_ws=False)
        else:
            y, need = conv(src, c.w, mode=1, gx=other, gstats=t, reps=r, use_ws=False)
        assert need == 0
        return y, t.cpu()

    y1, one = run(1)
    y2, many = run(reps)
    assert torch.equal(y1, y2)
    assert (many.abs().sum(dim=(1, 2, 3)) > 0).all()  # 18 blocks: every replica row took some
    e_rows = rel(many.sum(0), one[0])
    e_stats = rel(one[0], stat_table(y1, y1 if mode == 0 else c.x))
    print(dict(test="conv2d_bf16_replicas", mode=mode, reps=reps, rows=e_rows, stats=e_stats))
    assert e_rows < 1e-12
    assert e_stats < TOL_STATS
    assert rel(y1, c.fwd_same.clamp_min(0) if mode == 0 else c.dg) < TOL_SAME


@pytest.mark.parametrize("shape", NT2_FWD_SHAPES)
def test_forward_64_channel_block(shape):
    """conv2d_bf16_kernel<2>: the second n-tile's B stream and accumulators, and for three n-tiles its zero fragment"""
    try:
        nt, ksplit = check_forward(shape, use_ws=True)[0]
    finally:
        _CASES.pop(shape, None)  # (no other test uses these references: ~100 MB each)
    assert nt == 2 and ksplit == 1, f"nt {nt}, ksplit {ksplit} on {cus()} CUs"


def test_data_gradient_64_channel_block():
    try:
        nt, ksplit = check_data_gradient(NT2_DGRAD_SHAPE, use_ws=True)[0]
    finally:
        _CASES.pop(NT2_DGRAD_SHAPE, None)
    assert nt == 2 and ksplit == 1, f"nt {nt}, ksplit {ksplit} on {cus()} CUs"


@pytest.mark.parametrize("use_aff", [False, True])
@pytest.mark.parametrize("shape", WGRAD_MULTI_TILE_SHAPES)
def test_weight_gradient_multi_tile_blocks(shape, use_aff):
    """more than one tile per block: the tile loop of conv2d_wgrad_bf16_kernel restages both LDS images under live accumulators"""
    tps, nsplit = check_weight_gradient(shape, use_aff, exact=False)
    assert tps >= 2, f"tps {tps}, nsplit {nsplit} on {cus()} CUs"
