"""-m gpu: u3d_conv2d_f32s_res through the C-ABI — out = [relu](conv2d(a * x + b, w) + residual) on six bf16 MFMA products of exactly split
fp32 operands, the epilogue of conv3 of a ResNetBlock under `native_2d_residual_fp32_split` (csrc/u3d_conv2d_f32s.h, the RES variants of
c2s_conv_kernel).  Helpers and operands are those of tests/test_gpu_conv2d_f32s.py; the residual is drawn at the convolution output's
scale, so that neither term hides the other.

Exactness: the residual is ONE fp32 add onto the signed accumulator, before the ReLU and the statistics: the output equals the fp32 sum
u3d_conv2d_f32s(x) + residual bit for bit (and its clamp at zero with relu = 1), also with the residual aliasing the output and with any
number of replica rows.
fp32 grade: relative L2 against float64 relu(conv2d(g, w) + residual) <= 2.5x the error of u3d_conv2d_res_reps and <= 1/100 of the error
of u3d_conv2d_bf16_res on the same operands (the bars of tests/test_gpu_conv2d_f32s.py).
Statistics: within 1e-5 of the table's largest entry from the float64 sums of the STORED output (that file's TOL_STATS).

Measured on an MI355X (new / u3d_conv2d_res_reps): 0.80x, 1.17x, 1.44x, 1.12x in the order of SHAPES; against
u3d_conv2d_bf16_res 3.4e-5 - 1.4e-4 of its error."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv2d as C2
import test_gpu_conv2d_bf16 as C2B
import test_gpu_conv2d_f32s as CF
from conftest import diag
from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import VSrc, _p, _stream

pytestmark = pytest.mark.gpu

SHAPES = [  # (N, H, W, C, K)
    (2, 21, 37, 16, 32),   # ragged, one chunk
    (1, 17, 19, 32, 64),   # two chunks: result sign -1, NT = 2
    (1, 32, 48, 48, 96),   # three chunks, three n-tiles
    (1, 1, 1, 32, 32),     # single pixel
]
_CASES = {}


class Case:
    """operands, the residual, the float64 truth and the plain u3d_conv2d_f32s output of one shape: computed once, shared, left unchanged"""

    def __init__(self, shape):
        N, H, W, C, K = shape
        self.shape = shape
        self.x, self.w, _, self.aff, g32 = CF.operands(N, H, W, C, K, 11)
        conv = F.conv2d(g32.double(), self.w.double(), None, padding=1)
        g = torch.Generator().manual_seed(12 + H * W + C + K)
        self.res = (torch.randn(N, K, H, W, generator=g) * conv.std(unbiased=False).clamp_min(1e-3)).float()
        self.ref = conv + self.res.double()
        self.xd, self.affd, self.resd = CF.nhwc(self.x), self.aff.to(DEV), CF.nhwc(self.res)
        self.plain = CF.fwd(self.xd, self.w, affine=self.affd, relu=0)  # (N,H,W,K) on the device
        self.sum32 = self.plain + self.resd  # the fp32 sum the epilogue must reproduce


def case(shape) -> Case:
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


def fwd_res(c: Case, relu, out=None, residual=None, out_stats=None, reps=1):
    """u3d_conv2d_f32s_res on the case's tensors; returns (N,H,W,K) on the device"""
    N, H, W, C, K = c.shape
    y = torch.empty((N, H, W, K), dtype=torch.float32, device=DEV) if out is None else out
    r = c.resd if residual is None else residual
    nat.call("u3d_conv2d_f32s_res", 0, _stream(DEV), _p(c.xd), _p(c.affd), _p(CF.pack(c.w, 0)), _p(y), N, H, W, C, K, relu, _p(out_stats),
             reps, _p(r))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("shape", SHAPES)
def test_the_epilogue_is_one_exact_fp32_add_before_the_relu(shape):
    c = case(shape)
    N, H, W, C, K = shape
    y0 = fwd_res(c, 0)
    assert torch.equal(y0, c.sum32)
    y1 = fwd_res(c, 1)
    assert torch.equal(y1, c.sum32.clamp_min(0))
    # the residual aliasing the output: the same lane reads an element before it writes it
    buf = c.resd.clone()
    ya = fwd_res(c, 1, out=buf, residual=buf)
    assert ya.data_ptr() == buf.data_ptr() and torch.equal(ya, y1)
    # replica rows change neither the output nor the summed tables
    st1 = torch.zeros((1, N, K, 2), dtype=torch.float64, device=DEV)
    st3 = torch.zeros((3, N, K, 2), dtype=torch.float64, device=DEV)
    a, b = fwd_res(c, 1, out_stats=st1, reps=1), fwd_res(c, 1, out_stats=st3, reps=3)
    assert torch.equal(a, y1) and torch.equal(b, y1)
    want = CF.stat_table(CF.nchw(y1), CF.nchw(y1))
    CF.check_stats(st1[0], want, "reps 1")
    CF.check_stats(st3.sum(0), want, "reps 3")
    agree = (st3.sum(0) - st1[0]).abs().max().item() / want.abs().max().item()
    assert agree < CF.TOL_STATS, agree
    if N * ((H + 15) // 16) * ((W + 15) // 16) * (K // 64 if K % 64 == 0 else K // 32) >= 3:
        assert all(st3[r].abs().sum().item() > 0 for r in range(3))  # the blocks spread over the replica rows


@pytest.mark.parametrize("shape", SHAPES)
def test_statistics_without_relu_describe_the_stored_sum(shape):
    c = case(shape)
    N, H, W, C, K = shape
    st = torch.zeros((2, N, K, 2), dtype=torch.float64, device=DEV)
    y = CF.nchw(fwd_res(c, 0, out_stats=st, reps=2))
    CF.check_stats(st.sum(0), CF.stat_table(y, y), "relu 0")


@pytest.mark.parametrize("shape", SHAPES)
def test_the_result_is_fp32_grade(shape):
    c = case(shape)
    N, H, W, C, K = shape
    ref = c.ref.clamp_min(0)
    y = CF.nchw(fwd_res(c, 1))
    # the fp32 MFMA kernel with the same epilogue
    src = VSrc(c.xd.unsqueeze(1))
    y32 = torch.empty((N, 1, H, W, K), dtype=torch.float32, device=DEV)
    s = src.struct(c.affd)
    need = nat.get_lib().u3d_conv2d_workspace_floats(N, H, W, C, K)
    ws = torch.empty(need, dtype=torch.float32, device=DEV) if need > 0 else None
    nat.call("u3d_conv2d_res_reps", 0, _stream(DEV), ctypes.byref(s), _p(C2.pack2d(c.w, 0)), _p(y32), N, H, W, K, 1, None, None, None, _p(ws),
             need, 1, _p(c.resd))
    # the bf16-operand kernel with the same epilogue
    yb = torch.empty((N, H, W, K), dtype=torch.float32, device=DEV)
    needb = nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, C, K)
    wsb = torch.empty(needb, dtype=torch.float32, device=DEV) if needb > 0 else None
    nat.call("u3d_conv2d_bf16_res", 0, _stream(DEV), _p(c.xd), _p(c.affd), _p(C2B.pack(c.w, 0)), _p(yb), N, H, W, C, K, 1, None, None, None,
             _p(wsb), needb, 1, _p(c.resd))
    torch.cuda.synchronize()
    e_new, e_f32, e_b16 = CF.rel_l2(y, ref), CF.rel_l2(CF.nchw(y32.squeeze(1)), ref), CF.rel_l2(CF.nchw(yb), ref)
    diag(test="conv2d_f32s_res", shape=[N, H, W], C=C, K=K, l2_split=e_new, l2_f32mfma=e_f32, l2_bf16=e_b16,
         split_over_f32=e_new / e_f32, split_over_bf16=e_new / e_b16)
    assert e_new <= 2.5 * e_f32, (e_new, e_f32)
    assert e_new <= 1e-2 * e_b16, (e_new, e_b16)


def test_refusals_return_einval_and_launch_nothing():
    N, H, W = 1, 8, 8
    lib, core, st = nat.get_ext_lib(), nat.get_lib(), _stream(DEV)
    x = torch.randn(N, H, W, 64, device=DEV)
    res = torch.randn(N * H * W * 64 + 4, device=DEV)
    img = torch.zeros(27 * 64 * 64, dtype=torch.bfloat16, device=DEV)
    out = torch.full((N, H, W, 64), float("nan"), device=DEV)

    def f(C, K, r):
        return lib.u3d_conv2d_f32s_res(0, st, _p(x), None, _p(img), _p(out), N, H, W, C, K, 0, None, 1, r)

    for rc, what in ((f(32, 32, None), "a NULL residual"),
                     (f(32, 32, ctypes.c_void_p(res.data_ptr() + 4)), "a residual 4 bytes off"),
                     (f(8, 32, _p(res)), "C = 8"),
                     (f(32, 48, _p(res)), "K = 48")):
        torch.cuda.synchronize()
        assert rc == nat.U3D_EINVAL, what
        assert b"u3d_conv2d_f32s_res" in core.u3d_last_error(), what
        assert torch.isnan(out).all(), what
