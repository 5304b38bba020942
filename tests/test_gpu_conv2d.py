"""The 2-D kernels of csrc/u3d_conv2d.hip through the C-ABI (native_2d): Conv2d 3x3 forward, data gradient and weight gradient,
their statistics epilogues, virtual-concat sources, split-K, and MaxPool2d(2) — against float64 F.conv2d / autograd / F.max_pool2d on
the CPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import DEV
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import VSrc, _p, _stream

pytestmark = pytest.mark.gpu
TOL = 1e-4  # max-abs error relative to the float64 result's range (fp32 MFMA accumulation over K = 9 * Cin)


def nhwc(x):  # (N,C,H,W) cpu -> (N,1,H,W,C) gpu (the library's NDHWC with D = 1)
    return x.permute(0, 2, 3, 1).contiguous().unsqueeze(1).to(DEV)


def nchw(y):  # (N,1,H,W,C) gpu -> (N,C,H,W) cpu
    return y.squeeze(1).permute(0, 3, 1, 2).contiguous().cpu()


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def pack2d(w, mode):
    Cout, Cin = w.shape[:2]
    out = torch.empty(nat.get_lib().u3d_packed_weight2d_floats(Cin, Cout, mode), dtype=torch.float32, device=DEV)
    wd = w.float().contiguous().to(DEV)
    nat.call("u3d_pack_weights2d", 0, _stream(DEV), _p(wd), Cout, Cin, mode, _p(out))
    return out


def conv2d(src: VSrc, w, Cout, relu=0, affine=None, mode=0, out_stats=None, gx: VSrc = None, gstats=None, reps=1, use_ws=True):
    """one u3d_conv2d_ex_reps call; mode 1 = data gradient (w is the forward weight (Cin_fwd = Cout here, Cout_fwd = src.C))"""
    wp = pack2d(w, mode)
    y = torch.empty((src.N, 1, src.H, src.W, Cout), dtype=torch.float32, device=DEV)
    s = src.struct(affine)
    gs = gx.struct() if gx is not None else None
    need = nat.get_lib().u3d_conv2d_workspace_floats(src.N, src.H, src.W, src.C, Cout) if use_ws else 0
    ws = torch.empty(need, dtype=torch.float32, device=DEV) if need > 0 else None
    nat.call("u3d_conv2d_ex_reps", 0, _stream(DEV), ctypes.byref(s), _p(wp), _p(y), src.N, src.H, src.W, Cout, relu, _p(out_stats),
             ctypes.byref(gs) if gs is not None else None, _p(gstats), _p(ws), need, reps)
    return y, need


def wgrad2d(src: VSrc, dz, Cout, affine=None):
    dw = torch.empty((Cout, src.C, 3, 3), dtype=torch.float32, device=DEV)
    need = nat.get_lib().u3d_wgrad2d_workspace_floats(src.N, src.H, src.W, src.C, Cout)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
    s = src.struct(affine)
    nat.call("u3d_conv2d_wgrad", 0, _stream(DEV), ctypes.byref(s), _p(dz), _p(dw), src.N, src.H, src.W, Cout, _p(ws), need)
    return dw


def affine_table(N, C, g):
    a = 0.5 + torch.rand(N, C, generator=g)
    b = 0.3 * torch.randn(N, C, generator=g)
    return torch.stack((a, b), dim=-1).contiguous()


def apply_affine(x, aff):  # x (N,C,H,W) float64
    return x * aff[..., 0].double()[:, :, None, None] + aff[..., 1].double()[:, :, None, None]


def check_all(N, H, W, Cin, Cout, seed, relu, use_aff):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    aff = affine_table(N, Cin, g) if use_aff else None
    xa = apply_affine(x.double(), aff) if use_aff else x.double()
    ref = F.conv2d(xa, w.double(), padding=1)
    ref_y = ref.clamp_min(0) if relu else ref
    # forward (+ output statistics)
    st = torch.zeros(N * Cout * 2, dtype=torch.float64, device=DEV)
    y, _ = conv2d(VSrc(nhwc(x)), w, Cout, relu=relu, affine=aff.to(DEV) if use_aff else None, out_stats=st)
    assert rel(nchw(y), ref_y) < TOL
    s_ref = torch.stack((ref_y.sum((2, 3)), (ref_y * ref_y).sum((2, 3))), -1)
    assert rel(st.view(N, Cout, 2).cpu(), s_ref) < 1e-5
    # data gradient w.r.t. the affine output (+ GroupNorm-backward sums against the pre-affine input x)
    dz = torch.randn(N, Cout, H, W, generator=g)
    dg_ref = torch.nn.grad.conv2d_input(xa.shape, w.double(), dz.double(), padding=1)
    gst = torch.zeros(N * Cin * 2, dtype=torch.float64, device=DEV)
    dg, _ = conv2d(VSrc(nhwc(dz)), w, Cin, mode=1, gx=VSrc(nhwc(x)), gstats=gst)
    assert rel(nchw(dg), dg_ref) < TOL
    g_ref = torch.stack((dg_ref.sum((2, 3)), (dg_ref * x.double()).sum((2, 3))), -1)
    assert rel(gst.view(N, Cin, 2).cpu(), g_ref) < 1e-5
    # weight gradient
    dw_ref = torch.nn.grad.conv2d_weight(xa, w.shape, dz.double(), padding=1)
    dw = wgrad2d(VSrc(nhwc(x)), nhwc(dz), Cout, affine=aff.to(DEV) if use_aff else None)
    assert rel(dw.cpu(), dw_ref) < TOL


@pytest.mark.parametrize("Cin", [1, 3, 16, 20, 64, 96, 192])
@pytest.mark.parametrize("Cout", [1, 8, 16, 32, 64, 128])
def test_conv2d_small_images(Cin, Cout):
    for i, (H, W) in enumerate([(1, 1), (2, 3), (7, 9)]):
        check_all(2, H, W, Cin, Cout, seed=100 * Cin + Cout + i, relu=i % 2, use_aff=(i != 1))


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 64, 64, 64, 64), (1, 64, 64, 192, 128), (2, 64, 64, 20, 8), (2, 64, 64, 1, 8),
                                            (1, 64, 64, 96, 1), (1, 515, 512, 1, 32), (1, 515, 512, 32, 32), (1, 515, 512, 3, 16),
                                            (1, 515, 512, 64, 64)])
def test_conv2d_large_images(N, H, W, Cin, Cout):
    check_all(N, H, W, Cin, Cout, seed=7 + Cin + Cout, relu=1, use_aff=True)


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(1, 8, 8, 256, 128), (2, 16, 16, 128, 64), (1, 4, 5, 64, 32)])
def test_conv2d_split_k(N, H, W, Cin, Cout):
    """grids with fewer blocks than CUs split the channel reduction: same results (to round-off) and the same statistics contract"""
    need = nat.get_lib().u3d_conv2d_workspace_floats(N, H, W, Cin, Cout)
    assert need > 0
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    ref = F.conv2d(x.double(), w.double(), padding=1).clamp_min(0)
    outs = []
    for use_ws in (True, False):
        st = torch.zeros(2 * N * Cout * 2, dtype=torch.float64, device=DEV)
        y, n = conv2d(VSrc(nhwc(x)), w, Cout, relu=1, out_stats=st, reps=2, use_ws=use_ws)
        assert (n > 0) == use_ws
        assert rel(nchw(y), ref) < TOL
        s = st.view(2, N, Cout, 2).sum(0).cpu()
        assert rel(s, torch.stack((ref.sum((2, 3)), (ref * ref).sum((2, 3))), -1)) < 1e-5
        outs.append(y)
    assert rel(outs[0].cpu(), outs[1].cpu()) < 1e-5


@pytest.mark.parametrize("reps", [2, 8])
def test_conv2d_stat_replica_rows_sum_to_one_table(reps):
    g = torch.Generator().manual_seed(9)
    N, H, W, Cin, Cout = 2, 40, 37, 16, 32
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 12.0
    one = torch.zeros(N * Cout * 2, dtype=torch.float64, device=DEV)
    many = torch.zeros(reps * N * Cout * 2, dtype=torch.float64, device=DEV)
    y1, _ = conv2d(VSrc(nhwc(x)), w, Cout, relu=1, out_stats=one)
    y2, _ = conv2d(VSrc(nhwc(x)), w, Cout, relu=1, out_stats=many, reps=reps)
    assert torch.equal(y1, y2)
    assert rel(many.view(reps, -1).sum(0).cpu(), one.cpu()) < 1e-12


@pytest.mark.parametrize("hs,ws,hl,wl,C0,C1", [(16, 16, 8, 8, 16, 32), (33, 45, 16, 22, 8, 12), (67, 45, 33, 22, 16, 16),
                                               (3, 3, 1, 1, 4, 8)])
def test_conv2d_virtual_concat(hs, ws, hl, wl, C0, C1):
    """cat(skip, nearest(low)) never materialised: exact 2x and n -> 2n + 1 levels, forward / data-gradient sums / weight gradient"""
    g = torch.Generator().manual_seed(hs * 100 + C1)
    N, Cout = 2, 24
    skip = torch.randn(N, C0, hs, ws, generator=g)
    low = torch.randn(N, C1, hl, wl, generator=g)
    cat = torch.cat((skip, F.interpolate(low, size=(hs, ws), mode="nearest")), dim=1)
    Ct = C0 + C1
    w = torch.randn(Cout, Ct, 3, 3, generator=g) / (3.0 * Ct ** 0.5)
    aff = affine_table(N, Ct, g)
    ca = apply_affine(cat.double(), aff)
    src = VSrc(nhwc(skip), nhwc(low))
    y, _ = conv2d(src, w, Cout, relu=1, affine=aff.to(DEV))
    assert rel(nchw(y), F.conv2d(ca, w.double(), padding=1).clamp_min(0)) < TOL
    dz = torch.randn(N, Cout, hs, ws, generator=g)
    dg_ref = torch.nn.grad.conv2d_input(ca.shape, w.double(), dz.double(), padding=1)
    gst = torch.zeros(N * Ct * 2, dtype=torch.float64, device=DEV)
    dg, _ = conv2d(VSrc(nhwc(dz)), w, Ct, mode=1, gx=src, gstats=gst)
    assert rel(nchw(dg), dg_ref) < TOL
    assert rel(gst.view(N, Ct, 2).cpu(), torch.stack((dg_ref.sum((2, 3)), (dg_ref * cat.double()).sum((2, 3))), -1)) < 1e-5
    dw = wgrad2d(src, nhwc(dz), Cout, affine=aff.to(DEV))
    assert rel(dw.cpu(), torch.nn.grad.conv2d_weight(ca, w.shape, dz.double(), padding=1)) < TOL


def test_conv2d_padding_stays_zero_after_affine():
    """a large offset b: the padded taps must contribute exactly 0 (nn.Conv2d pads the GroupNorm OUTPUT)"""
    N, H, W, C = 1, 5, 6, 16
    x = torch.zeros(N, C, H, W)
    aff = torch.stack((torch.ones(N, C), torch.full((N, C), 3.0)), -1).contiguous()
    w = torch.ones(4, C, 3, 3)
    y, _ = conv2d(VSrc(nhwc(x)), w, 4, affine=aff.to(DEV))
    ref = F.conv2d(torch.full((N, C, H, W), 3.0, dtype=torch.float64), w.double(), padding=1)
    assert torch.equal(nchw(y).double(), ref)


def test_wgrad2d_is_bitwise_deterministic():
    g = torch.Generator().manual_seed(11)
    N, H, W, Cin, Cout = 4, 96, 80, 48, 40
    x, dz = nhwc(torch.randn(N, Cin, H, W, generator=g)), nhwc(torch.randn(N, Cout, H, W, generator=g))
    assert nat.get_lib().u3d_wgrad2d_workspace_floats(N, H, W, Cin, Cout) > 0  # the split path, reduced in a fixed order
    a = wgrad2d(VSrc(x), dz, Cout)
    b = wgrad2d(VSrc(x), dz, Cout)
    assert torch.equal(a, b)


@pytest.mark.parametrize("N,H,W,C", [(2, 7, 9, 5), (1, 515, 512, 8), (3, 2, 2, 16), (2, 33, 45, 12)])
def test_maxpool2d_forward_backward(N, H, W, C):
    g = torch.Generator().manual_seed(H * W + C)
    # integer values: many ties (first maximum in scan order wins, as ATen)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
    H2, W2 = H // 2, W // 2
    out = torch.empty((N, 1, H2, W2, C), dtype=torch.float32, device=DEV)
    am = torch.empty((N, 1, H2, W2, C), dtype=torch.uint8, device=DEV)
    xe = nhwc(x)
    nat.call("u3d_maxpool2d_fwd", 0, _stream(DEV), _p(xe), N, H, W, C, _p(out), _p(am), None)
    ref, idx = F.max_pool2d(x, 2, return_indices=True)
    assert torch.equal(nchw(out), ref)
    # argmax byte = 2 * dy + dx, from ATen's flat indices
    iy, ix = idx // W, idx % W
    k = 2 * (iy - 2 * torch.arange(H2).view(1, 1, -1, 1)) + (ix - 2 * torch.arange(W2).view(1, 1, 1, -1))
    assert torch.equal(nchw(am).long(), k)
    # backward merge: (skip + scatter(p * dg + q * pooled + r)) * (e > 0)
    dg = torch.randn(N, C, H2, W2, generator=g)
    skip = torch.randn(N, C, H, W, generator=g)
    coef = torch.randn(N, 3, C, generator=g)
    e = torch.randn(N, C, H, W, generator=g)
    dpool = coef[:, 0, :, None, None] * dg + coef[:, 1, :, None, None] * ref + coef[:, 2, :, None, None]
    scat = torch.zeros(N, C, H * W).scatter_add_(2, idx.view(N, C, -1), dpool.view(N, C, -1)).view(N, C, H, W)
    want = (skip + scat) * (e > 0)
    dg_d, coef_d, skip_d, e_d = nhwc(dg), coef.to(DEV), nhwc(skip), nhwc(e)  # (kept alive: the calls take raw pointers)
    res = torch.empty_like(e_d)
    nat.call("u3d_maxpool2d_bwd_merge", 0, _stream(DEV), _p(dg_d), _p(out), _p(am), _p(coef_d), _p(skip_d), _p(e_d), N, H, W, C, 1,
             _p(res))
    assert rel(nchw(res), want) < 1e-6
    # ... with the skip gradient as the GroupNorm backward of a wider (Ctot-channel) decoder gradient
    Ct = C + 3
    sdg = torch.randn(N, Ct, H, W, generator=g)
    scoef = torch.randn(N, 3, Ct, generator=g)
    sk = scoef[:, 0, :C, None, None] * sdg[:, :C] + scoef[:, 1, :C, None, None] * e + scoef[:, 2, :C, None, None]
    want = (sk + scat) * (e > 0)
    sdg_d, scoef_d = nhwc(sdg), scoef.to(DEV)
    nat.call("u3d_maxpool2d_bwd_merge_gn", 0, _stream(DEV), _p(dg_d), _p(out), _p(am), _p(coef_d), _p(sdg_d), Ct, _p(scoef_d), Ct,
             _p(e_d), N, H, W, C, 1, _p(res))
    assert rel(nchw(res), want) < 1e-5
