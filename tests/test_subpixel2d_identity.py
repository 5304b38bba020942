"""CPU side of the opt-in sub-pixel decoder path of a UNet2D (`native_2d_subpixel: true` / U3D_NATIVE_2D_SUBPIXEL=1): the identities
csrc/u3d_subpix2d.hip builds on (tests/subpixel2d_ref.py) against ATen's convolution over the nearest-upsampled tensor in float64, the
model key, and which decoder levels the executor hands to the sub-pixel kernels."""
import pytest
import torch
import torch.nn.functional as F

import subpixel2d_ref as sp

SHAPES = [(2, 1, 1, 4, 4), (2, 1, 3, 8, 24), (2, 9, 23, 12, 20)]  # (N, H1, W1, C1, Cout)
_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("N,H1,W1,C1,Cout", SHAPES)
def test_identity_against_aten_in_float64(N, H1, W1, C1, Cout):
    g = torch.Generator().manual_seed(H1 * 100 + W1)
    low = torch.randn(N, C1, H1, W1, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C1, 3, 3, generator=g, dtype=torch.float64)
    dz = torch.randn(N, Cout, 2 * H1, 2 * W1, generator=g, dtype=torch.float64)
    up = F.interpolate(low, size=(2 * H1, 2 * W1), mode="nearest")
    assert _rel(sp.forward(low, w), F.conv2d(up, w, padding=1)) < 1e-12
    dup = torch.nn.grad.conv2d_input(up.shape, w, dz, padding=1)
    dlow_ref = dup.view(N, C1, H1, 2, W1, 2).sum((3, 5))  # the children sum: backward of the nearest upsampling
    assert _rel(sp.dgrad_low(dz, w), dlow_ref) < 1e-12
    assert _rel(sp.dgrad_low_gather(dz, w), dlow_ref) < 1e-12  # the 4 x 4-tap stride-2 gather the kernel evaluates
    assert _rel(sp.wgrad(low, dz), torch.nn.grad.conv2d_weight(up, w.shape, dz, padding=1)) < 1e-12


def test_the_key_implies_native_2d_and_stays_fp32():
    M = _m()
    cfg = dict(name="UNet2D", **_SMALL)
    assert not M.get_model(dict(cfg)).native_supported  # default unchanged
    m = M.get_model(dict(cfg, native_2d_subpixel=True))
    assert m.native_supported and m.native_2d and m.native_2d_subpixel and not m.compute_bf16, m._native_blockers
    assert M.get_model(dict(cfg, native_2d=True)).native_2d_subpixel is False  # native_2d alone: nothing changes
    m = M.get_model(dict(cfg, native_2d_subpixel=True, native_2d_stem=True))  # allowed next to the stem
    assert m.native_supported and m.native_2d_subpixel and m.native_2d_stem


@pytest.mark.parametrize("name", ["ResidualUNet2D", "UNet3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, **_SMALL)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_subpixel=True))
    assert b.native_2d_subpixel is False
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d and a._native_blockers == b._native_blockers


@pytest.mark.parametrize("other", ["native_2d_bf16", "native_2d_bf16_vcat"])
def test_bf16_next_to_the_key_is_a_contradiction(other):
    M = _m()
    with pytest.raises(ValueError, match="native_2d_subpixel"):
        M.get_model(dict(name="UNet2D", **_SMALL, native_2d_subpixel=True, **{other: True}))


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_SUBPIXEL", "1")
    m = M.UNet2D(**_SMALL)
    assert m.native_supported and m.native_2d and m.native_2d_subpixel
    m = M.UNet2D(**_SMALL, native_2d_subpixel=False)  # the key wins
    assert not m.native_supported and not m.native_2d_subpixel
    assert M.UNet3D(**_SMALL).native_2d_subpixel is False and not M.ResidualUNet2D(**_SMALL).native_supported
    monkeypatch.setenv("U3D_NATIVE_2D_SUBPIXEL", "0")
    assert not M.UNet2D(**_SMALL).native_supported


def test_which_levels_take_the_sub_pixel_path():
    """per input size: exact-2x levels with C0, C1, Cout multiples of 4; an n -> 2n + 1 level keeps its virtual concat"""
    M = _m()
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32], num_groups=4)
    eng = M.get_model(dict(cfg, native_2d_subpixel=True))._get_engine()
    assert eng.is2d and eng.subpixel2d and eng.children == 4.0
    w = [id(c1.conv.weight) for c1, _ in eng.dec]  # deepest decoder first
    assert eng._subpixel_layers((1, 36, 40)) == {w[0]: (16, 32), w[1]: (8, 16)}
    assert eng._subpixel_layers((1, 34, 40)) == {w[1]: (8, 16)}  # 8 -> 17 is n -> 2n + 1, 17 -> 34 exact
    assert eng._subpixel_layers((1, 35, 29)) == {}
    assert not eng._subpixel_layers((1, 34, 40)).plus
    plain = M.get_model(dict(cfg, native_2d=True))._get_engine()
    assert not plain.subpixel2d and plain._subpixel_layers((1, 36, 40)) == {}
    odd = M.get_model(dict(cfg, f_maps=[6, 10, 14], layer_order="cr", native_2d_subpixel=True))._get_engine()
    assert odd._subpixel_layers((1, 36, 40)) == {}  # channel counts off the multiple of 4
    e3 = M.UNet3D(1, 1, f_maps=[8, 16], num_groups=4)._get_engine()  # the 3-D path keeps its 8 children
    assert e3.children == 8.0 and not e3.subpixel2d
