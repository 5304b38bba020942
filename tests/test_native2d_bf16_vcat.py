"""CPU side of the opt-in virtual concat of a UNet2D in bf16 (`native_2d_bf16_vcat: true` / U3D_NATIVE_2D_BF16_VCAT=1): the switch, what
it implies, refuses and leaves unchanged; the executor's one routing rule (`_bf16_vcat`) on channel pairs inside and outside the envelope
of the `_src` entry points; and their declarations in _native.py held against include/u3d.h."""
import ctypes
import os
import re

import pytest
import torch

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
_FIT = dict(in_channels=1, out_channels=1, f_maps=[32, 64, 128], num_groups=8)
SRC_NAMES = ("u3d_conv2d_bf16_src", "u3d_conv2d_bf16_dgrad_src", "u3d_conv2d_wgrad_bf16_src")


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
def test_the_key_implies_native_2d_bf16():
    M = _m()
    assert not M.UNet2D(**_SMALL).native_supported  # default unchanged
    m = M.UNet2D(**_SMALL, native_2d_bf16_vcat=True)
    assert m.native_supported and m.native_2d and m.native_2d_bf16 and m.native_2d_bf16_vcat and m.compute_bf16, m._native_blockers
    assert not m.native_2d_stem
    m = M.UNet2D(**_SMALL, native_2d_bf16_vcat=True, compute_dtype="bf16")
    assert m.native_supported and m.native_2d_bf16_vcat
    # it composes with the stem key
    m = M.UNet2D(**_SMALL, native_2d_bf16_vcat=True, native_2d_stem=True)
    assert m.native_supported and m.native_2d_bf16_vcat and m.native_2d_stem and m.native_2d_bf16
    e = m._get_engine()
    assert e.vcat and e.stem and e.bf16
    # without the key nothing changes
    for extra in (dict(native_2d=True), dict(native_2d_bf16=True), dict(native_2d_bf16=True, native_2d_stem=True)):
        m = M.UNet2D(**_SMALL, **extra)
        assert m.native_supported and m.native_2d_bf16_vcat is False and not m._get_engine().vcat


@pytest.mark.parametrize("dtype", ["fp32", "float32", "fp32_split"])
def test_a_contradicting_compute_dtype_names_the_key(dtype):
    M = _m()
    with pytest.raises(ValueError, match="native_2d_bf16_vcat"):
        M.UNet2D(**_SMALL, native_2d_bf16_vcat=True, compute_dtype=dtype)
    with pytest.raises(ValueError, match="native_2d_bf16_vcat"):
        M.UNet2D(**_SMALL, native_2d_bf16_vcat=True, native_2d_bf16=True, compute_dtype=dtype)
    # the parent key alone keeps its own message
    with pytest.raises(ValueError, match="native_2d_bf16 runs"):
        M.UNet2D(**_SMALL, native_2d_bf16=True, compute_dtype=dtype)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_BF16_VCAT", "1")
    m = M.UNet2D(**_SMALL)
    assert m.native_supported and m.native_2d and m.native_2d_bf16 and m.native_2d_bf16_vcat and m.compute_bf16
    m = M.UNet2D(**_SMALL, native_2d_bf16_vcat=False)  # the key wins
    assert not m.native_supported and not m.native_2d_bf16_vcat and not m.native_2d_bf16
    m = M.UNet2D(**_SMALL, native_2d_bf16_vcat=False, native_2d_bf16=True)
    assert m.native_supported and m.native_2d_bf16 and not m.native_2d_bf16_vcat
    assert not M.ResidualUNet2D(**_SMALL).native_supported  # other classes ignore the variable too
    assert M.UNet3D(**_SMALL).native_2d_bf16_vcat is False
    monkeypatch.setenv("U3D_NATIVE_2D_BF16_VCAT", "0")
    assert not M.UNet2D(**_SMALL).native_supported
    assert M.UNet2D(**_SMALL, native_2d_bf16_vcat=True).native_supported


@pytest.mark.parametrize("name", ["ResidualUNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, **_SMALL)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_bf16_vcat=True))
    assert b.native_2d_bf16_vcat is False and b.native_2d_bf16 is False
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d and a.compute_bf16 == b.compute_bf16
    assert a._native_blockers == b._native_blockers
    # ... including an explicit fp32 next to it (no contradiction where the key means nothing)
    c = M.get_model(dict(kw, native_2d_bf16_vcat=True, compute_dtype="fp32"))
    assert c.native_supported == a.native_supported and not c.compute_bf16
    r = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True, native_2d_bf16_vcat=True)
    assert r.native_supported and r.native_2d_bf16_vcat is False and not r._get_engine().vcat


def test_state_dict_unchanged_by_the_key():
    M = _m()
    cfg = dict(name="UNet2D", in_channels=1, out_channels=2, f_maps=[32, 64], layer_order="bcr", final_sigmoid=False)
    torch.manual_seed(3)
    a = M.get_model(dict(cfg)).state_dict()
    torch.manual_seed(3)
    b = M.get_model(dict(cfg, native_2d_bf16_vcat=True)).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- the routing rule ------------------------------------------------------------------------------------------------------------------
def _vsrc(C0, C1, H=6, W=7, H1=3, W1=3, dtype=torch.float32):
    from pytorch3dunet_amd.engine import VSrc

    return VSrc(torch.zeros(1, 1, H, W, C0, dtype=dtype), torch.zeros(1, 1, H1, W1, C1, dtype=dtype) if C1 else None)


@pytest.mark.parametrize("C0,C1,Cout,ok", [
    (32, 64, 32, True), (64, 128, 64, True), (64, 32, 32, True), (32, 32, 96, True), (128, 256, 128, True),
    (16, 32, 16, False), (16, 48, 64, False), (32, 48, 32, False), (48, 80, 32, False), (32, 64, 16, False), (32, 64, 48, False),
    (8, 16, 8, False), (32, 0, 32, False),
])
def test_routing_rule_on_channel_pairs(C0, C1, Cout, ok):
    M = _m()
    eng = M.UNet2D(**_FIT, native_2d_bf16_vcat=True, native_2d_stem=True)._get_engine()
    src = _vsrc(C0, C1)
    assert eng._bf16_vcat(src, Cout) is ok
    if C1:
        assert eng._bf16_routed(src, Cout) is ok  # the forward's and the backward's family decision
    # without the key no virtual source is ever routed to the bf16 family
    for extra in (dict(native_2d_bf16=True), dict(native_2d_bf16=True, native_2d_stem=True), dict(native_2d=True)):
        e0 = M.UNet2D(**_FIT, **extra)._get_engine()
        assert not e0._bf16_vcat(src, Cout) and (not C1 or not e0._bf16_routed(src, Cout))


def test_routing_rule_needs_pre_norm_and_fp32_halves(monkeypatch):
    M = _m()
    assert M.UNet2D(**_FIT, native_2d_bf16_vcat=True)._get_engine()._bf16_vcat(_vsrc(32, 64), 32)
    post = M.UNet2D(**_FIT, native_2d_bf16_vcat=True, layer_order="cgr")._get_engine()
    assert post.vcat and not post._bf16_vcat(_vsrc(32, 64), 32)
    eng = M.UNet2D(**_FIT, native_2d_bf16_vcat=True, layer_order="bcr")._get_engine()
    assert eng._bf16_vcat(_vsrc(32, 64), 32)
    assert not eng._bf16_vcat(_vsrc(32, 64, dtype=torch.bfloat16), 32)
    monkeypatch.setenv("U3D_BF16_CAT", "0")  # (the parent mode's switch for the bf16 concat layers covers this route too)
    assert not eng._bf16_vcat(_vsrc(32, 64), 32)


def test_eligible_decoders_stay_bf16_layers():
    """the decoders' first convolutions keep their BF16 images (never fp32-virtual or sub-pixel layers), with or without the key; the
    shared scratch of such a layer is sized by the bf16 plans"""
    M = _m()
    cfg = dict(name="UNet2D", **_FIT)
    a = M.get_model(dict(cfg, native_2d_bf16=True))._get_engine()
    b = M.get_model(dict(cfg, native_2d_bf16_vcat=True))._get_engine()
    assert not a._virtual_w and not b._virtual_w
    assert [tuple(w.shape) for w in a.images._each_bf16] == [tuple(w.shape) for w in b.images._each_bf16]
    assert [tuple(w.shape) for w in a.images._each] == [tuple(w.shape) for w in b.images._each]
    assert len(b._subpixel_layers((1, 35, 45))) == 0
    for c1, _ in b.dec:
        assert b._cat_bf16(c1)


# ---- C-ABI: _native.py against include/u3d.h -------------------------------------------------------------------------------------------
def _ctype(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("u3d_stream_t"):
        return ctypes.c_void_p
    if decl.startswith("long long"):
        return ctypes.c_int64
    assert decl.startswith("int "), decl
    return ctypes.c_int


def test_new_symbols_match_the_header():
    from pytorch3dunet_amd import _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "u3d.h")).read()
    for name in SRC_NAMES:
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert m, f"{name} is not declared in include/u3d.h"
        args = [a for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
        res, argtypes = nat._PROTOS[name]
        assert res is ctypes.c_int and argtypes == [_ctype(a) for a in args], (name, args, argtypes)
        assert name in nat.EXPORTED_SYMBOLS
    assert sum("const u3d_src_t*" in re.search(r"^int " + n + r"\(([^;]*)\);", header, re.M).group(1) for n in SRC_NAMES) == 3
    lib = nat.get_lib()  # (binds every declared symbol: AttributeError if the library does not export one)
    assert all(hasattr(lib, n) for n in SRC_NAMES)
    # the plans of the new entry points are the old queries on (N, H, W, C0 + C1, Cout): nothing new to ask
    assert "A launch plan depends on (N, H, W, C0 + C1, Cout) only" in header
