"""`ConvLayers._bwd_families` and `_family_ws_floats` — backward's kernel families and its scratch, read off the family forward recorded
(`ConvRec.family`) — against a frozen copy of the ladders backward walked before the record held the decision: `_conv_bwd`'s `bf16`
expression, `_bwd_family_2d`, `_wgrad_family`, `_dgrad_family` and `_layer_ws_floats`, which each derived it again from shapes and engine
flags.  Host logic only, on engines built without a GPU; the scratch queries are the library's own."""
import itertools
import types

import pytest
import torch

from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd._engine_base import ConvRec, VSrc, slab_boxes
from pytorch3dunet_amd._engine_conv import ConvLayers, _ConvCall, _SubLayers

CHANNELS = (1, 4, 8, 16, 32, 48, 64)
ENGINES = {  # name: (class, model keys)
    "unet3d": ("UNet3D", dict()),
    "unet3d_bf16": ("UNet3D", dict(compute_dtype="bf16")),
    "unet3d_f32s": ("UNet3D", dict(compute_dtype="fp32_split")),
    "unet2d": ("UNet2D", dict(native_2d=True)),
    "unet2d_subpixel": ("UNet2D", dict(native_2d_subpixel=True)),
    "unet2d_subpixel_plus": ("UNet2D", dict(native_2d_subpixel_plus=True)),
    "unet2d_stem": ("UNet2D", dict(native_2d_stem=True)),
    "unet2d_bf16": ("UNet2D", dict(native_2d_bf16=True)),
    "unet2d_bf16_stem": ("UNet2D", dict(native_2d_bf16=True, native_2d_stem=True)),
    "unet2d_bf16_vcat": ("UNet2D", dict(native_2d_bf16_vcat=True)),
    "unet2d_bf16_vcat_stem": ("UNet2D", dict(native_2d_bf16_vcat=True, native_2d_stem=True)),
    "unet2d_bf16_subpixel": ("UNet2D", dict(native_2d_bf16_subpixel=True)),
    "unet2d_bf16_subpixel_vcat": ("UNet2D", dict(native_2d_bf16_subpixel=True, native_2d_bf16_vcat=True)),
    "resunet2d": ("ResidualUNet2D", dict(native_2d_residual=True)),
    "resunet2d_bf16": ("ResidualUNet2D", dict(native_2d_residual_bf16=True)),
}
SIDE = {"off": (0, None), "on": (1 << 30, None), "debug": (1 << 30, {})}  # (`_BwdCtx.SIDE_MAX_VOXELS`, `engine.debug`)


# ---- the parent's ladders, conditions as they stood ---------------------------------------------------------------------------------------
def _frozen_bf16(eng, src, Cout, sub, small):
    return sub is None and not small and eng._bf16_routed(src, Cout)  # (`_conv_bwd`: "the forward's decision")


def _frozen_bwd_family_2d(eng, sub, bf16):
    if sub is not None:  # (the parent's `_*_subpixel2d` launchers began with `if self.subpixel2d_bf16: return self._*_subpixel2d_bf16(c)`)
        return "subpixel2d_bf16" if eng.subpixel2d_bf16 else "subpixel2d"
    return "conv2d_bf16" if bf16 else "conv2d"


def _frozen_wgrad_family(eng, src, Cout, sub, bf16, side_max_voxels):
    if eng.is2d:
        return _frozen_bwd_family_2d(eng, sub, bf16)
    if bf16 and Cout % 32 == 0:
        return "bf16"
    if sub is not None:
        return "subpixel"
    if eng.overlap_small_wgrad and src.N * src.D * src.H * src.W <= side_max_voxels and eng.debug is None:
        return "fp32_side"
    return "fp32"


def _frozen_dgrad_family(eng, src, Cout, sub, small, bf16):
    if eng.is2d:
        return _frozen_bwd_family_2d(eng, sub, bf16)
    if sub is not None:
        return "subpixel"
    if src.t1 is None and not small and eng._split_dgrad(src.C, Cout):
        return "f32s"
    return "bf16" if bf16 else "fp32"


def _frozen_families(eng, src, Cout, sub, small, need_dg, side_max_voxels):
    if small and not need_dg:
        return None, None  # (`_conv_bwd`'s one-pass branch, taken before either ladder)
    bf16 = _frozen_bf16(eng, src, Cout, sub, small)
    return _frozen_dgrad_family(eng, src, Cout, sub, small, bf16), _frozen_wgrad_family(eng, src, Cout, sub, bf16, side_max_voxels)


def _frozen_layer_ws_floats(eng, N, D, H, W, Cin, Cout, sub, small, virtual):
    lib = nat.get_lib()
    if eng.is2d:
        if sub is not None and eng.subpixel2d_bf16:  # (`_family_ws_floats`: `family == "subpixel2d" and self.subpixel2d_bf16`)
            return max(lib.u3d_wgrad2d_bf16_workspace_floats(N, H, W, sub[0], Cout),
                       lib.u3d_subpixel2d_wgrad_bf16_workspace_floats(N, H // 2, W // 2, sub[1], Cout),
                       lib.u3d_conv2d_bf16_workspace_floats(N, H, W, Cout, sub[0]))
        if sub is not None:
            boxes = slab_boxes((1, H, W), (0, H % 2, W % 2), 2)
            return max(lib.u3d_wgrad2d_workspace_floats(N, H, W, sub[0], Cout),
                       lib.u3d_subpixel2d_wgrad_workspace_floats(N, H // 2, W // 2, sub[1], Cout),
                       lib.u3d_conv2d_workspace_floats(N, H, W, Cout, sub[0]),
                       *(lib.u3d_wgrad2d_workspace_floats(N, b[4] - b[1], b[5] - b[2], sub[1], Cout) for b in boxes))
        if not small and eng._bf16_routed_weight(Cin, Cout, virtual):
            sfx = "_c16" if eng._c16(Cin, Cout) else ""
            return max(getattr(lib, f"u3d_wgrad2d_bf16{sfx}_workspace_floats")(N, H, W, Cin, Cout),
                       getattr(lib, f"u3d_conv2d_bf16{sfx}_workspace_floats")(N, H, W, Cout, Cin))
        need = max(lib.u3d_wgrad2d_workspace_floats(N, H, W, Cin, Cout), lib.u3d_conv2d_workspace_floats(N, H, W, Cout, Cin))
        return max(need, lib.u3d_small_cin2d_bwd_workspace_floats(N, H, W, Cin, Cout)) if small else need
    if small:
        return lib.u3d_small_cin_bwd_workspace_floats(N, D, H, W, Cin, Cout)
    if sub is not None:
        boxes = slab_boxes((D, H, W), (D % 2, H % 2, W % 2), 2)
        return max([lib.u3d_wgrad_workspace_floats(N, D, H, W, sub[0], Cout),
                    lib.u3d_subpixel_wgrad_workspace_floats(N, D // 2, H // 2, W // 2, sub[1], Cout),
                    lib.u3d_conv3d_workspace_floats(N, D, H, W, Cout, sub[0])] +
                   [lib.u3d_wgrad_workspace_floats(N, b[3] - b[0], b[4] - b[1], b[5] - b[2], sub[1], Cout) for b in boxes])
    if not virtual and eng._bf16_layer(Cin, Cout):
        return max(lib.u3d_conv3d_bf16_workspace_floats(N, D, H, W, Cout, Cin), lib.u3d_wgrad_bf16_workspace_floats(N, D, H, W, Cin, Cout))
    return max(lib.u3d_wgrad_workspace_floats(N, D, H, W, Cin, Cout), lib.u3d_conv3d_workspace_floats(N, D, H, W, Cout, Cin))


# ---- the grid -----------------------------------------------------------------------------------------------------------------------------
_SRC = {}


def _source(is2d, C, virtual, plus):
    """a single source of C channels, or cat(skip of C channels, low-res of C channels) at an exact-2x / an n -> 2n + 1 level"""
    key = (is2d, C, virtual, plus)
    if key not in _SRC:
        full, low = ((1, 7 if plus else 6, 8), (1, 3, 4)) if is2d else ((5 if plus else 4, 6, 4), (2, 3, 2))
        _SRC[key] = VSrc(torch.zeros(2, *full, C), torch.zeros(2, *low, C) if virtual else None)
    return _SRC[key]


def _layers(eng):
    """(src, Cout, sub) of every layer of the grid this engine could meet: single and virtual sources, the latter with and without a
    sub-pixel entry where `_subpixel_layers` could make one (channel counts % 4; an n -> 2n + 1 level only where the engine takes them;
    under `native_2d_bf16_subpixel` what `_bf16_subpixel` accepts: the exact-2x source with all channel counts % 32)"""
    takes_plus = eng.subpixel2d_plus if eng.is2d else eng.subpixel_plus
    for C, Cout in itertools.product(CHANNELS, repeat=2):
        yield _source(eng.is2d, C, False, False), Cout, None
        for plus in (False, True):
            src = _source(eng.is2d, C, True, plus)
            yield src, Cout, None
            if eng.subpixel and C % 4 == 0 and Cout % 4 == 0 and (takes_plus or not plus):
                yield src, Cout, (C, C)
            if eng.subpixel2d_bf16 and C % 32 == 0 and Cout % 32 == 0 and not plus:
                yield src, Cout, (C, C)


def _record(eng, src, Cout, pair):
    """the routing part of the record, as `_single_conv_fwd` fills it"""
    conv = types.SimpleNamespace(weight=object())
    sub = _SubLayers({id(conv.weight): pair} if pair is not None else {})  # (the family: as `_subpixel_layers` names it)
    sub.family = "subpixel2d_bf16" if eng.subpixel2d_bf16 else ("subpixel2d" if eng.is2d else "subpixel")
    call = _ConvCall(dev=None, conv=conv, src=src, affine=None, y=None, N=src.N, D=src.D, H=src.H, W=src.W, Ctot=src.C, Cout=Cout, relu=0,
                     stats=False, pool=None, residual=None, sub=sub, b16=False)
    family = eng._fwd_family(call, None)
    assert (family in ("subpixel", "subpixel2d", "subpixel2d_bf16")) == (pair is not None)
    return ConvRec(name="layer", src=src, affine=None, mean_rstd=None, y=torch.empty(0, Cout), gn_w=None, conv_w=None, G=1, family=family,
                   sub=pair, plus=eng._src_plus(src) if pair is not None else (0, 0, 0),
                   c16=family == "conv2d_bf16" and eng._c16(src.C, Cout))


@pytest.fixture(scope="module")
def engines():
    from pytorch3dunet_amd.unet3d.model import get_model

    out = {}
    for name, (cls, keys) in ENGINES.items():
        model = get_model(dict(name=cls, in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8, **keys))
        assert model.native_supported, (name, model._native_blockers)
        out[name] = model._get_engine()
    return out


def test_backward_families_are_the_old_ladders(engines):
    seen_fwd, seen_dgrad, seen_wgrad = set(), set(), set()
    for name, eng in engines.items():
        for src, Cout, pair in _layers(eng):
            rec = _record(eng, src, Cout, pair)
            seen_fwd.add(rec.family)
            assert rec.small == (rec.family in ("small", "small2d"))
            for need_dg, (side, (voxels, debug)) in itertools.product((True, False), SIDE.items()):
                eng.debug = debug
                try:
                    got = eng._bwd_families(types.SimpleNamespace(SIDE_MAX_VOXELS=voxels), rec, need_dg)
                    want = _frozen_families(eng, src, Cout, pair, rec.small, need_dg, voxels)
                finally:
                    eng.debug = None
                assert got == want, (name, src.C0, src.C1, Cout, pair, rec.family, need_dg, side)
                seen_dgrad.add(got[0])
                seen_wgrad.add(got[1])
    # every family of the three tables is met at least once (None: the small families' one-pass backward)
    assert seen_fwd == set(ConvLayers._FWD_KERNELS)
    assert seen_dgrad == set(ConvLayers._DGRAD_KERNELS) | {None}
    assert seen_wgrad == set(ConvLayers._WGRAD_KERNELS) | {None}


def test_scratch_sized_from_the_record_is_the_old_by_shape_answer(engines):
    sizes = set()
    for name, eng in engines.items():
        for src, Cout, pair in _layers(eng):
            rec = _record(eng, src, Cout, pair)
            virtual = src.t1 is not None and not eng._bf16_vcat(src, Cout)  # (what `_wgrad_workspace_floats` passed down)
            want = _frozen_layer_ws_floats(eng, src.N, src.D, src.H, src.W, src.C, Cout, pair, rec.small, virtual)
            assert eng._wgrad_workspace_floats([rec]) == want, (name, src.C0, src.C1, Cout, pair, rec.family)
            if src.t1 is None:  # the by-shape form (a layer no forward has recorded yet) gives the record's answer
                assert eng._layer_ws_floats(src.N, src.D, src.H, src.W, src.C, Cout, small=rec.small) == want, (name, src.C, Cout)
            sizes.add((rec.family, want > 0))
    assert {f for f, nonzero in sizes if nonzero} == set(ConvLayers._FWD_KERNELS)  # (no family's comparison is 0 == 0 throughout)
    assert engines["unet3d"]._wgrad_workspace_floats([]) == 0


def test_subpixel_table_names_the_family_of_its_layers(engines):
    seen = {}
    for name, eng in engines.items():
        sub = eng._subpixel_layers((1, 8, 8) if eng.is2d else (8, 8, 8))  # (f_maps 32, 64: one decoder, 32 + 64 -> 32 at exact 2x)
        assert len(sub) <= 1 and (not sub or sub.family in ConvLayers._FWD_KERNELS)
        if sub:
            seen[name] = sub.family
    assert seen == dict(unet3d="subpixel", unet3d_f32s="subpixel", unet2d_subpixel="subpixel2d", unet2d_subpixel_plus="subpixel2d",
                        unet2d_bf16_subpixel="subpixel2d_bf16", unet2d_bf16_subpixel_vcat="subpixel2d_bf16")


def test_tables_name_launchers_of_the_mixin():
    for table in (ConvLayers._FWD_KERNELS, ConvLayers._DGRAD_KERNELS, ConvLayers._WGRAD_KERNELS):
        assert all(callable(getattr(ConvLayers, fn)) for fn in table.values())
    for family in ConvLayers._FWD_KERNELS:  # a forward family's gradients: a row of both gradient tables
        bwd = ConvLayers._BWD_FAMILY.get(family, family)
        assert bwd in ConvLayers._DGRAD_KERNELS and bwd in ConvLayers._WGRAD_KERNELS, family
    assert set(ConvLayers._BWD_FAMILY) <= set(ConvLayers._FWD_KERNELS)
