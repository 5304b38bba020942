"""CPU side of the opt-in sub-pixel bf16 decoder path of a UNet2D (`native_2d_bf16_subpixel: true` / U3D_NATIVE_2D_BF16_SUBPIXEL=1): the
key — what it implies, forces, refuses and leaves unchanged —, the executor's one eligibility rule (`_bf16_subpixel`, through
`_subpixel_layers` of an engine built on the CPU) held against its restatement in tests/bf16_emul_2d_subpixel.py, the declarations of the
new entry points, and the emulation itself: exact without rounding, inside the stated bf16 bars with it."""
import os
import re

import pytest
import torch

import bf16_emul_2d_subpixel as SE

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
ENTRY_POINTS = ("u3d_subpixel2d_bf16_packed_elems", "u3d_pack_subpixel2d_weights_bf16", "u3d_subpixel2d_conv_fwd_bf16",
                "u3d_subpixel2d_conv_dgrad_bf16", "u3d_subpixel2d_wgrad_bf16_workspace_floats", "u3d_subpixel2d_conv_wgrad_bf16",
                "u3d_pack_weights2d_bf16_slice", "u3d_conv2d_wgrad_bf16_strided")


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
def test_the_key_implies_native_2d_bf16_and_forces_bf16():
    M = _m()
    assert not M.UNet2D(**_SMALL).native_supported  # default unchanged
    m = M.UNet2D(**_SMALL, native_2d_bf16_subpixel=True)
    assert m.native_supported and m.native_2d and m.native_2d_bf16 and m.native_2d_bf16_subpixel and m.compute_bf16, m._native_blockers
    assert not m.native_2d_stem and not m.native_2d_bf16_vcat and not m.native_2d_subpixel
    e = m._get_engine()
    assert e.subpixel2d_bf16 and e.bf16 and not e.subpixel2d and not e.subpixel and not e.vcat
    m = M.UNet2D(**_SMALL, native_2d_bf16_subpixel=True, compute_dtype="bf16")
    assert m.native_supported and m.native_2d_bf16_subpixel
    # it composes with the virtual concat and the stem
    m = M.UNet2D(**_SMALL, native_2d_bf16_subpixel=True, native_2d_bf16_vcat=True, native_2d_stem=True)
    e = m._get_engine()
    assert m.native_supported and e.subpixel2d_bf16 and e.vcat and e.stem
    # without the key nothing changes
    for extra in (dict(native_2d=True), dict(native_2d_bf16=True), dict(native_2d_bf16_vcat=True), dict(native_2d_subpixel=True)):
        m = M.UNet2D(**_SMALL, **extra)
        assert m.native_supported and m.native_2d_bf16_subpixel is False and not m._get_engine().subpixel2d_bf16


@pytest.mark.parametrize("dtype", ["fp32", "float32", "fp32_split"])
def test_a_contradicting_compute_dtype_names_the_key(dtype):
    M = _m()
    with pytest.raises(ValueError, match="native_2d_bf16_subpixel runs bf16"):
        M.UNet2D(**_SMALL, native_2d_bf16_subpixel=True, compute_dtype=dtype)
    with pytest.raises(ValueError, match="native_2d_bf16 runs"):  # the parent key alone keeps its own message
        M.UNet2D(**_SMALL, native_2d_bf16=True, compute_dtype=dtype)


@pytest.mark.parametrize("other", ["native_2d_subpixel", "native_2d_subpixel_plus"])
def test_the_refusal_of_the_fp32_sub_pixel_path_is_inherited(other):
    M = _m()
    with pytest.raises(ValueError, match=f"{other} is the fp32 sub-pixel decoder path; native_2d_bf16_subpixel contradicts it"):
        M.UNet2D(**_SMALL, native_2d_bf16_subpixel=True, **{other: True})


@pytest.mark.parametrize("name", ["ResidualUNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    cls = getattr(M, name)
    a, b = cls(**_SMALL), cls(**_SMALL, native_2d_bf16_subpixel=True, compute_dtype=None)
    assert b.native_2d_bf16_subpixel is False and b.native_2d_bf16 is False
    assert (a.native_supported, a.compute_bf16, list(a._native_blockers)) == (b.native_supported, b.compute_bf16, list(b._native_blockers))
    cls(**_SMALL, native_2d_bf16_subpixel=True, compute_dtype="fp32")  # (no contradiction where the key means nothing)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_BF16_SUBPIXEL", "1")
    m = M.UNet2D(**_SMALL)
    assert m.native_supported and m.native_2d and m.native_2d_bf16 and m.native_2d_bf16_subpixel and m.compute_bf16
    m = M.UNet2D(**_SMALL, native_2d_bf16_subpixel=False)  # the key wins
    assert not m.native_supported and not m.native_2d_bf16_subpixel and not m.native_2d_bf16


def test_the_key_is_a_row_of_the_table_and_of_the_docstring():
    from pytorch3dunet_amd.unet3d import native2d

    M = _m()
    names = [k.name for k in native2d.KEYS]
    assert names.index("native_2d_bf16_subpixel") == names.index("native_2d_bf16") - 1  # (a key stands before the key it implies)
    row = native2d.KEYS[names.index("native_2d_bf16_subpixel")]
    assert (row.env, row.implies, row.precision, row.refuses) == ("U3D_NATIVE_2D_BF16_SUBPIXEL", "native_2d_bf16", "bf16", None)
    assert "native_2d_bf16_subpixel" in native2d.TABLE and "U3D_NATIVE_2D_BF16_SUBPIXEL" in native2d.TABLE
    assert "native_2d_bf16_subpixel" in M.__doc__ and "native_2d_bf16_subpixel" in M._OPT_IN_KEYS


def test_entry_points_are_declared_in_the_header_and_bound():
    from pytorch3dunet_amd import _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "u3d.h")).read()
    lib = nat.get_lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in nat._PROTOS and hasattr(lib, name), name
    # host-only queries: the envelope
    assert lib.u3d_subpixel2d_bf16_packed_elems(64, 32, 0) == 16 * 64 * 32 == lib.u3d_subpixel2d_bf16_packed_elems(64, 32, 1)
    assert lib.u3d_subpixel2d_bf16_packed_elems(16, 32, 0) == 0 and lib.u3d_subpixel2d_bf16_packed_elems(32, 48, 0) == 0
    assert lib.u3d_subpixel2d_bf16_packed_elems(32, 32, 2) == 0


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f_maps", [[32, 64, 128], [16, 32, 64]])
@pytest.mark.parametrize("hw", [(32, 40), (36, 42), (35, 45)])
@pytest.mark.parametrize("extra", [{}, dict(native_2d_bf16_vcat=True, native_2d_stem=True)])
def test_the_restated_rule_is_the_engines(f_maps, hw, extra):
    M = _m()
    m = M.UNet2D(in_channels=1, out_channels=1, f_maps=f_maps, num_groups=8, native_2d_bf16_subpixel=True, **extra)
    got = dict(m._get_engine()._subpixel_layers((1,) + hw))
    want = {id(conv.weight): pair for conv, pair in SE.eligible_subpixel(m, (2, 1) + hw).items()}
    assert got == want
    expect = {(32, 40): 2, (36, 42): 1, (35, 45): 0} if f_maps[0] == 32 else {(32, 40): 1, (36, 42): 0, (35, 45): 0}
    assert len(got) == expect[hw]
    # a post-norm order has no eligible level, and without the key the bf16 modes list none
    post = M.UNet2D(in_channels=1, out_channels=1, f_maps=f_maps, num_groups=8, layer_order="cgr", native_2d_bf16_subpixel=True, **extra)
    assert len(post._get_engine()._subpixel_layers((1,) + hw)) == 0 and not SE.eligible_subpixel(post, (2, 1) + hw)
    off = M.UNet2D(in_channels=1, out_channels=1, f_maps=f_maps, num_groups=8, native_2d_bf16=True, **extra)
    assert len(off._get_engine()._subpixel_layers((1,) + hw)) == 0


# ---- the emulation -------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _runs(i):
    """(plain, emulation without rounding, emulation) of model case i, computed once and shared"""
    if i not in _RUNS:
        cfg, shape, _ = SE.MODEL_CASES[i]
        _, sd, x, target = SE.prep(cfg, shape)
        ln = SE.loss_name_of(cfg)
        _RUNS[i] = (SE.run(cfg, sd, x, target, ln, emulate=False), SE.run(cfg, sd, x, target, ln, emulate=True, rnd=SE.identity),
                    SE.run(cfg, sd, x, target, ln, emulate=True))
    return _RUNS[i]


_DISTINCT = [i for i, (_, _, extra) in enumerate(SE.MODEL_CASES) if not extra]  # (the vcat twin has the same emulation)


@pytest.mark.parametrize("i", _DISTINCT)
def test_without_rounding_the_emulation_is_the_plain_float64_run(i):
    cfg, shape, _ = SE.MODEL_CASES[i]
    model, _, _, _ = SE.prep(cfg, shape)
    assert SE.eligible_subpixel(model, shape), "the case has no sub-pixel layer"
    plain, exact, _ = _runs(i)
    e_l, e_g = SE.distances(exact, plain)
    print(dict(test="bf16_subpixel_emulation_exact", case=i, logits=e_l, grad_l2=e_g))
    assert e_l < 1e-12 and e_g < 1e-12


@pytest.mark.parametrize("i", _DISTINCT)
def test_the_emulation_alone_is_inside_the_bf16_bars(i):
    plain, _, emul = _runs(i)
    e_l, e_g = SE.distances(emul, plain)
    print(dict(test="bf16_subpixel_emulation_vs_plain", case=i, logits=e_l, grad_l2=e_g))
    assert e_l < SE.BF16_LOGITS_TOL and e_g < SE.BF16_GRAD_TOL
