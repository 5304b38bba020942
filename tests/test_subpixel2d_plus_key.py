"""CPU side of `native_2d_subpixel_plus: true` / U3D_NATIVE_2D_SUBPIXEL_PLUS=1: the model key (one row of unet3d/native2d.py, in front
of `native_2d_subpixel`, which it implies), the refusal it inherits, and which decoder levels the executor hands to the windowed
sub-pixel kernels + slab launches."""
import pytest

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
_CFG3 = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32], num_groups=4)


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def test_the_key_is_one_row_in_front_of_the_key_it_implies():
    from pytorch3dunet_amd.unet3d import native2d

    row = native2d._BY_NAME["native_2d_subpixel_plus"]
    assert row.env == "U3D_NATIVE_2D_SUBPIXEL_PLUS" and row.implies == "native_2d_subpixel"
    assert row.precision is None and row.refuses is None
    assert native2d.NAMES.index("native_2d_subpixel_plus") < native2d.NAMES.index("native_2d_subpixel")
    assert "native_2d_subpixel_plus" in native2d.TABLE and "native_2d_subpixel_plus" in _m().__doc__


def test_the_key_resolves_and_implies_the_sub_pixel_path():
    M = _m()
    cfg = dict(name="UNet2D", **_SMALL)
    m = M.get_model(dict(cfg, native_2d_subpixel_plus=True))
    assert m.native_supported and m.native_2d and m.keys_2d.native_2d_subpixel and m.keys_2d.native_2d_subpixel_plus, m._native_blockers
    assert not m.compute_bf16
    assert M.get_model(dict(cfg, native_2d_subpixel=True)).keys_2d.native_2d_subpixel_plus is False  # the implied key alone: unchanged
    m = M.get_model(dict(cfg, native_2d_subpixel_plus=True, native_2d_stem=True))  # allowed next to the stem
    assert m.native_supported and m.keys_2d.native_2d_subpixel_plus and m.keys_2d.native_2d_stem


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_SUBPIXEL_PLUS", "1")
    m = M.UNet2D(**_SMALL)
    assert m.native_supported and m.keys_2d.native_2d_subpixel and m.keys_2d.native_2d_subpixel_plus
    m = M.UNet2D(**_SMALL, native_2d_subpixel_plus=False)  # the key wins
    assert not m.native_supported and not m.keys_2d.native_2d_subpixel_plus
    assert M.UNet3D(**_SMALL).keys_2d.native_2d_subpixel_plus is False and not M.ResidualUNet2D(**_SMALL).native_supported


@pytest.mark.parametrize("other", ["native_2d_bf16", "native_2d_bf16_vcat"])
def test_bf16_next_to_the_key_is_a_contradiction_naming_the_most_derived_keys(other):
    M = _m()
    with pytest.raises(ValueError, match=f"native_2d_subpixel_plus is .*; {other} contradicts it"):
        M.get_model(dict(name="UNet2D", **_SMALL, native_2d_subpixel_plus=True, **{other: True}))
    with pytest.raises(ValueError, match="native_2d_subpixel is "):  # the implied key alone keeps its own text
        M.get_model(dict(name="UNet2D", **_SMALL, native_2d_subpixel=True, **{other: True}))


@pytest.mark.parametrize("name", ["ResidualUNet2D", "UNet3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, **_SMALL)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_subpixel_plus=True))
    assert b.keys_2d.native_2d_subpixel_plus is False and b.keys_2d.native_2d_subpixel is False
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d and a._native_blockers == b._native_blockers


def test_which_levels_take_the_windowed_path():
    M = _m()
    plus = M.get_model(dict(_CFG3, native_2d_subpixel_plus=True))._get_engine()
    old = M.get_model(dict(_CFG3, native_2d_subpixel=True))._get_engine()
    assert plus.is2d and plus.subpixel2d and plus.subpixel2d_plus and not old.subpixel2d_plus
    w = [id(c1.conv.weight) for c1, _ in plus.dec]  # deepest decoder first
    n_dec = len(plus.dec)
    assert len(plus._subpixel_layers((1, 35, 45))) == n_dec == 2 and len(old._subpixel_layers((1, 35, 45))) == 0
    sub = plus._subpixel_layers((1, 35, 29))  # 8 x 7 -> 17 x 14 shifts H only, 17 x 14 -> 35 x 29 both axes
    assert sub == {w[0]: (16, 32), w[1]: (8, 16)} and sub.plus == frozenset(w)
    sub = plus._subpixel_layers((1, 34, 40))  # 8 -> 17 is n -> 2n + 1, 17 -> 34 exact
    assert sub == {w[0]: (16, 32), w[1]: (8, 16)} and sub.plus == frozenset(w[:1])
    sub = plus._subpixel_layers((1, 36, 40))  # all exact: what the implied key alone takes
    assert sub == {w[0]: (16, 32), w[1]: (8, 16)} and not sub.plus
    assert sorted(old._subpixel_layers((1, 36, 40)).values()) == sorted(sub.values())
    odd = M.get_model(dict(_CFG3, f_maps=[6, 10, 14], layer_order="cr", native_2d_subpixel_plus=True))._get_engine()
    assert odd._subpixel_layers((1, 35, 29)) == {}  # channel counts off the multiple of 4
    e3 = M.UNet3D(1, 1, f_maps=[8, 16], num_groups=4, native_2d_subpixel_plus=True)._get_engine()
    assert e3.children == 8.0 and not e3.subpixel2d and not e3.subpixel2d_plus


def test_the_slab_boxes_of_a_2d_level():
    from pytorch3dunet_amd._engine_base import slab_boxes

    assert slab_boxes((1, 35, 29), (0, 1, 1), 2) == [(0, 0, 0, 1, 2, 29), (0, 2, 0, 1, 35, 2)]
    assert slab_boxes((1, 35, 29), (0, 1, 1), 3) == [(0, 0, 0, 1, 3, 29), (0, 3, 0, 1, 35, 3)]  # whole low-res cells: cell 0 owns [0, 3)
    assert slab_boxes((1, 3, 2), (0, 1, 0), 3) == [(0, 0, 0, 1, 3, 2)]
    assert slab_boxes((1, 34, 41), (0, 0, 1), 2) == [(0, 0, 0, 1, 34, 2)]
