"""`ConvLayers._up_family` — the one rule that picks a decoder's transposed-convolution kernels — against a frozen copy of the ladder
`ResUNetEngine.forward` walked before the rule was stated once (and of the two-way choice `UNet3DEngine.forward` made for
upsample='deconv').  Host logic only: the library's one answer the rule depends on is stubbed with both of its values."""
import itertools
import types

import pytest

from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd._engine_conv import ConvLayers

CHANNELS = (6, 8, 16, 32, 48)


def _frozen_ladder(is2d, bf16, bf16_deconv, subpixel, concat, Cl, Ct, t8_supported):
    """the residual executor's forward ladder at the parent commit, conditions written out"""
    if (bf16 and not is2d and t8_supported == 1) and not concat:
        return "t8"
    if is2d and (bf16_deconv and Cl % 32 == 0 and Ct % 32 == 0):
        return "convtr2d_bf16"
    if is2d:
        return "convtr2d"
    if subpixel and Cl % 4 == 0 and Ct % 4 == 0:
        return "convtr3d_subpixel"
    return "convtr3d"


@pytest.mark.parametrize("t8_supported", [0, 1])
def test_up_family_is_the_forward_ladder(monkeypatch, t8_supported):
    monkeypatch.setattr(nat, "get_lib", lambda: types.SimpleNamespace(u3d_convtr3d_t8_supported=lambda Cl, Ct: t8_supported))
    seen = set()
    for is2d, bf16, bf16_deconv, subpixel, concat in itertools.product((False, True), repeat=5):
        eng = ConvLayers.__new__(ConvLayers)
        eng.is2d, eng.bf16, eng.bf16_deconv, eng.subpixel = is2d, bf16, bf16_deconv, subpixel
        for Cl, Ct in itertools.product(CHANNELS, repeat=2):
            want = _frozen_ladder(is2d, bf16, bf16_deconv, subpixel, concat, Cl, Ct, t8_supported)
            assert eng._up_family(Cl, Ct, concat) == want, (is2d, bf16, bf16_deconv, subpixel, concat, Cl, Ct)
            if concat and not is2d:  # what the DoubleConv executor asks (its concat is virtual): its old two-way choice
                assert want == ("convtr3d_subpixel" if subpixel and Cl % 4 == 0 and Ct % 4 == 0 else "convtr3d")
            seen.add(want)
    assert seen == set(ConvLayers._UP_KERNELS) - (set() if t8_supported else {"t8"})


def test_up_kernels_rows_name_launchers_of_the_mixin():
    for family, (fwd, bwd, s2d) in ConvLayers._UP_KERNELS.items():
        assert callable(getattr(ConvLayers, fwd)) and callable(getattr(ConvLayers, bwd)), family
        assert s2d == (family == "t8")
    # the sub-pixel forward differs from the generic one in the forward only
    assert ConvLayers._UP_KERNELS["convtr3d_subpixel"][1] == ConvLayers._UP_KERNELS["convtr3d"][1]
