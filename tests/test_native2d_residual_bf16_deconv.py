"""CPU side of the opt-in bf16 ConvTranspose2d of ResidualUNet2D (`native_2d_residual_bf16_deconv: true` /
U3D_NATIVE_2D_RESIDUAL_BF16_DECONV=1): the switch, what it implies, refuses and leaves unchanged, the host-only queries of the new entry
points, and the float64 emulation the GPU tests compare against (tests/bf16_emul_res2d_deconv.py) held against the executor's own rule."""
import pytest
import torch

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
KEY = "native_2d_residual_bf16_deconv"


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def _lib():
    from pytorch3dunet_amd import _native as nat

    return nat.get_lib()


def test_the_key_implies_the_residual_bf16_mode():
    M = _m()
    assert not M.ResidualUNet2D(**_SMALL).native_supported  # default unchanged
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16_deconv=True)
    assert m.native_supported and m.native_2d and m.compute_bf16 and m.native_2d_residual_bf16 and m.native_2d_residual_bf16_deconv, \
        m._native_blockers
    assert not m.compute_split and m.native_2d_bf16 is False
    # the keys it implies, spelled out next to it, are accepted
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16_deconv=True, native_2d_residual_bf16=True, compute_dtype="bf16",
                         native_2d_residual=True, native_2d=True)
    assert m.native_supported and m.native_2d_residual_bf16_deconv
    m = M.get_model(dict(name="ResidualUNet2D", in_channels=1, out_channels=1, native_2d_residual_bf16_deconv=True))
    assert m.native_supported and m.compute_bf16 and m.native_2d_residual_bf16_deconv, m._native_blockers
    # native_2d_residual_bf16 alone does not switch it on
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True)
    assert m.native_supported and m.native_2d_residual_bf16 and m.native_2d_residual_bf16_deconv is False
    assert M.ResidualUNet2D(**_SMALL, native_2d_residual=True).native_2d_residual_bf16_deconv is False
    # (an explicit false of the implied key does not veto the key that implies it)
    assert M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16_deconv=True, native_2d_residual_bf16=False).native_2d_residual_bf16


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_RESIDUAL_BF16_DECONV", "1")
    m = M.ResidualUNet2D(**_SMALL)
    assert m.native_supported and m.native_2d_residual_bf16_deconv and m.native_2d_residual_bf16 and m.compute_bf16
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16_deconv=False)  # the key wins
    assert not m.native_supported and not m.native_2d_residual_bf16_deconv and not m.compute_bf16
    with pytest.raises(ValueError, match=KEY):
        M.ResidualUNet2D(**_SMALL, compute_dtype="fp32")
    for other in (M.UNet2D, M.UNet3D, M.ResidualUNet3D):  # other classes ignore the variable too
        o = other(**_SMALL)
        assert not o.compute_bf16 and not o.native_2d and o.native_2d_residual_bf16_deconv is False
    monkeypatch.setenv("U3D_NATIVE_2D_RESIDUAL_BF16_DECONV", "0")
    assert not M.ResidualUNet2D(**_SMALL).native_supported
    assert M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16_deconv=True).native_2d_residual_bf16_deconv


@pytest.mark.parametrize("dtype", ["fp32", "float32", "fp32_split"])
def test_contradicting_compute_dtype_raises_naming_the_key(dtype):
    M = _m()
    with pytest.raises(ValueError, match=KEY):
        M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16_deconv=True, compute_dtype=dtype)
    M.ResidualUNet2D(**_SMALL, compute_dtype=dtype)  # without the key: constructed as before


@pytest.mark.parametrize("kw", [dict(hip_graph=True), dict(checkpoint_encoders=True), dict(checkpoint_encoders=True, checkpoint_levels=1)])
def test_graph_and_checkpointing_stay_refused(kw):
    M = _m()
    with pytest.raises(ValueError, match="hip_graph" if "hip_graph" in kw else "checkpoint"):
        M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16_deconv=True, **kw)


@pytest.mark.parametrize("name", ["UNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, **_SMALL)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_residual_bf16_deconv=True))
    assert b.native_2d_residual_bf16_deconv is False and b.native_2d_residual_bf16 is False
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d and a.compute_bf16 == b.compute_bf16
    assert a._native_blockers == b._native_blockers
    M.get_model(dict(kw, native_2d_residual_bf16_deconv=True, compute_dtype="fp32"))  # no contradiction next to an ignored key
    assert not b._get_engine().bf16_deconv


def test_kinds_of_the_typed_cache():
    from pytorch3dunet_amd._engine_weights import _KINDS, Kind

    for kind, mode in ((Kind.CONVTR2D_BF16_FWD, 0), (Kind.CONVTR2D_BF16_DGRAD, 1)):
        spec = _KINDS[kind]
        assert spec.entry == "u3d_pack_convtr2d_bf16" and spec.mode == mode and spec.transposed and spec.dtype == torch.bfloat16
        assert spec.size(_lib(), 64, 32, spec.mode) == 9 * 64 * 32


@pytest.mark.parametrize("f_maps,groups,n_convtr,n_bf16", [([32, 64, 128], 8, 2, 2), ([8, 16], 4, 1, 0), ([16, 32, 64], 8, 2, 1)])
def test_emulation_rounds_exactly_the_transposed_convolutions_the_executor_routes(f_maps, groups, n_convtr, n_bf16):
    import bf16_emul_res2d_deconv as E

    M = _m()
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=f_maps, num_groups=groups)
    model = M.get_model(dict(cfg, native_2d_residual_bf16_deconv=True))
    assert len(E.convtr(model)) == n_convtr == len(f_maps) - 1
    mine = {id(c.weight) for c in E.eligible_convtr(model)}
    assert len(mine) == n_bf16
    eng = model._get_engine()  # (building the executor does not touch the GPU)
    assert eng.bf16_deconv and eng.is2d and eng.bf16
    for ct, _ in eng.dec:
        Cin, Cout = ct.weight.shape[:2]
        assert eng._bf16_convtr2d(Cin, Cout) == (id(ct.weight) in mine)
        assert (_lib().u3d_convtr2d_bf16_supported(Cin, Cout) == 1) == (id(ct.weight) in mine)  # the rule IS the kernels' envelope
    # without the key the rule never fires, whatever the channels
    off = M.get_model(dict(cfg, native_2d_residual_bf16=True))._get_engine()
    assert not off.bf16_deconv and not any(off._bf16_convtr2d(*ct.weight.shape[:2]) for ct, _ in off.dec)


def test_envelope_and_packed_sizes_through_the_host_only_calls():
    lib = _lib()
    for ci, co, ok in ((32, 32, 1), (1024, 512, 1), (96, 64, 1), (16, 32, 0), (32, 48, 0), (0, 32, 0), (32, -32, 0)):
        assert lib.u3d_convtr2d_bf16_supported(ci, co) == ok, (ci, co)
        for mode in (0, 1):
            assert lib.u3d_packed_convtr2d_bf16_elems(ci, co, mode) == (9 * ci * co if ok else 0), (ci, co, mode)
    assert lib.u3d_packed_convtr2d_bf16_elems(32, 32, 2) == 0
    assert lib.u3d_packed_convtr2d_bf16_elems(32768, 32768, 0) == 0  # 9 * Cin * Cout past 2^31: the limit of u3d_convtr2d_*


def test_workspace_sizes_and_variants_through_the_host_only_calls():
    lib = _lib()
    one = 9 * 32 * 64
    n = lib.u3d_convtr2d_wgrad_bf16_workspace_floats(2, 17, 19, 32, 64)
    assert n >= one and n % one == 0  # whole splits of [Cin][Cout][9] floats, at least one
    v = lib.u3d_convtr2d_wgrad_bf16_variant(2, 17, 19, 32, 64, -1)
    tps, nsplit = v >> 16, v & 0xFFFF
    tiles = 2 * 3 * 2  # 8 x 16-pixel tiles of 17 x 19
    assert nsplit * one == n and 1 <= nsplit <= tiles and (tps - 1) * nsplit < tiles <= tps * nsplit
    assert lib.u3d_convtr2d_wgrad_bf16_variant(2, 17, 19, 32, 64, n) == v
    # a workspace of one split runs one split over every tile; a shorter one is refused
    assert lib.u3d_convtr2d_wgrad_bf16_variant(2, 17, 19, 32, 64, one) == (tiles << 16) | 1
    assert lib.u3d_convtr2d_wgrad_bf16_variant(2, 17, 19, 32, 64, one - 1) == -1
    # outside the envelope / the size limits: nothing
    assert lib.u3d_convtr2d_wgrad_bf16_workspace_floats(2, 17, 19, 32, 48) == 0
    assert lib.u3d_convtr2d_wgrad_bf16_workspace_floats(0, 17, 19, 32, 64) == 0
    assert lib.u3d_convtr2d_wgrad_bf16_workspace_floats(1, 40000, 40000, 32, 64) == 0
    assert lib.u3d_convtr2d_wgrad_bf16_variant(2, 17, 19, 48, 64, -1) == -1
    # the data gradient's plan is shape-only: 64 produced channels per block when they divide evenly
    assert lib.u3d_convtr2d_dgrad_bf16_variant(1, 4, 4, 64, 32) == 2
    assert lib.u3d_convtr2d_dgrad_bf16_variant(1, 4, 4, 96, 64) == 1
    assert lib.u3d_convtr2d_dgrad_bf16_variant(1, 4, 4, 32, 64) == 1
    assert lib.u3d_convtr2d_dgrad_bf16_variant(1, 4, 4, 40, 64) == -1


def test_entry_points_are_declared_and_bound():
    from pytorch3dunet_amd import _native as nat

    names = ("u3d_convtr2d_bf16_supported", "u3d_packed_convtr2d_bf16_elems", "u3d_pack_convtr2d_bf16", "u3d_convtr2d_fwd_bf16",
             "u3d_convtr2d_dgrad_bf16", "u3d_convtr2d_dgrad_bf16_variant", "u3d_convtr2d_wgrad_bf16_workspace_floats",
             "u3d_convtr2d_wgrad_bf16_variant", "u3d_convtr2d_wgrad_bf16")
    assert set(names) <= set(nat.EXPORTED_SYMBOLS)
    lib = nat.get_lib()
    assert len(lib.u3d_convtr2d_fwd_bf16.argtypes) == len(lib.u3d_convtr2d_fwd.argtypes)
    assert len(lib.u3d_convtr2d_dgrad_bf16.argtypes) == len(lib.u3d_convtr2d_dgrad.argtypes)
    assert len(lib.u3d_convtr2d_wgrad_bf16.argtypes) == len(lib.u3d_convtr2d_wgrad.argtypes)


def test_emulation_with_the_rounding_switched_off_is_the_plain_float64_tree():
    import bf16_emul_res2d_deconv as E

    M = _m()
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="gcr", num_groups=8)
    torch.manual_seed(5)
    sd = M.get_model(dict(cfg, native_2d_residual_bf16_deconv=True)).state_dict()
    x, t = torch.randn(1, 1, 16, 20), (torch.rand(1, 1, 16, 20) > 0.5).float()
    plain = E.run(cfg, sd, x, t, "bce_dice", emulate=False)
    off = E.run(cfg, sd, x, t, "bce_dice", emulate=True, round_ops=False)  # through the emulating function, exact operands
    assert torch.equal(off[0], plain[0]) and off[1] == plain[1] and all(torch.equal(off[2][k], plain[2][k]) for k in plain[2])
    # with the rounding on it differs from the plain tree AND from the emulation that keeps ConvTranspose2d exact
    import bf16_emul_res2d as E3

    on = E.run(cfg, sd, x, t, "bce_dice", emulate=True)
    conv_only = E3.run(cfg, sd, x, t, "bce_dice", emulate=True)
    assert not torch.equal(on[0], plain[0]) and not torch.equal(on[0], conv_only[0])
    assert (on[0] - plain[0]).abs().max() < 0.05 * plain[0].abs().max()
    # a net without an eligible transposed convolution: the new emulation is the old one
    cfg8 = dict(cfg, f_maps=[8, 16], num_groups=4)
    torch.manual_seed(5)
    sd8 = M.get_model(dict(cfg8)).state_dict()
    a, b = E.run(cfg8, sd8, x, t, "bce_dice", emulate=True), E3.run(cfg8, sd8, x, t, "bce_dice", emulate=True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[2][k], b[2][k]) for k in b[2])
