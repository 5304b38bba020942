"""CPU side of the opt-in bf16 ResidualUNet2D path (`native_2d_residual_bf16: true` / U3D_NATIVE_2D_RESIDUAL_BF16=1): the switch, what it
implies, refuses and leaves unchanged, the new entry point's binding, and the float64 emulation the GPU tests compare against
(tests/bf16_emul_res2d.py) held against the executor's own routing."""
import pytest
import torch

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
KEY = "native_2d_residual_bf16"


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def test_the_key_opts_a_resunet2d_in():
    M = _m()
    assert not M.ResidualUNet2D(**_SMALL).native_supported  # default unchanged
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True)
    assert m.native_supported and m.native_2d and m.compute_bf16 and m.native_2d_residual_bf16 and not m.compute_split, m._native_blockers
    assert m.native_2d_bf16 is False  # (the UNet2D key's attribute stays what it was)
    # an explicit compute_dtype: bf16 next to it is accepted, and so are the keys it implies
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True, compute_dtype="bf16", native_2d_residual=True, native_2d=True)
    assert m.native_supported and m.compute_bf16
    m = M.get_model(dict(name="ResidualUNet2D", in_channels=1, out_channels=1, native_2d_residual_bf16=True))  # the reference defaults
    assert m.native_supported and m.compute_bf16, m._native_blockers
    # without the key nothing changes: fp32 native_2d_residual, and native_2d_residual + bf16 stays on the warning path
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual=True)
    assert m.native_supported and not m.compute_bf16 and m.native_2d_residual_bf16 is False
    assert not M.ResidualUNet2D(**_SMALL, native_2d_residual=True, compute_dtype="bf16").native_supported
    assert not M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=False, native_2d_residual=True, compute_dtype="bf16").native_supported
    # the UNet2D key keeps being ignored here
    r = M.ResidualUNet2D(**_SMALL, native_2d_residual=True, native_2d_bf16=True, compute_dtype="bf16")
    assert not r.native_supported and r.native_2d_bf16 is False


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_RESIDUAL_BF16", "1")
    m = M.ResidualUNet2D(**_SMALL)
    assert m.native_supported and m.native_2d_residual_bf16 and m.compute_bf16
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=False)  # the key wins
    assert not m.native_supported and not m.native_2d_residual_bf16 and not m.compute_bf16
    with pytest.raises(ValueError, match=KEY):
        M.ResidualUNet2D(**_SMALL, compute_dtype="fp32")
    for other in (M.UNet2D, M.UNet3D, M.ResidualUNet3D):  # other classes ignore the variable too
        o = other(**_SMALL)
        assert not o.compute_bf16 and not o.native_2d and o.native_2d_residual_bf16 is False
    assert not M.UNet2D(**_SMALL).native_supported
    monkeypatch.setenv("U3D_NATIVE_2D_RESIDUAL_BF16", "0")
    assert not M.ResidualUNet2D(**_SMALL).native_supported
    assert M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True).native_supported


@pytest.mark.parametrize("dtype", ["fp32", "float32", "fp32_split"])
def test_contradicting_compute_dtype_raises(dtype):
    M = _m()
    with pytest.raises(ValueError, match=KEY):
        M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True, compute_dtype=dtype)
    M.ResidualUNet2D(**_SMALL, compute_dtype=dtype)  # without the key: constructed as before


@pytest.mark.parametrize("kw", [dict(hip_graph=True), dict(checkpoint_encoders=True), dict(checkpoint_encoders=True, checkpoint_levels=1)])
def test_graph_and_checkpointing_stay_refused(kw):
    M = _m()
    with pytest.raises(ValueError, match="hip_graph" if "hip_graph" in kw else "checkpoint"):
        M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True, **kw)
    M.ResidualUNet2D(**_SMALL, **kw)  # without the key: constructed as before


@pytest.mark.parametrize("upsample,ok", [("default", True), ("deconv", True), ("nearest", False), ("bilinear", False)])
def test_upsample_rule_is_the_one_of_native_2d_residual(upsample, ok):
    M = _m()
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual_bf16=True, upsample=upsample)
    assert m.native_supported == ok, m._native_blockers
    assert M.ResidualUNet2D(**_SMALL, native_2d_residual=True, upsample=upsample).native_supported == ok


@pytest.mark.parametrize("order", ["gcr", "bcr", "cgr", "crg", "cr", "gcl", "gce", "cge", "bce", "cbr", "cl", "gcrd"])
def test_layer_orders_are_those_of_native_2d_residual(order):
    M = _m()
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order=order)
    fp32, bf16 = M.get_model(dict(cfg, native_2d_residual=True)), M.get_model(dict(cfg, native_2d_residual_bf16=True))
    assert bf16.native_supported == fp32.native_supported == (order != "gcrd"), (order, bf16._native_blockers)
    assert bf16._native_blockers == fp32._native_blockers
    assert bf16.compute_bf16 and not fp32.compute_bf16


@pytest.mark.parametrize("name", ["UNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, **_SMALL)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_residual_bf16=True))
    assert b.native_2d_residual_bf16 is False
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d and a.compute_bf16 == b.compute_bf16
    assert a.native_2d_bf16 == b.native_2d_bf16 and a.activation_bf16 == b.activation_bf16
    assert a._native_blockers == b._native_blockers
    # ... and an fp32 compute_dtype next to the ignored key is no contradiction there
    M.get_model(dict(kw, native_2d_residual_bf16=True, compute_dtype="fp32"))
    torch.manual_seed(3)
    sa = M.get_model(dict(kw)).state_dict()
    torch.manual_seed(3)
    sb = M.get_model(dict(kw, native_2d_residual_bf16=True)).state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_state_dict_unchanged_by_the_key():
    M = _m()
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=2, f_maps=[32, 64], layer_order="bcr", final_sigmoid=False)
    torch.manual_seed(3)
    a = M.get_model(dict(cfg)).state_dict()
    torch.manual_seed(3)
    b = M.get_model(dict(cfg, native_2d_residual_bf16=True)).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_the_residual_entry_point_is_declared_and_bound():
    from pytorch3dunet_amd import _native as nat

    assert "u3d_conv2d_bf16_res" in nat.EXPORTED_SYMBOLS
    fn = nat.get_lib().u3d_conv2d_bf16_res
    plain = nat.get_lib().u3d_conv2d_bf16
    assert len(fn.argtypes) == len(plain.argtypes) + 1  # the arguments of u3d_conv2d_bf16 plus the residual


# ---- the emulation helper of the GPU model tests ----------------------------------------------------------------------------------
# expected counts from the module tree: a ResNetBlock holds two 3x3 convolutions (conv2, conv3), a net of L levels L encoder and L - 1
# decoder blocks: 2 * (2L - 1) convolutions, each out_channels -> out_channels of its block
@pytest.mark.parametrize("cfg,n_3x3,n_bf16", [
    (dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="gcr", num_groups=8), 10, 10),
    (dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="cge", num_groups=8), 6, 6),
    (dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], upsample="deconv", num_groups=8), 6, 6),
    (dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[16, 32], layer_order="gcr", num_groups=8), 6, 2),  # the 32-wide block only
    (dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], layer_order="gcr", num_groups=4), 6, 0),
])
def test_emulation_rounds_exactly_the_layers_the_executor_routes_to_bf16(cfg, n_3x3, n_bf16):
    import bf16_emul_res2d as E

    M = _m()
    model = M.get_model(dict(cfg, native_2d_residual_bf16=True))
    assert len(E.conv3x3(model)) == n_3x3 == 2 * (2 * len(cfg["f_maps"]) - 1)
    mine = [id(c.weight) for c in E.eligible(model)]
    eng = model._get_engine()  # (building the executor does not touch the GPU)
    images = eng.images
    assert len(mine) == n_bf16
    assert sorted(mine) == sorted(id(w) for w in images._each_bf16)
    assert sorted(id(c.weight) for c in E.conv3x3(model) if id(c.weight) not in mine) == sorted(id(w) for w in images._each)
    # activations stay fp32 in HBM: the 2-D kernels have no bf16-storage forms
    assert model.activation_bf16 and not eng.act_bf16 and eng.adt == torch.float32
    # the forward / backward rule and the scratch sizing agree with the images on every layer (one real source each)
    from pytorch3dunet_amd._engine_base import VSrc

    for c in E.conv3x3(model):
        src = VSrc(torch.empty(1, 1, 4, 4, c.in_channels))
        assert eng._bf16_routed(src, c.out_channels) == (id(c.weight) in mine)


def test_explicit_bf16_activation_storage_warns_and_stays_fp32():
    M = _m()
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[64, 128], native_2d_residual_bf16=True)
    with pytest.warns(UserWarning, match="activations stay fp32"):
        eng = M.get_model(dict(cfg, activation_dtype="bf16"))._get_engine()
    assert not eng.act_bf16
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # 'auto': silently fp32
        assert not M.get_model(dict(cfg))._get_engine().act_bf16


def test_emulation_without_eligible_layers_is_the_plain_float64_run():
    import bf16_emul_res2d as E

    M = _m()
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], layer_order="gcr", num_groups=4)
    torch.manual_seed(5)
    sd = M.get_model(dict(cfg, native_2d_residual_bf16=True)).state_dict()
    x, t = torch.randn(1, 1, 16, 20), (torch.rand(1, 1, 16, 20) > 0.5).float()
    a = E.run(cfg, sd, x, t, "bce_dice", emulate=True)
    b = E.run(cfg, sd, x, t, "bce_dice", emulate=False)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and all(torch.equal(a[2][k], b[2][k]) for k in b[2])
    # ... and with eligible layers it is not
    cfg = dict(cfg, f_maps=[32, 64], num_groups=8)
    torch.manual_seed(5)
    sd = M.get_model(dict(cfg)).state_dict()
    a = E.run(cfg, sd, x, t, "bce_dice", emulate=True)
    b = E.run(cfg, sd, x, t, "bce_dice", emulate=False)
    assert not torch.equal(a[0], b[0]) and (a[0] - b[0]).abs().max() < 0.05 * b[0].abs().max()


def test_the_3d_space_to_depth_branch_stays_off_in_2d():
    """`compute_bf16` is now true on a 2-D residual engine: `_convtr_t8` (ConvTranspose3d as a 2x2x2 space-to-depth convolution on the
    3-D bf16 kernels) must not fire there — the decoders' ConvTranspose2d stays on u3d_convtr2d_* — and still fires for the 3-D net"""
    M = _m()
    cfg = dict(in_channels=1, out_channels=1, f_maps=[64, 128], num_groups=8)
    e2 = M.ResidualUNet2D(**cfg, native_2d_residual_bf16=True)._get_engine()
    e3 = M.ResidualUNet3D(**cfg, compute_dtype="bf16")._get_engine()
    assert e2.bf16 and e2.is2d and e3.bf16 and not e3.is2d
    assert e3._convtr_t8(128, 64) and not e2._convtr_t8(128, 64)
    assert e2._t8_weights() == [] and len(e3._t8_weights()) == 1
