"""CPU side of the opt-in UNet2D stem (`native_2d_stem: true` / U3D_NATIVE_2D_STEM=1): the switch, what it implies, refuses and leaves
unchanged; the host-only queries of the small-Cin kernels (csrc/u3d_conv2d.hip) and of the `_c16` entry points of the bf16 family
(csrc/u3d_conv2d_bf16.hip); and the float64 emulation the GPU tests compare against (tests/bf16_emul_2d_stem.py) held against the
executor's own routing."""
import pytest
import torch

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def _lib():
    from pytorch3dunet_amd import _native as nat

    return nat.get_lib()


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
def test_the_key_implies_native_2d_and_no_precision():
    M = _m()
    assert not M.UNet2D(**_SMALL).native_supported  # default unchanged
    m = M.UNet2D(**_SMALL, native_2d_stem=True)
    assert m.native_supported and m.native_2d and m.native_2d_stem and not m.compute_bf16 and not m.native_2d_bf16, m._native_blockers
    m = M.UNet2D(**_SMALL, native_2d_stem=True, native_2d=True)
    assert m.native_supported and m.native_2d_stem and not m.compute_bf16
    m = M.UNet2D(**_SMALL, native_2d_stem=True, native_2d_bf16=True)
    assert m.native_supported and m.native_2d_stem and m.native_2d_bf16 and m.compute_bf16
    # without the key nothing changes
    for extra in (dict(native_2d=True), dict(native_2d_bf16=True)):
        m = M.UNet2D(**_SMALL, **extra)
        assert m.native_supported and m.native_2d_stem is False
    # it implies no precision: bf16 next to it without native_2d_bf16 stays on the warning path, as under native_2d
    assert not M.UNet2D(**_SMALL, native_2d_stem=True, compute_dtype="bf16").native_supported


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_STEM", "1")
    m = M.UNet2D(**_SMALL)
    assert m.native_supported and m.native_2d and m.native_2d_stem and not m.compute_bf16
    m = M.UNet2D(**_SMALL, native_2d_stem=False)  # the key wins
    assert not m.native_supported and not m.native_2d_stem and not m.native_2d
    assert not M.ResidualUNet2D(**_SMALL).native_supported  # other classes ignore the variable too
    assert M.UNet3D(**_SMALL).native_2d_stem is False
    monkeypatch.setenv("U3D_NATIVE_2D_STEM", "0")
    assert not M.UNet2D(**_SMALL).native_supported
    assert M.UNet2D(**_SMALL, native_2d_stem=True).native_supported


@pytest.mark.parametrize("name", ["ResidualUNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, **_SMALL)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_stem=True))
    assert b.native_2d_stem is False
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d and a.compute_bf16 == b.compute_bf16
    assert a._native_blockers == b._native_blockers
    # a native ResidualUNet2D is the same executor with or without it
    r = M.ResidualUNet2D(**_SMALL, native_2d_residual=True, native_2d_stem=True)
    assert r.native_supported and r.native_2d_stem is False and not r._get_engine().stem


def test_state_dict_unchanged_by_the_key():
    M = _m()
    cfg = dict(name="UNet2D", in_channels=1, out_channels=2, f_maps=[32, 64], layer_order="bcr", final_sigmoid=False)
    torch.manual_seed(3)
    a = M.get_model(dict(cfg)).state_dict()
    torch.manual_seed(3)
    b = M.get_model(dict(cfg, native_2d_stem=True, native_2d_bf16=True)).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("base", [dict(), dict(native_2d=True), dict(native_2d_bf16=True)])
def test_refusals_are_those_of_the_mode_it_sits_on(base):
    M = _m()
    with pytest.raises(ValueError, match="hip_graph"):
        M.UNet2D(**_SMALL, native_2d_stem=True, hip_graph=True, **base)
    for upsample, ok in [("default", True), ("nearest", True), ("deconv", False), ("bilinear", False)]:
        a = M.UNet2D(**_SMALL, upsample=upsample, **(base or dict(native_2d=True)))
        b = M.UNet2D(**_SMALL, upsample=upsample, native_2d_stem=True, **base)
        assert a.native_supported == b.native_supported == ok and a._native_blockers == b._native_blockers
    if base.get("native_2d_bf16"):
        with pytest.raises(ValueError, match="native_2d_bf16"):
            M.UNet2D(**_SMALL, native_2d_stem=True, compute_dtype="fp32", **base)
    else:
        assert not M.UNet2D(**_SMALL, native_2d_stem=True, compute_dtype="fp32_split", **base).native_supported


# ---- routing: the emulation's restated rule against the executor's ------------------------------------------------------------------------
MODEL_CASES = [
    # cfg, small-family layers, layers on the bf16 family under native_2d_bf16 + stem, of which on the `_c16` entry points
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="gcr", num_groups=8), 1, 9, 1),  # all but 1 -> 16
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="bcr"), 1, 5, 1),
    (dict(name="UNet2D", in_channels=2, out_channels=3, f_maps=[32, 64], final_sigmoid=False, num_groups=8), 1, 5, 1),
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[16, 32], layer_order="gcr", num_groups=8), 1, 4, 4),  # 8 -> 16 stays fp32
    (dict(name="UNet2D", in_channels=3, out_channels=2, f_maps=[32, 64], layer_order="cgr", num_groups=8, final_sigmoid=False), 1, 4, 1),
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], layer_order="gcr", num_groups=4), 2, 0, 0),  # 1 -> 4 and 4 -> 8
]


@pytest.mark.parametrize("cfg,n_small,n_bf16,n_c16", MODEL_CASES)
def test_emulation_rule_is_the_executors_routing(cfg, n_small, n_bf16, n_c16):
    import bf16_emul_2d as E0
    import bf16_emul_2d_stem as E

    M = _m()
    model = M.get_model(dict(cfg, native_2d_bf16=True, native_2d_stem=True))
    eng = model._get_engine()  # (building the executor does not touch the GPU)
    images = eng.images
    sm, el, c16 = ([id(c.weight) for c in f(model)] for f in (E.small, E.eligible, E.c16))
    assert (len(sm), len(el), len(c16)) == (n_small, n_bf16, n_c16)
    assert sorted(c16) == sorted(id(w) for w in images._each_bf16_c16)
    assert sorted(set(el) - set(c16)) == sorted(id(w) for w in images._each_bf16)
    every = {id(m.weight): m for m in model.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)}
    assert {id(w) for w in images._each} == set(every) - set(sm) - set(el)  # (a small-family layer gets no packed image up front)
    virt = eng._virtual_w
    assert {i for i, m in every.items() if eng._small2d(m.in_channels, m.out_channels, i in virt)} == set(sm)
    assert {i for i, m in every.items() if eng._bf16_routed_weight(m.in_channels, m.out_channels, i in virt) and i not in sm} == set(el)
    # next to native_2d alone: the small family only; every other layer keeps an fp32 image
    m32 = M.get_model(dict(cfg, native_2d_stem=True))
    e32 = m32._get_engine()
    every32 = {id(m.weight): m for m in m32.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)}
    assert not e32.images._each_bf16 and not e32.images._each_bf16_c16
    assert len(every32) - len(e32.images._each) == n_small
    # without the stem key: today's sets (tests/bf16_emul_2d.py), no small family
    m0 = M.get_model(dict(cfg, native_2d_bf16=True))
    e0 = m0._get_engine()
    assert not e0.stem and not e0.images._each_bf16_c16
    assert sorted(id(c.weight) for c in E0.eligible(m0)) == sorted(id(w) for w in e0.images._each_bf16)
    assert len(e0.images._each) + len(e0.images._each_bf16) == len(every)


def test_emulation_keeps_the_small_family_exact_and_rounds_the_16_channel_layers():
    import bf16_emul_2d as E0
    import bf16_emul_2d_stem as E

    M = _m()
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[16, 32], layer_order="gcr", num_groups=8)
    torch.manual_seed(5)
    sd = M.get_model(dict(cfg)).state_dict()
    x, t = torch.randn(1, 1, 16, 20), (torch.rand(1, 1, 16, 20) > 0.5).float()
    plain = E.run(cfg, sd, x, t, "bce_dice", emulate=False)
    stem = E.run(cfg, sd, x, t, "bce_dice", emulate=True)
    old = E0.run(cfg, sd, x, t, "bce_dice", emulate=True)  # the rule of native_2d_bf16 alone rounds nothing in this net
    assert torch.equal(old[0], plain[0])
    assert not torch.equal(stem[0], plain[0]) and (stem[0] - plain[0]).abs().max() < 0.05 * plain[0].abs().max()
    # a net whose every 3x3 layer is small-family, 8-channel or a virtual concat: the emulation is the plain run
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], layer_order="gcr", num_groups=4)
    torch.manual_seed(5)
    sd = M.get_model(dict(cfg)).state_dict()
    a, b = E.run(cfg, sd, x, t, "bce_dice", emulate=True), E.run(cfg, sd, x, t, "bce_dice", emulate=False)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and all(torch.equal(a[2][k], b[2][k]) for k in b[2])


# ---- host-only queries -----------------------------------------------------------------------------------------------------------------
def test_c16_envelope_and_the_old_queries_unchanged():
    lib = _lib()
    for Cin, Cout in [(16, 32), (32, 16), (16, 16), (48, 80), (32, 32)]:
        assert lib.u3d_conv2d_bf16_c16_supported(Cin, Cout) == 1 and lib.u3d_conv2d_wgrad_bf16_c16_supported(Cin, Cout) == 1
    for Cin, Cout in [(20, 32), (32, 8), (0, 16), (16, 0), (8, 16)]:
        assert lib.u3d_conv2d_bf16_c16_supported(Cin, Cout) == 0 and lib.u3d_conv2d_wgrad_bf16_c16_supported(Cin, Cout) == 0
    # the old queries answer as before (tests/test_native2d_bf16.py)
    assert lib.u3d_conv2d_bf16_supported(16, 32) == 1 and lib.u3d_conv2d_bf16_supported(32, 16) == 0
    assert lib.u3d_conv2d_bf16_supported(16, 16) == 0 and lib.u3d_conv2d_bf16_supported(48, 80) == 0
    assert lib.u3d_conv2d_wgrad_bf16_supported(32, 96) == 1 and lib.u3d_conv2d_wgrad_bf16_supported(16, 32) == 0
    assert lib.u3d_conv2d_wgrad_bf16_supported(32, 16) == 0
    assert lib.u3d_packed_weight2d_bf16_elems(16, 32, 1) == 0 and lib.u3d_packed_weight2d_bf16_elems(32, 16, 0) == 0
    assert lib.u3d_conv2d_bf16_variant(1, 8, 8, 32, 16, 1) == -1 and lib.u3d_conv2d_wgrad_bf16_variant(1, 8, 8, 16, 32) == -1
    assert lib.u3d_conv2d_bf16_workspace_floats(1, 8, 8, 256, 16) == 0 and lib.u3d_wgrad2d_bf16_workspace_floats(2, 64, 64, 16, 32) == 0


def test_c16_image_and_workspace_sizes():
    lib = _lib()
    # image [K / 16][9 taps][ceil(N / 32)][64 lanes][8] 2-byte elements: a half n-tile is stored whole
    assert lib.u3d_packed_weight2d_bf16_c16_elems(16, 32, 0) == 9 * 512 and lib.u3d_packed_weight2d_bf16_c16_elems(16, 32, 1) == 2 * 9 * 512
    assert lib.u3d_packed_weight2d_bf16_c16_elems(32, 16, 0) == 2 * 9 * 512 and lib.u3d_packed_weight2d_bf16_c16_elems(16, 16, 1) == 9 * 512
    assert lib.u3d_packed_weight2d_bf16_c16_elems(48, 80, 0) == 3 * 9 * 3 * 512 and lib.u3d_packed_weight2d_bf16_c16_elems(48, 80, 1) == 5 * 9 * 2 * 512
    for mode in (0, 1):  # inside the old envelope: the old size
        assert lib.u3d_packed_weight2d_bf16_c16_elems(32, 64, mode) == lib.u3d_packed_weight2d_bf16_elems(32, 64, mode) > 0
    assert lib.u3d_packed_weight2d_bf16_c16_elems(20, 32, 0) == 0 and lib.u3d_packed_weight2d_bf16_c16_elems(32, 8, 1) == 0
    assert lib.u3d_packed_weight2d_bf16_c16_elems(16, 16, 2) == 0
    # no split-K scratch on a full-resolution stem layer or outside the envelope; whole multiples of the output where the grid is small
    assert lib.u3d_conv2d_bf16_c16_workspace_floats(32, 515, 512, 16, 32) == 0
    assert lib.u3d_conv2d_bf16_c16_workspace_floats(32, 515, 512, 32, 16) == 0
    small = lib.u3d_conv2d_bf16_c16_workspace_floats(1, 8, 8, 256, 16)
    assert small > 0 and small % (8 * 8 * 16) == 0
    assert lib.u3d_conv2d_bf16_c16_workspace_floats(1, 8, 8, 16, 16) == 0  # one input chunk: nothing to split
    assert lib.u3d_conv2d_bf16_c16_workspace_floats(1, 8, 8, 20, 32) == 0
    assert lib.u3d_wgrad2d_bf16_c16_workspace_floats(1, 1, 1, 16, 16) == 0  # one tile: written directly
    assert lib.u3d_wgrad2d_bf16_c16_workspace_floats(0, 8, 8, 16, 32) == 0 and lib.u3d_wgrad2d_bf16_c16_workspace_floats(1, 8, 8, 16, 8) == 0


def test_c16_plan_queries():
    lib = _lib()
    for bad in [(1, 8, 8, 20, 32), (1, 8, 8, 32, 8), (0, 8, 8, 16, 16), (1, 0, 8, 16, 16), (1, 8, 0, 16, 16)]:
        assert lib.u3d_conv2d_bf16_c16_variant(*bad, 1) == -1 and lib.u3d_conv2d_wgrad_bf16_c16_variant(*bad) == -1
    shapes = [(2, 19, 21, 32, 16), (1, 16, 16, 16, 16), (1, 35, 45, 48, 80), (1, 33, 17, 32, 48), (2, 250, 245, 32, 16), (1, 8, 8, 256, 16),
              (32, 515, 512, 16, 32), (1, 139, 141, 16, 32)]
    for N, H, W, Cin, Cout in shapes:
        v = lib.u3d_conv2d_bf16_c16_variant(N, H, W, Cin, Cout, 1)
        nt, ksplit = v & 255, v >> 8
        assert nt in (1, 2) and 1 <= ksplit <= Cin // 16, (N, H, W, Cin, Cout, v)
        assert lib.u3d_conv2d_bf16_c16_workspace_floats(N, H, W, Cin, Cout) == (ksplit * N * H * W * Cout if ksplit > 1 else 0)
        assert lib.u3d_conv2d_bf16_c16_variant(N, H, W, Cin, Cout, 0) == (1 << 8) | nt
        v = lib.u3d_conv2d_wgrad_bf16_c16_variant(N, H, W, Cin, Cout)
        tps, nsplit = v >> 16, v & 0xFFFF
        ntiles = N * ((H + 15) // 16) * ((W + 15) // 16)
        assert tps >= 1 and (nsplit - 1) * tps < ntiles <= nsplit * tps, (N, H, W, Cin, Cout, v)
        assert lib.u3d_wgrad2d_bf16_c16_workspace_floats(N, H, W, Cin, Cout) == (nsplit * Cout * Cin * 9 if nsplit > 1 else 0)
    # inside the old envelope the plans are the old ones
    for shape in [(2, 17, 19, 32, 64), (1, 8, 8, 256, 128), (32, 515, 512, 32, 64)]:
        assert lib.u3d_conv2d_bf16_c16_variant(*shape, 1) == lib.u3d_conv2d_bf16_variant(*shape, 1)
        assert lib.u3d_conv2d_wgrad_bf16_c16_variant(*shape) == lib.u3d_conv2d_wgrad_bf16_variant(*shape)
    assert lib.u3d_conv2d_bf16_c16_variant(32, 515, 512, 16, 32, 1) == (1 << 8) | 1  # a full-resolution stem layer: one n-tile, unsplit


def test_small_cin_queries():
    lib = _lib()
    for bad in [(1, 8, 8, 5, 16), (1, 8, 8, 1, 33), (1, 8, 8, 0, 8), (0, 8, 8, 1, 16), (1, 0, 8, 1, 16), (1, 8, 0, 1, 16), (70000, 8, 8, 1, 16)]:
        assert lib.u3d_conv2d_small_cin_fwd_variant(*bad) == -1 and lib.u3d_conv2d_small_cin_bwd_variant(*bad) == -1
        assert lib.u3d_small_cin2d_bwd_workspace_floats(*bad) == 0
    # forward: bit 0 matrix pipe (Cout % 4 == 0), bit 1 several tiles per block (more tiles than 512 / N blocks per sample)
    assert lib.u3d_conv2d_small_cin_fwd_variant(2, 19, 21, 1, 16) == 1 and lib.u3d_conv2d_small_cin_fwd_variant(1, 7, 5, 1, 6) == 0
    assert lib.u3d_conv2d_small_cin_fwd_variant(32, 515, 512, 1, 16) == 3 and lib.u3d_conv2d_small_cin_fwd_variant(2, 368, 368, 2, 6) == 2
    # backward: bit 0 two row tiles (Cout > 16), bit 1 several tiles per block, bit 2 more than one partial per sample
    assert lib.u3d_conv2d_small_cin_bwd_variant(1, 16, 16, 3, 32) == 1 and lib.u3d_conv2d_small_cin_bwd_variant(1, 5, 3, 4, 12) == 0
    assert lib.u3d_conv2d_small_cin_bwd_variant(2, 19, 21, 1, 16) == 4 and lib.u3d_conv2d_small_cin_bwd_variant(32, 515, 512, 1, 16) == 6
    # workspace: one [Cout][9][Cin + 1] partial per block, min(1024 / N, tiles) blocks per sample
    assert lib.u3d_small_cin2d_bwd_workspace_floats(1, 16, 16, 3, 32) == 32 * 9 * 4
    assert lib.u3d_small_cin2d_bwd_workspace_floats(2, 19, 21, 1, 16) == 2 * 4 * 16 * 9 * 2
    assert lib.u3d_small_cin2d_bwd_workspace_floats(32, 515, 512, 1, 16) == 32 * 32 * 16 * 9 * 2
    # the executor sizes the shared scratch for the small backward AND its data-gradient fall-through
    M = _m()
    eng = M.UNet2D(**_SMALL, native_2d_stem=True)._get_engine()
    need = eng._layer_ws_floats(2, 1, 35, 45, 1, 4, small=True)
    assert need >= lib.u3d_small_cin2d_bwd_workspace_floats(2, 35, 45, 1, 4) and need >= lib.u3d_wgrad2d_workspace_floats(2, 35, 45, 1, 4)
