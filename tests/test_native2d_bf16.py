"""CPU side of the opt-in bf16 2-D path (`native_2d_bf16: true` / U3D_NATIVE_2D_BF16=1): the switch, what it implies, refuses and leaves
unchanged, the host-only sizes of the bf16 2-D images and workspaces, and the float64 emulation the GPU tests compare against
(tests/bf16_emul_2d.py) held against the executor's own routing."""
import pytest
import torch

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def test_native_2d_bf16_switch_opts_unet2d_in():
    M = _m()
    assert not M.UNet2D(**_SMALL).native_supported  # default unchanged
    m = M.UNet2D(**_SMALL, native_2d_bf16=True)
    assert m.native_supported and m.native_2d and m.native_2d_bf16 and m.compute_bf16 and not m.compute_split, m._native_blockers
    # an explicit compute_dtype: bf16 next to it is accepted, and so is native_2d: true
    m = M.UNet2D(**_SMALL, native_2d_bf16=True, compute_dtype="bf16", native_2d=True)
    assert m.native_supported and m.compute_bf16
    # without the key nothing changes: fp32 native_2d, and native_2d + bf16 stays on the warning path
    m = M.UNet2D(**_SMALL, native_2d=True)
    assert m.native_supported and not m.compute_bf16 and not m.native_2d_bf16
    assert not M.UNet2D(**_SMALL, native_2d=True, compute_dtype="bf16").native_supported
    assert not M.UNet2D(**_SMALL, native_2d_bf16=False, native_2d=True, compute_dtype="bf16").native_supported


@pytest.mark.parametrize("order", ["gcr", "bcr", "cgr", "crg", "cr", "gcl", "bce", "cbr"])
def test_every_native_layer_order_works_under_the_key(order):
    M = _m()
    m = M.get_model(dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order=order, native_2d_bf16=True))
    assert m.native_supported and m.compute_bf16, (order, m._native_blockers)


@pytest.mark.parametrize("upsample,ok", [("default", True), ("nearest", True), ("deconv", False), ("bilinear", False)])
def test_upsample_rule_is_the_one_of_native_2d(upsample, ok):
    M = _m()
    m = M.UNet2D(**_SMALL, native_2d_bf16=True, upsample=upsample)
    assert m.native_supported == ok, m._native_blockers


@pytest.mark.parametrize("dtype", ["fp32", "float32", "fp32_split"])
def test_contradicting_compute_dtype_raises(dtype):
    M = _m()
    with pytest.raises(ValueError, match="native_2d_bf16"):
        M.UNet2D(**_SMALL, native_2d_bf16=True, compute_dtype=dtype)
    M.UNet2D(**_SMALL, compute_dtype=dtype)  # without the key: constructed as before


def test_hip_graph_stays_refused():
    M = _m()
    with pytest.raises(ValueError, match="hip_graph"):
        M.UNet2D(**_SMALL, native_2d_bf16=True, hip_graph=True)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_BF16", "1")
    m = M.UNet2D(**_SMALL)
    assert m.native_supported and m.native_2d_bf16 and m.compute_bf16
    m = M.UNet2D(**_SMALL, native_2d_bf16=False)  # the key wins
    assert not m.native_supported and not m.native_2d_bf16 and not m.compute_bf16
    with pytest.raises(ValueError, match="native_2d_bf16"):
        M.UNet2D(**_SMALL, compute_dtype="fp32")
    assert not M.ResidualUNet2D(**_SMALL).native_supported  # other classes ignore the variable too
    assert not M.UNet3D(**_SMALL).compute_bf16
    monkeypatch.setenv("U3D_NATIVE_2D_BF16", "0")
    assert not M.UNet2D(**_SMALL).native_supported
    assert M.UNet2D(**_SMALL, native_2d_bf16=True).native_supported


@pytest.mark.parametrize("name", ["ResidualUNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, **_SMALL)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_bf16=True))
    assert b.native_2d_bf16 is False
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d and a.compute_bf16 == b.compute_bf16
    assert a._native_blockers == b._native_blockers
    # ... and an fp32 compute_dtype next to the ignored key is no contradiction there
    M.get_model(dict(kw, native_2d_bf16=True, compute_dtype="fp32"))
    # a ResidualUNet2D in bf16 stays on the warning path, with or without the key
    r = M.ResidualUNet2D(**_SMALL, native_2d_residual=True, native_2d_bf16=True, compute_dtype="bf16")
    assert not r.native_supported and r._native_blockers


def test_state_dict_unchanged_by_the_key():
    M = _m()
    cfg = dict(name="UNet2D", in_channels=1, out_channels=2, f_maps=[32, 64], layer_order="bcr", final_sigmoid=False)
    torch.manual_seed(3)
    a = M.get_model(dict(cfg)).state_dict()
    torch.manual_seed(3)
    b = M.get_model(dict(cfg, native_2d_bf16=True)).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_host_sizes_of_bf16_2d_images_and_workspaces():
    from pytorch3dunet_amd import _native as nat

    lib = nat.get_lib()
    assert lib.u3d_conv2d_bf16_supported(16, 32) == 1 and lib.u3d_conv2d_bf16_supported(32, 16) == 0
    assert lib.u3d_conv2d_bf16_supported(20, 32) == 0 and lib.u3d_conv2d_bf16_supported(32, 8) == 0
    assert lib.u3d_conv2d_wgrad_bf16_supported(32, 96) == 1 and lib.u3d_conv2d_wgrad_bf16_supported(16, 32) == 0
    # image [K / 16][9 taps][N / 32][64 lanes][8] 2-byte elements; mode 0: K = Cin, N = Cout; mode 1: roles swapped
    assert lib.u3d_packed_weight2d_bf16_elems(32, 64, 0) == 2 * 9 * 2 * 512
    assert lib.u3d_packed_weight2d_bf16_elems(32, 64, 1) == 4 * 9 * 1 * 512
    assert lib.u3d_packed_weight2d_bf16_elems(16, 32, 0) == 9 * 512 and lib.u3d_packed_weight2d_bf16_elems(16, 32, 1) == 0
    assert lib.u3d_packed_weight2d_bf16_elems(32, 32, 2) == 0
    # split-K scratch only where the grid is small: whole multiples of the output, none on a large image or outside the envelope
    assert lib.u3d_conv2d_bf16_workspace_floats(32, 515, 512, 32, 32) == 0
    small = lib.u3d_conv2d_bf16_workspace_floats(1, 8, 8, 256, 128)
    assert small > 0 and small % (8 * 8 * 128) == 0
    assert lib.u3d_conv2d_bf16_workspace_floats(1, 8, 8, 16, 128) == 0  # one input chunk: nothing to split
    assert lib.u3d_conv2d_bf16_workspace_floats(1, 8, 8, 20, 32) == 0
    wg = lib.u3d_wgrad2d_bf16_workspace_floats(2, 64, 64, 64, 64)
    assert wg == 0 or wg % (64 * 64 * 9) == 0
    assert lib.u3d_wgrad2d_bf16_workspace_floats(1, 1, 1, 32, 32) == 0  # one tile: written directly
    assert lib.u3d_wgrad2d_bf16_workspace_floats(0, 8, 8, 32, 32) == 0


def test_plan_queries_of_the_bf16_2d_launches():
    """u3d_conv2d_bf16_variant / u3d_conv2d_wgrad_bf16_variant report the plans the workspace sizes come from (properties that hold for
    every CU count; the GPU tests assert the variants of their pinned shapes)"""
    from pytorch3dunet_amd import _native as nat

    lib = nat.get_lib()
    for bad in [(1, 8, 8, 20, 32), (1, 8, 8, 32, 8), (0, 8, 8, 32, 32), (1, 0, 8, 32, 32), (1, 8, 0, 32, 32)]:
        assert lib.u3d_conv2d_bf16_variant(*bad, 1) == -1 and lib.u3d_conv2d_wgrad_bf16_variant(*bad) == -1
    assert lib.u3d_conv2d_bf16_variant(1, 8, 8, 16, 32, 1) > 0 and lib.u3d_conv2d_wgrad_bf16_variant(1, 8, 8, 16, 32) == -1
    shapes = [(1, 4, 5, 32, 32), (2, 17, 19, 32, 64), (1, 8, 8, 256, 128), (1, 8, 8, 16, 128), (2, 250, 245, 16, 64), (1, 250, 245, 32, 96),
              (32, 515, 512, 32, 64), (1, 139, 141, 128, 128), (1, 70, 75, 256, 256)]
    for N, H, W, Cin, Cout in shapes:
        v = lib.u3d_conv2d_bf16_variant(N, H, W, Cin, Cout, 1)
        nt, ksplit = v & 255, v >> 8
        assert nt in (1, 2) and 1 <= ksplit <= Cin // 16, (N, H, W, Cin, Cout, v)
        need = lib.u3d_conv2d_bf16_workspace_floats(N, H, W, Cin, Cout)
        assert need == (ksplit * N * H * W * Cout if ksplit > 1 else 0)
        assert lib.u3d_conv2d_bf16_variant(N, H, W, Cin, Cout, 0) == (1 << 8) | nt  # no scratch: the same block, never split
        if Cin % 32 == 0:
            v = lib.u3d_conv2d_wgrad_bf16_variant(N, H, W, Cin, Cout)
            tps, nsplit = v >> 16, v & 0xFFFF
            ntiles = N * ((H + 15) // 16) * ((W + 15) // 16)
            assert tps >= 1 and (nsplit - 1) * tps < ntiles <= nsplit * tps, (N, H, W, Cin, Cout, v)
            assert lib.u3d_wgrad2d_bf16_workspace_floats(N, H, W, Cin, Cout) == (nsplit * Cout * Cin * 9 if nsplit > 1 else 0)
    assert lib.u3d_conv2d_bf16_variant(1, 8, 8, 16, 128, 1) >> 8 == 1  # one input chunk: nothing to split
    assert lib.u3d_conv2d_bf16_variant(32, 515, 512, 32, 64, 1) == (1 << 8) | 2  # a full-resolution level: the 64-channel block, unsplit
    assert lib.u3d_conv2d_bf16_variant(32, 515, 512, 32, 32, 1) == (1 << 8) | 1  # one n-tile in all


# ---- the emulation helper of the GPU model tests ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,n_bf16", [
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="gcr", num_groups=8), 8),  # all but 1->16, 16->32
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="bcr"), 4),
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64], layer_order="cgr", num_groups=8), 3),  # virtual concat: fp32
    (dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], layer_order="gcr", num_groups=4), 0),
])
def test_emulation_rounds_exactly_the_layers_the_executor_routes_to_bf16(cfg, n_bf16):
    import bf16_emul_2d as E

    M = _m()
    model = M.get_model(dict(cfg, native_2d_bf16=True))
    mine = [id(c.weight) for c in E.eligible(model)]
    images = model._get_engine().images  # (building the executor does not touch the GPU)
    assert len(mine) == n_bf16
    assert sorted(mine) == sorted(id(w) for w in images._each_bf16)
    assert not set(mine) & {id(w) for w in images._each}


def test_emulation_function_rounds_the_operands_of_its_three_gemms():
    import torch.nn.functional as F

    import bf16_emul_2d as E

    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 32, 7, 9, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(32, 32, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn(2, 32, 7, 9, generator=g, dtype=torch.float64)
    y = E.Bf16Conv2d.apply(x, w)
    y.backward(dz)
    xr, wr, dzr = E.r16(x.detach()), E.r16(w.detach()), E.r16(dz)
    assert not torch.equal(xr, x.detach()) and torch.equal(E.r16(xr), xr)
    assert torch.equal(y.detach(), F.conv2d(xr, wr, padding=1))
    assert torch.equal(x.grad, torch.nn.grad.conv2d_input(x.shape, wr, dzr, padding=1))
    assert torch.equal(w.grad, torch.nn.grad.conv2d_weight(xr, w.shape, dzr, padding=1))


def test_emulation_without_eligible_layers_is_the_plain_float64_run():
    import bf16_emul_2d as E

    M = _m()
    cfg = dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[8, 16], layer_order="gcr", num_groups=4)
    torch.manual_seed(5)
    model = M.get_model(dict(cfg, native_2d_bf16=True))
    sd = model.state_dict()
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
