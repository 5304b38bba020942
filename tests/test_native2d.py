"""CPU side of the opt-in native 2-D path (`native_2d: true` / U3D_NATIVE_2D=1): the switch, what it leaves unchanged, the float64
module tree the GPU tests compare against (reproducing the live reference's UNet2D runs, tests/golden/r6_reference_unet2d.npz), and
the host-only sizes of the 2-D weight images and workspaces."""
import pytest
import torch

from reference_records_2d import CASES, Run2D


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def test_native_2d_switch_opts_unet2d_in():
    M = _m()
    assert not M.UNet2D(1, 1, f_maps=8, num_levels=2, num_groups=4).native_supported  # default unchanged
    m = M.UNet2D(1, 1, f_maps=8, num_levels=2, num_groups=4, native_2d=True)
    assert m.native_supported and m.native_2d, m._native_blockers
    assert M.get_model(dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="bcr",
                            native_2d=True)).native_supported
    assert not M.get_model(dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=[32, 64, 128], layer_order="bcr")).native_supported
    # a 3-D model ignores the key
    m3 = M.UNet3D(1, 1, f_maps=8, num_levels=2, num_groups=4, native_2d=True)
    assert m3.native_supported and not m3.native_2d


def test_native_2d_environment_default(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D", "1")
    assert M.UNet2D(1, 1, f_maps=8, num_levels=2, num_groups=4).native_supported
    assert not M.UNet2D(1, 1, f_maps=8, num_levels=2, num_groups=4, native_2d=False).native_supported  # the key wins
    monkeypatch.setenv("U3D_NATIVE_2D", "0")
    assert not M.UNet2D(1, 1, f_maps=8, num_levels=2, num_groups=4).native_supported


@pytest.mark.parametrize("kw", [dict(name="ResidualUNet2D"), dict(name="UNet2D", compute_dtype="bf16"),
                                dict(name="UNet2D", compute_dtype="fp32_split"), dict(name="UNet2D", upsample="deconv")])
def test_native_2d_blockers_keep_the_warning_path(kw):
    M = _m()
    m = M.get_model(dict(dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4, native_2d=True), **kw))
    assert not m.native_supported and m._native_blockers


def test_native_2d_with_hip_graph_is_refused():
    M = _m()
    with pytest.raises(ValueError, match="hip_graph"):
        M.UNet2D(1, 1, f_maps=8, num_levels=2, num_groups=4, native_2d=True, hip_graph=True)


def test_state_dict_unchanged_by_the_key():
    M = _m()
    cfg = dict(name="UNet2D", in_channels=1, out_channels=2, f_maps=[8, 16, 32], layer_order="bcr", final_sigmoid=False)
    torch.manual_seed(3)
    a = M.get_model(dict(cfg)).state_dict()
    torch.manual_seed(3)
    b = M.get_model(dict(cfg, native_2d=True)).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", list(CASES))
def test_module_tree_reproduces_reference_unet2d(case):
    """the CPU module tree (what the GPU tests' float64 checker runs) against the live reference's recorded run"""
    import unet3d_oracle as orc

    M = _m()
    run = Run2D(case)
    model = M.get_model(dict(run.cfg))
    model.load_state_dict(run.sd)
    model.train()
    probs, logits = model(run.x, return_logits=True)
    loss = orc.bce_dice_loss(logits, run.target)
    loss.backward()
    assert orc.rel_err(logits.detach(), run.logits) < 1e-5 and orc.rel_err(probs.detach(), run.probs) < 1e-5
    assert abs(loss.item() - run.loss) < 1e-6
    for k, p in model.named_parameters():
        assert run.grad_rel_err(k, p.grad) < 1e-4, k
    sd = model.state_dict()
    for k, v in run.buffers.items():
        assert torch.allclose(sd[k], v, rtol=1e-5, atol=1e-6), k


def test_host_sizes_of_2d_images_and_workspaces():
    from pytorch3dunet_amd import _native as nat

    lib = nat.get_lib()
    # image [ceil(K / 16)][9 taps][2][ceil(N / 32)][64 lanes][4]; mode 0: K = Cin, N = Cout; mode 1: roles swapped
    assert lib.u3d_packed_weight2d_floats(1, 8, 0) == 1 * 9 * 2 * 1 * 256
    assert lib.u3d_packed_weight2d_floats(20, 64, 0) == 2 * 9 * 2 * 2 * 256
    assert lib.u3d_packed_weight2d_floats(20, 64, 1) == 4 * 9 * 2 * 1 * 256
    assert lib.u3d_packed_weight2d_floats(96, 192, 1) == 12 * 9 * 2 * 3 * 256
    assert lib.u3d_packed_weight2d_floats(8, 8, 2) == 0
    # split-K scratch only where the grid is small: whole multiples of the output, none on a large image
    assert lib.u3d_conv2d_workspace_floats(32, 515, 512, 32, 32) == 0
    small = lib.u3d_conv2d_workspace_floats(1, 64, 64, 256, 128)
    assert small > 0 and small % (64 * 64 * 128) == 0
    assert lib.u3d_conv2d_workspace_floats(1, 64, 64, 16, 128) == 0  # one input chunk: nothing to split
    # weight gradient: a whole (Cout, Cin, 3, 3) partial per pixel range, or none
    wg = lib.u3d_wgrad2d_workspace_floats(2, 64, 64, 64, 64)
    assert wg == 0 or wg % (64 * 64 * 9) == 0
    assert lib.u3d_wgrad2d_workspace_floats(1, 1, 1, 8, 8) == 0  # one tile: written directly
    assert lib.u3d_wgrad2d_workspace_floats(0, 8, 8, 8, 8) == 0
