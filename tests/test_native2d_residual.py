"""CPU side of the opt-in native ResidualUNet2D path (`native_2d_residual: true` / U3D_NATIVE_2D_RESIDUAL=1): the switch, what stays
blocked or is refused, what it leaves unchanged, the fp32 module tree the GPU tests compare against (reproducing the live reference's
ResidualUNet2D runs, tests/golden/r7_reference_resunet2d.npz), and the host-only sizes of the ConvTranspose2d image and workspace."""
import pytest
import torch

from reference_records_resunet2d import CASES, RunRes2D

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


def test_native_2d_residual_switch_opts_resunet2d_in():
    M = _m()
    assert not M.ResidualUNet2D(**_SMALL).native_supported  # default unchanged
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual=True)
    assert m.native_supported and m.native_2d, m._native_blockers
    assert M.get_model(dict(name="ResidualUNet2D", in_channels=1, out_channels=1, layer_order="bcr", native_2d_residual=True)).native_supported
    # explicit deconv (concat joining) is covered on a ResidualUNet2D
    assert M.ResidualUNet2D(**_SMALL, upsample="deconv", native_2d_residual=True).native_supported
    # native_2d alone keeps the warning path and names the new key
    m = M.ResidualUNet2D(**_SMALL, native_2d=True)
    assert not m.native_supported and any("native_2d_residual" in r for r in m._native_blockers), m._native_blockers


@pytest.mark.parametrize("name", ["UNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    kw = dict(name=name, in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
    a, b = M.get_model(dict(kw)), M.get_model(dict(kw, native_2d_residual=True))
    assert a.native_supported == b.native_supported and a.native_2d == b.native_2d
    assert a._native_blockers == b._native_blockers
    # the UNet2D blocker of an explicit deconv stays
    assert not M.UNet2D(**_SMALL, upsample="deconv", native_2d=True, native_2d_residual=True).native_supported


def test_native_2d_residual_environment_default(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_RESIDUAL", "1")
    assert M.ResidualUNet2D(**_SMALL).native_supported
    assert not M.ResidualUNet2D(**_SMALL, native_2d_residual=False).native_supported  # the key wins
    assert not M.UNet2D(**_SMALL).native_supported  # other classes ignore the variable too
    monkeypatch.setenv("U3D_NATIVE_2D_RESIDUAL", "0")
    assert not M.ResidualUNet2D(**_SMALL).native_supported
    assert M.ResidualUNet2D(**_SMALL, native_2d_residual=True).native_supported


@pytest.mark.parametrize("kw", [dict(compute_dtype="bf16"), dict(compute_dtype="fp32_split"), dict(upsample="nearest"),
                                dict(upsample="bilinear"), dict(layer_order="gcrd"), dict(conv_kernel_size=5, conv_padding=2),
                                dict(out_channels=2000), dict(f_maps=[512, 1024])])
def test_native_2d_residual_blockers_keep_the_warning_path(kw):
    M = _m()
    cfg = dict(dict(name="ResidualUNet2D", native_2d_residual=True, **_SMALL), **kw)
    m = M.get_model(cfg)
    assert not m.native_supported and m._native_blockers


def test_native_2d_residual_environment_blockers(monkeypatch):
    M = _m()
    for var in ("U3D_BF16", "U3D_F32_SPLIT"):
        monkeypatch.setenv(var, "1")
        assert not M.ResidualUNet2D(**_SMALL, native_2d_residual=True).native_supported
        monkeypatch.delenv(var)


@pytest.mark.parametrize("kw", [dict(hip_graph=True), dict(checkpoint_encoders=True), dict(checkpoint_encoders=True, checkpoint_levels=1)])
def test_native_2d_residual_refuses_graph_and_checkpointing(kw):
    M = _m()
    with pytest.raises(ValueError, match="hip_graph" if "hip_graph" in kw else "checkpoint"):
        M.ResidualUNet2D(**_SMALL, native_2d_residual=True, **kw)
    M.ResidualUNet2D(**_SMALL, **kw)  # without the key: constructed as before


def test_native_2d_residual_4d_only():
    """a 5-D input to the 2-D model keeps today's answer (the module tree, which torch's Conv2d rejects)"""
    M = _m()
    m = M.ResidualUNet2D(**_SMALL, native_2d_residual=True)
    with pytest.raises(RuntimeError):
        m(torch.randn(1, 1, 2, 16, 16))


def test_state_dict_unchanged_by_the_key():
    M = _m()
    cfg = dict(name="ResidualUNet2D", in_channels=1, out_channels=2, f_maps=[8, 16, 32], layer_order="bcr", final_sigmoid=False)
    torch.manual_seed(3)
    a = M.get_model(dict(cfg)).state_dict()
    torch.manual_seed(3)
    b = M.get_model(dict(cfg, native_2d_residual=True)).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", list(CASES))
def test_module_tree_reproduces_reference_resunet2d(case):
    """the CPU module tree (what the GPU tests' float64 checker runs) against the live reference's recorded run"""
    import unet3d_oracle as orc

    M = _m()
    run = RunRes2D(case)
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


def test_host_sizes_of_convtr2d_image_and_workspace():
    from pytorch3dunet_amd import _native as nat

    lib = nat.get_lib()
    # weight image [9 taps][Cin][Cout] (either mode); double weight-gradient sums in the reference layout (Cin, Cout, 3, 3)
    assert lib.u3d_convtr2d_packed_floats(1024, 512) == 9 * 1024 * 512
    assert lib.u3d_convtr2d_packed_floats(3, 5) == 135
    assert lib.u3d_convtr2d_packed_floats(0, 5) == 0
    assert lib.u3d_convtr2d_wgrad_workspace_doubles(64, 32) == 9 * 64 * 32
    assert lib.u3d_convtr2d_wgrad_workspace_doubles(4, 0) == 0
