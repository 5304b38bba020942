"""CPU side of the opt-in sub-pixel bf16 decoder path of a UNet3D (`bf16_subpixel: true` / U3D_BF16_SUBPIXEL=1): the key — what it implies,
refuses and leaves unchanged —, the executor's one eligibility rule (`_bf16_subpixel3d`, through `_subpixel_layers` of an engine built on
the CPU) held against its restatement in tests/bf16_emul_3d_subpixel.py, the declarations of the new entry points, and the emulation
itself: exact without rounding (against F.conv3d over the nearest-upsampled tensor and its gradients, and as a whole model), inside 2/3 of
the stated bf16 bars with it.

One figure of the issue does not hold as written: a 3-level net with f_maps [16, 32, 64] HAS a level inside the channel rule (its bottom
decoder joins 32 skip and 64 upsampled channels into 32), so it counts 1 / 0 / 0 eligible levels at the three shapes, not 0 everywhere; the
net with no level inside the channel rule at any size is `SE.NET_OUTSIDE_CHANNEL_RULE` (f_maps [24, 48, 96])."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bf16_emul_3d_subpixel as SE

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
ENTRY_POINTS = ("u3d_subpixel_bf16_packed_elems", "u3d_pack_subpixel_weights_bf16", "u3d_subpixel_conv_fwd_bf16",
                "u3d_subpixel_conv_dgrad_bf16", "u3d_subpixel_wgrad_bf16_workspace_floats", "u3d_subpixel_conv_wgrad_bf16",
                "u3d_pack_weights_bf16_slice", "u3d_conv3d_wgrad_bf16_strided")


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


# ---- the identities, without rounding ----------------------------------------------------------------------------------------------------
def up2(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def childsum(d):
    N, C, D, H, W = d.shape
    return d.view(N, C, D // 2, 2, H // 2, 2, W // 2, 2).sum((3, 5, 7))


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 3, 5), (5, 9, 11)])
def test_without_rounding_the_three_forms_are_conv3d_over_the_upsampled_tensor(dims):
    g = torch.Generator().manual_seed(7 + sum(dims))
    N, C1, Cout = 2, 3, 4
    low = torch.randn(N, C1, *dims, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C1, 3, 3, 3, generator=g, dtype=torch.float64)
    dz = torch.randn(N, Cout, *(2 * d for d in dims), generator=g, dtype=torch.float64)
    up = up2(low)
    y = SE.up_forward(low, SE.presum_fwd(w, SE.identity))
    dlow = SE.up_dgrad(dz, SE.presum_dgrad(w, SE.identity))
    dw = SE.up_wgrad(low, dz)
    assert _rel(y, F.conv3d(up, w, padding=1)) < 1e-12
    assert _rel(dlow, childsum(torch.nn.grad.conv3d_input(up.shape, w, dz, padding=1))) < 1e-12
    assert _rel(dw, torch.nn.grad.conv3d_weight(up, w.shape, dz, padding=1)) < 1e-12


def test_without_rounding_the_split_layer_is_conv3d_of_the_concat():
    g = torch.Generator().manual_seed(3)
    N, C0, C1, Cout, dims = 1, 2, 3, 4, (2, 3, 5)
    skip = torch.randn(N, C0, *(2 * d for d in dims), generator=g, dtype=torch.float64)
    low = torch.randn(N, C1, *dims, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C0 + C1, 3, 3, 3, generator=g, dtype=torch.float64)
    dz = torch.randn(N, Cout, *(2 * d for d in dims), generator=g, dtype=torch.float64)
    xa = torch.cat((skip, up2(low)), 1).requires_grad_(True)
    wa = w.clone().requires_grad_(True)
    F.conv3d(xa, wa, padding=1).backward(dz)
    xb = xa.detach().clone().requires_grad_(True)
    wb = w.clone().requires_grad_(True)
    yb = SE.SubpixelBf16Conv3d.apply(xb, wb, C0, SE.identity)
    yb.backward(dz)
    assert _rel(yb.detach(), F.conv3d(xa.detach(), w, padding=1)) < 1e-12
    assert _rel(wb.grad, wa.grad) < 1e-12
    assert _rel(xb.grad[:, :C0], xa.grad[:, :C0]) < 1e-12
    assert _rel(xb.grad[:, C0:, ::2, ::2, ::2], childsum(xa.grad[:, C0:])) < 1e-12  # the children sum sits on one child


# ---- the key -----------------------------------------------------------------------------------------------------------------------------
def test_the_key_implies_bf16_and_is_off_by_default():
    M = _m()
    m = M.UNet3D(**_SMALL)
    assert m.bf16_subpixel is False and not m.compute_bf16 and not m._get_engine().subpixel_bf16
    m = M.UNet3D(**_SMALL, bf16_subpixel=True)
    assert m.native_supported and m.bf16_subpixel is True and m.compute_bf16 and not m.compute_split
    e = m._get_engine()
    assert e.subpixel_bf16 and e.bf16
    m = M.UNet3D(**_SMALL, bf16_subpixel=True, compute_dtype="bf16")
    assert m.bf16_subpixel and m.compute_bf16
    m = M.UNet3D(**_SMALL, compute_dtype="bf16")  # the parent mode alone does not switch it on
    assert m.bf16_subpixel is False and not m._get_engine().subpixel_bf16
    assert M.get_model(dict(name="UNet3D", **_SMALL, bf16_subpixel=True)).bf16_subpixel


@pytest.mark.parametrize("dtype", ["fp32", "float32", "fp32_split"])
def test_a_contradicting_compute_dtype_names_the_key(dtype):
    with pytest.raises(ValueError, match="bf16_subpixel runs bf16"):
        _m().UNet3D(**_SMALL, bf16_subpixel=True, compute_dtype=dtype)


def test_a_2d_model_is_pointed_at_its_own_key():
    M = _m()
    for cls in (M.UNet2D, M.ResidualUNet2D):
        with pytest.raises(ValueError, match="native_2d_bf16_subpixel"):
            cls(**_SMALL, bf16_subpixel=True)


def test_hip_graph_is_refused_next_to_the_key():
    M = _m()
    with pytest.raises(ValueError, match="hip_graph is not available with bf16_subpixel"):
        M.UNet3D(**_SMALL, bf16_subpixel=True, hip_graph=True)
    assert M.UNet3D(**_SMALL, hip_graph=True, compute_dtype="bf16").hip_graph  # (the parent mode keeps its graph)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_BF16_SUBPIXEL", "1")
    m = M.UNet3D(**_SMALL)
    assert m.bf16_subpixel and m.compute_bf16
    m = M.UNet3D(**_SMALL, bf16_subpixel=False)  # the key wins
    assert not m.bf16_subpixel and not m.compute_bf16
    assert not M.UNet2D(**_SMALL).bf16_subpixel  # the environment only sets a 3-D model's default


@pytest.mark.parametrize("name", ["ResidualUNet3D", "ResidualUNetSE3D"])
def test_residual_nets_accept_the_key_and_list_no_level(name):
    M = _m()
    m = getattr(M, name)(in_channels=1, out_channels=1, f_maps=[32, 64, 128], num_groups=8, bf16_subpixel=True)
    assert m.bf16_subpixel and m.compute_bf16 and m.native_supported
    # (the residual executor has no sub-pixel table at all: its joins are transposed convolutions and sums)
    assert m._get_engine().bf16 and not SE.eligible_subpixel(m, (1, 1, 16, 32, 32))
    for up in ("deconv", "trilinear"):
        m = M.UNet3D(in_channels=1, out_channels=1, f_maps=[32, 64, 128], num_groups=8, upsample=up, bf16_subpixel=True)
        assert len(m._get_engine()._subpixel_layers((16, 32, 32))) == 0 and not SE.eligible_subpixel(m, (1, 1, 16, 32, 32))


def test_the_key_is_in_the_docstring_and_the_opt_in_keys():
    M = _m()
    assert "bf16_subpixel" in M._OPT_IN_KEYS
    assert "`bf16_subpixel: true`" in M.__doc__ and "U3D_BF16_SUBPIXEL" in M.__doc__


def test_entry_points_are_declared_in_the_header_and_bound():
    from pytorch3dunet_amd import _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # declared in include/u3d_subpix_bf16.h, the part of the header that u3d.h includes inside its extern "C" block
    assert re.search(r"^#include <u3d_subpix_bf16\.h>$", open(os.path.join(root, "include", "u3d.h")).read(), flags=re.M)
    header = open(os.path.join(root, "include", "u3d_subpix_bf16.h")).read()
    assert nat.PART_PATHS == (os.path.join(root, "include", "u3d_subpix_bf16.h"),) and nat.PART_SYMBOLS == ENTRY_POINTS
    lib = nat.get_lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in nat._PART_PROTOS and name not in nat._PROTOS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == nat._PART_PROTOS[name][1]
    from pytorch3dunet_amd._engine_conv import ConvLayers
    assert all(callable(getattr(ConvLayers, fn)) for fn in ConvLayers._RECORDED_ONLY["subpixel_bf16"])
    assert lib.u3d_version() == 128
    # host-only queries: the envelope
    assert lib.u3d_subpixel_bf16_packed_elems(64, 32, 0) == 64 * 64 * 32 == lib.u3d_subpixel_bf16_packed_elems(64, 32, 1)
    assert lib.u3d_subpixel_bf16_packed_elems(16, 32, 0) == 0 and lib.u3d_subpixel_bf16_packed_elems(32, 48, 0) == 0
    assert lib.u3d_subpixel_bf16_packed_elems(32, 32, 2) == 0


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def _bf16_levels(model, dhw):
    sub = model._get_engine()._subpixel_layers(dhw)
    return {wid: pair for wid, pair in sub.items() if sub.family_of(wid) == "subpixel_bf16"}


@pytest.mark.parametrize("f_maps,dhw,count", [
    (32, (16, 32, 32), 2), (32, (12, 20, 26), 1), (32, (11, 15, 19), 0),  # (12, 20, 26): the 6 -> 13 axis is n -> 2n + 1
    ([16, 32, 64], (16, 32, 32), 1), ([16, 32, 64], (12, 20, 26), 0), ([16, 32, 64], (11, 15, 19), 0),  # (see the module docstring)
    ([24, 48, 96], (16, 32, 32), 0), ([24, 48, 96], (12, 20, 26), 0)])
def test_the_restated_rule_is_the_engines(f_maps, dhw, count):
    M = _m()
    cfg = dict(in_channels=1, out_channels=1, f_maps=f_maps, num_levels=3, num_groups=4 if f_maps == [24, 48, 96] else 8)
    m = M.UNet3D(**cfg, bf16_subpixel=True)
    got = _bf16_levels(m, dhw)
    want = {id(conv.weight): pair for conv, pair in SE.eligible_subpixel(m, (1, 1) + dhw).items()}
    assert got == want and len(got) == count
    # a post-norm order has no eligible level, and without the key the bf16 mode lists none
    post = M.UNet3D(**cfg, layer_order="cgr", bf16_subpixel=True)
    assert not _bf16_levels(post, dhw) and not SE.eligible_subpixel(post, (1, 1) + dhw)
    off = M.UNet3D(**cfg, compute_dtype="bf16")
    assert not _bf16_levels(off, dhw)
    # ... and the levels outside `_cat_bf16` are listed exactly as without the key (the fp32 sub-pixel kernels)
    sub_on, sub_off = m._get_engine()._subpixel_layers(dhw), off._get_engine()._subpixel_layers(dhw)
    ids_on = {wid for wid in sub_on if sub_on.family_of(wid) != "subpixel_bf16"}
    assert len(ids_on) == len(sub_off) and all(sub_on.family_of(w) == "subpixel" for w in ids_on)


# ---- the emulation -------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _runs(i):
    """(plain, emulation without rounding, emulation) of model case i, computed once and shared"""
    if i not in _RUNS:
        cfg, shape = SE.MODEL_CASES[i]
        _, sd, x, target = SE.prep(cfg, shape)
        ln = SE.loss_name_of(cfg)
        _RUNS[i] = (SE.run(cfg, sd, x, target, ln, emulate=False), SE.run(cfg, sd, x, target, ln, emulate=True, rnd=SE.identity),
                    SE.run(cfg, sd, x, target, ln, emulate=True))
    return _RUNS[i]


@pytest.mark.parametrize("i", range(len(SE.MODEL_CASES)))
def test_without_rounding_the_emulation_is_the_plain_float64_run(i):
    cfg, shape = SE.MODEL_CASES[i]
    model, _, _, _ = SE.prep(cfg, shape)
    assert SE.eligible_subpixel(model, shape), "the case has no sub-pixel layer"
    plain, exact, _ = _runs(i)
    e_l, e_g = SE.distances(exact, plain)
    print(dict(test="bf16_subpixel3d_emulation_exact", case=i, logits=e_l, grad_l2=e_g))
    assert e_l < 1e-12 and e_g < 1e-12


@pytest.mark.parametrize("i", range(len(SE.MODEL_CASES)))
def test_the_emulation_alone_is_inside_two_thirds_of_the_bf16_bars(i):
    plain, _, emul = _runs(i)
    e_l, e_g = SE.distances(emul, plain)
    print(dict(test="bf16_subpixel3d_emulation_vs_plain", case=i, logits=e_l, grad_l2=e_g))
    assert e_l <= SE.BF16_LOGITS_TOL * 2 / 3 and e_g <= SE.BF16_GRAD_TOL * 2 / 3


# ---- the C-ABI as a whole, and the family `subpixel_bf16` in the executor's tables ---------------------------------------------------------------
def test_the_library_exports_exactly_what_the_header_and_its_part_declare():
    """u3d.h's own 250 declarations + the 8 of the part it includes = the u3d_* symbols of the shared library, no more and no fewer"""
    import shutil
    import subprocess

    from pytorch3dunet_amd import _native as nat

    assert nat.ALL_SYMBOLS == nat.EXPORTED_SYMBOLS + nat.PART_SYMBOLS and len(set(nat.ALL_SYMBOLS)) == len(nat.ALL_SYMBOLS) == 258
    lib = nat.get_lib()
    assert all(hasattr(lib, name) for name in nat.ALL_SYMBOLS)
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    if nm is not None:  # (without binutils the ctypes lookups above are the check)
        out = subprocess.run([nm, "-D", "--defined-only", nat.LIB_PATH], check=True, capture_output=True, text=True, timeout=60).stdout
        exported = {line.split()[-1] for line in out.splitlines() if re.search(r"\sT\s+u3d_[a-z0-9_]+$", line)}
        assert exported == set(nat.ALL_SYMBOLS)


def _sub_engine():
    m = _m().UNet3D(in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8, bf16_subpixel=True)
    return m, m._get_engine()


def test_the_family_is_recorded_and_backward_reads_it():
    """what tests/test_conv_family.py holds for the families of the three tables, for `subpixel_bf16`: forward names it from the `sub` table,
    backward's two families are the record's under every side-stream / debug setting, the scratch is the maximum of its three kernels'"""
    import types

    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd._engine_base import ConvRec, VSrc
    from pytorch3dunet_amd._engine_conv import ConvLayers, _ConvCall

    m, eng = _sub_engine()
    conv = m.decoders[0].basic_module.SingleConv1.conv
    sub = eng._subpixel_layers((8, 8, 8))  # one decoder, 32 + 64 -> 32 at exact 2x
    assert dict(sub) == {id(conv.weight): (32, 64)} and sub.family_of(id(conv.weight)) == "subpixel_bf16" and not sub.plus
    assert sub.family_of(id(object())) == sub.family == "subpixel"
    src = VSrc(torch.zeros(2, 8, 8, 8, 32), torch.zeros(2, 4, 4, 4, 64))
    call = _ConvCall(dev=None, conv=conv, src=src, affine=None, y=None, N=2, D=8, H=8, W=8, Ctot=96, Cout=32, relu=0, stats=False, pool=None,
                     residual=None, sub=sub, b16=False)
    assert eng._fwd_family(call, None) == "subpixel_bf16"
    assert eng._fwd_family(call, torch.zeros(1)) != "subpixel_bf16"  # (a residual in the epilogue: never a sub-pixel layer)
    rec = ConvRec(name="dec0.c1", src=src, affine=None, mean_rstd=None, y=torch.empty(0, 32), gn_w=None, conv_w=conv.weight, G=8,
                  family="subpixel_bf16", sub=(32, 64), plus=(0, 0, 0), c16=False)
    assert not rec.small
    for need_dg in (True, False):
        for voxels, debug in ((0, None), (1 << 30, None), (1 << 30, {})):
            eng.debug = debug
            try:
                assert eng._bwd_families(types.SimpleNamespace(SIDE_MAX_VOXELS=voxels), rec, need_dg) == ("subpixel_bf16", "subpixel_bf16")
            finally:
                eng.debug = None
    lib = nat.get_lib()
    want = max(lib.u3d_wgrad_bf16_workspace_floats(2, 8, 8, 8, 32, 32), lib.u3d_subpixel_wgrad_bf16_workspace_floats(2, 4, 4, 4, 64, 32),
               lib.u3d_conv3d_bf16_workspace_floats(2, 8, 8, 8, 32, 32))
    assert eng._wgrad_workspace_floats([rec]) == want > 0
    # the family's three launchers, and every row of the three tables, resolve through the one lookup
    assert set(ConvLayers._RECORDED_ONLY) == {"subpixel_bf16"} and not set(ConvLayers._RECORDED_ONLY) & set(ConvLayers._FWD_KERNELS)
    assert [eng._launcher(i, "subpixel_bf16").__name__ for i in range(3)] == ["_fwd_subpixel_bf16", "_dgrad_subpixel_bf16", "_wgrad_subpixel_bf16"]
    for i, table in enumerate((ConvLayers._FWD_KERNELS, ConvLayers._DGRAD_KERNELS, ConvLayers._WGRAD_KERNELS)):
        assert all(eng._launcher(i, family).__name__ == fn for family, fn in table.items())


def test_the_image_cache_lists_the_four_images_of_a_sub_pixel_layer():
    from pytorch3dunet_amd._engine_weights import _KINDS, _SUB_KINDS, Kind, WeightImages

    skip, up, slab = _SUB_KINDS[(Kind.BF16_FWD, Kind.BF16_DGRAD)]
    assert skip == (Kind.SKIP_BF16_FWD, Kind.SKIP_BF16_DGRAD) and up == (Kind.UP_BF16_FWD, Kind.UP_BF16_DGRAD) and slab is None
    assert [_KINDS[k].entry for k in skip + up] == ["u3d_pack_weights_bf16_slice"] * 2 + ["u3d_pack_subpixel_weights_bf16"] * 2
    assert [(_KINDS[k].half, _KINDS[k].mode, _KINDS[k].up_args) for k in skip + up] == [(0, 0, False), (0, 1, False), (1, 0, True), (1, 1, True)]
    m, eng = _sub_engine()
    w = m.decoders[0].basic_module.SingleConv1.conv.weight
    sub = eng._subpixel_layers((8, 8, 8))
    assert WeightImages._layer_kinds(w, 2, (Kind.BF16_FWD, Kind.BF16_DGRAD), sub) == ((32, 64), skip + up)
    assert WeightImages._layer_kinds(w, 1, (Kind.BF16_FWD, Kind.BF16_DGRAD), sub) == ((32, 64), skip[:1] + up[:1])
    assert any(x is w for x in eng.images._bf16)  # (the list whose layers `_repack_bf16` packs: the four images replace the BF16_* pair)
