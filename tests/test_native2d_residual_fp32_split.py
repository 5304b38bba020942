"""CPU side of `native_2d_residual_fp32_split: true` / U3D_NATIVE_2D_RESIDUAL_FP32_SPLIT=1 (a ResidualUNet2D in fp32_split): the key's row
and what `resolve` makes of it, the executor's routing held against its restatement in tests/f32s_emul_res2d.py on an engine built on the
CPU (a whole forward with the native call recorded instead of issued), and the binding of u3d_conv2d_f32s_res from include/u3d_ext.h."""
import ctypes
import os
import re

import pytest
import torch

import f32s_emul_res2d as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
_ROUTED = dict(in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8)
_MIXED = dict(in_channels=1, out_channels=1, f_maps=[16, 32, 64], num_groups=8)
KEY = FR.KEY
ENV = "U3D_NATIVE_2D_RESIDUAL_FP32_SPLIT"


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


# ---- the key -----------------------------------------------------------------------------------------------------------------------------
def test_the_row_and_its_position():
    from pytorch3dunet_amd.unet3d import native2d
    from pytorch3dunet_amd.unet3d.buildingblocks import ResNetBlock

    k = native2d._BY_NAME[KEY]
    assert (k.name, k.env, k.block, k.implies, k.precision, k.refuses, k.kernels) == (
        KEY, ENV, ResNetBlock, "native_2d_residual", "fp32_split", None, "u3d_conv2d_f32s.h")
    assert native2d.NAMES.index(KEY) == native2d.NAMES.index("native_2d_residual") - 1  # a key stands before the key it implies
    M = _m()
    assert KEY in M._OPT_IN_KEYS
    row = next(line for line in native2d.TABLE.splitlines() if line.strip().startswith(KEY + " "))
    assert ENV in row and "ResidualUNet2D" in row and "native_2d_residual " in row and "fp32_split" in row and "u3d_conv2d_f32s.h" in row
    assert row in M.__doc__


def test_the_key_implies_the_residual_path_and_fp32_split():
    M = _m()
    m = M.ResidualUNet2D(**_ROUTED, **{KEY: True})
    assert m.native_2d_residual_fp32_split is True and m.native_2d_residual is True and m.native_2d is True
    assert m.compute_split is True and not m.compute_bf16
    assert m.native_supported and m._native_blockers == []  # the "2-D model with compute_dtype" blocker does not fire
    assert m.native_2d_fp32_split is False and m.native_2d_residual_bf16 is False  # (the other keys' attributes stay what they were)
    assert M.ResidualUNet2D(**_ROUTED, **{KEY: True}, compute_dtype="fp32_split").native_supported
    assert M.get_model(dict(name="ResidualUNet2D", **_ROUTED, **{KEY: True})).native_2d_residual_fp32_split
    # off by default; compute_dtype fp32_split without the key stays blocked
    m = M.ResidualUNet2D(**_ROUTED, native_2d_residual=True)
    assert m.native_2d_residual_fp32_split is False and not m.compute_split and m.native_supported
    m = M.ResidualUNet2D(**_ROUTED, native_2d_residual=True, compute_dtype="fp32_split")
    assert not m.native_supported and any("2-D model with compute_dtype 'fp32_split'" in r for r in m._native_blockers)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv(ENV, "1")
    m = M.ResidualUNet2D(**_SMALL)
    assert m.native_2d_residual_fp32_split and m.native_2d_residual and m.native_2d and m.compute_split and m.native_supported
    m = M.ResidualUNet2D(**_SMALL, **{KEY: False})  # the key wins
    assert not m.native_2d_residual_fp32_split and not m.native_2d_residual and not m.native_2d and not m.compute_split
    for other in (M.UNet2D, M.UNet3D, M.ResidualUNet3D):  # other classes ignore the variable too
        o = other(**_SMALL)
        assert not o.compute_split and not o.native_2d and o.native_2d_residual_fp32_split is False


@pytest.mark.parametrize("dtype", ["fp32", "float32", "bf16", "bfloat16"])
def test_a_contradicting_compute_dtype_names_the_fp32_path(dtype):
    with pytest.raises(ValueError) as ei:
        _m().ResidualUNet2D(**_SMALL, **{KEY: True}, compute_dtype=dtype)
    msg = str(ei.value)
    assert msg.startswith(f"u3d: {KEY} runs fp32_split operands; compute_dtype '{dtype}' contradicts it")
    assert "(native_2d_residual: true is the fp32 2-D path)" in msg


@pytest.mark.parametrize("other", ["native_2d_residual_bf16", "native_2d_residual_bf16_deconv"])
def test_a_residual_bf16_key_next_to_it_names_both_keys(other):
    with pytest.raises(ValueError) as ei:
        _m().ResidualUNet2D(**_SMALL, **{KEY: True, other: True})
    msg = str(ei.value)
    assert msg == f"u3d: {other} runs bf16 operands and {KEY} runs fp32_split operands — drop one of the two keys"


@pytest.mark.parametrize("kw", [dict(hip_graph=True), dict(checkpoint_encoders=True), dict(checkpoint_encoders=True, checkpoint_levels=1)])
def test_graph_and_checkpointing_stay_refused(kw):
    with pytest.raises(ValueError, match="hip_graph" if "hip_graph" in kw else "checkpoint"):
        _m().ResidualUNet2D(**_SMALL, **{KEY: True}, **kw)


@pytest.mark.parametrize("name", ["UNet2D", "UNet3D", "ResidualUNet3D", "ResidualUNetSE3D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    with_key, without = getattr(M, name)(**_SMALL, **{KEY: True}), getattr(M, name)(**_SMALL)
    for a in ("native_2d", "native_2d_residual", "native_2d_fp32_split", KEY, "compute_split", "compute_bf16", "native_supported",
              "_native_blockers"):
        assert getattr(with_key, a) == getattr(without, a), a
    assert getattr(with_key, KEY) is False
    assert getattr(M, name)(**_SMALL, **{KEY: True}, compute_dtype="bf16").compute_bf16  # ... a contradicting compute_dtype included
    u = M.UNet2D(**_SMALL, **{KEY: True}, native_2d=True)
    assert u.native_supported and not u.compute_split and not u._get_engine().split2d


# ---- the executor, built on the CPU --------------------------------------------------------------------------------------------------------
SPLIT_FWD = ("u3d_conv2d_f32s", "u3d_conv2d_f32s_res")
FP32_FWD = ("u3d_conv2d_ex_reps", "u3d_conv2d_res_reps")


def _forward_recorded(model, shape, monkeypatch):
    """a whole forward on the CPU with the native call recorded instead of issued: (the tape, [(name, args)])"""
    from pytorch3dunet_amd import _engine_conv as EC
    from pytorch3dunet_amd import _engine_res as ER
    from pytorch3dunet_amd import _engine_unet as EU
    from pytorch3dunet_amd import _engine_weights as EW
    from pytorch3dunet_amd import _native as nat

    issued = []
    monkeypatch.setattr(nat, "call", lambda name, *args, flops=0.0: issued.append((name, args)))
    for mod in (EC, EU, EW, ER):
        monkeypatch.setattr(mod, "_stream", lambda dev: None)
    _, _, tape = model._get_engine().forward(torch.zeros(shape), True)
    return tape, issued


@pytest.mark.parametrize("order", ["gcr", "gce", "cge", "cr"])
def test_the_restated_rule_is_the_engines(order, monkeypatch):
    from pytorch3dunet_amd import _native as nat

    M = _m()
    on = M.ResidualUNet2D(**_MIXED, layer_order=order, **{KEY: True})
    want = FR.routed(on)
    assert [w for _, w, _ in want] == [32, 32, 64, 64, 32, 32]  # conv2, conv3 of encoders.1, encoders.2, decoders.0; not the 16-wide blocks
    assert [r for _, _, r in want] == [False, FR.pre_norm(order)] * 3
    eng = on._get_engine()
    assert eng.split2d is True and eng.is2d is True and eng.split is False and eng.bf16 is False
    # the restated rule gives exactly the weights that are missing from the fp32 image list
    named = dict(on.named_parameters())
    routed_ids = {id(named[n]) for n, _, _ in want}
    assert eng._split2d_weights() == routed_ids
    assert {id(w) for w in eng.images._each} == {id(c.weight) for c in FR.conv3x3(on)} - routed_ids
    assert eng.images._each_bf16 == [] and eng.images._each_bf16_c16 == []
    # a forward: per routed layer one six-product launch, `_res` exactly where the restated rule puts the residual into the epilogue
    tape, issued = _forward_recorded(on, (1, 1, 35, 45), monkeypatch)
    names = {id(p): n for n, p in on.named_parameters()}
    assert [(names[id(r.conv_w)], r.y.shape[-1]) for r in tape.convs if r.f32s] == [(n, w) for n, w, _ in want]
    assert all(r.family == "conv2d" for r in tape.convs)
    got = [n for n, _ in issued if n in SPLIT_FWD + FP32_FWD]
    res = iter(want)
    expect = []
    for r in tape.convs:
        if r.f32s:
            expect.append("u3d_conv2d_f32s_res" if next(res)[2] else "u3d_conv2d_f32s")
        else:
            expect.append("u3d_conv2d_res_reps" if (r.name.endswith(".c3") and FR.pre_norm(order)) else "u3d_conv2d_ex_reps")
    assert got == expect
    for n, a in issued:
        if n == "u3d_conv2d_f32s_res":  # (device, stream, x, affine, packed_w, out, N, H, W, Cin, Cout, relu, out_stats, stat_reps, residual)
            assert len(a) == 15 and a[9] == a[10] and a[9] % 32 == 0 and a[14] is not None
            assert a[11] == (1 if order == "gcr" else 0)  # `e`: the epilogue runs without ReLU, the activation pass follows
    all_names = [n for n, _ in issued]
    assert all_names.count("u3d_pack_weights2d_f32s") == len(want)  # (forward images; the data gradient's are packed when first asked for)
    if order == "gce":
        assert all_names.count("u3d_act_fwd") >= len(tape.convs) // 2
    monkeypatch.undo()

    # `native_2d_residual` alone: every launch is the fp32 path's and the extension library is never asked for
    def boom():
        raise AssertionError("the extension library was loaded with the key off")

    monkeypatch.setattr(nat, "get_ext_lib", boom)
    off = M.ResidualUNet2D(**_MIXED, layer_order=order, native_2d_residual=True)
    eng = off._get_engine()
    assert eng.split2d is False and eng._split2d_weights() == set() and not eng._split2d_counts(32, 0, 32)
    assert len(eng.images._each) == len(FR.conv3x3(off))
    tape, issued = _forward_recorded(off, (1, 1, 35, 45), monkeypatch)
    assert not any(r.f32s for r in tape.convs) and not any("f32s" in n for n, _ in issued)
    assert eng._wgrad_workspace_floats(tape.convs) > 0 and eng._layer_ws_floats(2, 1, 40, 56, 32, 32) > 0


def test_the_scratch_of_a_routed_layer_is_the_extensions_plan():
    from pytorch3dunet_amd import _native as nat

    M = _m()
    on = M.ResidualUNet2D(**_MIXED, **{KEY: True})._get_engine()
    lib, ext = nat.get_lib(), nat.get_ext_lib()
    shape = (2, 1, 40, 56)
    plan = ext.u3d_wgrad2d_f32s_workspace_floats(2, 40, 56, 32, 32)
    core = max(lib.u3d_wgrad2d_workspace_floats(2, 40, 56, 32, 32), lib.u3d_conv2d_workspace_floats(2, 40, 56, 32, 32))
    assert plan > 0 and plan % (9 * 32 * 32) == 0
    assert on._family_ws_floats("conv2d", *shape, 32, 32, f32s=True) == plan
    assert on._layer_ws_floats(*shape, 32, 32) == plan
    assert on._layer_ws_floats(*shape, 16, 16) == max(lib.u3d_wgrad2d_workspace_floats(2, 40, 56, 16, 16),
                                                      lib.u3d_conv2d_workspace_floats(2, 40, 56, 16, 16))
    off = M.ResidualUNet2D(**_MIXED, native_2d_residual=True)._get_engine()
    assert off._layer_ws_floats(*shape, 32, 32) == core


def test_compute_split_is_no_blocker_on_a_fully_routed_net():
    m = _m().ResidualUNet2D(**_ROUTED, **{KEY: True})
    assert m.compute_split and m.native_supported and m._native_blockers == []
    assert len(FR.routed(m)) == 6 == len(FR.conv3x3(m)) and m._get_engine().images._each == []


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_read_from_the_header_exported_typed_and_absent_from_the_core():
    from pytorch3dunet_amd import _native as nat

    name = FR.NEW_NAME
    i, vp = ctypes.c_int, ctypes.c_void_p
    # (device, stream, x, affine, packed_w, out, N, H, W, Cin, Cout, relu, out_stats, stat_reps, residual)
    assert nat._EXT_PROTOS[name] == (i, [i, vp] + [vp] * 4 + [i] * 6 + [vp, i, vp])
    order = list(nat._EXT_PROTOS)
    assert order.index(name) == order.index("u3d_conv2d_f32s_supported") - 1  # declared before the `native_2d_fp32_split` block
    path = os.path.join(ROOT, "include", "u3d_ext.h")
    assert "#" not in re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)  # still a header part
    lib = nat.get_ext_lib()
    fn = getattr(lib, name)
    assert (fn.restype, fn.argtypes) == nat._EXT_PROTOS[name]
    assert name not in nat.ALL_SYMBOLS and not hasattr(nat.get_lib(), name)
    assert lib.u3d_ext_version() == nat.U3D_EXT_VERSION == 2 and nat.get_lib().u3d_version() == 128
    assert len(nat.EXPORTED_SYMBOLS) == 250  # (the core header is untouched)
    # a refusal needs no device: outside the envelope nothing is looked at but the counts
    buf = (ctypes.c_float * 4)()
    assert lib.u3d_conv2d_f32s_res(0, None, buf, None, buf, buf, 1, 8, 8, 8, 32, 0, None, 1, buf) != nat.U3D_OK
    assert lib.u3d_conv2d_f32s_res(0, None, buf, None, buf, buf, 1, 8, 8, 32, 48, 0, None, 1, buf) != nat.U3D_OK
