"""CPU side of `native_2d_fp32_split: true` / U3D_NATIVE_2D_FP32_SPLIT=1 (a UNet2D in fp32_split): the key — what it implies, refuses and
leaves unchanged —, the executor's one routing rule (`_split2d`, decided in forward, kept in `ConvRec.f32s`, read by the three `conv2d`
launchers) held against its restatement in tests/f32s_emul_2d.py on an engine built on the CPU (a whole forward with the native call
recorded instead of issued, then the two backward launchers on every record), the binding of the new entry points from
include/u3d_ext.h, their host-only answers, and the arithmetic the kernels are built on."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import f32s_emul_2d as FE2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
KEY = "native_2d_fp32_split"


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


# ---- the key -----------------------------------------------------------------------------------------------------------------------------
def test_the_key_implies_native_2d_and_fp32_split_and_is_off_by_default():
    M = _m()
    m = M.UNet2D(**_SMALL, native_2d=True)
    assert m.native_2d_fp32_split is False and not m.compute_split
    e = m._get_engine()
    assert e.split2d is False and e.split is False
    m = M.UNet2D(**_SMALL, **{KEY: True})
    assert m.native_2d_fp32_split is True and m.native_2d is True and m.compute_split is True and not m.compute_bf16
    assert m.native_supported and m._native_blockers == []  # the "2-D model with compute_dtype" blocker does not fire
    e = m._get_engine()
    assert e.split2d is True and e.is2d is True and e.split is False and e.bf16 is False  # `split` is the 3-D flag
    assert M.UNet2D(**_SMALL, **{KEY: True}, compute_dtype="fp32_split").native_supported
    assert M.get_model(dict(name="UNet2D", **_SMALL, **{KEY: True})).native_2d_fp32_split
    # compute_dtype fp32_split WITHOUT the key stays blocked, with the text the matrix fixture pins
    m = M.UNet2D(**_SMALL, native_2d=True, compute_dtype="fp32_split")
    assert not m.native_supported and any("2-D model with compute_dtype 'fp32_split'" in r for r in m._native_blockers)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_NATIVE_2D_FP32_SPLIT", "1")
    m = M.UNet2D(**_SMALL)
    assert m.native_2d_fp32_split and m.native_2d and m.compute_split and m.native_supported
    m = M.UNet2D(**_SMALL, **{KEY: False})  # the key wins
    assert not m.native_2d_fp32_split and not m.native_2d and not m.compute_split


@pytest.mark.parametrize("dtype", ["fp32", "float32", "bf16", "bfloat16"])
def test_a_contradicting_compute_dtype_is_the_tables_precision_error(dtype):
    with pytest.raises(ValueError, match=f"u3d: {KEY} runs fp32_split operands; compute_dtype '{dtype}' contradicts it"):
        _m().UNet2D(**_SMALL, **{KEY: True}, compute_dtype=dtype)


@pytest.mark.parametrize("other", ["native_2d_bf16", "native_2d_bf16_vcat", "native_2d_bf16_subpixel"])
def test_a_bf16_key_next_to_it_names_both_keys(other):
    with pytest.raises(ValueError) as ei:
        _m().UNet2D(**_SMALL, **{KEY: True, other: True})
    msg = str(ei.value)
    assert KEY in msg and other in msg and "runs bf16 operands" in msg and "runs fp32_split operands" in msg
    assert "compute_dtype" not in msg  # not the misleading "compute_dtype 'bf16' contradicts it"


def test_the_sub_pixel_keys_are_refused_through_the_rows_refuses_field():
    M = _m()
    from pytorch3dunet_amd.unet3d import native2d

    assert native2d._BY_NAME[KEY].refuses[0] == "native_2d_subpixel"
    with pytest.raises(ValueError, match=f"u3d: {KEY} is the fp32_split 2-D path.*; native_2d_subpixel contradicts it"):
        M.UNet2D(**_SMALL, **{KEY: True}, native_2d_subpixel=True)
    with pytest.raises(ValueError, match=f"u3d: {KEY} is the fp32_split 2-D path.*; native_2d_subpixel_plus contradicts it"):
        M.UNet2D(**_SMALL, **{KEY: True}, native_2d_subpixel_plus=True)  # inherits the refusal


def test_the_stem_key_composes_and_hip_graph_is_refused():
    M = _m()
    m = M.UNet2D(**_SMALL, **{KEY: True}, native_2d_stem=True)
    assert m.native_supported and m.native_2d_stem and m.compute_split
    e = m._get_engine()
    assert e.stem and e.split2d and e._small2d(1, 16, False) and not e._split2d_counts(16, 0, 32) and e._split2d_counts(32, 0, 32)
    with pytest.raises(ValueError, match="hip_graph is not available with native_2d"):
        M.UNet2D(**_SMALL, **{KEY: True}, hip_graph=True)


@pytest.mark.parametrize("name", ["UNet3D", "ResidualUNet3D", "ResidualUNetSE3D", "ResidualUNet2D"])
def test_other_classes_ignore_the_key(name):
    M = _m()
    cfg = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
    with_key, without = getattr(M, name)(**cfg, **{KEY: True}), getattr(M, name)(**cfg)
    for a in ("native_2d", "native_2d_fp32_split", "compute_split", "compute_bf16", "native_supported", "_native_blockers"):
        assert getattr(with_key, a) == getattr(without, a), a
    assert with_key.native_2d_fp32_split is False
    # ... a contradicting compute_dtype next to it included
    assert getattr(M, name)(**cfg, **{KEY: True}, compute_dtype="bf16").compute_bf16


def test_the_key_is_in_the_table_and_the_model_docstring():
    M = _m()
    from pytorch3dunet_amd.unet3d import native2d

    assert KEY in native2d.NAMES and KEY in M._OPT_IN_KEYS
    row = next(line for line in native2d.TABLE.splitlines() if line.strip().startswith(KEY + " "))
    assert "U3D_NATIVE_2D_FP32_SPLIT" in row and "UNet2D" in row and "fp32_split" in row and "u3d_conv2d_f32s.h" in row
    assert row in M.__doc__
    assert os.path.exists(os.path.join(ROOT, "pytorch-3dunet_amd", "csrc", "u3d_conv2d_f32s.h"))
    assert native2d._DTYPE_NAMES["fp32_split"] == ("fp32_split",)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
NEW_CALLS = ("u3d_conv2d_f32s", "u3d_conv2d_f32s_dgrad", "u3d_conv2d_wgrad_f32s")
OLD_CALLS = ("u3d_conv2d_ex_reps", "u3d_conv2d_wgrad")


def _engine_routed(model, shape, monkeypatch):
    """what the engine issues per 3x3 layer of `model` on an input of `shape`, with the native call recorded instead of issued: a whole
    forward on the CPU (which decides and records), then the data-gradient and the weight-gradient launcher of every record.  Returns
    ([(weight name, C0, C1, Cout)] of the layers on the new kernels, the recorded call names); checks per layer that all three directions
    go the same way and that a routed weight-gradient launch leaves the GroupNorm-backward job alone."""
    from pytorch3dunet_amd import _engine_conv as EC
    from pytorch3dunet_amd import _engine_unet as EU
    from pytorch3dunet_amd import _engine_weights as EW
    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd._engine_base import _StatPool

    eng = model._get_engine()
    issued = []
    monkeypatch.setattr(nat, "call", lambda name, *args, flops=0.0: issued.append((name, args)))
    for mod in (EC, EU, EW):
        monkeypatch.setattr(mod, "_stream", lambda dev: None)
    names = {id(p): n for n, p in model.named_parameters()}
    _, _, tape = eng.forward(torch.zeros(shape), True)
    fwd = [(n, a) for n, a in issued if n in NEW_CALLS + OLD_CALLS]
    all_names = [n for n, _ in issued]
    assert len(fwd) == len(tape.convs) - sum(r.family == "small2d" for r in tape.convs)
    out = []
    cpu = torch.device("cpu")
    for rec in tape.convs:
        if rec.family != "conv2d":
            assert not rec.f32s
            continue
        src, Cout = rec.src, rec.y.shape[-1]
        cx = types.SimpleNamespace(dev=cpu, ws=torch.zeros(4), gview=lambda i: torch.zeros(1), ensure_ws=lambda n: torch.zeros(4),
                                   pool=_StatPool(cpu, 1 << 14))
        job = object()
        c = EC._BwdCall(cx, rec, torch.zeros(src.N, 1, src.H, src.W, Cout), src, src.N, 1, src.H, src.W, Cout, False, job=job)
        del issued[:]
        eng._launcher(1, "conv2d")(c)
        eng._launcher(2, "conv2d")(c)
        got = [n for n, _ in issued if n in NEW_CALLS + OLD_CALLS]
        assert c.job is job  # (the conv2d weight gradients take no job, routed or not)
        if rec.f32s:
            assert got == ["u3d_conv2d_f32s_dgrad", "u3d_conv2d_wgrad_f32s"], (rec.name, got)
            a = issued[-1][1]  # (device, stream, p0, p1, ymap, xmap, C0, C1, H1, W1, ...)
            assert (a[3] is None) == (src.t1 is None) and a[6] + a[7] == src.C
            out.append((names[id(rec.conv_w)], a[6], a[7], Cout))
        else:
            assert got == ["u3d_conv2d_ex_reps", "u3d_conv2d_wgrad"], (rec.name, got)
        all_names += [n for n, _ in issued]
    # the forward launches went the same way, layer by layer
    routed_fwd = [a[6:8] + (a[16],) for n, a in fwd if n == "u3d_conv2d_f32s"]
    assert routed_fwd == [(c0, c1, co) for _, c0, c1, co in out]
    return out, all_names


RULE_CASES = [  # (model keywords, input shape, layers on the new kernels)
    (dict(f_maps=[32, 64, 128], num_groups=8), (1, 1, 40, 56), 8),   # not 1 -> 16, 16 -> 32; both decoders' virtual concats
    (dict(f_maps=32, num_levels=4, num_groups=8), (1, 1, 67, 45), 12),  # n -> 2n + 1 levels: the general nearest tables
    (dict(f_maps=[20, 40], num_groups=2), (1, 1, 24, 20), 0),        # nothing routed
]


@pytest.mark.parametrize("kw,shape,count", RULE_CASES)
def test_the_restated_rule_is_the_engines(kw, shape, count, monkeypatch):
    from pytorch3dunet_amd import _native as nat

    M = _m()
    cfg = dict(in_channels=1, out_channels=1, **kw)
    on = M.UNet2D(**cfg, **{KEY: True})
    want = FE2.routed(on)
    assert len(want) == count
    if kw["f_maps"] == [32, 64, 128]:
        assert ("decoders.1.basic_module.SingleConv1.conv.weight", 32, 64, 32) in want  # the 96 -> 32 virtual concat at full resolution
        assert ("decoders.0.basic_module.SingleConv1.conv.weight", 64, 128, 64) in want
        assert not any(n.startswith("encoders.0.") for n, _, _, _ in want)
    got, names = _engine_routed(on, shape, monkeypatch)
    assert got == want
    eng = on._get_engine()
    assert {id(p) for n, p in on.named_parameters() if n in {w for w, _, _, _ in want}} == eng._split2d_weights()
    assert [w for w in eng.images._each if id(w) in eng._split2d_weights()] == []  # routed layers get no fp32 images up front
    if count == 0:
        assert not any(n in NEW_CALLS + ("u3d_pack_weights2d_f32s",) for n in names)
    else:
        assert names.count("u3d_pack_weights2d_f32s") == 2 * count  # forward and data-gradient images, of the routed layers only
    monkeypatch.undo()

    # key off: every launch is today's and the extension library is never asked for
    def boom():
        raise AssertionError("the extension library was loaded with the key off")

    monkeypatch.setattr(nat, "get_ext_lib", boom)
    off = M.UNet2D(**cfg, native_2d=True)
    assert FE2.routed(off, key=False) == []
    got, names = _engine_routed(off, shape, monkeypatch)
    assert got == [] and not any(n in NEW_CALLS + ("u3d_pack_weights2d_f32s",) for n in names)
    assert off._get_engine()._split2d_weights() == set()


def test_the_scratch_asks_the_new_plan_under_the_key_only(monkeypatch):
    from pytorch3dunet_amd import _native as nat

    M = _m()
    cfg = dict(in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8)
    on = M.UNet2D(**cfg, **{KEY: True})._get_engine()
    lib, ext = nat.get_lib(), nat.get_ext_lib()
    shape = (2, 1, 40, 56)
    plan = ext.u3d_wgrad2d_f32s_workspace_floats(2, 40, 56, 32, 32)
    core = max(lib.u3d_wgrad2d_workspace_floats(2, 40, 56, 32, 32), lib.u3d_conv2d_workspace_floats(2, 40, 56, 32, 32))
    assert plan > 0 and plan % (9 * 32 * 32) == 0
    assert on._family_ws_floats("conv2d", *shape, 32, 32, f32s=True) == plan
    assert on._family_ws_floats("conv2d", *shape, 32, 32) == core
    assert on._layer_ws_floats(*shape, 32, 32) == plan and on._layer_ws_floats(*shape, 16, 32) == max(
        lib.u3d_wgrad2d_workspace_floats(2, 40, 56, 16, 32), lib.u3d_conv2d_workspace_floats(2, 40, 56, 32, 16))
    off = M.UNet2D(**cfg, native_2d=True)._get_engine()

    def boom():
        raise AssertionError("the extension library was loaded with the key off")

    monkeypatch.setattr(nat, "get_ext_lib", boom)
    assert off._layer_ws_floats(*shape, 32, 32) == core and not off._split2d_counts(32, 0, 32)


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------
def test_the_new_names_are_read_from_the_header_exported_typed_and_absent_from_the_core():
    from pytorch3dunet_amd import _native as nat

    path = os.path.join(ROOT, "include", "u3d_ext.h")
    protos = nat.read_part(path, {**nat._PROTOS, **nat._PART_PROTOS})
    assert protos == nat._EXT_PROTOS
    assert "#" not in re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)  # still a header part: declarations and comments only
    assert tuple(protos)[-len(FE2.NEW_NAMES):] == FE2.NEW_NAMES  # appended, in the issue's order
    lib = nat.get_ext_lib()
    for name in FE2.NEW_NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == protos[name], name
        assert name not in nat.ALL_SYMBOLS and not hasattr(nat.get_lib(), name), name
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    assert protos["u3d_conv2d_f32s_supported"] == protos["u3d_conv2d_wgrad_f32s_supported"] == (i, [i, i])
    assert protos["u3d_packed_weight2d_f32s_elems"] == (ll, [i, i, i])
    assert protos["u3d_pack_weights2d_f32s"] == (i, [i, vp, vp, i, i, i, vp])
    assert protos["u3d_conv2d_f32s"] == (i, [i, vp] + [vp] * 4 + [i] * 4 + [vp] * 3 + [i] * 5 + [vp, i])
    assert protos["u3d_conv2d_f32s_dgrad"] == (i, [i, vp, vp, vp, vp] + [i] * 4 + [vp] * 4 + [i] * 4 + [vp, i])
    assert protos["u3d_wgrad2d_f32s_workspace_floats"] == (ll, [i] * 5)
    assert protos["u3d_conv2d_wgrad_f32s"] == (i, [i, vp] + [vp] * 4 + [i] * 4 + [vp] * 3 + [i] * 4 + [vp, ll])
    assert lib.u3d_ext_version() == nat.U3D_EXT_VERSION == 2 and nat.get_lib().u3d_version() == 128
    assert len(nat.EXPORTED_SYMBOLS) == 250  # (the core header is untouched)


def test_a_stale_extension_library_raises_the_rebuild_error(monkeypatch):
    from pytorch3dunet_amd import _native as nat

    monkeypatch.setattr(nat, "_ext_lib", None)
    monkeypatch.setattr(nat, "_EXT_PROTOS", {**nat._EXT_PROTOS, "u3d_a_name_the_library_lacks": (ctypes.c_int, [])})
    with pytest.raises(nat.U3DError, match="does not export u3d_a_name_the_library_lacks.*rebuild it"):
        nat.get_ext_lib()


def test_host_only_answers():
    from pytorch3dunet_amd import _native as nat

    lib = nat.get_ext_lib()
    pairs = ((32, 32), (16, 32), (32, 16), (24, 32), (0, 32))
    assert [lib.u3d_conv2d_f32s_supported(k, n) for k, n in pairs] == [1, 1, 0, 0, 0]  # contraction % 16, produced % 32
    assert [lib.u3d_conv2d_wgrad_f32s_supported(ci, co) for ci, co in pairs] == [1, 0, 0, 0, 0]  # both % 32
    for ci, co in pairs:
        for mode in (0, 1):
            n = lib.u3d_packed_weight2d_f32s_elems(ci, co, mode)
            k, nn = (ci, co) if mode == 0 else (co, ci)
            assert n == (3 * 9 * k * nn if lib.u3d_conv2d_f32s_supported(k, nn) else 0), (ci, co, mode)
        ws = lib.u3d_wgrad2d_f32s_workspace_floats(2, 21, 37, ci, co)
        if lib.u3d_conv2d_wgrad_f32s_supported(ci, co):
            assert ws > 0 and ws % (9 * ci * co) == 0
        else:
            assert ws == 0
    assert lib.u3d_packed_weight2d_f32s_elems(32, 32, 2) == 0
    assert lib.u3d_wgrad2d_f32s_workspace_floats(0, 8, 8, 32, 32) == 0 and lib.u3d_wgrad2d_f32s_workspace_floats(1, 1 << 16, 1 << 16, 32, 32) == 0
    # a refusal needs no device: outside the envelope nothing is looked at but the counts
    buf = (ctypes.c_float * 4)()
    assert lib.u3d_conv2d_f32s(0, None, buf, None, None, None, 24, 0, 0, 0, None, buf, buf, 1, 8, 8, 32, 0, None, 1) != nat.U3D_OK
    assert lib.u3d_conv2d_f32s_dgrad(0, None, buf, buf, buf, 1, 8, 8, 32, None, None, None, None, 48, 0, 0, 0, None, 1) != nat.U3D_OK
    assert lib.u3d_conv2d_wgrad_f32s(0, None, buf, None, None, None, 16, 0, 0, 0, None, buf, buf, 1, 8, 8, 32, buf, 4) != nat.U3D_OK


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------------
def test_the_six_partial_convolutions_are_fp32_grade():
    """32 -> 32 at 9 x 11: the float64 convolution of the split operands against the plain float64 convolution, within 2^-22 of the
    output's largest magnitude (each dropped product class is below 2^-24 of its product; 288 of them add up at random signs)"""
    import f32s_emul as FE

    # the kernels' product order is the emulation's: (A part, B part) per class, smallest class first, in both kernels of the header
    text = open(os.path.join(ROOT, "pytorch-3dunet_amd", "csrc", "u3d_conv2d_f32s.h")).read()
    orders = re.findall(r"PA\[6\] = \{([\d, ]+)\}, PB\[6\] = \{([\d, ]+)\}", text)
    assert len(orders) == 2
    for pa, pb in orders:
        pairs = list(zip(map(int, pa.split(",")), map(int, pb.split(","))))
        assert sorted(pairs) == sorted(FE.PRODUCTS)  # the same six products ...
        assert [a + b for a, b in pairs] == [2, 2, 2, 1, 1, 0]  # ... the 2^-16 class first, hh last (h = 0, m = 1, l = 2)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 32, 9, 11, generator=g) * (1.0 + 3.0 * torch.rand(1, 32, 1, 1, generator=g))
    w = torch.randn(32, 32, 3, 3, generator=g) / (9 * 32) ** 0.5
    exact = F.conv2d(x.double(), w.double(), None, padding=1)
    err = (FE2.conv2d_six_products(x, w) - exact).abs().max().item() / exact.abs().max().item()
    print(dict(test="conv2d_six_products", worst_in_units_of_2_pow_minus_24=err * 2.0 ** 24))
    assert err <= 2.0 ** -22
    # ... and negating the weight (the images' (-1)^chunk) negates every part exactly
    assert torch.equal(FE2.conv2d_six_products(x, -w), -FE2.conv2d_six_products(x, w))
