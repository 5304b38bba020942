"""CPU side of the opt-in split weight gradient (`fp32_split_wgrad: true` / U3D_F32_SPLIT_WGRAD=1): the key — what it implies, refuses and
leaves unchanged —, the executor's one routing rule (`_split_wgrad`, asked inside `_wgrad_fp32` and `_wgrad_subpixel`) held against its
restatement in tests/f32s_emul.py on an engine built on the CPU (the launchers run with the native call recorded instead of issued), the
binding of the new entry points from include/u3d_ext.h, and the arithmetic the kernel is built on: the exact three-way split and the six
partial products."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import pytest
import torch
from torch import nn

import f32s_emul as FE

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("u3d_conv3d_wgrad_f32s_supported", "u3d_wgrad_f32s_workspace_floats", "u3d_conv3d_wgrad_f32s")


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


# ---- the key -----------------------------------------------------------------------------------------------------------------------------
def test_the_key_implies_fp32_split_and_is_off_by_default():
    M = _m()
    m = M.UNet3D(**_SMALL)
    assert m.fp32_split_wgrad is False and not m.compute_split and not m._get_engine().split_wgrad
    m = M.UNet3D(**_SMALL, fp32_split_wgrad=True)
    assert m.native_supported and m.fp32_split_wgrad is True and m.compute_split and not m.compute_bf16
    e = m._get_engine()
    assert e.split_wgrad and e.split
    assert M.UNet3D(**_SMALL, fp32_split_wgrad=True, compute_dtype="fp32_split").compute_split
    m = M.UNet3D(**_SMALL, compute_dtype="fp32_split")  # the parent mode alone does not switch it on
    assert m.fp32_split_wgrad is False and not m._get_engine().split_wgrad
    assert M.get_model(dict(name="UNet3D", **_SMALL, fp32_split_wgrad=True)).fp32_split_wgrad
    both = M.UNet3D(**_SMALL, fp32_split_wgrad=True, checkpoint_encoders=True, checkpoint_levels=1)  # composes
    assert both.fp32_split_wgrad and both.checkpoint_encoders and both.checkpoint_levels == 1 and both.native_supported


@pytest.mark.parametrize("dtype", ["fp32", "float32", "bf16", "bfloat16"])
def test_a_contradicting_compute_dtype_names_the_key(dtype):
    with pytest.raises(ValueError, match="fp32_split_wgrad is the weight gradient of compute_dtype fp32_split"):
        _m().UNet3D(**_SMALL, fp32_split_wgrad=True, compute_dtype=dtype)


@pytest.mark.parametrize("other", ["bf16_subpixel", "bf16_stem"])
def test_the_bf16_keys_are_refused_next_to_it(other):
    with pytest.raises(ValueError, match=f"fp32_split_wgrad runs fp32-grade split operands; {other} implies compute_dtype bf16"):
        _m().UNet3D(**_SMALL, fp32_split_wgrad=True, **{other: True})


def test_a_2d_model_is_refused():
    M = _m()
    for cls in (M.UNet2D, M.ResidualUNet2D):
        with pytest.raises(ValueError, match="fp32_split_wgrad is a 3-D key"):
            cls(**_SMALL, fp32_split_wgrad=True)


def test_hip_graph_is_refused_next_to_the_key():
    M = _m()
    with pytest.raises(ValueError, match="hip_graph is not available with fp32_split_wgrad"):
        M.UNet3D(**_SMALL, fp32_split_wgrad=True, hip_graph=True)
    assert M.UNet3D(**_SMALL, hip_graph=True, compute_dtype="fp32_split").hip_graph  # (the parent mode keeps its graph)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_F32_SPLIT_WGRAD", "1")
    m = M.UNet3D(**_SMALL)
    assert m.fp32_split_wgrad and m.compute_split
    m = M.UNet3D(**_SMALL, fp32_split_wgrad=False)  # the key wins
    assert not m.fp32_split_wgrad and not m.compute_split
    assert not M.UNet2D(**_SMALL).fp32_split_wgrad  # the environment only sets a 3-D model's default


@pytest.mark.parametrize("name", ["ResidualUNet3D", "ResidualUNetSE3D"])
def test_residual_classes_accept_the_key(name):
    M = _m()
    m = getattr(M, name)(in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8, fp32_split_wgrad=True)
    assert m.fp32_split_wgrad and m.compute_split and m.native_supported
    eng = m._get_engine()
    assert eng.split_wgrad and eng._split_wgrad(32, 32) and not eng._split_wgrad(16, 32)


def test_the_key_is_in_the_docstring_and_the_opt_in_keys():
    M = _m()
    assert "fp32_split_wgrad" in M._OPT_IN_KEYS
    assert "`fp32_split_wgrad: true`" in M.__doc__ and "U3D_F32_SPLIT_WGRAD" in M.__doc__


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def _engine_routed(model, size, monkeypatch):
    """what the engine's weight-gradient launchers issue per 3x3x3 layer of `model` at input size `size`, with the native call recorded
    instead of issued: [(weight name, Cin, Cout, dw_cin_stride)] of the u3d_conv3d_wgrad_f32s launches; also checks that such a launch
    leaves the GroupNorm-backward job to the caller and that any other one takes it"""
    from pytorch3dunet_amd import _engine_conv as EC
    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd._engine_base import VSrc

    eng = model._get_engine()
    sub = {} if model._residual else eng._subpixel_layers(size)  # (a residual net joins by summation: no concat, no sub-pixel level)
    names = {id(p): n for n, p in model.named_parameters()}
    first = set() if model._residual else {id(d.basic_module.SingleConv1.conv) for d in model.decoders}
    issued = []
    monkeypatch.setattr(nat, "call", lambda name, *args, flops=0.0: issued.append((name, args)))
    monkeypatch.setattr(EC, "_stream", lambda dev: None)
    out = []
    for mod in model.modules():
        if not isinstance(mod, nn.Conv3d) or tuple(mod.kernel_size) != (3, 3, 3):
            continue
        Cin, Cout = mod.in_channels, mod.out_channels
        pair = sub.get(id(mod.weight))
        if id(mod) in first:
            C0 = pair[0] if pair else Cin // 3  # (any split of a virtual concat: it is not routed)
            src = VSrc(torch.zeros(1, 2, 2, 2, C0), torch.zeros(1, 1, 1, 1, Cin - C0))
        else:
            src = VSrc(torch.zeros(1, 2, 2, 2, Cin))
        rec = types.SimpleNamespace(sub=pair, plus=(0, 0, 0), affine=torch.zeros(1, Cin, 2), affine_lo=None, affine_hi=None, idx_w=0)
        cx = types.SimpleNamespace(dev=torch.device("cpu"), ws=torch.zeros(4), gview=lambda i: torch.zeros(Cout * Cin * 27),
                                   ensure_ws=lambda n: torch.zeros(4))
        job = nat.U3DGnBwdJob()
        c = EC._BwdCall(cx, rec, torch.zeros(1, 2, 2, 2, Cout), src, 1, 2, 2, 2, Cout, False, job=job)
        del issued[:]
        (eng._wgrad_subpixel if pair else eng._wgrad_fp32)(c)
        split = [a for n, a in issued if n == "u3d_conv3d_wgrad_f32s"]
        assert len(split) <= 1
        if split:
            assert c.job is job  # no job in the split launch: _conv_bwd runs the reduction on its own
            assert not any(n == "u3d_conv3d_wgrad_job" for n, _ in issued)
            out.append((names[id(mod.weight)], split[0][11], split[0][12], split[0][6]))
        else:
            assert c.job is None and [n for n, _ in issued].count("u3d_conv3d_wgrad_job") == 1
    return out


RULE_CASES = [  # (class, f_maps, input size, launches on the new kernel)
    ("UNet3D", 32, (16, 32, 32), 12),               # 6 encoder layers, 3 skip slices, 3 decoder second convolutions; not 1 -> 16, 16 -> 32
    ("UNet3D", 32, (16, 36, 32), 12),               # 36 -> 18 -> 9 -> 4: an n -> 2n + 1 level (9 = 2 * 4 + 1) is a sub-pixel level too
    ("UNet3D", [20, 40, 80], (8, 16, 16), 0),       # no layer inside the envelope
    ("ResidualUNet3D", [32, 64, 128], (16, 24, 24), 10),
]


@pytest.mark.parametrize("cls,f_maps,size,count", RULE_CASES)
def test_the_restated_rule_is_the_engines(cls, f_maps, size, count, monkeypatch):
    M = _m()
    cfg = dict(in_channels=1, out_channels=1, f_maps=f_maps, num_groups=2 if f_maps == [20, 40, 80] else 8)
    m = getattr(M, cls)(**cfg, fp32_split_wgrad=True)
    want = FE.routed(m, size)
    assert len(want) == count
    names = [n for n, _, _, _ in want]
    if cls == "UNet3D" and f_maps == 32:
        assert "encoders.0.basic_module.SingleConv1.conv.weight" not in names  # 1 -> 16
        assert "encoders.0.basic_module.SingleConv2.conv.weight" not in names  # 16 -> 32
        assert ("decoders.2.basic_module.SingleConv1.conv.weight", 32, 32, 96) in want  # the skip slice, strided into the wide gradient
    assert _engine_routed(m, size, monkeypatch) == want
    # with the key off no layer is routed
    off = getattr(M, cls)(**cfg, compute_dtype="fp32_split")
    assert FE.routed(off, size, key=False) == [] and _engine_routed(off, size, monkeypatch) == []


def test_a_virtual_concat_and_the_side_stream_family_keep_their_kernels(monkeypatch):
    from pytorch3dunet_amd import _engine_conv as EC
    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd._engine_base import VSrc

    M = _m()
    m = M.UNet3D(in_channels=1, out_channels=1, f_maps=32, num_groups=8, fp32_split_wgrad=True)
    # 20 -> 10 -> 5 -> 2: the deepest decoder (5 from 2) is n -> 2n + 1, the one above (10 from 5) exact; with U3D_SUBPIXEL_PLUS off the
    # former reads a virtual concat and its first convolution is not routed
    eng = m._get_engine()
    eng.subpixel_plus = False
    got = _engine_routed(m, (20, 20, 20), monkeypatch)
    assert "decoders.0.basic_module.SingleConv1.conv.weight" not in [n for n, _, _, _ in got] and len(got) == 11
    assert set(EC.ConvLayers._WGRAD_KERNELS) >= {"fp32", "fp32_side", "subpixel"} and set(EC.ConvLayers._RECORDED_ONLY) == {"subpixel_bf16"}


def test_the_scratch_gains_the_plan_under_the_key_only(monkeypatch):
    from pytorch3dunet_amd import _native as nat

    M = _m()
    cfg = dict(in_channels=1, out_channels=1, f_maps=32, num_groups=8)
    on = M.UNet3D(**cfg, fp32_split_wgrad=True)._get_engine()
    lib, ext = nat.get_lib(), nat.get_ext_lib()
    shape = (2, 16, 32, 32)
    plan = ext.u3d_wgrad_f32s_workspace_floats(*shape, 32, 32)
    core = max(lib.u3d_wgrad_workspace_floats(*shape, 32, 32), lib.u3d_conv3d_workspace_floats(*shape, 32, 32))
    assert plan > 0 and plan % (27 * 32 * 32) == 0
    assert on._family_ws_floats("fp32", *shape, 32, 32) == on._family_ws_floats("f32s", *shape, 32, 32) == max(core, plan)
    assert on._family_ws_floats("fp32", *shape, 16, 32) == max(lib.u3d_wgrad_workspace_floats(*shape, 16, 32),
                                                              lib.u3d_conv3d_workspace_floats(*shape, 32, 16))
    assert on._family_ws_floats("subpixel", *shape, 96, 32, sub=(32, 64)) >= plan
    # with the key off the extension library is not even asked
    off = M.UNet3D(**cfg, compute_dtype="fp32_split")._get_engine()

    def boom():
        raise AssertionError("the extension library was loaded with the key off")

    monkeypatch.setattr(nat, "get_ext_lib", boom)
    assert off._family_ws_floats("fp32", *shape, 32, 32) == core and not off._split_wgrad(32, 32)
    assert off._family_ws_floats("subpixel", *shape, 96, 32, sub=(32, 64)) == max(
        lib.u3d_wgrad_workspace_floats(*shape, 32, 32), lib.u3d_subpixel_wgrad_workspace_floats(2, 8, 16, 16, 64, 32),
        lib.u3d_conv3d_workspace_floats(*shape, 32, 32))


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------
def test_the_new_names_are_read_from_the_header_exported_bound_and_typed():
    from pytorch3dunet_amd import _native as nat

    path = os.path.join(ROOT, "include", "u3d_ext.h")
    text = open(path).read()
    protos = nat.read_part(path, {**nat._PROTOS, **nat._PART_PROTOS})
    assert protos == nat._EXT_PROTOS
    assert "#" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # still a header part: declarations and comments only
    lib = nat.get_ext_lib()
    for name in NEW_NAMES:
        assert name in protos and name in nat.EXT_SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == protos[name], name
        assert name not in nat.ALL_SYMBOLS and not hasattr(nat.get_lib(), name), name  # the core library is untouched
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    assert protos["u3d_conv3d_wgrad_f32s_supported"] == (i, [i, i])
    assert protos["u3d_wgrad_f32s_workspace_floats"] == (ll, [i] * 6)
    assert protos["u3d_conv3d_wgrad_f32s"] == (i, [i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp, ll])
    assert lib.u3d_ext_version() == nat.U3D_EXT_VERSION == 2
    assert nat.get_lib().u3d_version() == 128
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    if nm is not None:  # (without binutils the ctypes lookups above are the check)
        out = subprocess.run([nm, "-D", "--defined-only", nat.EXT_LIB_PATH], check=True, capture_output=True, text=True, timeout=60).stdout
        exported = {line.split()[-1] for line in out.splitlines() if re.search(r"\sT\s+u3d_[a-z0-9_]+$", line)}
        assert set(NEW_NAMES) <= exported


def test_the_build_links_both_units_of_the_extension():
    import __graft_entry__ as g

    assert isinstance(g.EXT_SOURCE, list) and g.EXT_SOURCE == ["u3d_c16_bf16.hip", "u3d_wgrad_f32s.hip"]
    assert all(os.path.exists(os.path.join(g.CSRC, s)) for s in g.EXT_SOURCE) and not set(g.EXT_SOURCE) & set(g.HIP_SOURCES)


def test_host_only_answers():
    from pytorch3dunet_amd import _native as nat

    lib = nat.get_ext_lib()
    assert [lib.u3d_conv3d_wgrad_f32s_supported(ci, co) for ci, co in ((32, 32), (64, 96), (16, 32), (32, 48), (0, 32))] == [1, 1, 0, 0, 0]
    for ci, co in ((16, 32), (32, 48), (0, 32), (32, -32)):
        assert lib.u3d_wgrad_f32s_workspace_floats(1, 8, 8, 8, ci, co) == 0
    assert lib.u3d_wgrad_f32s_workspace_floats(0, 8, 8, 8, 32, 32) == 0 and lib.u3d_wgrad_f32s_workspace_floats(1, 2048, 2048, 2048, 32, 32) == 0
    n = lib.u3d_wgrad_f32s_workspace_floats(1, 8, 8, 8, 64, 96)
    assert n > 0 and n % (27 * 64 * 96) == 0
    # a refusal needs no device: outside the envelope nothing is looked at but the counts
    buf = (ctypes.c_float * 4)()
    assert lib.u3d_conv3d_wgrad_f32s(0, None, buf, None, buf, buf, 16, 1, 8, 8, 8, 16, 32, buf, 4) != nat.U3D_OK


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------------
def _lognormal(n, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(2.0 * torch.randn(n, generator=g))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def test_the_three_way_split_is_exact():
    x = torch.cat((_lognormal(1 << 20, 1), torch.tensor([0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 3.0 - 2.0 ** -22, 2.0 ** -60, 65504.0, 1e30])))
    h, m, l = FE.split3(x)
    for part in (h, m, l):
        assert torch.equal(part.bfloat16().float(), part)  # each part is a bf16 value
    assert torch.equal(h.double() + m.double() + l.double(), x.double())  # bit for bit
    assert torch.equal((h + m) + l, x)  # ... and in fp32 arithmetic too
    nh, nm_, nl = FE.split3(-x)  # negation commutes with the split (the kernel's sign alternation is exact)
    assert torch.equal(nh, -h) and torch.equal(nm_, -m) and torch.equal(nl, -l)


def test_the_six_products_leave_less_than_an_fp32_ulp():
    a, b = _lognormal(1 << 20, 2), _lognormal(1 << 20, 3)
    exact = a.double() * b.double()
    err = ((FE.six_products(a, b) - exact).abs() / exact.abs()).max().item()
    print(dict(test="six_products_worst_rel", worst_in_units_of_2_pow_minus_24=err * 2.0 ** 24))
    assert err <= 2.0 ** -23
