"""CPU side of the opt-in 16-channel bf16 path of a UNet3D (`bf16_stem: true` / U3D_BF16_STEM=1): the key — what it implies, refuses and
leaves unchanged —, the executor's one routing rule (`_bf16_routed_weight`, read through `_weight_images`, `_cat_bf16`, `_fwd_family` and
the scratch sizing of an engine built on the CPU) held against its restatement in tests/bf16_emul_3d_stem.py, the binding of the extension
library libu3d_ext_hip.so from include/u3d_ext.h, and the emulation's own distance from the plain float64 run per model case.

Two figures of the issue do not hold as written, because a DoubleConv encoder's first convolution produces max(out / 2, in) channels:
`f_maps: [24, 48, 96]` is NOT a net without a layer inside the rule (48 -> 48, 48 -> 96 and the 144 -> 48 / 48 -> 48 decoder are multiples
of 16: four layers), and `f_maps: [32, 64]` has the 16 -> 32 layer in `encoders.0`.  The nets without a 16-channel layer used here are
`f_maps: [20, 40, 80]` and `[64, 128]` (tests/test_gpu_model_bf16_stem.py runs the latter)."""
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import bf16_emul_3d_stem as TE
import bf16_emul_3d_subpixel as SE

_SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _m():
    from pytorch3dunet_amd.unet3d import model as M

    return M


# ---- the key -----------------------------------------------------------------------------------------------------------------------------
def test_the_key_implies_bf16_and_is_off_by_default():
    M = _m()
    m = M.UNet3D(**_SMALL)
    assert m.bf16_stem is False and not m.compute_bf16 and not m._get_engine().stem3d
    m = M.UNet3D(**_SMALL, bf16_stem=True)
    assert m.native_supported and m.bf16_stem is True and m.compute_bf16 and not m.compute_split
    e = m._get_engine()
    assert e.stem3d and e.bf16
    assert M.UNet3D(**_SMALL, bf16_stem=True, compute_dtype="bf16").compute_bf16
    m = M.UNet3D(**_SMALL, compute_dtype="bf16")  # the parent mode alone does not switch it on
    assert m.bf16_stem is False and not m._get_engine().stem3d
    assert M.get_model(dict(name="UNet3D", **_SMALL, bf16_stem=True)).bf16_stem
    both = M.UNet3D(**_SMALL, bf16_stem=True, bf16_subpixel=True, checkpoint_encoders=True)  # composes
    assert both.bf16_stem and both.bf16_subpixel and both.checkpoint_encoders and both.native_supported


@pytest.mark.parametrize("dtype", ["fp32", "float32", "fp32_split"])
def test_a_contradicting_compute_dtype_names_the_key(dtype):
    with pytest.raises(ValueError, match="bf16_stem runs bf16"):
        _m().UNet3D(**_SMALL, bf16_stem=True, compute_dtype=dtype)


def test_a_2d_model_is_pointed_at_its_own_key():
    M = _m()
    for cls in (M.UNet2D, M.ResidualUNet2D):
        with pytest.raises(ValueError, match="native_2d_stem"):
            cls(**_SMALL, bf16_stem=True)


def test_hip_graph_is_refused_next_to_the_key():
    M = _m()
    with pytest.raises(ValueError, match="hip_graph is not available with bf16_stem"):
        M.UNet3D(**_SMALL, bf16_stem=True, hip_graph=True)
    assert M.UNet3D(**_SMALL, hip_graph=True, compute_dtype="bf16").hip_graph  # (the parent mode keeps its graph)


def test_environment_default_and_the_key_winning_over_it(monkeypatch):
    M = _m()
    monkeypatch.setenv("U3D_BF16_STEM", "1")
    m = M.UNet3D(**_SMALL)
    assert m.bf16_stem and m.compute_bf16
    m = M.UNet3D(**_SMALL, bf16_stem=False)  # the key wins
    assert not m.bf16_stem and not m.compute_bf16
    assert not M.UNet2D(**_SMALL).bf16_stem  # the environment only sets a 3-D model's default


@pytest.mark.parametrize("name", ["ResidualUNet3D", "ResidualUNetSE3D"])
def test_residual_nets_accept_the_key_and_route_no_layer(name):
    M = _m()
    m = getattr(M, name)(in_channels=1, out_channels=1, f_maps=[16, 32, 64], num_groups=8, bf16_stem=True)
    assert m.bf16_stem and m.compute_bf16 and m.native_supported
    eng = m._get_engine()
    assert eng.bf16 and not eng.stem3d and not eng.images._each_bf16_c16 and not TE.routed_c16(m)
    assert not eng._bf16_routed_weight(16, 32, False) and eng._bf16_routed_weight(32, 32, False)


def test_the_key_is_in_the_docstring_and_the_opt_in_keys():
    M = _m()
    assert "bf16_stem" in M._OPT_IN_KEYS
    assert "`bf16_stem: true`" in M.__doc__ and "U3D_BF16_STEM" in M.__doc__


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def _engine_c16(model):
    return {id(w) for w in model._get_engine().images._each_bf16_c16}


RULE_CASES = [  # (f_maps, layer order, number of layers on the new kernels)
    (32, "gcr", 1),              # encoders.0: 16 -> 32
    ([16, 32, 64], "gcr", 4),    # 16 -> 16, 16 -> 32, the top decoder's 48 -> 16 (written-out concat) and 16 -> 16
    ([16, 32, 64], "cgr", 3),    # post-norm: the single-source layers; the decoder's first convolution stays a virtual concat
    ([24, 48, 96], "gcr", 4),    # 48 -> 48, 48 -> 96, 144 -> 48, 48 -> 48 (see the module docstring)
    ([20, 40, 80], "gcr", 0),    # no layer inside the rule
    ([64, 128], "gcr", 0),
]


@pytest.mark.parametrize("f_maps,order,count", RULE_CASES)
def test_the_restated_rule_is_the_engines(f_maps, order, count):
    from pytorch3dunet_amd._engine_weights import Kind

    M = _m()
    cfg = dict(in_channels=1, out_channels=1, f_maps=f_maps, num_levels=3, layer_order=order,
               num_groups={24: 4, 20: 2}.get(f_maps[0] if isinstance(f_maps, list) else f_maps, 8))
    m = M.UNet3D(**cfg, bf16_stem=True)
    eng = m._get_engine()
    want = {id(conv.weight) for conv in TE.routed_c16(m)}
    assert _engine_c16(m) == want and len(want) == count
    assert eng.images._c16_kinds == (Kind.BF16_FWD_C16, Kind.BF16_DGRAD_C16)
    # the other lists: a layer inside the old rule keeps the batch launch, a layer outside both keeps its fp32 image
    assert {id(w) for w in eng.images._bf16} == {id(c.weight) for c in SE.eligible(m)}
    assert {id(w) for w in eng.images._f32} == {id(c.weight) for c in TE.fp32_mfma_layers(m)}
    # a decoder's concat is written out exactly when its first convolution is on a bf16 kernel
    on_bf16 = want | {id(c.weight) for c in SE.eligible(m)}
    for c1, _ in eng.dec:
        assert eng._cat_bf16(c1) == (id(c1.conv.weight) in on_bf16)
    # with the key off the set is empty and the lists are plain bf16's
    off = M.UNet3D(**cfg, compute_dtype="bf16")
    assert not _engine_c16(off) and not TE.routed_c16(off, key=False)
    assert {id(w) for w in off._get_engine().images._bf16} == {id(c.weight) for c in SE.eligible(off)}
    assert len(off._get_engine().images._f32) == len(eng.images._f32) + count


def test_forward_and_backward_read_the_rule_and_the_record():
    """`_fwd_family` keeps family `bf16` with `c16` beside it; a residual or bf16 tensors keep a 16-channel layer off; backward's Cout % 32
    rule does not fire for a `c16` record; the scratch is the extension's weight-gradient plan"""
    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd._engine_base import ConvRec, VSrc
    from pytorch3dunet_amd._engine_conv import ConvLayers, _ConvCall

    M = _m()
    m = M.UNet3D(in_channels=1, out_channels=1, f_maps=[16, 32], num_groups=8, bf16_stem=True)
    eng = m._get_engine()
    conv = m.decoders[0].basic_module.SingleConv1.conv  # 48 -> 16
    src = VSrc(torch.zeros(1, 4, 4, 4, 48))

    def call(src, Cin, Cout, b16=False):
        return _ConvCall(dev=None, conv=conv, src=src, affine=None, y=None, N=1, D=4, H=4, W=4, Ctot=Cin, Cout=Cout, relu=0, stats=False,
                         pool=None, residual=None, sub=(), b16=b16)

    assert eng._fwd_family(call(src, 48, 16), None) == "bf16" and eng._c16(48, 16)
    assert eng._fwd_family(call(src, 32, 32), None) == "bf16" and not eng._c16(32, 32)
    assert eng._fwd_family(call(src, 32, 32), torch.zeros(1)) == "bf16"           # (inside the old rule a residual rides in the epilogue)
    assert eng._fwd_family(call(src, 48, 16), torch.zeros(1)) == "fp32"           # no residual on the new kernels
    assert eng._fwd_family(call(src, 48, 16, b16=True), None) == "fp32"           # fp32 activation storage only
    assert eng._fwd_family(call(VSrc(torch.zeros(1, 4, 4, 4, 16), torch.zeros(1, 2, 2, 2, 32)), 48, 16), None) == "fp32"  # one real source
    assert eng._fwd_family(call(src, 8, 16), None) == "fp32" and eng._fwd_family(call(src, 24, 16), None) == "fp32"
    off = M.UNet3D(in_channels=1, out_channels=1, f_maps=[16, 32], num_groups=8, compute_dtype="bf16")._get_engine()
    assert off._fwd_family(call(src, 48, 16), None) == "fp32" and off._fwd_family(call(src, 32, 32), None) == "bf16"
    cx = types.SimpleNamespace(SIDE_MAX_VOXELS=0)
    for Cin, Cout in ((48, 16), (16, 32), (16, 16)):
        rec = ConvRec(name="x", src=VSrc(torch.zeros(1, 4, 4, 4, Cin)), affine=None, mean_rstd=None, y=torch.empty(0, Cout), gn_w=None,
                      conv_w=conv.weight, G=8, family="bf16", sub=None, plus=(0, 0, 0), c16=True)
        assert eng._bwd_families(cx, rec) == ("bf16", "bf16")
        want = nat.get_ext_lib().u3d_wgrad_bf16_c16_workspace_floats(1, 4, 4, 4, Cin, Cout)
        assert eng._wgrad_workspace_floats([rec]) == want == eng._layer_ws_floats(1, 4, 4, 4, Cin, Cout) > 0
    assert off._layer_ws_floats(1, 4, 4, 4, 48, 16) == off._family_ws_floats("fp32", 1, 4, 4, 4, 48, 16)
    # no family row was added: the layer keeps `bf16`
    assert set(ConvLayers._RECORDED_ONLY) == {"subpixel_bf16"} and "bf16" in ConvLayers._FWD_KERNELS


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------
def test_every_name_of_the_extension_header_is_exported_bound_and_typed():
    from pytorch3dunet_amd import _native as nat

    path = os.path.join(ROOT, "include", "u3d_ext.h")
    assert nat.EXT_HEADER_PATH == path
    text = open(path).read()
    protos = nat.read_part(path, {**nat._PROTOS, **nat._PART_PROTOS})  # the strict reader takes it unchanged: a header part
    assert protos == nat._EXT_PROTOS and tuple(protos) == nat.EXT_SYMBOLS
    assert "#" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # declarations only: no guard, no wrapper, no constants
    assert "u3d_ext.h" not in open(os.path.join(ROOT, "include", "u3d.h")).read()  # u3d.h does not include it
    lib = nat.get_ext_lib()
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name
        assert name not in nat._PROTOS and name not in nat._PART_PROTOS and name not in nat.ALL_SYMBOLS, name
    for name in ("u3d_ext_version", "u3d_conv3d_bf16_c16_supported", "u3d_packed_weight_bf16_c16_elems", "u3d_pack_weights_bf16_c16",
                 "u3d_conv3d_bf16_c16_workspace_floats", "u3d_conv3d_bf16_c16", "u3d_wgrad_bf16_c16_workspace_floats",
                 "u3d_conv3d_wgrad_bf16_c16"):
        assert name in protos, name
    assert lib.u3d_ext_version() == nat.U3D_EXT_VERSION
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    if nm is not None:  # (without binutils the ctypes lookups above are the check)
        out = subprocess.run([nm, "-D", "--defined-only", nat.EXT_LIB_PATH], check=True, capture_output=True, text=True, timeout=60).stdout
        exported = {line.split()[-1] for line in out.splitlines() if re.search(r"\sT\s+u3d_[a-z0-9_]+$", line)}
        assert set(protos) <= exported
    # the core tables are untouched: its library does not export the extension's names, and `call` resolves them in the extension
    core = nat.get_lib()
    assert not any(hasattr(core, name) for name in protos)
    assert core.u3d_version() == 128


def test_a_missing_extension_library_names_build(monkeypatch):
    from pytorch3dunet_amd import _native as nat

    monkeypatch.setattr(nat, "_ext_lib", None)
    monkeypatch.setattr(nat, "EXT_LIB_PATH", os.path.join(ROOT, "no_such_dir", "libu3d_ext_hip.so"))
    with pytest.raises(nat.U3DError, match=r"build\(\)"):
        nat.call("u3d_conv3d_bf16_c16_supported", 16, 32)


def test_host_only_envelope_queries_answer_as_specified():
    from pytorch3dunet_amd import _native as nat

    lib = nat.get_ext_lib()
    assert [lib.u3d_conv3d_bf16_c16_supported(ci, co) for ci, co in ((16, 32), (32, 16), (16, 16), (48, 16), (80, 48), (8, 16), (16, 24),
                                                                    (0, 16), (16, 0))] == [1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert lib.u3d_packed_weight_bf16_c16_elems(16, 32, 0) == 27 * 512 and lib.u3d_packed_weight_bf16_c16_elems(16, 32, 1) == 2 * 27 * 512
    assert lib.u3d_packed_weight_bf16_c16_elems(48, 16, 0) == 3 * 27 * 512  # half an n-tile is stored whole
    assert lib.u3d_packed_weight_bf16_c16_elems(8, 16, 0) == lib.u3d_packed_weight_bf16_c16_elems(16, 24, 1) == 0
    assert lib.u3d_packed_weight_bf16_c16_elems(16, 16, 2) == 0
    assert lib.u3d_conv3d_bf16_c16_workspace_floats(2, 64, 128, 128, 16, 32) == 0
    assert lib.u3d_wgrad_bf16_c16_workspace_floats(1, 4, 4, 4, 8, 16) == 0
    # the core's envelopes are what they were
    core = nat.get_lib()
    assert core.u3d_conv3d_bf16_supported(16, 48) == 0 and core.u3d_pack_weights_bf16_blocks(64, 16, 6) == 0


# ---- the emulation -------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _runs(i):
    """(plain, emulation) float64 runs of model case i, computed once and shared"""
    if i not in _RUNS:
        cfg, shape, seed = TE.MODEL_CASES[i]
        _, sd, x, target = TE.prep(cfg, shape, seed)
        ln = TE.loss_name_of(cfg)
        _RUNS[i] = (TE.run(cfg, sd, x, target, ln, emulate=False), TE.run(cfg, sd, x, target, ln, emulate=True))
    return _RUNS[i]


@pytest.mark.parametrize("i", range(len(TE.MODEL_CASES)))
def test_the_emulations_own_distance_decides_gate_2(i):
    """a case is held to gate 2 on the GPU (tests/test_gpu_model_bf16_stem.py) exactly when its emulation alone is inside 2/3 of both bars"""
    cfg, shape, seed = TE.MODEL_CASES[i]
    model, _, _, _ = TE.prep(cfg, shape, seed)
    assert TE.routed_c16(model), "the case has no layer on the new kernels"
    plain, emul = _runs(i)
    e_l, e_g = TE.distances(emul, plain)
    print(dict(test="bf16_stem3d_emulation_vs_plain", case=i, logits=e_l, grad_l2=e_g))
    inside = e_l <= TE.BF16_LOGITS_TOL * 2 / 3 and e_g <= TE.BF16_GRAD_TOL * 2 / 3
    assert inside == (i in TE.GATE2), (e_l, e_g)


def test_at_least_three_cases_keep_both_gates():
    assert len(set(TE.GATE2)) >= 3 and set(TE.GATE2) <= set(range(len(TE.MODEL_CASES)))


def test_with_the_key_off_the_emulation_rounds_no_16_channel_layer():
    """the helper's emulation of a case without `bf16_stem` rounds the layers of the 32-channel rule only: none in this net"""
    cfg, shape, seed = TE.MODEL_CASES[2]
    _, sd, x, target = TE.prep(TE.base_of(cfg), shape, seed)
    a = TE.run(TE.base_of(cfg), sd, x, target, "bce_dice", emulate=True)
    b = SE.run(TE.base_of(cfg), sd, x, target, "bce_dice", emulate=False)  # (f_maps [16, 32] has no layer inside the 32-channel rule: plain)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
