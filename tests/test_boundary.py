"""CPU: the drop-in boundary — API surface, state_dict compatibility, error behaviour, and that
the C-ABI library loads and exports every symbol include/u3d.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import Golden, ROOT
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d import buildingblocks as bb
from pytorch3dunet_amd.unet3d import model as M
from pytorch3dunet_amd.unet3d.utils import get_class, number_of_features_per_level
from reference_records import STATE_DICT_CFGS, misc, state_dict_id

ALL_CFGS = [
    dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=16),
    dict(name="UNet3D", in_channels=3, out_channels=2, f_maps=[16, 32, 64], num_groups=4, final_sigmoid=False),
    dict(name="ResidualUNet3D", in_channels=1, out_channels=1, f_maps=16),
    dict(name="ResidualUNetSE3D", in_channels=1, out_channels=1, f_maps=16, num_levels=3),
    dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=16),
    dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=16, num_levels=3),
]


def test_header_symbols_exported():
    """every function declared in include/u3d.h is exported by libu3d_hip.so and bound in _native.py"""
    hdr = open(os.path.join(ROOT, "include", "u3d.h")).read()
    declared = set(re.findall(r"\b(u3d_[a-z0-9_]+)\s*\(", hdr)) - {"u3d_stream_t", "u3d_src_t"}
    assert declared, "no declarations parsed"
    assert declared == set(nat.EXPORTED_SYMBOLS)
    assert len(nat.EXPORTED_SYMBOLS) == 250  # (the table is read from the same header: not an empty parse on both sides)
    if not nat.lib_available():
        pytest.fail(f"{nat.LIB_PATH} missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert nat.get_lib().u3d_version() == 128


def test_host_only_entry_points():
    lib = nat.get_lib()
    # packed image: (ceil(K/16) chunks x 54 steps + 5 zero pad steps) x ceil(N/32) n-tiles x 256 floats
    assert lib.u3d_packed_weight_floats(96, 32, 0) == (6 * 54 + 5) * 1 * 256
    assert lib.u3d_packed_weight_floats(96, 32, 1) == (2 * 54 + 5) * 3 * 256
    # <= 16 output channels: two more images are appended — the paired-y kernel variant's (72 k-steps per chunk) and, since round 4,
    # the 16-column variant's (27 k-steps per chunk, one per tap)
    assert lib.u3d_packed_weight_floats(1, 16, 0) == (1 * 54 + 5) * 1 * 256 + (1 * 72 + 5) * 256 + (1 * 27 + 5) * 256
    assert lib.u3d_packed_weight_floats(32, 16, 1) == (1 * 54 + 5) * 1 * 256  # dgrad of 32->16: 32 output channels
    ws = lib.u3d_wgrad_workspace_floats(1, 64, 128, 128, 96, 32)
    assert ws % (27 * 1024) == 0 and 0 < ws < (1 << 28)
    # bf16 path, host-only decisions (round 4): tile shape of the bf16-storage weight gradient per level of config 4 (4 x 8 x 8 wherever it
    # wastes no more voxels than 2 x 8 x 16; the old kernel beyond 2 GiB; -1 for unsupported channel counts) ...
    lv = [((80, 160, 160), 64), ((40, 80, 80), 128), ((20, 40, 40), 256), ((10, 20, 20), 512), ((5, 10, 10), 1024)]
    assert [lib.u3d_conv3d_wgrad_bf16_b16_variant(1, *sh, c, c) for sh, c in lv] == [8, 8, 8, 8, 16]
    assert lib.u3d_conv3d_wgrad_bf16_b16_variant(8, 80, 160, 160, 128, 128) == 0 and lib.u3d_conv3d_wgrad_bf16_b16_variant(1, 8, 8, 8, 48, 64) == -1
    assert lib.u3d_wgrad_bf16_workspace_floats(1, 20, 40, 40, 256, 256) % (27 * 2048) == 0
    # ... and the split-K rule of the transposed convolution's data gradient: only the two bottom levels ask for scratch
    t8 = [(5, 10, 10, 1024, 512), (10, 20, 20, 512, 256), (20, 40, 40, 256, 128), (40, 80, 80, 128, 64)]
    need = [lib.u3d_convtr3d_dgrad_t8_workspace_floats(1, *a) for a in t8]
    # (round 5: the bottom level's bf16-storage launch takes the flat 5 x 10 x 10 tile with 16 splits — the scratch has room for either plan)
    assert need[0] == 16 * 500 * 1024 and need[1] == 5 * 4000 * 512 and need[2] == 0 and need[3] == 0, need
    # ... and its forward only at the bottom level (flat tile with 4 splits; elsewhere one block per CU needs no split: the plain plan)
    assert [lib.u3d_convtr3d_fwd_t8_workspace_floats(1, *a) for a in t8] == [4 * 500 * 8 * 512, 0, 0, 0]
    v = [lib.u3d_conv3d_bf16_tile_variant(1, *sh, c, c, 1) for sh, c in lv]
    assert [(x >> 8) & 255 for x in v] == [8, 8, 4, 5, 5] and [x >> 16 for x in v] == [1, 1, 1, 4, 16], v


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(nat, "_lib", None)
    monkeypatch.setattr(nat, "LIB_PATH", "/nonexistent/libu3d_hip.so")
    with pytest.raises(nat.U3DError):
        nat.get_lib()


def test_struct_layout_matches_header():
    # 6 pointers + 5 int32, padded to pointer alignment
    assert ctypes.sizeof(nat.U3DSrc) == 72
    assert nat.U3DSrc.C0.offset == 48 and nat.U3DSrc.W1.offset == 64


def test_get_model_and_class_lookup():
    m = M.get_model(dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=16, some_unknown_key=3))
    assert isinstance(m, M.UNet3D) and m.native_supported
    with pytest.raises(RuntimeError):
        get_class("NoSuchNet", [M.__name__])
    assert number_of_features_per_level(32, 4) == [32, 64, 128, 256]
    assert M.is_model_2d(M.UNet2D(1, 1, f_maps=16)) and not M.is_model_2d(M.UNet3D(1, 1, f_maps=16))
    assert M.is_model_2d(torch.nn.DataParallel(M.UNet2D(1, 1, f_maps=16)))


def test_constructor_validation():
    with pytest.raises(ValueError):
        bb.create_conv(4, 8, 3, "gcx", 8, 1, 0.1, True)
    with pytest.raises(AssertionError):
        bb.create_conv(4, 8, 3, "gr", 8, 1, 0.1, True)  # no conv
    with pytest.raises(AssertionError):
        bb.create_conv(4, 8, 3, "rcg", 8, 1, 0.1, True)  # non-linearity first
    with pytest.raises(AssertionError):
        bb.create_conv(12, 8, 3, "gcr", 8, 1, 0.1, True)  # 12 % 8 != 0
    with pytest.raises(AssertionError):
        M.UNet3D(1, 1, f_maps=[16])
    # fewer channels than groups -> one group (buildingblocks.py:69-70)
    layers = dict(bb.create_conv(1, 16, 3, "gcr", 8, 1, 0.1, True))
    assert layers["groupnorm"].num_groups == 1 and layers["conv"].bias is None
    assert dict(bb.create_conv(4, 8, 3, "cr", 8, 1, 0.1, True))["conv"].bias is not None


def test_encoder_decoder_widths_unet3d_f32():
    m = M.UNet3D(1, 1, f_maps=32)
    w = [(tuple(sc.conv.weight.shape[:2])) for e in m.encoders for sc in (e.basic_module.SingleConv1, e.basic_module.SingleConv2)]
    assert w == [(16, 1), (32, 16), (32, 32), (64, 32), (64, 64), (128, 64), (128, 128), (256, 128)]
    w = [(tuple(sc.conv.weight.shape[:2])) for d in m.decoders for sc in (d.basic_module.SingleConv1, d.basic_module.SingleConv2)]
    assert w == [(128, 384), (128, 128), (64, 192), (64, 64), (32, 96), (32, 32)]
    assert sum(p.numel() for p in m.parameters()) == 4081267


@pytest.mark.parametrize("name", ["g1_unet3d_small", "g2_unet3d_multi_odd", "g3_unet3d_regression"])
def test_golden_state_dict_loads_strict_and_cpu_forward_matches(name):
    g = Golden(name)
    model = g.build_model()
    x, _ = g.inputs()
    model.train()
    probs, logits = model(x, return_logits=True)  # CPU tensors -> torch.nn module tree
    assert torch.allclose(logits, g.tensor("logits"), atol=1e-5, rtol=1e-5)
    assert torch.allclose(probs, g.tensor("probs"), atol=1e-6, rtol=1e-5)
    single = model(x)
    assert torch.equal(single, probs)


@pytest.mark.parametrize("cfg", ALL_CFGS, ids=lambda c: c["name"] + str(c["in_channels"]))
def test_state_dict_keys_shapes_match_reference(cfg):
    """key order, shapes and the bytes of the seeded initialisation (SHA-256) of the reference's state_dict, recorded by
    tests/golden/make_reference_records.py; a state_dict with exactly those keys and shapes loads strictly"""
    import hashlib

    assert cfg in STATE_DICT_CFGS
    rs = misc("sd/" + state_dict_id(cfg))  # [[key, shape, sha256 of the tensor's bytes], ...]
    torch.manual_seed(0)
    m = M.get_model(dict(cfg))
    ms = m.state_dict()
    assert [k for k, _, _ in rs] == list(ms.keys())
    for k, shape, digest in rs:
        assert list(ms[k].shape) == shape
        assert hashlib.sha256(ms[k].contiguous().numpy().tobytes()).hexdigest() == digest, f"seeded init differs at {k}"
    m.load_state_dict({k: torch.zeros(shape, dtype=ms[k].dtype) for k, shape, _ in rs}, strict=True)


def test_reference_property_tests_on_cpu():
    """the reference's own tests for this path (tests/test_models.py:8-69) are range checks on odd-sized inputs"""
    for cls, shape in [(M.UNet3D, (1, 1, 33, 65, 65)), (M.ResidualUNet3D, (1, 1, 17, 33, 33)), (M.UNet2D, (1, 1, 65, 65))]:
        model = cls(1, 1, f_maps=16, final_sigmoid=True).eval()
        with torch.no_grad():
            y = model(torch.rand(shape))
        assert torch.all(0 <= y) and torch.all(y <= 1)
    for out_c in (64, 32):
        blk = bb.ResNetBlock(33, out_c, is3d=False, order="cgr").eval()
        with torch.no_grad():
            assert torch.all(blk(torch.rand(1, 33, 65, 65)) >= 0)


def test_nearest_maps_match_interpolate():
    from pytorch3dunet_amd.engine import nearest_map_host

    for n_in, n_out in [(8, 16), (16, 33), (5, 9), (7, 7), (10, 21), (1, 3)]:
        m = nearest_map_host(n_in, n_out)
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1, 1).expand(1, 1, n_in, 2, 2)
        up = torch.nn.functional.interpolate(src, size=(n_out, 2, 2), mode="nearest")[0, 0, :, 0, 0]
        assert torch.equal(m.float(), up)
        lo = torch.searchsorted(m.long(), torch.arange(n_in + 1))
        assert lo[0] == 0 and lo[-1] == n_out
        for i in range(n_in):  # children ranges partition the output
            assert torch.all(m[lo[i]:lo[i + 1]] == i)


def test_product_never_imports_oracle():
    """the shipped package (pytorch-3dunet_amd/) must not import, load or mention anything under oracle/ — the oracle
    is the checker, never part of the product path"""
    pkg = os.path.join(ROOT, "pytorch-3dunet_amd")
    bad = []
    for dirpath, _dirs, files in os.walk(pkg):
        for f in files:
            if not f.endswith((".py", ".hip", ".h", ".cpp")):
                continue
            src = open(os.path.join(dirpath, f), errors="ignore").read()
            for needle in ("unet3d_oracle", "ref_ops", "ref_import", "oracle/", "libref_ops", "c_ops"):
                if needle in src:
                    bad.append((os.path.join(dirpath, f), needle))
    assert not bad, bad


def _fake_replicate(model):
    """what torch.nn.parallel.replicate() does to a module tree (replicate.py): every module is shallow-copied with an EMPTY
    `_parameters`, the broadcast parameter copies (non-leaf tensors) are plain attributes + `_former_parameters`"""
    from collections import OrderedDict

    mods = list(model.modules())
    copies = {}
    for m in mods:
        r = m._replicate_for_data_parallel()
        r._former_parameters = OrderedDict()
        copies[m] = r
    for m in mods:
        r = copies[m]
        for key, child in m._modules.items():
            if child is not None:
                setattr(r, key, copies[child])
        for key, p in m._parameters.items():
            if p is None:
                r._parameters[key] = None  # e.g. Conv3d(bias=False): the replica's _parameters is NOT empty
            else:
                c = p * 1.0  # non-leaf, requires grad, like Broadcast's outputs
                setattr(r, key, c)
                r._former_parameters[key] = c
    return copies[model]


def test_dataparallel_replica_gets_its_own_engine_over_the_broadcast_parameters():
    """reference trainer.py:202-205 / predict.py:63-66 wrap in nn.DataParallel when several devices are visible"""
    from pytorch3dunet_amd.engine import module_params
    from pytorch3dunet_amd.unet3d.model import ResidualUNetSE3D, UNet3D

    for cls in (UNet3D, ResidualUNetSE3D):
        model = cls(1, 1, f_maps=[8, 16], num_groups=4)
        assert [id(p) for p in module_params(model)] == [id(p) for p in model.parameters()]
        eng = model._get_engine()
        assert model._get_engine() is eng
        rep = _fake_replicate(model)
        assert len(list(rep.parameters())) == 0 and rep._engine is eng  # the shallow copy still points at the original's
        rparams = module_params(rep)
        assert len(rparams) == len(eng.params) and all(not p.is_leaf and p.requires_grad for p in rparams)
        assert [tuple(p.shape) for p in rparams] == [tuple(p.shape) for p in eng.params]
        reng = rep._get_engine()
        assert reng is not eng and reng.model is rep and model._get_engine() is eng  # nothing shared, original untouched
        assert [id(p) for p in reng.params] == [id(p) for p in rparams]
        assert reng.n_enc_params == eng.n_enc_params and reng.poffs == eng.poffs
        # parameters replaced wholesale -> a new executor; the data-parallel hook survives
        eng.grad_sync = object()
        model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, assign=True)
        eng2 = model._get_engine()
        assert eng2 is not eng and eng2.grad_sync is eng.grad_sync


def test_explicit_deconv_on_residual_blocks_has_its_own_layout():
    """ResidualUNet3D(upsample='deconv') keeps concat joining + a 1x1x1 conv in the decoder blocks
    (buildingblocks.py:441-468).  Round 1 wrongly ran it through the summation-joining executor; it is native since round 2
    through the executor's concat branch (engine.ResUNetEngine.dec_concat; GPU parity in tests/test_gpu_orders.py) — the
    interpolation modes, which the reference itself cannot run on residual nets, stay on the module tree"""
    import torch

    from pytorch3dunet_amd.unet3d.model import ResidualUNet3D

    m = ResidualUNet3D(1, 1, f_maps=[8, 16], num_groups=4, upsample="deconv")
    assert m.native_supported and m.decoders[0].concat and m.decoders[0].basic_module.conv1.weight.shape == (8, 16, 1, 1, 1)
    assert m._get_engine().dec_concat == [True]
    assert m(torch.randn(1, 1, 4, 8, 8)).shape == (1, 1, 4, 8, 8)
    d = ResidualUNet3D(1, 1, f_maps=[8, 16], num_groups=4)
    assert d.native_supported and d._get_engine().dec_concat == [False]
    assert not ResidualUNet3D(1, 1, f_maps=[8, 16], num_groups=4, upsample="nearest").native_supported


def test_tape_stash_roundtrip_keeps_structure_and_references_parameters_by_position():
    import torch

    from pytorch3dunet_amd.engine import ConvRec, Tape, VSrc, stash_tape, unstash_tape
    from pytorch3dunet_amd.unet3d.model import UNet3D

    eng = UNet3D(1, 1, f_maps=[8, 16], num_groups=4)._get_engine()
    a, b = torch.zeros(1, 2, 2, 2, 4), torch.ones(1, 1, 1, 1, 4)
    t = Tape()
    t.convs.append(ConvRec("enc0.c1", VSrc(a, b), a, b, a, eng.params[0], eng.params[2], 2, 0, 1, 2))
    t.pools.append((a, b, a))
    t.dims = (1, 1, 2, 2, 2)
    skel, bag = stash_tape(t, eng._pindex)
    assert all(isinstance(x, torch.Tensor) for x in bag) and not any(x is eng.params[2] for x in bag)
    assert sum(x is a for x in bag) == 1  # shared tensors are saved once
    t2 = unstash_tape(skel, bag, eng.params)
    r = t2.convs[0]
    assert r.src.t0 is a and r.src.t1 is b and r.conv_w is eng.params[2] and r.gn_w is eng.params[0] and r.name == "enc0.c1"
    assert r.src.maps[0] is t.convs[0].src.maps[0] and t2.pools[0][1] is b and t2.dims == (1, 1, 2, 2, 2)


def test_tape_stash_backward_scratch_is_taken_once():
    """the backward's zeroed scratch rides on the tape and the skeleton shares it with every unstashed copy: the first backward takes it,
    a second one over the same skeleton (retain_graph=True) must not get it as fresh"""
    import torch

    from pytorch3dunet_amd.engine import Tape, _StatPool, stash_tape, unstash_tape
    from pytorch3dunet_amd.unet3d.model import UNet3D

    eng = UNet3D(1, 1, f_maps=[8, 16], num_groups=4)._get_engine()
    t = Tape()
    t.bwd_pool = _StatPool(torch.device("cpu"), 64).carve(16)
    skel, bag = stash_tape(t, eng._pindex)
    first = unstash_tape(skel, bag, eng.params).bwd_pool
    assert first.claim()
    first.take(8).fill_(1.0)  # the first backward's sums
    again = unstash_tape(skel, bag, eng.params).bwd_pool
    assert not again.claim() and not again.claim()


@pytest.mark.parametrize("reps", [1, 3, 8])
def test_stat_table_checks_its_size_and_folds_replica_rows(reps):
    import torch

    from pytorch3dunet_amd.engine import StatTable, _StatPool

    N, C = 2, 5
    t = torch.randn(reps, N, C, 2, dtype=torch.float64)
    tab = StatTable(t.view(-1), N, C, reps)
    f = tab.folded()
    assert (f.N, f.C, f.reps, f.scale) == (N, C, 1, 1.0)
    assert torch.equal(f.t, t.sum(0).view(-1)) and torch.equal(f.t, t.view(reps, -1).sum(0))
    assert (f is tab) == (reps == 1)
    for bad in (t.view(-1)[:-1], torch.zeros(reps * N * C * 2 + 2, dtype=torch.float64)):
        with pytest.raises(AssertionError):
            StatTable(bad, N, C, reps)
    with pytest.raises(AssertionError):
        StatTable(t.view(-1), N, C + 1, reps)
    p = _StatPool(torch.device("cpu"), 4 * reps * N * C)
    g = p.table(N, C, reps)
    assert g.t.numel() == reps * N * C * 2 and g.reps == reps and not g.t.any()


@pytest.mark.parametrize("mode", ["trilinear", "area"])
@pytest.mark.parametrize("n_in,n_out", [(4, 8), (4, 9), (5, 11), (1, 2), (7, 7), (6, 13)])
def test_resample_tables_reproduce_f_interpolate(mode, n_in, n_out):
    """the host tables of csrc/u3d_interp.hip (engine.resample_tables_host: <= 2 source samples per output index, ATen's float32
    index formulas) applied as a dense matrix equal F.interpolate along one axis, and the adjoint ranges cover every use"""
    import torch.nn.functional as F
    from pytorch3dunet_amd.engine import resample_tables_host

    idx, wt, rng = resample_tables_host(mode, n_in, n_out)
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        for a in range(2):
            M[o, idx[o, a]] += float(wt[o, a])
    x = torch.randn(1, 1, n_in, 1, 1, dtype=torch.float64)
    ref = F.interpolate(x, size=(n_out, 1, 1), mode=mode).flatten()
    assert torch.allclose(M @ x.flatten(), ref, atol=1e-6)
    for i in range(n_in):
        used = M[:, i].nonzero().flatten()
        assert used.numel() > 0 and int(rng[i, 0]) <= int(used[0]) and int(used[-1]) < int(rng[i, 1])


def test_layer_order_grammar_of_the_native_executor():
    """engine.layer_spec: which order strings of create_conv's mini language (buildingblocks.py:10-96) run natively — every order
    the reference documents ('cr', 'gcr', 'cl', 'ce', 'bcr', 'crg') and the ones its tests build ('cgr') included"""
    from pytorch3dunet_amd.engine import ACT_ELU, ACT_LEAKY, ACT_NONE, ACT_RELU, layer_spec, parse_order

    native = ["gcr", "gcl", "gce", "gc", "cgr", "cgl", "cge", "cg", "crg", "clg", "ceg", "bcr", "bcl", "bc", "cbr", "cb", "crb",
              "cr", "cl", "ce", "c", "gcrd", "gcrD", "cgld", "crd", "cD", "bcrD"]
    for o in native:
        assert layer_spec(o) is not None and parse_order(o) is not None, o
    for o in ["", "gr", "gcrg", "gbcr", "dgcr", "gcdr", "gced", "crle", "gcrr", "gcx", "ccr"]:
        assert layer_spec(o) is None, o
    sp = layer_spec("gcr")
    assert (sp.norm, sp.pre, sp.act, sp.inner, sp.drop) == ("g", True, ACT_RELU, ACT_NONE, None)
    sp = layer_spec("crg")
    assert (sp.norm, sp.pre, sp.act, sp.inner) == ("g", False, ACT_NONE, ACT_RELU)
    sp = layer_spec("cblD")
    assert (sp.norm, sp.pre, sp.act, sp.slope, sp.drop) == ("b", False, ACT_LEAKY, 0.01, "D")
    sp = layer_spec("ce")
    assert (sp.norm, sp.act) == (None, ACT_ELU)
    # the model-level switch follows the grammar (+ dropout stays out of residual blocks)
    assert M.UNet3D(1, 1, f_maps=[8, 16], num_groups=4, layer_order="cbr").native_supported
    assert M.UNet3D(1, 1, f_maps=[8, 16], num_groups=4, layer_order="crd").native_supported
    assert not M.UNet3D(1, 1, f_maps=[8, 16], num_groups=4, layer_order="gcrg").native_supported
    assert M.ResidualUNet3D(1, 1, f_maps=[8, 16], num_groups=4, layer_order="cbr").native_supported
    assert not M.ResidualUNet3D(1, 1, f_maps=[8, 16], num_groups=4, layer_order="gcrd").native_supported


def test_one_backend_by_default_policy_for_uncovered_variants(monkeypatch):
    """VERDICT r03 item 7, host logic (the GPU twin is tests/test_gpu_model.py): on a HIP device a 3-D model outside the executor's
    envelope raises unless U3D_ALLOW_TORCH_FALLBACK=1; 2-D models (reference model.py:281-358, outside the 3-D path) keep the
    one-time warning; U3D_STRICT=1 turns both into errors.  CPU tensors always run the torch.nn module tree, like the reference."""
    import warnings

    from pytorch3dunet_amd.unet3d.model import ResidualUNet3D, UNet2D

    for k in ("U3D_ALLOW_TORCH_FALLBACK", "U3D_STRICT"):
        monkeypatch.delenv(k, raising=False)
    m3 = ResidualUNet3D(1, 1, f_maps=8, num_levels=2, num_groups=4, layer_order="gcrd")  # dropout inside residual blocks: not native
    m2 = UNet2D(1, 1, f_maps=8, num_levels=2, num_groups=4)
    assert not m3.native_supported and not m2.native_supported
    assert m3(torch.rand(1, 1, 4, 8, 8)).shape == (1, 1, 4, 8, 8)  # device: cpu -> module tree, no policy involved
    with pytest.raises(NotImplementedError, match="U3D_ALLOW_TORCH_FALLBACK"):
        m3._uncovered_on_hip("layer_order 'gcrd'")
    with pytest.warns(UserWarning, match="stock PyTorch-ROCm operators"):
        m2._uncovered_on_hip("2-D model")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m2._uncovered_on_hip("2-D model")  # one-time warning
    monkeypatch.setenv("U3D_ALLOW_TORCH_FALLBACK", "1")
    with pytest.warns(UserWarning, match="stock PyTorch-ROCm operators"):
        m3._uncovered_on_hip("layer_order 'gcrd'")
    monkeypatch.setenv("U3D_STRICT", "1")
    for m in (m2, m3):
        with pytest.raises(NotImplementedError):
            m._uncovered_on_hip("x")


def test_bench_self_launch_fails_at_the_gpu_check_not_at_usage():
    """`python bench.py --gpus 2` without torch.distributed.run launches its own ranks; on this CPU-only container that path must stop
    at "needs an MI355X" (VERDICT r04 item 3), not at a usage message"""
    import subprocess

    if torch.cuda.is_available():
        pytest.skip("CPU-container check")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                          capture_output=True, text=True, env=env, timeout=300)
    assert proc.returncode != 0
    assert "needs an MI355X" in proc.stderr and "launch with" not in proc.stderr, proc.stderr[-1500:]
    # a rank that dies names itself (round 6): here the launched ranks die at the same check inside torch.distributed.run
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0"],
                          capture_output=True, text=True, env=dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"), timeout=300)
    assert proc.returncode == 1 and "[bench rank 0 of 1, local rank 0] failed: AssertionError" in proc.stderr, proc.stderr[-1500:]


@pytest.mark.parametrize("cfg", ALL_CFGS[:4], ids=lambda c: c["name"])
def test_models_pickle_and_torch_save_like_the_reference_modules(cfg, tmp_path):
    """the reference's models are plain picklable nn.Modules (torch.save(model), mp.spawn arguments, copy.deepcopy): ADVICE r04 —
    a lambda in the load_state_dict post-hook dict broke that"""
    import copy
    import pickle

    torch.manual_seed(0)
    model = M.get_model(dict(cfg))
    blob = pickle.dumps(model)
    twin = pickle.loads(blob)
    path = tmp_path / "m.pt"
    torch.save(model, path)
    loaded = torch.load(path, weights_only=False)
    for other in (twin, loaded, copy.deepcopy(model)):
        assert type(other) is type(model) and other.__dict__.get("_engine") is None
        for (k, a), (k2, b) in zip(model.state_dict().items(), other.state_dict().items()):
            assert k == k2 and torch.equal(a, b)
        other.load_state_dict(model.state_dict())          # the hook survives the round trip ...
        assert other.__dict__["_engine_stale"] is True     # ... and still marks the executor stale


def test_checkpoint_encoders_accepts_a_number_of_levels(monkeypatch):
    """`checkpoint_encoders: true` (or any truthy YAML value such as 1) = every encoder block is recomputed in backward;
    `checkpoint_levels: k` (its own key) = only the k highest-resolution levels; an integer `checkpoint_encoders: k >= 2` is
    still read as that; false / absent = none; the environment variables set the defaults of the model keys"""
    import warnings

    from pytorch3dunet_amd.unet3d.model import get_model

    cfg = dict(name="ResidualUNet3D", in_channels=1, out_channels=1, f_maps=8, num_groups=4)
    for v, want in ((True, (True, None)), (False, (False, None)), (2, (True, 2)), (1, (True, None)), (0, (False, None))):
        m = get_model(dict(cfg, checkpoint_encoders=v))
        assert (m.checkpoint_encoders, m.checkpoint_levels) == want, v
    m = get_model(dict(cfg, checkpoint_encoders=True, checkpoint_levels=1))
    assert (m.checkpoint_encoders, m.checkpoint_levels) == (True, 1)
    m = get_model(dict(cfg, checkpoint_encoders=False, checkpoint_levels=2))
    assert (m.checkpoint_encoders, m.checkpoint_levels) == (False, None)
    with pytest.raises(ValueError):
        get_model(dict(cfg, checkpoint_encoders=True, checkpoint_levels=0))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = get_model(dict(cfg, checkpoint_encoders=True, checkpoint_levels=9))
    assert m.checkpoint_levels == 5 and any("exceeds" in str(x.message) for x in w)
    m = get_model(dict(cfg))
    assert (m.checkpoint_encoders, m.checkpoint_levels) == (False, None)
    monkeypatch.setenv("U3D_CHECKPOINT", "1")
    assert get_model(dict(cfg)).checkpoint_levels is None and get_model(dict(cfg)).checkpoint_encoders
    monkeypatch.setenv("U3D_CHECKPOINT_LEVELS", "2")
    assert get_model(dict(cfg)).checkpoint_levels == 2
    monkeypatch.setenv("U3D_CHECKPOINT_LEVELS", "0")
    with pytest.raises(ValueError):
        get_model(dict(cfg))
    monkeypatch.delenv("U3D_CHECKPOINT_LEVELS")
    with pytest.raises(ValueError):
        get_model(dict(cfg, checkpoint_encoders="yes"))
