"""The executor's weight-image cache (pytorch3dunet_amd/_engine_weights.py: `engine.images`) on small models of every family.  The packer
tests elsewhere compare kernels with kernels; these pin the HOST side: which pointer / channel slice / C-ABI mode each named image
kind stands for, when images are repacked and through which entry points, that their buffers stay put and are pinned for graph replay."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FAMILIES = {
    # sub-pixel decoder levels: (5,9,11) over (2,4,5) upsamples n -> 2n + 1 on every axis, the two levels above it exactly 2x
    "unet3d_fp32": (dict(name="UNet3D", f_maps=16, num_groups=8), (1, 1, 20, 36, 44)),
    "resunet3d_deconv": (dict(name="ResidualUNet3D", f_maps=[16, 32, 64], num_groups=8, upsample="deconv"), (1, 1, 16, 32, 32)),
    "bf16_storage": (dict(name="ResidualUNet3D", f_maps=[64, 128, 256], num_groups=8, compute_dtype="bf16", activation_dtype="bf16"),
                     (1, 1, 16, 32, 32)),
    "fp32_split": (dict(name="UNet3D", f_maps=[32, 64, 128], num_groups=8, compute_dtype="fp32_split"), (1, 1, 16, 32, 32)),
    "unet2d": (dict(name="UNet2D", f_maps=[16, 32, 64], num_groups=8, native_2d=True), (1, 1, 64, 64)),
    "resunet2d": (dict(name="ResidualUNet2D", f_maps=[16, 32, 64], num_groups=8, native_2d_residual=True), (1, 1, 64, 64)),
}
# the image kinds a training step of each family must read (a family that stops reading one no longer tests it)
KINDS = {
    "unet3d_fp32": "FWD DGRAD SKIP_FWD SKIP_DGRAD UP_FWD UP_DGRAD SLAB_FWD SLAB_DGRAD",
    "resunet3d_deconv": "FWD DGRAD CONVTR_SUBPIXEL CONVTR_DGRAD",
    "bf16_storage": "BF16_FWD BF16_DGRAD T8_FWD T8_DGRAD",
    "fp32_split": "F32S_FWD F32S_DGRAD UP_FWD UP_DGRAD",
    "unet2d": "FWD2D DGRAD2D",
    "resunet2d": "FWD2D DGRAD2D CONVTR2D_FWD CONVTR2D_DGRAD",
}


class _Recorder:
    """stands in for nat.profiler: the ordered entry-point names (and arguments) of every native call"""

    def __init__(self):
        self.calls = []

    def wrap(self, name, fn, args, flops):
        self.calls.append((name, args))
        return fn(*args)

    def packed_images(self):
        """how many images the recorded calls packed: a batch launch packs `n` (its 4th argument), every other packer one"""
        return sum(args[3] if "_batch" in name else 1 for name, args in self.calls if "u3d_pack" in name)

    def pack_names(self):
        return [name for name, _ in self.calls if "u3d_pack" in name]


class _Run:
    def __init__(self, family):
        import gpu_utils as U
        from pytorch3dunet_amd import _native as nat
        from pytorch3dunet_amd.unet3d.model import get_model

        cfg, shape = FAMILIES[family]
        torch.manual_seed(5)
        self.nat, self.dev = nat, U.DEV
        self.model = get_model(dict(in_channels=1, out_channels=1, final_sigmoid=True, **cfg)).to(U.DEV)
        self.x = torch.randn(shape, device=U.DEV)
        self.t = (torch.rand(shape, device=U.DEV) > 0.5).float()
        self.eng = self.model._get_engine()
        self.handed = {}  # (id(w), kind, pair) -> (w, image) of every lookup since the last clear
        inner = self.eng.images.get

        def get(w, kind, dev, pair=None):
            out = inner(w, kind, dev, pair)
            self.handed[(id(w), kind, pair)] = (w, out)
            return out

        self.eng.images.get = get

    def step(self, train=True):
        """one forward (+ backward); returns the recorder of its native calls"""
        rec = _Recorder()
        self.handed.clear()
        self.model.train(train)
        self.nat.profiler = rec
        try:
            if train:
                logits = self.model(self.x, return_logits=True)[1]
                self.model.zero_grad()
                torch.nn.functional.binary_cross_entropy_with_logits(logits, self.t).backward()
            else:
                with torch.no_grad():
                    self.model(self.x)
            torch.cuda.synchronize()
        finally:
            self.nat.profiler = None
        return rec


def _fresh_image(nat, w, kind, pair):
    """the image as the kind's own single-image entry point writes it into a fresh buffer (channel slices: of a contiguous copy of
    the slice, so that no pointer / stride arithmetic of the cache is repeated here)"""
    import gpu_utils as U
    from pytorch3dunet_amd.engine import _p, _stream

    lib, dev, name = nat.get_lib(), U.DEV, kind.name
    mode = 1 if name.endswith("DGRAD") or name.endswith("DGRAD2D") else 0
    w = w.detach()
    A, B = w.shape[:2]  # conv: (Cout, Cin); transposed conv: (Cin, Cout)

    def run(entry, n, dtype, *args):
        out = torch.empty(n, dtype=dtype, device=dev)
        nat.call(entry, 0, _stream(dev), *args, _p(out))
        return out

    if name in ("FWD", "DGRAD"):
        return U.pack(w, mode)
    if name.startswith("SKIP_"):
        return U.pack(w[:, :pair[0]].contiguous(), mode)
    if name.startswith("SLAB_"):
        return U.pack(w[:, pair[0]:].contiguous(), mode)
    if name == "UP_FWD":
        return run("u3d_pack_subpixel_weights", lib.u3d_subpixel_packed_floats(pair[1], A), torch.float32, _p(w), A, B, *pair)
    if name == "UP_DGRAD":
        return run("u3d_pack_subpixel_dgrad_weights", lib.u3d_subpixel_dgrad_packed_floats(A, pair[1]), torch.float32, _p(w), A, B, *pair)
    if name.startswith("BF16_"):
        return run("u3d_pack_weights_bf16", lib.u3d_packed_weight_bf16_elems(B, A, mode), torch.bfloat16, _p(w), A, B, mode)
    if name.startswith("F32S_"):
        ws = w if pair is None else w[:, :pair[0]].contiguous()
        Ci = ws.shape[1]
        return run("u3d_pack_weights_f32s", lib.u3d_packed_weight_f32s_elems(Ci, A, mode), torch.bfloat16, _p(ws), A, Ci, mode, Ci, 0)
    if name == "CONVTR_SUBPIXEL":
        return run("u3d_pack_convtr3d_subpixel", lib.u3d_convtr3d_subpixel_packed_floats(A, B), torch.float32, _p(w), A, B)
    if name.startswith("CONVTR2D_"):
        return run("u3d_pack_convtr2d", lib.u3d_convtr2d_packed_floats(A, B), torch.float32, _p(w), A, B, mode)
    if name.startswith("CONVTR_"):
        return run("u3d_pack_convtr_weights", 27 * A * B, torch.float32, _p(w), A, B, mode)
    if name.startswith("T8_"):
        return run("u3d_pack_convtr3d_t8", lib.u3d_convtr3d_t8_packed_elems(A, B, mode), torch.bfloat16, _p(w), A, B, mode)
    assert name in ("FWD2D", "DGRAD2D"), name
    return run("u3d_pack_weights2d", lib.u3d_packed_weight2d_floats(B, A, mode), torch.float32, _p(w), A, B, mode)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _assert_images_current(run):
    assert run.handed
    for (_, kind, pair), (w, img) in run.handed.items():
        want = _fresh_image(run.nat, w, kind, pair)
        assert img.dtype == want.dtype and img.numel() == want.numel(), (kind.name, pair)
        assert torch.equal(_bits(img), _bits(want)), (kind.name, pair, tuple(w.shape))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_image_is_what_its_single_image_entry_point_writes(family):
    run = _Run(family)
    run.step(train=True)
    assert {k.name for _, k, _ in run.handed} >= set(KINDS[family].split()), sorted(k.name for _, k, _ in run.handed)
    _assert_images_current(run)
    run.step(train=False)  # (a no-grad forward after a training one repacks the forward images)
    _assert_images_current(run)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_inference_repacks_only_what_changed(family):
    run = _Run(family)
    cold = run.step(train=False)
    n_all = cold.packed_images()
    assert n_all >= len(run.handed) > 0  # a cold cache packs every image the forward reads
    assert run.step(train=False).pack_names() == []  # the second inference forward: every lookup is a hit
    # a tracked in-place update of ONE weight — a whole-weight layer, then a sub-pixel layer if the family has one: exactly its forward
    # images are packed again, and hold the new values.  (fp32_split: the fp32 batch launch also packs the layer's FWD / SKIP_FWD image,
    # which the split kernels do not read — one image more than the lookups show.)
    for paired in (False, True):
        keys = [k for k in run.handed if (k[2] is not None) == paired]
        if not keys:
            continue
        w = run.handed[keys[len(keys) // 2]][0]
        mine = [k for k in run.handed if k[0] == id(w)]
        with torch.no_grad():
            w.mul_(1.5)
        rec = run.step(train=False)
        assert rec.packed_images() == len(mine) + (family == "fp32_split"), (rec.pack_names(), mine)
        _assert_images_current(run)
        assert run.step(train=False).pack_names() == []
    # invalidate(): everything again
    run.model.invalidate_native_caches()
    assert run.step(train=False).packed_images() == n_all
    assert run.step(train=False).pack_names() == []


def test_training_step_pack_launches():
    """one launch per step for every image of the model: the LDS cell packer for fp32 images (all of these models' batch images are
    16-byte aligned with channel counts % 4 == 0, so the element-wise launch has nothing to do), one launch for all bf16 images;
    transposed-convolution gather images and 2-D images are packed one launch each"""
    for family, want in (("unet3d_fp32", ["u3d_pack_weights_batch_cells"]), ("bf16_storage", ["u3d_pack_weights_bf16_batch"]),
                         ("fp32_split", ["u3d_pack_weights_batch_cells", "u3d_pack_weights_f32s"])):
        run = _Run(family)
        for _ in range(2):
            names = run.step(train=True).pack_names()
            assert sorted(set(names)) == want and names.count(want[0]) == 1, (family, names)
    run = _Run("resunet3d_deconv")
    names = run.step(train=True).pack_names()
    assert names.count("u3d_pack_weights_batch_cells") == 1 and "u3d_pack_weights_batch" not in names, names
    assert set(names) == {"u3d_pack_weights_batch_cells", "u3d_pack_convtr3d_subpixel", "u3d_pack_convtr_weights"}, names


@pytest.mark.parametrize("family", list(FAMILIES))
def test_buffers_stay_put_and_are_pinned(family):
    run = _Run(family)
    run.step(train=True)
    first = {k: img.data_ptr() for k, (_, img) in run.handed.items()}
    with torch.no_grad():
        for p in run.model.parameters():
            p.mul_(0.999)  # (an optimizer step)
    run.step(train=True)
    assert {k: img.data_ptr() for k, (_, img) in run.handed.items()} == first
    _assert_images_current(run)

    def flat(o):
        return [o] if isinstance(o, torch.Tensor) else [t for x in o for t in flat(x)] if isinstance(o, (list, tuple)) else []

    for pins in (run.eng.images.pins(), run.eng.graph_pins()):
        held = {t.data_ptr() for t in flat(pins)}
        assert set(first.values()) <= held
    # the descriptor tables of the batch launches are pinned with them: a device table is a uint8 tensor
    if family not in ("unet2d", "resunet2d"):
        assert any(t.dtype == torch.uint8 for t in flat(run.eng.images.pins()))
