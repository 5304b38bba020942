"""Weight images of the native executor: the packed / pre-summed / bf16 / split-fp32 forms of every convolution weight that the
kernels read (include/u3d.h: u3d_pack_weights*), cached per parameter version and re-packed in ONE launch per step.  One
`WeightImages` object per executor (`engine.images`); reference counterpart: none (ATen reorders weights inside its convolution
algorithms, buildingblocks.py:56)."""
from __future__ import annotations

import enum
import os
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import _native as nat
from ._engine_base import _ALWAYS_REPACK, _F32, _empty, _p, _stream

_PACK_BOTH = os.environ.get("U3D_PACK_BOTH", "1") != "0"  # A/B: 0 = the forward and data-gradient bf16 images of a weight as two reads of it
_PACK_ELEMENTWISE = os.environ.get("U3D_PACK_ELEMENTWISE", "0") == "1"  # A/B: every image through the thread-per-slot packer
_BF16 = torch.bfloat16


class Kind(enum.IntEnum):
    """every image a kernel reads; `_KINDS` says how each one is sized and packed.  A decoder first conv on the sub-pixel path has the
    SKIP_* / UP_* images (and SLAB_* at a level that upsamples n -> 2n + 1) of its two input-channel halves instead of the whole-weight
    pair of its family: `_SUB_KINDS` says which."""

    FWD = enum.auto()           # fp32 3x3x3 forward ...
    DGRAD = enum.auto()         # ... and data gradient (flipped taps, swapped roles)
    SKIP_FWD = enum.auto()      # sub-pixel layer: the first C0 (skip) input channels
    SKIP_DGRAD = enum.auto()
    UP_FWD = enum.auto()        # ... the pre-summed parity-class image of the remaining C1 (upsampled) channels
    UP_DGRAD = enum.auto()
    SLAB_FWD = enum.auto()      # ... the plain 27-tap images of those C1 channels: slab launches of an n -> 2n + 1 level
    SLAB_DGRAD = enum.auto()
    BF16_FWD = enum.auto()      # compute_dtype bf16
    BF16_DGRAD = enum.auto()
    F32S_FWD = enum.auto()      # compute_dtype fp32_split: three bf16 images, of the whole weight or of a sub-pixel layer's skip channels
    F32S_DGRAD = enum.auto()
    CONVTR_FWD = enum.auto()    # ConvTranspose3d gather kernels: [tap][Cin][Cout] ...
    CONVTR_DGRAD = enum.auto()  # ... [tap][Cout][Cin]
    CONVTR_SUBPIXEL = enum.auto()  # ... fragment image of its sub-pixel forward kernel
    T8_FWD = enum.auto()        # ConvTranspose3d in space-to-depth form on the bf16 kernels
    T8_DGRAD = enum.auto()
    FWD2D = enum.auto()         # 3x3 convolutions of a 2-D net
    DGRAD2D = enum.auto()
    CONVTR2D_FWD = enum.auto()
    CONVTR2D_DGRAD = enum.auto()
    BF16_FWD2D = enum.auto()    # ... of a 2-D net in bf16 (`native_2d_bf16`, `native_2d_residual_bf16`): the layers the bf16 kernels cover
    BF16_DGRAD2D = enum.auto()
    BF16_FWD2D_C16 = enum.auto()    # ... the 16-channel stem layers among them (`native_2d_stem`): half n-tiles stored whole, zero upper columns
    BF16_DGRAD2D_C16 = enum.auto()
    F32S_FWD2D = enum.auto()        # ... of a UNet2D in fp32_split (`native_2d_fp32_split`): three bf16 images of the layers `_split2d` routes,
    F32S_DGRAD2D = enum.auto()      # written by the extension library (u3d_pack_weights2d_f32s)
    BF16_FWD_C16 = enum.auto()      # the 16-channel 3x3x3 layers of a UNet3D in bf16 (`bf16_stem`): images of the extension library's kernels
    BF16_DGRAD_C16 = enum.auto()
    CONVTR2D_BF16_FWD = enum.auto()    # ConvTranspose2d on the bf16 kernels (`native_2d_residual_bf16_deconv`): B[ci][co] per tap ...
    CONVTR2D_BF16_DGRAD = enum.auto()  # ... B[co][ci] per tap
    SKIP_FWD2D = enum.auto()    # sub-pixel layer of a 2-D net (`native_2d_subpixel`): the first C0 (skip) input channels ...
    SKIP_DGRAD2D = enum.auto()
    UP_FWD2D = enum.auto()      # ... the pre-summed parity-class images of the remaining C1 (upsampled) channels
    UP_DGRAD2D = enum.auto()
    SLAB_FWD2D = enum.auto()    # ... the plain 3x3 images of those C1 channels: slab launches of an n -> 2n + 1 level (`native_2d_subpixel_plus`)
    SLAB_DGRAD2D = enum.auto()
    SKIP_BF16_FWD2D = enum.auto()    # sub-pixel layer of a 2-D net in bf16 (`native_2d_bf16_subpixel`): the first C0 (skip) input channels ...
    SKIP_BF16_DGRAD2D = enum.auto()
    UP_BF16_FWD2D = enum.auto()      # ... the parity-class images of the remaining C1 channels: taps pre-summed in fp32, rounded once
    UP_BF16_DGRAD2D = enum.auto()
    SKIP_BF16_FWD = enum.auto()      # sub-pixel layer of a UNet3D in bf16 (`bf16_subpixel`): the first C0 (skip) input channels, 27 taps ...
    SKIP_BF16_DGRAD = enum.auto()
    UP_BF16_FWD = enum.auto()        # ... the parity-class images of the remaining C1 channels: taps pre-summed in fp32, rounded once
    UP_BF16_DGRAD = enum.auto()


@dataclass(frozen=True)
class _Spec:
    size: Callable                # (lib, Cin, Cout, mode) -> elements of the image
    dtype: torch.dtype
    entry: Optional[str]          # single-image entry point; None (channel slices): a one-row table through u3d_pack_weights_batch
    mode: Optional[int]           # C-ABI mode of the size query and the single-image entry point (None: they take none)
    batch: Optional[int] = None   # C-ABI mode of the image's row in the per-step batch launch of its dtype (None: packed on demand)
    half: Optional[int] = None    # the image may be / is of one half of a sub-pixel pair (C0, C1): 0 = skip, 1 = upsampled channels
    transposed: bool = False      # ConvTranspose weight (Cin, Cout, ...): the entry point takes (Cin, Cout), else (Cout, Cin)
    up_args: bool = False         # u3d_pack_subpixel2d_* / u3d_pack_subpixel_weights_bf16: the entry point takes (Cout, Cin_total, c_off, C1[, mode])


_f32 = lambda lib, ci, co, m: lib.u3d_packed_weight_floats(ci, co, m)  # noqa: E731
_bf16 = lambda lib, ci, co, m: lib.u3d_packed_weight_bf16_elems(ci, co, m)  # noqa: E731
_f32s = lambda lib, ci, co, m: lib.u3d_packed_weight_f32s_elems(ci, co, m)  # noqa: E731
_t8 = lambda lib, ci, co, m: lib.u3d_convtr3d_t8_packed_elems(ci, co, m)  # noqa: E731
_taps = lambda lib, ci, co, m: 27 * ci * co  # noqa: E731
_2d = lambda lib, ci, co, m: lib.u3d_packed_weight2d_floats(ci, co, m)  # noqa: E731
_tr2d = lambda lib, ci, co, m: lib.u3d_convtr2d_packed_floats(ci, co)  # noqa: E731
_2db = lambda lib, ci, co, m: lib.u3d_packed_weight2d_bf16_elems(ci, co, m)  # noqa: E731
_2db16 = lambda lib, ci, co, m: lib.u3d_packed_weight2d_bf16_c16_elems(ci, co, m)  # noqa: E731
_3db16 = lambda lib, ci, co, m: nat.get_ext_lib().u3d_packed_weight_bf16_c16_elems(ci, co, m)  # noqa: E731  (include/u3d_ext.h)
_2df32s = lambda lib, ci, co, m: nat.get_ext_lib().u3d_packed_weight2d_f32s_elems(ci, co, m)  # noqa: E731  (include/u3d_ext.h)
_tr2db = lambda lib, ci, co, m: lib.u3d_packed_convtr2d_bf16_elems(ci, co, m)  # noqa: E731
_up2db = lambda lib, ci, co, m: lib.u3d_subpixel2d_bf16_packed_elems(ci, co, m)  # noqa: E731
_up3db = lambda lib, ci, co, m: lib.u3d_subpixel_bf16_packed_elems(ci, co, m)  # noqa: E731

# the C-ABI mode numbers of include/u3d.h live in this table (and `_BF16_BOTH`) and nowhere else in the package
_KINDS = {
    Kind.FWD: _Spec(_f32, _F32, "u3d_pack_weights", 0, batch=0),
    Kind.DGRAD: _Spec(_f32, _F32, "u3d_pack_weights", 1, batch=1),
    Kind.SKIP_FWD: _Spec(_f32, _F32, None, 0, batch=0, half=0),
    Kind.SKIP_DGRAD: _Spec(_f32, _F32, None, 1, batch=1, half=0),
    Kind.UP_FWD: _Spec(lambda lib, ci, co, m: lib.u3d_subpixel_packed_floats(ci, co), _F32, None, None, batch=2, half=1),
    Kind.UP_DGRAD: _Spec(lambda lib, ci, co, m: lib.u3d_subpixel_dgrad_packed_floats(co, ci), _F32, None, None, batch=3, half=1),
    Kind.SLAB_FWD: _Spec(_f32, _F32, None, 0, batch=0, half=1),
    Kind.SLAB_DGRAD: _Spec(_f32, _F32, None, 1, batch=1, half=1),
    Kind.BF16_FWD: _Spec(_bf16, _BF16, "u3d_pack_weights_bf16", 0, batch=0),
    Kind.BF16_DGRAD: _Spec(_bf16, _BF16, "u3d_pack_weights_bf16", 1, batch=1),
    Kind.F32S_FWD: _Spec(_f32s, _BF16, "u3d_pack_weights_f32s", 0, half=0),
    Kind.F32S_DGRAD: _Spec(_f32s, _BF16, "u3d_pack_weights_f32s", 1, half=0),
    Kind.CONVTR_FWD: _Spec(_taps, _F32, "u3d_pack_convtr_weights", 0, transposed=True),
    Kind.CONVTR_DGRAD: _Spec(_taps, _F32, "u3d_pack_convtr_weights", 1, transposed=True),
    Kind.CONVTR_SUBPIXEL: _Spec(lambda lib, ci, co, m: lib.u3d_convtr3d_subpixel_packed_floats(ci, co), _F32,
                                "u3d_pack_convtr3d_subpixel", None, transposed=True),
    Kind.T8_FWD: _Spec(_t8, _BF16, "u3d_pack_convtr3d_t8", 0, batch=4, transposed=True),
    Kind.T8_DGRAD: _Spec(_t8, _BF16, "u3d_pack_convtr3d_t8", 1, batch=5, transposed=True),
    Kind.FWD2D: _Spec(_2d, _F32, "u3d_pack_weights2d", 0),
    Kind.DGRAD2D: _Spec(_2d, _F32, "u3d_pack_weights2d", 1),
    Kind.CONVTR2D_FWD: _Spec(_tr2d, _F32, "u3d_pack_convtr2d", 0, transposed=True),
    Kind.CONVTR2D_DGRAD: _Spec(_tr2d, _F32, "u3d_pack_convtr2d", 1, transposed=True),
    Kind.BF16_FWD2D: _Spec(_2db, _BF16, "u3d_pack_weights2d_bf16", 0),
    Kind.BF16_DGRAD2D: _Spec(_2db, _BF16, "u3d_pack_weights2d_bf16", 1),
    Kind.BF16_FWD2D_C16: _Spec(_2db16, _BF16, "u3d_pack_weights2d_bf16_c16", 0),
    Kind.BF16_DGRAD2D_C16: _Spec(_2db16, _BF16, "u3d_pack_weights2d_bf16_c16", 1),
    Kind.F32S_FWD2D: _Spec(_2df32s, _BF16, "u3d_pack_weights2d_f32s", 0),
    Kind.F32S_DGRAD2D: _Spec(_2df32s, _BF16, "u3d_pack_weights2d_f32s", 1),
    Kind.BF16_FWD_C16: _Spec(_3db16, _BF16, "u3d_pack_weights_bf16_c16", 0),
    Kind.BF16_DGRAD_C16: _Spec(_3db16, _BF16, "u3d_pack_weights_bf16_c16", 1),
    Kind.CONVTR2D_BF16_FWD: _Spec(_tr2db, _BF16, "u3d_pack_convtr2d_bf16", 0, transposed=True),
    Kind.CONVTR2D_BF16_DGRAD: _Spec(_tr2db, _BF16, "u3d_pack_convtr2d_bf16", 1, transposed=True),
    Kind.SKIP_FWD2D: _Spec(_2d, _F32, "u3d_pack_weights2d_slice", 0, half=0),
    Kind.SKIP_DGRAD2D: _Spec(_2d, _F32, "u3d_pack_weights2d_slice", 1, half=0),
    Kind.UP_FWD2D: _Spec(lambda lib, ci, co, m: lib.u3d_subpixel2d_packed_floats(ci, co), _F32, "u3d_pack_subpixel2d_weights", None,
                         half=1, up_args=True),
    Kind.UP_DGRAD2D: _Spec(lambda lib, ci, co, m: lib.u3d_subpixel2d_dgrad_packed_floats(co, ci), _F32,
                           "u3d_pack_subpixel2d_dgrad_weights", None, half=1, up_args=True),
    Kind.SLAB_FWD2D: _Spec(_2d, _F32, "u3d_pack_weights2d_slice", 0, half=1),
    Kind.SLAB_DGRAD2D: _Spec(_2d, _F32, "u3d_pack_weights2d_slice", 1, half=1),
    Kind.SKIP_BF16_FWD2D: _Spec(_2db, _BF16, "u3d_pack_weights2d_bf16_slice", 0, half=0),
    Kind.SKIP_BF16_DGRAD2D: _Spec(_2db, _BF16, "u3d_pack_weights2d_bf16_slice", 1, half=0),
    Kind.UP_BF16_FWD2D: _Spec(_up2db, _BF16, "u3d_pack_subpixel2d_weights_bf16", 0, half=1, up_args=True),
    Kind.UP_BF16_DGRAD2D: _Spec(_up2db, _BF16, "u3d_pack_subpixel2d_weights_bf16", 1, half=1, up_args=True),
    Kind.SKIP_BF16_FWD: _Spec(_bf16, _BF16, "u3d_pack_weights_bf16_slice", 0, half=0),
    Kind.SKIP_BF16_DGRAD: _Spec(_bf16, _BF16, "u3d_pack_weights_bf16_slice", 1, half=0),
    Kind.UP_BF16_FWD: _Spec(_up3db, _BF16, "u3d_pack_subpixel_weights_bf16", 0, half=1, up_args=True),
    Kind.UP_BF16_DGRAD: _Spec(_up3db, _BF16, "u3d_pack_subpixel_weights_bf16", 1, half=1, up_args=True),
}
# the images a sub-pixel layer reads, stated once: (forward, data-gradient) pair of the whole weight in a `repack` list -> the pairs of its
# skip half, its upsampled half and — an n -> 2n + 1 level — the slab (None: the family takes exact-2x levels only)
_SUB_KINDS = {
    (Kind.FWD, Kind.DGRAD): ((Kind.SKIP_FWD, Kind.SKIP_DGRAD), (Kind.UP_FWD, Kind.UP_DGRAD), (Kind.SLAB_FWD, Kind.SLAB_DGRAD)),
    (Kind.FWD2D, Kind.DGRAD2D): ((Kind.SKIP_FWD2D, Kind.SKIP_DGRAD2D), (Kind.UP_FWD2D, Kind.UP_DGRAD2D), (Kind.SLAB_FWD2D, Kind.SLAB_DGRAD2D)),
    (Kind.BF16_FWD2D, Kind.BF16_DGRAD2D): ((Kind.SKIP_BF16_FWD2D, Kind.SKIP_BF16_DGRAD2D), (Kind.UP_BF16_FWD2D, Kind.UP_BF16_DGRAD2D), None),
    (Kind.BF16_FWD, Kind.BF16_DGRAD): ((Kind.SKIP_BF16_FWD, Kind.SKIP_BF16_DGRAD), (Kind.UP_BF16_FWD, Kind.UP_BF16_DGRAD), None),
}
_BF16_BOTH = 6  # batch row that writes BF16_FWD and, right behind it in one buffer, BF16_DGRAD from one read of the weight


class WeightImages:
    """The image cache of one executor.  `f32` / `bf16` / `t8` / `each` / `each_bf16` / `each_bf16_c16`: the weights whose images ride in the fp32 batch
    launch, in the bf16 batch launch (3x3x3 layers, space-to-depth transposed convolutions) or are packed one launch each (2-D nets: fp32
    images, bf16 images of the layers on the bf16 kernels) at the start of a forward (`repack`); every other image is packed when `get`
    first misses it.  Constructing it does not touch the native library."""

    def __init__(self, f32=(), bf16=(), t8=(), each=(), each_bf16=(), each_bf16_c16=(), c16_kinds=(Kind.BF16_FWD2D_C16, Kind.BF16_DGRAD2D_C16)):
        self._f32, self._bf16, self._t8, self._each = list(f32), list(bf16), list(t8), list(each)
        self._each_bf16, self._each_bf16_c16 = list(each_bf16), list(each_bf16_c16)
        self._c16_kinds = tuple(c16_kinds)  # (forward, data-gradient) image of an `each_bf16_c16` weight: the 2-D pair, or a UNet3D's (`bf16_stem`)
        self._images: dict = {}  # (id(weight), kind, sub-pixel pair or None) -> (version key, device buffer)
        self._tables: dict = {}  # batch launch -> (its stale set, descriptor tables + the buffers they point at): one live plan each
        self._salt = 0           # advanced by begin_forward / invalidate: see _ver
        self._last_training = False

    def _ver(self, w: torch.Tensor):
        """Cache key of a packed weight image.  Autograd's version counter sees optimizer steps, load_state_dict and every other
        tracked in-place update, but NOT writes through `param.data` (EMA swaps, hand-written updates): a TRAINING forward
        therefore always repacks (weights change every step anyway: `_salt` advances), an inference forward trusts version +
        storage pointer — after `param.data` edits in eval mode call model.invalidate_native_caches() (or set U3D_ALWAYS_REPACK=1)."""
        return (w._version, w.data_ptr(), self._salt)

    def begin_forward(self, training: bool):
        # the FIRST inference forward after a training forward also repacks: weights written through `param.data` while training
        # (EMA swap before validation, trainer-side weight surgery) are then picked up without anybody calling
        # invalidate_native_caches(); later inference forwards trust version + storage pointer again
        if training or _ALWAYS_REPACK or self._last_training:
            self._salt += 1
        self._last_training = training

    def invalidate(self):
        """every image is stale from now on (model.invalidate_native_caches)"""
        self._salt += 1

    def pins(self) -> list:
        """every device buffer this object holds — the images and the descriptor tables of the batch launches: what a captured step
        may dereference and GraphStep therefore keeps alive"""
        return [[buf for _, buf in self._images.values()], [plan for _, plan in self._tables.values()]]

    # -- one image --------------------------------------------------------------------------------
    @staticmethod
    def _source(w, kind, pair):
        """(spec, source pointer, Cin, Cout, input channels per weight row, first channel, elements) of an image: of the whole weight, or
        with `pair` = (C0, C1) of the kind's half of a sub-pixel layer's input channels"""
        spec = _KINDS[kind]
        co, ci = (w.shape[1], w.shape[0]) if spec.transposed else (w.shape[0], w.shape[1])
        ld, off = ci, 0
        if pair is not None:
            off, ci = sum(pair[:spec.half]), pair[spec.half]
        return spec, w.data_ptr() + off * 27 * 4, ci, co, ld, off, spec.size(nat.get_lib(), ci, co, spec.mode)  # (slices: 3x3x3 fp32 rows)

    def _buffer(self, key, n, dtype, dev):
        """last step's buffer of this image when its element count, dtype and device still fit (stable pointers), else a new one"""
        hit = self._images.get(key)
        if hit is not None and hit[1].numel() == n and hit[1].dtype == dtype and hit[1].device == dev:
            return hit[1]
        return _empty(n, dtype=dtype, device=dev)

    def get(self, w: torch.Tensor, kind: Kind, dev, pair: Optional[tuple] = None) -> torch.Tensor:
        """the image `kind` of weight `w` (of its half of the sub-pixel pair (C0, C1), if given), packed now unless the cached one is
        current — the batch launch of this forward normally made it so"""
        key = (id(w), kind, pair)
        ver = self._ver(w)
        hit = self._images.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
        spec, wptr, ci, co, ld, off, n = self._source(w, kind, pair)
        assert n > 0 and (pair is None or spec.half is not None) and (pair is not None or spec.entry is not None)
        out = self._buffer(key, n, spec.dtype, dev)
        if spec.entry is None:  # (e.g. a no-grad forward packed only the forward images of a sub-pixel layer)
            table, _, total = self._desc_table([(w, kind, pair, spec.batch, out, n)], dev)
            nat.call("u3d_pack_weights_batch", dev.index, _stream(dev), _p(table), 1, total)
        else:
            args = (ci, co) if spec.transposed else (co, ci)
            args += () if spec.mode is None else (spec.mode,)
            args += (ld, off) if spec.half is not None else ()
            if spec.up_args:
                args = (co, ld, off, ci) + (() if spec.mode is None else (spec.mode,))
            nat.call(spec.entry, dev.index, _stream(dev), _p(w.detach()), *args, _p(out))
        self._images[key] = (ver, out)
        return out

    # -- the batch launches of a forward ----------------------------------------------------------------
    def _desc_table(self, rows, dev):
        """device U3DPackDesc table of rows (weight, kind, pair, C-ABI mode, buffer, extent); a row's `first` is the summed extent
        (blocks or elements, as its launch counts them) of the rows before it.  Returns (table, rows, total extent)."""
        descs = (nat.U3DPackDesc * max(len(rows), 1))()
        first = 0
        for d, (w, kind, pair, mode, buf, extent) in zip(descs, rows):
            _, wptr, ci, co, ld, _, _ = self._source(w, kind, pair)
            d.w, d.packed, d.first = wptr, buf.data_ptr(), first
            d.Cout, d.Cin, d.mode, d.cin_stride = co, ci, mode, (0 if pair is None else ld)
            first += extent
        return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev), len(rows), first

    def _stale(self, refs):
        """the (weight, kind, pair) of `refs` whose cached image is missing or of another parameter version"""
        out = []
        for ref in refs:
            hit = self._images.get((id(ref[0]), ref[1], ref[2]))
            if hit is None or hit[0] != self._ver(ref[0]):
                out.append(ref)
        return out

    def _plan(self, launch, stale, build):
        """the descriptor tables + buffers of a batch launch, rebuilt only when its stale set changes (every training step has the same)"""
        key = tuple((id(w), kind, pair, w.data_ptr()) for w, kind, pair in stale)
        hit = self._tables.get(launch)
        if hit is None or hit[0] != key:
            hit = self._tables[launch] = (key, build())
        return hit[1]

    @staticmethod
    def _layer_kinds(w, nd, whole, sub):
        """(pair, kinds) of one weight of a `repack` list: the first `nd` of its `whole`-weight images, or — a layer of `sub` — of each
        pair `_SUB_KINDS` names, with its (C0, C1)"""
        pair = sub.get(id(w)) if sub else None
        if pair is None:
            return None, whole[:nd]
        skip, up, slab = _SUB_KINDS[whole]
        return pair, skip[:nd] + up[:nd] + (slab[:nd] if id(w) in sub.plus else ())

    def repack(self, dev, grads: bool, sub=None):
        """(Re)pack the images of ALL conv weights whose parameter changed since the last pack — one launch for the whole model
        (u3d_pack_weights_batch_cells; bf16 mode: u3d_pack_weights_bf16_batch) instead of one per layer and image; the buffers and the
        device descriptor tables are allocated once and reused (stable pointers).  `grads`: the data-gradient images too.  `sub`:
        the `_SubLayers` of this forward, {id(weight): (C0, C1)} of the layers on the sub-pixel path, `sub.plus` the ids with slab images."""
        nd = 2 if grads else 1
        for w in self._each:  # 2-D images: one small launch per weight and image (u3d_pack_weights2d)
            pair, kinds = self._layer_kinds(w, nd, (Kind.FWD2D, Kind.DGRAD2D), sub)  # (`native_2d_subpixel`: the two halves instead)
            for kind in kinds:
                self.get(w, kind, dev, pair)
        for w in self._each_bf16:  # ... and of the 2-D layers on the bf16 kernels (u3d_pack_weights2d_bf16)
            pair, kinds = self._layer_kinds(w, nd, (Kind.BF16_FWD2D, Kind.BF16_DGRAD2D), sub)  # (`native_2d_bf16_subpixel`: likewise)
            for kind in kinds:
                self.get(w, kind, dev, pair)
        for w in self._each_bf16_c16:  # ... and of its 16-channel stem layers (u3d_pack_weights2d_bf16_c16; a UNet3D's: u3d_pack_weights_bf16_c16)
            for kind in self._c16_kinds[:nd]:
                self.get(w, kind, dev)
        if self._bf16 or self._t8:
            self._repack_bf16(dev, nd, sub)
        refs = []
        for w in self._f32:
            pair, kinds = self._layer_kinds(w, nd, (Kind.FWD, Kind.DGRAD), sub)
            refs += [(w, kind, pair) for kind in kinds]
        stale = self._stale(refs)
        if not stale:
            return
        lib = nat.get_lib()

        def build():
            # two descriptor tables: images whose runs are 16-byte aligned go through the LDS cell kernel (u3d_pack_weights_batch_cells,
            # `first` = first block), the rest through the element-wise kernel (`first` = first float)
            tables, bufs = ([], []), []
            for w, kind, pair in stale:
                spec, wptr, ci, co, ld, _, n = self._source(w, kind, pair)
                blocks = 0 if _PACK_ELEMENTWISE else lib.u3d_pack_weights_cells_blocks(wptr, ci, co, spec.batch, 0 if pair is None else ld)
                bufs.append(self._buffer((id(w), kind, pair), n, _F32, dev))
                tables[blocks == 0].append((w, kind, pair, spec.batch, bufs[-1], blocks or n))
            return [self._desc_table(rows, dev) for rows in tables], bufs

        ((tc, nc, bc), (te, ne, fe)), bufs = self._plan("f32", stale, build)
        if nc:
            nat.call("u3d_pack_weights_batch_cells", dev.index, _stream(dev), _p(tc), nc, bc)
        if ne:
            nat.call("u3d_pack_weights_batch", dev.index, _stream(dev), _p(te), ne, fe)
        for (w, kind, pair), buf in zip(stale, bufs):
            self._images[(id(w), kind, pair)] = (self._ver(w), buf)

    def _repack_bf16(self, dev, nd, sub=None):
        """bf16 fragment images of every bf16 layer whose parameter changed: ONE launch at HBM rate (u3d_pack_weights_bf16_batch)
        instead of one strided-read launch per layer and image (36 + 36 per config-4 step, 1.0 ms -> 0.25 ms).  The space-to-depth
        images of the transposed convolutions ride in the same launch (round 5; the per-weight kernel read 4 bytes per lane at a
        stride of 27 floats: 8 launches of ~33 us per config-4 step)."""
        lib = nat.get_lib()
        refs = []
        for w in self._bf16:
            if sub and id(w) in sub:  # (`bf16_subpixel`: the four images of the layer's two halves instead, one small launch each)
                pair, kinds = self._layer_kinds(w, nd, (Kind.BF16_FWD, Kind.BF16_DGRAD), sub)
                for kind in kinds:
                    self.get(w, kind, dev, pair)
                continue
            if w.data_ptr() % 16 == 0:  # (the batch kernel reads 16 bytes per lane; an unaligned view is packed on demand by `get`)
                refs += [(w, kind, None) for kind in (Kind.BF16_FWD, Kind.BF16_DGRAD)[:nd]]
        for w in self._t8:
            if w.data_ptr() % 16 == 0 and lib.u3d_pack_weights_bf16_blocks(w.shape[0], w.shape[1], _KINDS[Kind.T8_FWD].batch) > 0:
                refs += [(w, kind, None) for kind in (Kind.T8_FWD, Kind.T8_DGRAD)[:nd]]  # (Cout % 32 != 0: on demand as well)
        stale = self._stale(refs)
        if not stale:
            return

        def build():
            # a 3x3x3 weight whose forward AND data-gradient image are stale (every training step) is read ONCE: one row writes both
            # images, the data-gradient one right behind the forward one in one buffer (round 6; the two modes read 1.13 GB per
            # config-4 step)
            both = set()
            if _PACK_BOTH:
                both = {id(w) for w, kind, _ in stale if kind == Kind.BF16_FWD} & {id(w) for w, kind, _ in stale if kind == Kind.BF16_DGRAD}
            rows, bufs = [], []  # bufs: one per stale image, in order
            for w, kind, pair in stale:
                spec, _, ci, co, _, _, n = self._source(w, kind, pair)
                merged = id(w) in both and lib.u3d_pack_weights_bf16_blocks(ci, co, _BF16_BOTH) > 0
                if merged and kind == Kind.BF16_DGRAD:
                    continue  # (written by the row of the forward image, which precedes it in `stale`)
                if merged:
                    n1 = spec.size(lib, ci, co, _KINDS[Kind.BF16_DGRAD].mode)
                    b0 = self._buffer((id(w), Kind.BF16_FWD, None), n, _BF16, dev)
                    b1 = self._buffer((id(w), Kind.BF16_DGRAD, None), n1, _BF16, dev)
                    if not (b1.data_ptr() == b0.data_ptr() + 2 * n and b0.untyped_storage().data_ptr() == b1.untyped_storage().data_ptr()):
                        whole = _empty(n + n1, dtype=_BF16, device=dev)  # (else: the two views of last step's buffer)
                        b0, b1 = whole[:n], whole[n:]
                    bufs += [b0, b1]
                    rows.append((w, kind, pair, _BF16_BOTH, b0, lib.u3d_pack_weights_bf16_blocks(ci, co, _BF16_BOTH)))
                else:
                    bufs.append(self._buffer((id(w), kind, pair), n, _BF16, dev))
                    rows.append((w, kind, pair, spec.batch, bufs[-1], lib.u3d_pack_weights_bf16_blocks(ci, co, spec.batch)))
            return self._desc_table(rows, dev), bufs

        (table, n, total), bufs = self._plan("bf16", stale, build)
        nat.call("u3d_pack_weights_bf16_batch", dev.index, _stream(dev), _p(table), n, total)
        for (w, kind, pair), buf in zip(stale, bufs):
            self._images[(id(w), kind, pair)] = (self._ver(w), buf)
