"""The DoubleConv executor (UNet3D: reference model.py:152-190, buildingblocks.py:138-227): whole-model forward and backward as
kernel sequences over the layer building blocks of _engine_conv.py and the weight images of _engine_weights.py."""
from __future__ import annotations

import copy
import ctypes
import dataclasses
import os
import threading
from dataclasses import dataclass, field
from typing import List, Optional

import torch
import torch.nn.functional as F

from . import _native as nat
from ._native import U3DSrc

from ._engine_base import *  # noqa: F401,F403  (explicit __all__: helpers, records, activation codes)
from ._engine_conv import ConvLayers
from ._engine_weights import Kind, WeightImages



class UNet3DEngine(ConvLayers):
    """Executes the forward / backward of a UNet3D-family model natively.  Built once per model by
    `pytorch3dunet_amd.unet3d.model.AbstractUNet`; holds no tensors between calls except caches keyed on
    parameter versions (packed weights) and index maps."""

    def __init__(self, model):
        self.model = model
        self.grad_sync = None  # set by parallel.GradSync (RCCL all-reduce overlapped with the encoder backward)
        self.debug = None  # dict -> backward stores clones of per-layer dz / dg (tools/gpu_layer_diag.py)
        self.fused_stats = True
        # (unet3d/native2d.py: a bf16 key has compute_bf16, `native_2d_subpixel` stands next to no bf16 mode on a model the executor covers)
        keys = model.keys_2d
        self.is2d = keys.native_2d  # (N,C,H,W) runs as (N,C,1,H,W): 3x3 convolutions on the `conv2d` families, 2x2 pooling
        self.stem = keys.native_2d_stem  # the first layer on the small-Cin 2-D kernels (`_small2d`)
        self.subpixel2d = keys.native_2d_subpixel  # exact-2x decoder levels on csrc/u3d_subpix2d.hip
        self.subpixel2d_plus = keys.native_2d_subpixel_plus  # ... and the n -> 2n + 1 levels on a shifted window + the slab's box launches
        self.vcat = keys.native_2d_bf16_vcat  # a decoder's first conv reads its concat inside the bf16 kernels (`_bf16_vcat`)
        self.subpixel2d_bf16 = keys.native_2d_bf16_subpixel  # exact-2x decoder levels on the sub-pixel bf16 kernels (`_bf16_subpixel`)
        self.subpixel_bf16 = bool(getattr(model, "bf16_subpixel", False))  # a UNet3D's exact-2x decoder levels on the sub-pixel bf16 kernels (`_bf16_subpixel3d`)
        # `bf16_stem`: a UNet3D's 16-channel layers on the bf16 kernels of the extension library (`_bf16_routed_weight`); a residual class
        # accepts the key and routes no layer
        self.stem3d = bool(getattr(model, "bf16_stem", False)) and not getattr(model, "_residual", False)
        self.bf16_deconv = keys.native_2d_residual_bf16_deconv  # the decoders' ConvTranspose2d on the bf16 matrix pipe (`_bf16_convtr2d`)
        self.children = 4.0 if self.is2d else 8.0  # full-res voxels a low-res voxel of an exact-2x level stands for
        self._up_scale_t = None  # `_up_scale`'s memo
        self._in_recompute = False  # activation checkpointing is re-running a block's forward inside backward (ResUNetEngine)
        # replica rows of the statistics tables the persistent fp32 convolutions write (u3d_conv3d_ex_reps; 1 = plain tables)
        self.stat_reps = max(1, min(64, int(os.environ.get("U3D_STAT_REPS", "8"))))
        self.small_cin = True  # dedicated kernels for the in_channels<=4 first layer
        self.overlap_small_wgrad = True  # weight gradients of small layers on a second HIP stream (see _BwdCtx)
        # decoder first convs over an exact-2x upsampling: sub-pixel convolution of the upsampled half (csrc/u3d_subpix.hip)
        self.subpixel = os.environ.get("U3D_SUBPIXEL", "1") != "0" and (not self.is2d or self.subpixel2d)
        # ... and over a level that upsamples n -> 2n + 1 along some axes (an odd skip size: 42 -> 85 in the shipped 80 x 170 x 170 patch):
        # sub-pixel kernels on a shifted window + the general kernels on the near-boundary slab (round 5; U3D_SUBPIXEL_PLUS=0: such
        # levels keep the 27-tap virtual-concat kernels)
        self.subpixel_plus = os.environ.get("U3D_SUBPIXEL_PLUS", "1") != "0"
        # opt-in (BASELINE config 4): bf16 MFMA operands with fp32 accumulation for the 3x3x3 convolutions whose channel
        # counts allow it (csrc/u3d_bf16.hip), fp32 master weights / activations / statistics; and recomputation of the
        # encoder blocks in backward instead of keeping their intermediates.  Set through the model
        # (`compute_dtype: bf16`, `checkpoint_encoders: true` in the YAML's model section, or U3D_BF16=1 / U3D_CHECKPOINT=1).
        self.bf16 = model.compute_bf16
        # opt-in `compute_dtype: fp32_split`: FP32-grade convolutions on the bf16 matrix pipe — every fp32 operand split exactly
        # into three bf16 values, six partial products per multiply accumulated in fp32 (csrc/u3d_bf16.hip, u3d_conv3d_f32s);
        # forward and data gradients only, weight gradients stay on the fp32 MFMA kernels
        # (a 2-D net reaches fp32_split only through `native_2d_fp32_split`, whose flag is `split2d`: the 3-D image packing and the
        # `_split_fwd` paths stay off)
        self.split = model.compute_split and not self.is2d
        # opt-in `native_2d_fp32_split`: the 3x3 layers of a UNet2D inside `_split2d` on the six-product Conv2d kernels of the extension
        # library (csrc/u3d_conv2d_f32s.h: u3d_conv2d_f32s, u3d_conv2d_f32s_dgrad, u3d_conv2d_wgrad_f32s), all three directions;
        # `native_2d_residual_fp32_split`: the same for conv2 / conv3 of a ResidualUNet2D's blocks (u3d_conv2d_f32s_res: the residual epilogue)
        self.split2d = keys.native_2d_fp32_split or keys.native_2d_residual_fp32_split
        # opt-in `fp32_split_wgrad`: ... and the weight gradients inside `_split_wgrad` on the six-product kernel of the extension library
        # (csrc/u3d_wgrad_f32s.hip, u3d_conv3d_wgrad_f32s)
        self.split_wgrad = bool(getattr(model, "fp32_split_wgrad", False))
        self.checkpoint_encoders = model.checkpoint_encoders
        self.checkpoint_levels = model.checkpoint_levels  # None: every encoder level; k: the k highest-resolution ones
        # with activation checkpointing the tape is also RELEASED block by block during backward (ResUNetEngine.backward): a feature
        # whose only purpose is memory must move the peak, and with one autograd node owning the whole tape it otherwise does not
        self.lean_tape = False  # (ResUNetEngine turns it on together with checkpoint_encoders)
        # bf16 ACTIVATION STORAGE (`activation_dtype: bf16`; ResUNetEngine decides whether the model qualifies): every NDHWC
        # activation / gradient tensor between kernels is bf16, through the `_b16` entry points of include/u3d.h
        self.act_bf16 = False
        self.adt = _F32  # ... and their dtype
        # WHICH decoder first convs take the sub-pixel path depends on the input size and is per-call state (`sub` argument /
        # ConvRec.sub, handed to `images` with every lookup), never stored on the engine: forwards at different sizes, other threads
        # and nn.DataParallel replicas must not see each other's choice
        self._lock = threading.RLock()  # host-side enqueue of one forward / backward at a time per engine
        # opt-in static-shape step runner (`hip_graph: true` in the YAML's model section or U3D_GRAPH=1): the ~70 forward and ~110
        # backward launches of a TRAINING step are captured once per input shape in two hipGraphs and replayed (GraphStep below)
        self.hip_graph = model.hip_graph
        self._graph_steps: dict = {}
        self._graph_off_reason = None
        self._placed = None  # check_placement's memo
        self._const: dict = {}
        # the model-wide layer order (every SingleConv of a DoubleConv net shares it): non-linearity of the layer outputs
        spec = parse_order(model.layer_order) or (False, ACT_RELU, 0.0)
        self.post_norm, self.act, self.slope = spec
        self.mask = 1 if self.act == ACT_RELU else 0  # ReLU backward is a fused mask in the consumer kernels
        self.params = module_params(model)
        self._pids = [id(p) for p in self.params]
        # where the first parameter lives (model._get_engine's sentinel reads it back without walking the module tree)
        self._first_param_owner, self._first_param_name = next(
            ((mod, name) for mod in model.modules() for name, p in mod._parameters.items() if p is self.params[0]), (None, None))
        self._pindex = _PIndex({id(p): i for i, p in enumerate(self.params)})
        self._build_layer_table(model)
        self._virtual_w = self._virtual_weights()
        self.images = self._weight_images()  # the packed forms of the conv weights that the kernels read (_engine_weights.py)
        # split point of the flat gradient buffer: encoders first (module order), then decoders + head
        n_enc = sum(p.numel() for p in module_params(model.encoders))
        self.n_enc_params = n_enc
        # per-level offsets inside the encoder part [enc0 | enc1 | ...]: the encoder backward walks the levels deepest first, and the
        # deepest levels hold most of the parameters (config 4: 170 of 305 MB in the last one) — their gradients are final early and
        # are handed to RCCL level by level (`_enc_bucket_plan`)
        self.enc_level_offs = [0]
        for enc in model.encoders:
            self.enc_level_offs.append(self.enc_level_offs[-1] + sum(p.numel() for p in module_params(enc)))
        assert self.enc_level_offs[-1] == n_enc
        self.n_params = sum(p.numel() for p in self.params)
        offs, o = [], 0
        for p in self.params:
            offs.append(o)
            o += p.numel()
        self.poffs = offs

    # gradient buckets smaller than this are merged with the next (shallower) encoder level's: an all-reduce costs ~20-30 us of latency
    MIN_BUCKET_FLOATS = int(os.environ.get("U3D_MIN_BUCKET_MB", "1")) * (1 << 20) // 4

    def _sync_encoder_level(self, cx, flat, level: int, pending_hi: int) -> int:
        """Called by backward when encoder level `level` is done (levels run deepest first).  Hands the gradient slice
        [offs[level], pending_hi) to the exchange once it holds MIN_BUCKET_FLOATS (or level 0 is reached) and returns the new upper end
        of the not-yet-exchanged range.  With the decoder + head bucket that makes 2 + (number of big encoder levels) collectives per
        step; the last one is followed by `finish()`."""
        lo = self.enc_level_offs[level]
        if level > 0 and pending_hi - lo < self.MIN_BUCKET_FLOATS:
            return pending_hi
        if pending_hi > lo:
            cx.join()  # (a side-stream weight gradient of this level may still be writing its slice)
            self.grad_sync.launch(flat[lo:pending_hi])
        return lo

    def _weight_images(self) -> WeightImages:
        """the image cache, told which weights' images ride in which of a forward's batch pack launches"""
        ws = [mod.weight for mod in self.model.modules()  # every 3x3x3 (UNet2D under native_2d: 3x3) weight the MFMA kernels read
              if (isinstance(mod, torch.nn.Conv3d) and mod.kernel_size == (3, 3, 3))
              or (isinstance(mod, torch.nn.Conv2d) and mod.kernel_size == (3, 3))]
        if self.is2d:  # (2-D nets in bf16: the single-source layers with both channel counts % 32 read bf16 images, `_bf16_routed`)
            bf16 = {id(w) for w in ws if self._bf16_routed_weight(w.shape[1], w.shape[0], id(w) in self._virtual_w)}
            # (a small-family layer reads the reference layout: no image up front; a data-gradient fall-through packs its own on demand)
            small = {id(w) for w in ws if self._small2d(w.shape[1], w.shape[0], id(w) in self._virtual_w)}
            c16 = {id(w) for w in ws if id(w) in bf16 and self._c16(w.shape[1], w.shape[0])}  # (stem layers: the `*_C16` images)
            f32s = self._split2d_weights()  # (`native_2d_fp32_split`: the routed layers read F32S_*2D images, packed when first asked for)
            return WeightImages(each=[w for w in ws if id(w) not in bf16 | small | f32s], each_bf16=[w for w in ws if id(w) in bf16 - c16],
                                each_bf16_c16=[w for w in ws if id(w) in c16])
        bf16 = {id(w) for w in ws if self._bf16_routed_weight(w.shape[1], w.shape[0], id(w) in self._virtual_w)}
        # (`bf16_stem`: the 16-channel layers' BF16_*_C16 images, one launch per weight and image, not in the batch pack launch)
        c16 = {id(w) for w in ws if id(w) in bf16 and self._c16(w.shape[1], w.shape[0])}
        return WeightImages(
            # (not the first layer: its dedicated kernels read the reference layout)
            f32=[w for w in ws if id(w) not in bf16 and not (self.small_cin and w.shape[1] <= 4 and w.shape[0] <= 32)],
            bf16=[w for w in ws if id(w) in bf16 - c16], t8=self._t8_weights() if self.bf16 else (),
            each_bf16_c16=[w for w in ws if id(w) in c16], c16_kinds=(Kind.BF16_FWD_C16, Kind.BF16_DGRAD_C16))

    def _split2d_weights(self) -> set:
        """ids of the conv weights `_split2d` routes (`native_2d_fp32_split`; empty with the key off): from the layer table, a decoder's
        first convolution with its skip / upsampled channel counts"""
        if not self.split2d:
            return set()
        out = set()
        for _, c1, c2 in self.enc:
            out |= {id(c.conv.weight) for c in (c1, c2) if self._split2d_counts(c.conv.in_channels, 0, c.conv.out_channels)}
        skips = [c2.conv.out_channels for _, _, c2 in self.enc][:-1][::-1]
        for (c1, c2), C0 in zip(self.dec, skips):
            if self._split2d_counts(C0, c1.conv.in_channels - C0, c1.conv.out_channels):
                out.add(id(c1.conv.weight))
            if self._split2d_counts(c2.conv.in_channels, 0, c2.conv.out_channels):
                out.add(id(c2.conv.weight))
        return out

    def _t8_weights(self) -> list:
        """ConvTranspose3d weights whose forward / data gradient may run in space-to-depth form (`_convtr_t8`)"""
        return []

    def graph_pins(self) -> list:
        """every lazily built device buffer a captured step may dereference (GraphStep keeps this list alive): the weight images with
        their pack descriptor tables, the constant tables"""
        return [self.images.pins(), list(self._const.values())]

    def _virtual_weights(self):
        """ids of the conv weights whose input is a virtual concat (decoder first convs) and which therefore run on the fp32 /
        sub-pixel kernels.  In bf16 mode a decoder whose first conv fits the bf16 kernels MATERIALISES its concat instead (`_cat_bf16`)
        and is an ordinary bf16 layer."""
        return {id(c1.conv.weight) for c1, _ in self.dec if not self._cat_bf16(c1)}

    def _cat_bf16(self, c1) -> bool:
        """`compute_dtype: bf16` and this decoder's first conv (in = skip + upsampled channels) fits the bf16 kernels: its input
        torch.cat((skip, interpolate(x)), dim=1) (buildingblocks.py:491) is written out once by u3d_nearest_cat_fwd and the layer runs
        forward, data gradient and weight gradient on the bf16 matrix pipe like any single-source layer — 27 taps over
        all channels at bf16 rates instead of the fp32 kernels' 27 (skip) + 8 (sub-pixel) taps at fp32 rates.  Round 4.  The bf16 sub-pixel
        kernels VERDICT r03 item 6 asked for are the opt-in `bf16_subpixel` (csrc/u3d_subpix_bf16.hip): a level `_bf16_subpixel3d` accepts
        at this input size runs its two halves on them instead (listed by `_subpixel_layers`) and writes no concat; every other level
        `_cat_bf16` accepts keeps the written-out copy described here.  Under `native_2d_bf16_vcat` a layer
        that also fits `_bf16_vcat` stays such a bf16 layer (same images, never an fp32-virtual or sub-pixel one) but reads the two
        halves in place: `forward` skips the copy.  Under `native_2d_bf16_subpixel` a level that `_bf16_subpixel` accepts at this input
        size runs its two halves on the sub-pixel bf16 kernels instead (listed by `_subpixel_layers`): no copy either."""
        return bool(self.bf16) and layer_spec(c1.order).pre and self._bf16_routed_weight(c1.conv.in_channels, c1.conv.out_channels, False) and \
            os.environ.get("U3D_BF16_CAT", "1") != "0"

    def _build_layer_table(self, model):
        self.enc = []
        for enc in model.encoders:
            bm = enc.basic_module
            self.enc.append((enc.pooling is not None, bm.SingleConv1, bm.SingleConv2))
        self.dec = []
        self.dec_up = []  # upsample='deconv' (buildingblocks.py:445-451): the decoder's ConvTranspose3d, else None (nearest)
        for dec in model.decoders:
            bm = dec.basic_module
            self.dec.append((bm.SingleConv1, bm.SingleConv2))
            self.dec_up.append(getattr(getattr(dec.upsampling, "upsample", None), "conv_transposed", None))
        # upsample='trilinear' / 'area' (buildingblocks.py:598-614): materialised by csrc/u3d_interp.hip, then a same-size concat
        self.dec_interp = [getattr(dec.upsampling, "mode", None) if getattr(dec.upsampling, "mode", None) in ("trilinear", "area")
                           else None for dec in model.decoders]

    # -- the frame around the level loops, shared with ResUNetEngine ----------------------------------
    def _enter(self, x: torch.Tensor, save: bool):
        """(x0, dims, tape_or_None): the network input as NDHWC, its (N, Cin, D, H, W), the tape when `save`"""
        dev = x.device
        if self.is2d:
            assert x.dim() == 4, "the 2-D executor takes (N,C,H,W)"
            x = x.unsqueeze(2)  # (N,C,1,H,W): NHWC is NDHWC with D = 1
        N, Cin, D, H, W = x.shape
        x = x.contiguous()
        if Cin == 1:
            x0 = x.view(N, D, H, W, 1)  # NCDHW == NDHWC when C == 1
        else:
            x0 = _empty((N, D, H, W, Cin), dtype=_F32, device=dev)
            nat.call("u3d_ncdhw_to_ndhwc", dev.index, _stream(dev), _p(x), _p(x0), N, Cin, D * H * W)
        tape = Tape() if save else None
        if tape is not None:
            tape.x0 = x0
            tape.dims = (N, Cin, D, H, W)
        return x0, (N, Cin, D, H, W), tape

    def _maxpool_fwd(self, cur, dev):
        """(pooled, argmax) of MaxPool3d(2) (2-D: MaxPool2d, D stays 1)"""
        Np, Dp, Hp, Wp, Cp = cur.shape
        pooled = _empty((Np, Dp if self.is2d else Dp // 2, Hp // 2, Wp // 2, Cp), dtype=self.adt, device=dev)
        argmax = _empty(pooled.shape, dtype=torch.uint8, device=dev)
        if self.is2d:
            nat.call("u3d_maxpool2d_fwd", dev.index, _stream(dev), _p(cur), Np, Hp, Wp, Cp, _p(pooled), _p(argmax), None)
        elif self.act_bf16:
            nat.call("u3d_maxpool2_fwd_b16", dev.index, _stream(dev), _p(cur), Np, Dp, Hp, Wp, Cp, _p(pooled), _p(argmax))
        else:
            nat.call("u3d_maxpool2_fwd", dev.index, _stream(dev), _p(cur), Np, Dp, Hp, Wp, Cp, _p(pooled), _p(argmax), None)
        return pooled, argmax

    def _head_fwd(self, cur, dims, tape):
        """(logits, probs_or_None): 1x1x1 conv + bias + activation (model.py:141-147), outputs in the reference's layout"""
        dev = cur.device
        N, _, D, H, W = dims
        fc = self.model.final_conv
        Co = fc.out_channels
        logits = _empty((N, Co, D, H, W), dtype=_F32, device=dev)
        act = 0
        probs = None
        if self.model.final_activation is not None:
            act = 1 if isinstance(self.model.final_activation, torch.nn.Sigmoid) else 2
            probs = _empty_like(logits)
        nat.call("u3d_conv1x1_head_fwd" + ("_b16" if self.act_bf16 else ""), dev.index, _stream(dev), _p(cur), _p(fc.weight.detach()),
                 _p(fc.bias.detach()), N, D * H * W, fc.in_channels, Co, act, _p(logits), _p(probs))
        if tape is not None:
            tape.head_x = cur
            if self.debug is not None:
                self.debug["tape"] = tape
        if self.is2d:  # (N,Cout,H,W), the reference's 2-D layout
            logits = logits.view(N, Co, H, W)
            probs = probs.view(N, Co, H, W) if probs is not None else None
        return logits, probs

    def _exit_dx(self, dx0, dims):
        """the input gradient in the reference's layout from its NDHWC form (None: not asked for)"""
        if dx0 is None:
            return None
        N, Cin, D, H, W = dims
        if dx0.dtype != _F32:
            dx0 = dx0.to(_F32)  # (input gradients are rare; the network input and its gradient are fp32 tensors)
        if Cin == 1:
            dx = dx0.reshape(N, 1, D, H, W)
        else:
            dx = _empty((N, Cin, D, H, W), dtype=_F32, device=dx0.device)
            nat.call("u3d_ndhwc_to_ncdhw", dx0.device.index, _stream(dx0.device), _p(dx0), _p(dx), N, Cin, D * H * W)
        return dx.view(N, Cin, H, W) if self.is2d else dx

    # -- forward ------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, save: bool):
        """x: (N,C,D,H,W) fp32 on a gfx950 device.  Returns (logits, probs_or_None, tape_or_None), both
        outputs in the reference's NCDHW layout."""
        dev = x.device
        x0, dims, tape = self._enter(x, save)
        N, _, D, H, W = dims
        sub = self._subpixel_layers((D, H, W))
        self.images.repack(dev, save, sub)
        # stat doubles: every conv output + every GN input computed standalone; generous upper bound
        tot = 0
        R = self.stat_reps
        for _, c1, c2 in self.enc:
            tot += N * (4 * c1.conv.in_channels + (3 + R) * (c1.conv.out_channels + c2.conv.out_channels)) * 2
        for c1, c2 in self.dec:
            tot += N * (4 * c1.conv.in_channels + (3 + R) * (c1.conv.out_channels + c2.conv.out_channels)) * 2
        # (round 6) the backward pass's zeroed scratch — head (dw, db) + 2 doubles per (n, input channel) of every conv — rides in the same
        # fill launch; handed over through the tape, used by the FIRST backward over it
        fcm = self.model.final_conv
        btot = 0
        if save:
            btot = R * (fcm.out_channels * fcm.in_channels + fcm.out_channels)
            for _, c1, c2 in self.enc:
                btot += R * N * (c1.conv.in_channels + c2.conv.in_channels) * 2
            for c1, c2 in self.dec:
                btot += R * N * (c1.conv.in_channels + c2.conv.in_channels) * 2
        pool = _StatPool(dev, tot + btot)
        if tape is not None:
            tape.bwd_pool = pool.carve(btot)

        feats = []  # (tensor, stats) of every encoder output
        cur, cur_st = x0, None
        for i, (has_pool, c1, c2) in enumerate(self.enc):
            if has_pool:
                pst = None if self.post_norm else pool.table(cur.shape[0], cur.shape[-1], self.stat_reps)
                pooled, argmax = self._maxpool_fwd(cur, dev)
                if pst is not None:  # (the pooled tensor's statistics: a pass of its own — fused into the pool it was slower — into replica rows)
                    s_p = VSrc(pooled).struct()
                    nat.call("u3d_chan_stats_reps", dev.index, _stream(dev), ctypes.byref(s_p), *pooled.shape[:4], *_tab(pst))
                if tape is not None:
                    tape.pools.append((pooled, argmax, cur))
                cur, cur_st = pooled, pst
            src = VSrc(cur)
            stats_of = (lambda *a: None) if self.post_norm else self._stats_of  # only a GroupNorm on the conv INPUT needs them
            y1, s1 = self._single_conv_fwd(c1, f"enc{i}.c1", src, stats_of(src, cur_st, None, pool, dev), pool, tape)
            src2 = VSrc(y1)
            y2, s2 = self._single_conv_fwd(c2, f"enc{i}.c2", src2, stats_of(src2, s1, None, pool, dev), pool, tape)
            feats.append((y2, s2))
            cur, cur_st = y2, s2

        skips = feats[:-1][::-1]  # model.py:126-133
        for j, ((c1, c2), (sk, sk_st)) in enumerate(zip(self.dec, skips)):
            ct = self.dec_up[j]
            if ct is not None:
                # upsample='deconv': ConvTranspose3d(k3, s2, p1) -> 2n-1 voxels (buildingblocks.py:617-664); the nearest resize
                # to the skip's size (:650-651) and the concat are virtual, like the interpolation path
                family = self._up_family(cur.shape[-1], ct.out_channels, True)
                t = getattr(self, self._UP_KERNELS[family][0])(dev, ct, cur)
                if tape is not None:
                    tape.ups.append(UpRec(cur, ct.weight, None, tuple(t.shape[1:4]), family))
                cur, cur_st = t, None
            elif self.dec_interp[j] is not None:
                # F.interpolate(mode='trilinear' | 'area') to the skip's size: a real tensor (2-tap separable gather), joined by
                # a same-size virtual concat
                Nl, D1, H1, W1, Cl = cur.shape
                _, Ds, Hs, Ws, _ = sk.shape
                tabs = [_resample_tables(dev, self.dec_interp[j], a, b) for a, b in ((D1, Ds), (H1, Hs), (W1, Ws))]
                up = _empty((Nl, Ds, Hs, Ws, Cl), dtype=_F32, device=dev)
                nat.call("u3d_resample2_fwd", dev.index, _stream(dev), _p(cur), _p(tabs[0][0]), _p(tabs[1][0]), _p(tabs[2][0]),
                         _p(tabs[0][1]), _p(tabs[1][1]), _p(tabs[2][1]), Nl, D1, H1, W1, Ds, Hs, Ws, Cl, _p(up))
                if tape is not None:
                    tape.ups.append(UpRec(cur, None, tabs, (Ds, Hs, Ws), self.dec_interp[j]))
                cur, cur_st = up, None
            src = VSrc(sk, cur)  # skip channels first (buildingblocks.py:491)
            in_sub = id(c1.conv.weight) in sub  # (a sub-pixel level of this forward: its two halves run as plain tensors)
            st_in = stats_of(src, sk_st, cur_st, pool, dev, in_sub and sub.family == "subpixel2d_bf16")
            # ONE question per decoder: is the concat written out?  bf16 mode, a layer that fits the bf16 kernels (`_cat_bf16`) and is neither
            # a sub-pixel level nor read in place by the `_src` entry points (`native_2d_bf16_vcat`, `_bf16_vcat`) — it then runs as an
            # ordinary single-source bf16 layer; the per-channel sums of the virtual tensor describe the materialised one exactly
            if self._cat_bf16(c1) and not in_sub and not self._bf16_routed(src, c1.conv.out_channels):
                cat = _empty((src.N, src.D, src.H, src.W, src.C), dtype=_F32, device=dev)
                nat.call("u3d_nearest_cat_fwd", dev.index, _stream(dev), _p(sk), _p(cur), _p(src.maps[0]), _p(src.maps[1]), _p(src.maps[2]),
                         src.N, src.D, src.H, src.W, src.D1, src.H1, src.W1, src.C0, src.C1, _p(cat))
                if tape is not None:
                    tape.cats[j] = src
                y1, s1 = self._single_conv_fwd(c1, f"dec{j}.c1", VSrc(cat), st_in, pool, tape)
                del cat
            else:  # (every other join keeps the virtual source, on the tape too; `sub` changes nothing for a level outside it)
                y1, s1 = self._single_conv_fwd(c1, f"dec{j}.c1", src, st_in, pool, tape, sub=sub)
            src2 = VSrc(y1)
            y2, s2 = self._single_conv_fwd(c2, f"dec{j}.c2", src2, stats_of(src2, s1, None, pool, dev), pool, tape)
            cur, cur_st = y2, s2

        return (*self._head_fwd(cur, dims, tape), tape)

    # -- backward -----------------------------------------------------------------------------------
    def backward(self, tape: Tape, dlogits: torch.Tensor, need_input_grad: bool):
        """Returns (flat_grad, dx_or_None).  flat_grad holds every parameter gradient in module order."""
        dev = dlogits.device
        N, _, D, H, W = tape.dims
        V = D * H * W
        dlogits = dlogits.contiguous()
        flat = _empty(self.n_params, dtype=_F32, device=dev)
        # zeroed double scratch: head (dw,db) + 2 doubles per (n, channel) per conv layer
        fc = self.model.final_conv
        Co, Cf = fc.out_channels, fc.in_channels
        tot = self.stat_reps * (Co * Cf + Co) + sum(self.stat_reps * N * r.src.C * 2 for r in tape.convs)
        pool = tape.bwd_pool  # zeroed by the forward's fill launch; a second backward over the tape takes a fresh one
        tape.bwd_pool = None
        # (a backward pass being captured into a hipGraph is replayed without its forward: it zeroes its own scratch inside the graph;
        # claim() last: only the pass that takes the pool marks it used)
        if (pool is None or pool.buf.numel() < tot or pool.buf.device != dev or torch.cuda.is_current_stream_capturing()
                or not pool.claim()):
            pool = _StatPool(dev, tot)
        ws = self._wgrad_workspace(tape, dev)
        cx = _BwdCtx(dev, pool, ws, flat, self)

        # ---- head backward: dz of the last decoder conv (ReLU mask fused)
        hreps = self.stat_reps  # (replica rows of the head's f64 accumulator: 2048 blocks on the same Co * (Cf + 1) doubles)
        hacc = pool.take(hreps * (Co * Cf + Co))
        dz = _empty_like(tape.head_x)
        nat.call("u3d_conv1x1_head_bwd_reps", dev.index, _stream(dev), _p(dlogits), _p(tape.head_x), _p(fc.weight.detach()), N, V,
                 Cf, Co, self.mask, _p(dz), _p(hacc), hreps)
        self._unact(dev, dz, tape.head_x)
        iw, ib = self._pindex[id(fc.weight)], self._pindex[id(fc.bias)]
        assert self.poffs[ib] == self.poffs[iw] + Co * Cf
        nat.call("u3d_cvt_f64_f32_sum", dev.index, _stream(dev), _p(hacc), _p(cx.gview(iw)), Co * Cf + Co, hreps)

        n_levels = len(self.enc)
        n_dec = len(self.dec)
        mk = self.mask  # 1: the producers' ReLU masks are applied inside the consumer kernels; else _unact afterwards
        skip_grad = {}  # encoder level -> gradient arriving through the skip connection (pre-mask)

        recs = tape.convs  # order: enc0.c1, enc0.c2, enc1.c1, ..., dec0.c1, dec0.c2, ...
        enc_recs = [(recs[2 * i], recs[2 * i + 1]) for i in range(n_levels)]
        dec_recs = [(recs[2 * n_levels + 2 * j], recs[2 * n_levels + 2 * j + 1]) for j in range(n_dec)]

        # ---- decoders, last to first
        for j in range(n_dec - 1, -1, -1):
            r1, r2 = dec_recs[j]
            dg2, coef2, _ = self._conv_bwd(cx, r2, dz)
            dz1 = self._plain_apply(cx, dg2, coef2, r2.src.t0, mk)  # r2.src.t0 is r1.y (post-activation)
            self._unact(dev, dz1, r2.src.t0)
            del dg2
            dg1, coef1, coef_hi = self._conv_bwd(cx, r1, dz1)
            src = tape.cats.get(j, r1.src)  # (bf16 mode: r1 ran on the materialised concat; its two halves are what the gradient splits into)
            C0, C1, Ct = src.C0, src.C1, src.C
            # skip half -> gradient of the encoder feature: its GroupNorm backward (p*dg + q*e + r on the first C0 channels)
            # is evaluated inside the max-pool merge kernel of that encoder level, never written to HBM
            lvl = n_levels - 2 - j
            dzl = _empty_like(src.t1)
            if r1.sub is not None:
                dg0, dlow = dg1
                skip_grad[lvl] = (dg0, C0, coef1, Ct)
                if any(r1.plus):
                    # n -> 2n + 1 along some axes: the first low-res cell of such an axis has three children
                    if self.is2d:  # (`native_2d_subpixel_plus`: one child along the z axis a 2-D tensor does not have)
                        nat.call("u3d_gn_bwd_apply_children2d", dev.index, _stream(dev), _p(dlow), _p(src.t1), _p(coef1), Ct, C0, src.N,
                                 src.H1, src.W1, C1, *r1.plus[1:], mk, _p(dzl))
                    else:
                        nat.call("u3d_gn_bwd_apply_children", dev.index, _stream(dev), _p(dlow), _p(src.t1), _p(coef1), Ct, C0, src.N,
                                 src.D1, src.H1, src.W1, C1, *r1.plus, mk, _p(dzl))
                else:
                    # dlow already holds the children sums: (p*dlow + 8*(q*x + r)) * (x > 0) on the low-res producer (2-D: 4 children)
                    coef_up = coef_hi if coef_hi is not None else coef1[:, :, C0:] * self._up_scale(dev)
                    nat.call("u3d_gn_bwd_apply", dev.index, _stream(dev), _p(dlow), C1, 0, _p(src.t1), C1, _p(coef_up), C1,
                             src.D1 * src.H1 * src.W1, src.N, mk, _p(dzl))
                del dg0, dlow
            else:
                skip_grad[lvl] = (dg1, Ct, coef1, Ct)
                # upsampled half -> low-res producer (previous decoder's conv2 or the deepest encoder), ReLU mask fused
                lz, ly, lx = src.los
                nat.call("u3d_gn_bwd_apply_up", dev.index, _stream(dev), _p(dg1), Ct, C0, _p(src.t1), C1, _p(coef1), Ct, src.N,
                         src.D, src.H, src.W, src.D1, src.H1, src.W1, _p(lz), _p(ly), _p(lx),
                         0 if (self.dec_up[j] is not None or self.dec_interp[j] is not None) else mk, _p(dzl))
            del dg1
            if self.dec_up[j] is not None:
                # dzl is the gradient of the transposed convolution's (linear) output: its two gradients, with the non-linearity
                # of the tensor it upsampled
                up = tape.ups[j]
                dzl = getattr(self, self._UP_KERNELS[up.family][1])(cx, up, dzl, mk)
                self._unact(dev, dzl, up.x_low)
            elif self.dec_interp[j] is not None:
                # dzl is the gradient of the interpolated (linear) tensor: the adjoint of the gather, then the non-linearity of
                # the tensor that was upsampled
                up = tape.ups[j]
                xl = up.x_low
                Nl, D1, H1, W1, Cl = xl.shape
                Ds, Hs, Ws = up.tdims
                tz, ty, tx = up.los
                dxl = _empty_like(xl)
                nat.call("u3d_resample2_bwd", dev.index, _stream(dev), _p(dzl), _p(tz[2]), _p(ty[2]), _p(tx[2]), _p(tz[0]), _p(ty[0]),
                         _p(tx[0]), _p(tz[1]), _p(ty[1]), _p(tx[1]), Nl, D1, H1, W1, Ds, Hs, Ws, Cl, _p(dxl))
                if self.act != ACT_NONE:
                    nat.call("u3d_act_bwd", dev.index, _stream(dev), _p(dxl), _p(xl), dxl.numel(), self.act, self.slope, _p(dxl))
                dzl = dxl
            else:
                self._unact(dev, dzl, src.t1)
            dz = dzl

        # decoder + head gradients are final: start their all-reduce now, overlapped with the encoder backward
        if self.grad_sync is not None:
            cx.join()
            self.grad_sync.launch(flat[self.n_enc_params :])

        # ---- encoders, deepest to first
        dx0 = None
        pending_hi = self.n_enc_params  # upper end of the encoder gradients not yet handed to the exchange
        for i in range(n_levels - 1, -1, -1):
            r1, r2 = enc_recs[i]
            dg2, coef2, _ = self._conv_bwd(cx, r2, dz)
            dz1 = self._plain_apply(cx, dg2, coef2, r2.src.t0, mk)
            self._unact(dev, dz1, r2.src.t0)
            del dg2
            dg1, coef1, _ = self._conv_bwd(cx, r1, dz1, need_dg=(i > 0 or need_input_grad))
            if self.grad_sync is not None:
                pending_hi = self._sync_encoder_level(cx, flat, i, pending_hi)  # this level's parameter gradients are final
            if i > 0:
                pooled, argmax, e_in = tape.pools[i - 1]
                Ne, De, He, We, Ce = e_in.shape
                out = _empty_like(e_in)
                sk = skip_grad.pop(i - 1, None)
                # (2-D: the same merges over 2x2 windows, u3d_maxpool2d_*)
                pdims = (Ne, He, We, Ce) if self.is2d else (Ne, De, He, We, Ce)
                sfx = "2d" if self.is2d else "2"
                if sk is None:
                    nat.call(f"u3d_maxpool{sfx}_bwd_merge", dev.index, _stream(dev), _p(dg1), _p(pooled), _p(argmax), _p(coef1), None,
                             _p(e_in), *pdims, mk, _p(out))
                else:
                    sdg, sCdg, scoef, sCt = sk
                    nat.call(f"u3d_maxpool{sfx}_bwd_merge_gn", dev.index, _stream(dev), _p(dg1), _p(pooled), _p(argmax), _p(coef1),
                             _p(sdg), sCdg, _p(scoef), sCt, _p(e_in), *pdims, mk, _p(out))
                    del sk, sdg, scoef
                self._unact(dev, out, e_in)
                dz = out
            elif need_input_grad:
                dx0 = self._plain_apply(cx, dg1, coef1, tape.x0, 0)
            del dg1

        cx.join()
        if self.grad_sync is not None:
            self.grad_sync.finish()

        return flat, self._exit_dx(dx0, tape.dims)
