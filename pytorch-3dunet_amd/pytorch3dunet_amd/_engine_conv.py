"""One SingleConv / ResNetBlock convolution (reference buildingblocks.py:99-135) forward and backward on the native kernels: which
kernel FAMILY runs a layer (first-layer small-Cin, sub-pixel decoder in fp32 or bf16, split-fp32, bf16 operands / bf16 storage, fp32 MFMA)
is decided ONCE, in forward (`_fwd_family`), and kept in the layer's record: `ConvRec.family`, with `sub`, `plus`, `c16`, `f32s` beside it.  Backward maps
the recorded family to its (data-gradient, weight-gradient) families in one place (`_BWD_FAMILY`; `_bwd_families` holds the few
decisions that are backward's own), the shared scratch is sized from the same record (`_family_ws_floats`), and every launcher reads the
record instead of asking the routing rules again — a new family is a new entry in the tables, not a new flag inside the layer code.
Mixin of `engine.UNet3DEngine`."""
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
from ._engine_weights import Kind


class _SubLayers(dict):
    """{id(conv weight): (C0, C1)} of the decoder first convs that take the sub-pixel path at one input size; `plus` = the ids whose level
    upsamples n -> 2n + 1 along some axis; `family` = the `_FWD_KERNELS` row the entries run on (`_subpixel_layers` chooses it) but for
    those of `bf16_ids`, a UNet3D's levels under `bf16_subpixel`, whose row is `subpixel_bf16` (the other entries of such a table are the
    layers outside `_cat_bf16`, on the fp32 sub-pixel kernels as without the key): ask `family_of`"""

    plus = frozenset()
    family = None
    bf16_ids = frozenset()

    def family_of(self, wid):
        return "subpixel_bf16" if wid in self.bf16_ids else self.family


@dataclass
class _ConvCall:
    """everything a forward kernel family needs to launch one convolution (filled by ConvLayers._single_conv_fwd)"""
    dev: torch.device
    conv: torch.nn.Module
    src: VSrc
    affine: torch.Tensor
    y: torch.Tensor
    N: int
    D: int
    H: int
    W: int
    Ctot: int
    Cout: int
    relu: int
    stats: bool                          # the epilogue accumulates (sum, sum of squares) of the written values
    pool: _StatPool
    residual: Optional[torch.Tensor]     # added before the ReLU inside the conv epilogue (pre-norm residual blocks)
    sub: dict                            # sub-pixel layers of this forward (`_SubLayers`): id(weight) -> (C0, C1), and their family
    b16: bool                            # bf16 activation storage
    affine_lo: Optional[torch.Tensor] = None  # sub-pixel layers: compact rows of `affine` for the skip / upsampled channels
    affine_hi: Optional[torch.Tensor] = None
    plus: tuple = (0, 0, 0)              # `_src_plus` of a sub-pixel layer's source
    c16: bool = False                    # a `conv2d_bf16` (`native_2d_stem`) or 3-D `bf16` (`bf16_stem`) layer on the `_c16` envelope
    f32s: bool = False                   # a `conv2d` layer on the six-product kernels of the extension library (`_split2d`)

    def take_stats(self, reps: int = 1) -> Optional[StatTable]:
        return self.pool.table(self.N, self.Cout, reps) if self.stats else None

    @property
    def flops(self):
        return 54.0 * self.Ctot * self.Cout * self.N * self.D * self.H * self.W


@dataclass
class _BwdCall:
    """everything a backward kernel family needs for one convolution (filled by ConvLayers._conv_bwd)"""
    cx: "_BwdCtx"
    rec: ConvRec
    dz: torch.Tensor
    src: VSrc
    N: int
    D: int
    H: int
    W: int
    Cout: int
    b16: bool    # bf16 activation storage
    job: object = None  # U3DGnBwdJob for the weight-gradient reduce launch to carry (the family that takes it sets it back to None)
    greps: int = 1      # replica rows requested for the GroupNorm-backward sums the fp32 data-gradient kernel writes (u3d_conv3d_ex_reps)

    @property
    def flops(self):
        return 54.0 * self.src.C * self.Cout * self.N * self.D * self.H * self.W


class ConvLayers:
    """mixin: layer-level forward / backward building blocks shared by the DoubleConv and the residual executors"""

    def _identity_affine(self, N, C, dev):
        """(N,C,2) table a = 1, b = 0: the 'GroupNorm affine' of a conv input that has no GroupNorm (post-norm orders)"""
        key = ("ida", N, C, str(dev))
        t = self._const.get(key)
        if t is None:
            t = self._const[key] = torch.tensor([1.0, 0.0], dtype=_F32, device=dev).repeat(N, C, 1).contiguous()
        return t

    def _identity_coef(self, N, C, dev):
        """(N,3,C) table p = 1, q = 0, r = 0: GroupNorm backward of 'no GroupNorm' (dx = dg)"""
        key = ("idc", N, C, str(dev))
        t = self._const.get(key)
        if t is None:
            t = self._const[key] = torch.tensor([1.0, 0.0, 0.0], dtype=_F32, device=dev).view(1, 3, 1).repeat(N, 1, C).contiguous()
        return t

    def _unact(self, dev, g, y):
        """in place: gradient w.r.t. the activated tensor y -> gradient w.r.t. its pre-activation (LeakyReLU / ELU; ReLU is
        fused into the producing kernels as a mask, 'no activation' needs nothing)"""
        if self.act in (ACT_LEAKY, ACT_ELU):
            nat.call("u3d_act_bwd", dev.index, _stream(dev), _p(g), _p(y), g.numel(), self.act, self.slope, _p(g))

    def _up_scale(self, dev):
        """(1, 8, 8) on the (p, q, r) rows of a GroupNorm-backward coefficient table: a low-res voxel stands for 8 children (a 2-D
        net: 4, `self.children`)"""
        t = self._up_scale_t
        if t is None or t.device != dev:
            t = self._up_scale_t = torch.tensor([1.0, self.children, self.children], dtype=_F32, device=dev).view(1, 3, 1)
        return t

    def _src_plus(self, src: VSrc):
        """`src.plus` of a sub-pixel layer's source; a 2-D net (D = D1 = 1 is no axis): (0, py, px) under `native_2d_subpixel_plus`, whose
        sub-pixel levels may upsample n -> 2n + 1 along H and W; without it they are exact 2x.  Asked by `_single_conv_fwd`, which records
        the answer (`ConvRec.plus`, `_ConvCall.plus`: what every launcher and backward read), and by `_stats_of`, which runs before it"""
        if not self.is2d:
            return src.plus
        if not self.subpixel2d_plus or src.t1 is None:
            return (0, 0, 0)
        e = (0, src.H - 2 * src.H1, src.W - 2 * src.W1)
        return e if all(v in (0, 1) for v in e) else (0, 0, 0)

    def _subpixel_layers(self, size):
        """decoder first convs whose low-res input is upsampled by exactly 2 — or, round 5, from n to 2n + 1 voxels — in every dimension at
        this input size: {id(weight): (C0, C1)} (+ `.plus`: the ids with an n -> 2n + 1 axis, `.family`: the kernel family of them all) —
        per-call state, handed down as `sub`: forward, `_stats_of` and the image cache read the join of a decoder from it"""
        is2d = self.is2d
        bf16_sub = is2d and self.subpixel2d_bf16  # (`native_2d_bf16_subpixel`: the levels `_bf16_subpixel` accepts, on the bf16 kernels)
        assert not (bf16_sub and self.subpixel)  # (`native_2d_subpixel` refuses the bf16 keys: one family per table)
        bf16_sub3d = not is2d and self.subpixel_bf16  # (`bf16_subpixel`: the levels `_bf16_subpixel3d` accepts, listed in `bf16_ids`)
        if not (self.subpixel or bf16_sub or bf16_sub3d) or any(ct is not None for ct in self.dec_up) or any(self.dec_interp):
            return _SubLayers()  # (a transposed convolution yields 2n-1 voxels, resized to the skip: never an exact 2x replication)
        dims = [tuple(size)[1:] if is2d else tuple(size)]  # (2-D, `native_2d_subpixel`: H and W only)
        for has_pool, _, _ in self.enc:
            if has_pool:
                dims.append(tuple(d // 2 for d in dims[-1]))
        out, plus, bf16_ids = _SubLayers(), set(), set()
        out.family = "subpixel2d_bf16" if bf16_sub else ("subpixel2d" if is2d else "subpixel")
        L = len(self.enc)
        for j, (c1, _) in enumerate(self.dec):
            skip_lvl, low_lvl = L - 2 - j, L - 1 - j
            if skip_lvl < 0 or low_lvl >= len(dims):
                continue
            C0 = self.enc[skip_lvl][2].conv.out_channels
            C1 = c1.conv.in_channels - C0
            # (bf16 mode: the concat is materialised or read in place, an ordinary layer — but for `_bf16_subpixel`, which asks `_cat_bf16`
            # itself: under `native_2d_bf16_subpixel` a layer outside it keeps its fp32 virtual concat)
            if bf16_sub or self._cat_bf16(c1):
                if bf16_sub and self._bf16_subpixel(c1, C0, C1, dims[skip_lvl], dims[low_lvl]):
                    out[id(c1.conv.weight)] = (C0, C1)
                if bf16_sub3d and self._bf16_subpixel3d(c1, C0, C1, dims[skip_lvl], dims[low_lvl]):
                    out[id(c1.conv.weight)] = (C0, C1)
                    bf16_ids.add(id(c1.conv.weight))
                continue
            if not self.subpixel:  # (U3D_SUBPIXEL=0 next to `bf16_subpixel`: no fp32 sub-pixel level)
                continue
            # every axis upsampled by exactly 2, or n -> 2n + 1 (the pooled size of an odd level; round 5: the sub-pixel kernels on a
            # shifted window + the general kernels on the near-boundary slab, _fwd_subpixel / _dgrad_subpixel / _wgrad_subpixel)
            ratio = [a - 2 * b for a, b in zip(dims[skip_lvl], dims[low_lvl])]
            # (2-D: exact 2x only unless `native_2d_subpixel_plus` is set — without it an n -> 2n + 1 level keeps its virtual concat)
            if (all(r in (0, 1) for r in ratio) and ((self.subpixel2d_plus if is2d else self.subpixel_plus) or not any(ratio)) and C0 > 0 and C1 > 0 and C0 % 4 == 0
                    and C1 % 4 == 0 and c1.conv.out_channels % 4 == 0):
                out[id(c1.conv.weight)] = (C0, C1)
                if any(ratio):
                    plus.add(id(c1.conv.weight))
        out.bf16_ids = frozenset(bf16_ids)
        out.plus = frozenset(plus)  # the layers of this call whose packed set includes the slab images (WeightImages.repack)
        return out

    def _stats_of(self, src: VSrc, st0: Optional[StatTable], st1: Optional[StatTable], pool: _StatPool, dev, sub2d_bf16: bool = False):
        """(lo, hi) tables of the per-channel sums of a (virtual) tensor: `hi` holds the upsampled half's when it has a table of its
        own, else None (`lo` covers every channel).  st0 / st1: the producers' tables of the two halves, if they wrote any.
        sub2d_bf16: the layer is a sub-pixel one under `native_2d_bf16_subpixel` (an exact-2x level by `_bf16_subpixel`)."""
        if src.t1 is None:
            if st0 is None:
                st0 = pool.table(src.N, src.C0, self.stat_reps)
                s = src.struct()
                nat.call("u3d_chan_stats_reps", dev.index, _stream(dev), ctypes.byref(s), src.N, src.D, src.H, src.W, *_tab(st0))
            return st0, None
        # (a 2-D net, D = D1 = 1: H and W, and only under `native_2d_subpixel`)
        exact2x = ((self.subpixel2d or sub2d_bf16) and src.H == 2 * src.H1 and src.W == 2 * src.W1) if self.is2d else src.exact2x
        if st0 is not None and st1 is not None and exact2x and self.fused_stats:
            # every low-res voxel is replicated exactly 8x (2-D: every pixel 4x): reuse the producer's sums
            return st0, dataclasses.replace(st1, scale=self.children)
        plus = self._src_plus(src)
        if st0 is not None and plus is not None and any(plus) and self.fused_stats and src.C1 % 4 == 0 and src.t1.dtype == _F32:
            # n -> 2n + 1 along some axes: the first low-res cell of such an axis has three children, every other cell two — the sums of
            # the upsampled half as a weighted pass over the LOW-RES tensor (round 6), the skip half from its producer
            st1w = pool.table(src.N, src.C1)
            if self.is2d:  # (`native_2d_subpixel_plus`: a low-res pixel has one child along z)
                nat.call("u3d_chan_stats_children2d", dev.index, _stream(dev), _p(src.t1), src.N, src.H1, src.W1, src.C1, *plus[1:],
                         _p(st1w.t))
            else:
                nat.call("u3d_chan_stats_children", dev.index, _stream(dev), _p(src.t1), src.N, src.D1, src.H1, src.W1, src.C1, *plus,
                         _p(st1w.t))
            return st0, st1w
        st = pool.table(src.N, src.C, self.stat_reps)
        s = src.struct()
        nat.call("u3d_chan_stats_reps", dev.index, _stream(dev), ctypes.byref(s), src.N, src.D, src.H, src.W, *_tab(st))
        return st, None

    def _norm_finalize(self, kind, mod, lo: StatTable, hi: Optional[StatTable], G, count, affine, dev, split=None):
        """per-(n,c) sums (the `_stats_of` pair) -> the (a, b) table the convolutions / apply passes use; returns what backward needs
        (mean, rstd).  `split` = (Csplit, affine_lo, affine_hi): compact tables of the channel ranges [0, Csplit) / [Csplit, C) written
        in the same launch (GroupNorm over a virtual concat whose halves are read by different kernels; None entries are skipped)"""
        N, C0, sc0 = lo.N, lo.C, lo.scale
        C1, sc1 = (hi.C, hi.scale) if hi is not None else (0, 0.0)
        if kind == "g" and (lo.reps > 1 or (hi is not None and hi.reps > 1)):
            mean_rstd = _empty((N, G, 2), dtype=_F32, device=dev)
            sp = split if split is not None else (0, None, None)
            p1, r1 = _tab(hi)
            nat.call("u3d_gn_finalize_reps", dev.index, _stream(dev), _p(lo.t), C0, sc0, lo.reps, p1, C1, sc1, r1, N, G, count,
                     _p(mod.weight.detach()), _p(mod.bias.detach()), float(mod.eps), _p(affine), _p(mean_rstd), sp[0], _p(sp[1]), _p(sp[2]))
            return mean_rstd
        st0 = lo.folded().t
        st1 = hi.folded().t if hi is not None else None
        if kind == "g":
            mean_rstd = _empty((N, G, 2), dtype=_F32, device=dev)
            if split is not None:
                nat.call("u3d_gn_finalize_split", dev.index, _stream(dev), _p(st0), C0, sc0, _p(st1), C1, sc1, N, G, count,
                         _p(mod.weight.detach()), _p(mod.bias.detach()), float(mod.eps), _p(affine), _p(mean_rstd), split[0],
                         _p(split[1]), _p(split[2]))
                return mean_rstd
            nat.call("u3d_gn_finalize", dev.index, _stream(dev), _p(st0), C0, sc0, _p(st1), C1, sc1, N, G, count,
                     _p(mod.weight.detach()), _p(mod.bias.detach()), float(mod.eps), _p(affine), _p(mean_rstd))
            return mean_rstd
        # nn.BatchNorm3d (buildingblocks.py:78-88): batch statistics + running-estimate update in training, running statistics in eval
        C = C0 + C1
        training = bool(mod.training) or mod.running_mean is None
        mean_rstd = _empty((C, 2), dtype=_F32, device=dev)
        momentum = 0.0
        rm, rv = mod.running_mean, mod.running_var
        if training and rm is not None:
            if self._in_recompute:
                rm = rv = None  # activation checkpointing re-runs this forward in backward: the estimates were updated the first time
            else:
                mod.num_batches_tracked.add_(1)  # (ATen's batch_norm does the same before the kernel)
                momentum = (1.0 / float(mod.num_batches_tracked.item())) if mod.momentum is None else float(mod.momentum)
        nat.call("u3d_bn_finalize", dev.index, _stream(dev), _p(st0), C0, sc0, _p(st1), C1, sc1, N, count, _p(mod.weight.detach()),
                 _p(mod.bias.detach()), float(mod.eps), 1 if training else 0, momentum, _p(rm), _p(rv), _p(affine), _p(mean_rstd))
        return mean_rstd

    def _norm_bwd_job(self, cx, rec: ConvRec, gst, count, coef):
        """The GroupNorm-backward reduction of a layer's input as a job for the launch that reduces the layer's weight gradient
        (u3d_conv3d_wgrad_job: one launch less per layer).  `gst` = (lo, hi): the data gradient's sums, `hi` those of a sub-pixel
        layer's upsampled channels (else None).  Returns (job, coef_hi); job None when the reduction has to run on its own
        (_norm_bwd_finalize); coef_hi: the compact (N,3,C1) table (p, 8q, 8r) of the upsampled channels the job writes, or None."""
        lo, hi = gst
        N, C = lo.N, lo.C + (hi.C if hi is not None else 0)
        if rec.norm != "g" or nat.get_lib().u3d_conv3d_wgrad_job_supported(N, C, rec.G) != 1:
            return None, None
        dev, gview = cx.dev, cx.gview
        job = nat.U3DGnBwdJob()
        coef_hi = None
        job.gstats_lo, job.C0, job.reps_lo = _p(lo.t), lo.C, lo.reps
        if hi is not None:
            coef_hi = _empty((N, 3, hi.C), dtype=_F32, device=dev) if not any(rec.plus) else None
            job.gstats_hi, job.C1, job.hi_scale, job.reps_hi, job.coef_hi = (_p(hi.t), hi.C, self.children, hi.reps,
                                                                             _p(coef_hi))
        else:
            job.gstats_hi, job.C1, job.hi_scale, job.reps_hi, job.coef_hi = None, 0, 1.0, 1, None
        job.mean_rstd, job.gamma = _p(rec.mean_rstd), _p(rec.gn_w.detach())
        job.dgamma, job.dbeta, job.coef = _p(gview(rec.idx_gw)), _p(gview(rec.idx_gb)), _p(coef)
        job.count, job.N, job.G = count, N, rec.G
        return job, coef_hi

    def _norm_bwd_finalize(self, cx, rec: ConvRec, gst, count, coef):
        """the same reduction as launches of its own (`gst` as for _norm_bwd_job); returns coef_hi as _norm_bwd_job does"""
        dev, gview = cx.dev, cx.gview
        lo, hi = gst
        lo = lo.folded()
        N, C = lo.N, lo.C
        g = lo.t
        if hi is not None:
            # sub-pixel decoder layer: the sums of the skip / upsampled channels come from two kernels as two tables
            hi = hi.folded()
            C = lo.C + hi.C
            if rec.norm == "g" and nat.get_lib().u3d_gn_bwd_finalize_split_supported(N, C, rec.G) == 1:
                # ... and the low-res apply pass of an exact-2x level wants the upper channels' (p, 8q, 8r) as a compact table
                coef_hi = _empty((N, 3, hi.C), dtype=_F32, device=dev) if not any(rec.plus) else None
                nat.call("u3d_gn_bwd_finalize_split", dev.index, _stream(dev), _p(lo.t), lo.C, _p(hi.t), hi.C, _p(rec.mean_rstd),
                         _p(rec.gn_w.detach()), N, rec.G, count, _p(gview(rec.idx_gw)), _p(gview(rec.idx_gb)), _p(coef),
                         self.children, _p(coef_hi))
                return coef_hi
            g = torch.cat((lo.t.view(N, lo.C, 2), hi.t.view(N, hi.C, 2)), dim=1)
        if rec.norm == "g":
            nat.call("u3d_gn_bwd_finalize", dev.index, _stream(dev), _p(g), _p(rec.mean_rstd), _p(rec.gn_w.detach()), N, C, rec.G,
                     count, _p(gview(rec.idx_gw)), _p(gview(rec.idx_gb)), _p(coef))
        else:
            nat.call("u3d_bn_bwd_finalize", dev.index, _stream(dev), _p(g), _p(rec.mean_rstd), _p(rec.gn_w.detach()), N, C, count,
                     1 if rec.bn_training else 0, _p(gview(rec.idx_gw)), _p(gview(rec.idx_gb)), _p(coef))
        return None

    def _bf16_layer(self, Cin: int, Cout: int) -> bool:
        """forward AND data gradient of a (Cin -> Cout) 3x3x3 conv can run on the bf16 kernels (both directions need the
        contraction channels % 16 and the produced channels % 32)"""
        return self.bf16 and Cin % 32 == 0 and Cout % 32 == 0

    def _bf16_routed_weight(self, Cin: int, Cout: int, virtual: bool) -> bool:
        """THE rule for a 2-D net in bf16 (`native_2d_bf16`, `native_2d_residual_bf16`), stated once: a 3x3 layer runs forward, data
        gradient and weight gradient on the `conv2d_bf16` family when it reads ONE real tensor (`virtual`: its input is a virtual concat)
        and `_bf16_layer` holds — with or without a residual in its epilogue (u3d_conv2d_bf16_res).  Asked in this form by
        `_weight_images` (which weights get BF16_FWD2D / BF16_DGRAD2D images) and `_layer_ws_floats` (scratch of a layer not yet recorded),
        and through `_bf16_routed` by `_fwd_family` (backward reads its answer from the record), and by `_cat_bf16` for a decoder's
        written-out concat.  Under `native_2d_stem`
        the rule widens to both channel counts % 16 (the net's 16-channel stem layers); a layer only inside the wider rule runs on the
        `_c16` entry points with the `*_C16` images (`_c16`), a layer inside the old one keeps today's.
        THE rule for a UNet3D in bf16 as well: `_bf16_layer`, widened under `bf16_stem` (`stem3d`: the key on a DoubleConv net with fp32
        activation storage) to both channel counts % 16 — such a layer keeps family `bf16` with `c16` in its record and runs on the
        u3d_*_bf16_c16 entry points of the extension library (include/u3d_ext.h) with the BF16_*_C16 images.  Asked by `_fwd_family`
        (which adds the per-call conditions: one real source, no residual, fp32 tensors), `_weight_images`, `_cat_bf16` (a pre-norm
        decoder's 48 -> 16 first convolution runs on its written-out concat) and `_layer_ws_floats`."""
        if virtual:
            return False
        return self._bf16_layer(Cin, Cout) or bool(self.bf16 and (self.stem or self.stem3d) and Cin % 16 == 0 and Cout % 16 == 0)

    def _bf16_vcat(self, src: VSrc, Cout: int) -> bool:
        """THE rule for a decoder's first conv under `native_2d_bf16_vcat`, stated once: the layer runs on the `_src` entry points of the
        `conv2d_bf16` family — reading cat(skip, nearest(low)) through two bases, BF16_FWD2D / BF16_DGRAD2D images as any bf16 layer —
        when the key is on, the model's layer order is pre-norm (as `_cat_bf16` requires), both halves are fp32 tensors with channel
        counts % 32 (the kernels choose the source per 16-channel chunk / 32-channel block) and `_bf16_layer` holds on (C0 + C1, Cout).
        A decoder outside it (16-channel halves under `native_2d_stem`, odd counts) keeps the written-out concat of `_cat_bf16`."""
        return (self.vcat and not self.post_norm and src.t1 is not None and src.C0 > 0 and src.C1 > 0
                and src.C0 % 32 == 0 and src.C1 % 32 == 0 and self._bf16_layer(src.C, Cout)
                and src.t0.dtype == _F32 and src.t1.dtype == _F32 and os.environ.get("U3D_BF16_CAT", "1") != "0")

    def _bf16_subpixel(self, c1, C0: int, C1: int, dims_skip, dims_low) -> bool:
        """THE rule for a decoder's first conv under `native_2d_bf16_subpixel`, stated once: the key is on; the layer is one `_cat_bf16`
        accepts (bf16, a pre-norm order); its level upsamples by exactly 2 on both axes (H == 2 * H1 and W == 2 * W1); C0 % 32 == C1 % 32
        == Cout % 32 == 0 (the envelope of the sub-pixel bf16 kernels and of the skip half's sliced images); both halves are fp32 tensors
        (every activation of a 2-D net is); the upsampling is nearest (`_subpixel_layers` returns before asking when a decoder has a
        transposed convolution or an interpolation).  Asked by `_subpixel_layers` alone: forward, `_stats_of` and the image cache read its
        answer from the `sub` table of the call, backward from the record.  A level outside it — n -> 2n + 1, 16-channel halves under
        `native_2d_stem` — keeps its written-out concat (`_cat_bf16`) or the `_src` entry points (`_bf16_vcat`)."""
        return (self.subpixel2d_bf16 and self._cat_bf16(c1) and not self.post_norm and not self.act_bf16
                and all(a == 2 * b for a, b in zip(dims_skip, dims_low))
                and C0 > 0 and C1 > 0 and C0 % 32 == 0 and C1 % 32 == 0 and c1.conv.out_channels % 32 == 0)

    def _bf16_subpixel3d(self, c1, C0: int, C1: int, dims_skip, dims_low) -> bool:
        """THE rule for a decoder's first conv of a UNet3D under `bf16_subpixel`, stated once: the key is on; the layer is one `_cat_bf16`
        accepts (bf16, a pre-norm order, channel counts the bf16 kernels take); the layer order is pre-norm; bf16 activation storage is
        off; its level upsamples by exactly 2 on all three axes at this input size (the upsampling is nearest: `_subpixel_layers` returns
        before asking when a decoder has a transposed convolution or an interpolation); C0 % 32 == C1 % 32 == Cout % 32 == 0 (the envelope
        of the sub-pixel bf16 kernels and of the skip half's sliced images).  Asked by `_subpixel_layers` alone: forward and the image
        cache read its answer from the `sub` table of the call (`family_of`), backward from the record.  A level outside it — n -> 2n + 1
        on some axis, other channel counts, a post-norm order — keeps its written-out concat (`_cat_bf16`) or, where `_cat_bf16` is
        false, the fp32 virtual-concat kernels, as without the key."""
        return (self.subpixel_bf16 and self._cat_bf16(c1) and not self.post_norm and not self.act_bf16
                and len(dims_skip) == 3 and all(a == 2 * b for a, b in zip(dims_skip, dims_low))
                and C0 > 0 and C1 > 0 and C0 % 32 == 0 and C1 % 32 == 0 and c1.conv.out_channels % 32 == 0)

    def _c16(self, Cin: int, Cout: int) -> bool:
        """a layer `_bf16_routed_weight` accepts lies outside today's envelope: the `_c16` entry points and `*_C16` images are its"""
        return not self._bf16_layer(Cin, Cout)

    def _bf16_routed(self, src: VSrc, Cout: int) -> bool:
        """`_bf16_routed_weight` for a layer about to run on `src` (a virtual one: `_bf16_vcat`)"""
        if src.t1 is not None:
            return self._bf16_vcat(src, Cout)
        return self._bf16_routed_weight(src.C, Cout, False)

    def _bf16_convtr2d(self, Cin: int, Cout: int) -> bool:
        """THE rule for a decoder's ConvTranspose2d under `native_2d_residual_bf16_deconv`, stated once: forward, data gradient and weight
        gradient run on the bf16 u3d_convtr2d_*_bf16 kernels when both channel counts are multiples of 32 (their envelope).  Asked by
        `_up_family` alone."""
        return self.bf16_deconv and Cin % 32 == 0 and Cout % 32 == 0

    def _split_fwd(self, Cin: int, Cout: int) -> bool:
        return self.split and Cin % 16 == 0 and Cout % 32 == 0

    def _split_dgrad(self, Cin: int, Cout: int) -> bool:
        """data gradient of a (Cin -> Cout) conv: contraction over Cout, produces Cin channels"""
        return self.split and Cout % 16 == 0 and Cin % 32 == 0

    def _split_wgrad(self, Cin: int, Cout: int) -> bool:
        """THE rule for the split weight gradient under `fp32_split_wgrad`, stated once: a (Cin -> Cout) weight gradient over ONE real fp32
        source — a single-source layer of the `fp32` weight-gradient family, or the skip slice of a `subpixel` layer — runs on
        u3d_conv3d_wgrad_f32s of the extension library (csrc/u3d_wgrad_f32s.hip) when both channel counts lie in its envelope (% 32).
        Asked by `_wgrad_fp32`, `_wgrad_subpixel`, `_conv_bwd` (that launch takes no GroupNorm-backward job) and `_family_ws_floats`;
        with the key off the extension library is not even loaded."""
        return bool(self.split_wgrad) and nat.get_ext_lib().u3d_conv3d_wgrad_f32s_supported(Cin, Cout) == 1

    def _split_wgrad_call(self, c: "_BwdCall", x, affine, Cin: int, dw, dw_cin_stride: int):
        """u3d_conv3d_wgrad_f32s of one real source into channels [dw, dw + Cin) of the layer's gradient; scratch through `ensure_ws`"""
        cx, dev = c.cx, c.cx.dev
        ws = cx.ensure_ws(nat.get_ext_lib().u3d_wgrad_f32s_workspace_floats(c.N, c.D, c.H, c.W, Cin, c.Cout))
        nat.call("u3d_conv3d_wgrad_f32s", dev.index, _stream(dev), _p(x), _p(affine), _p(c.dz), _p(dw), dw_cin_stride, c.N, c.D, c.H, c.W,
                 Cin, c.Cout, _p(ws), ws.numel(), flops=54.0 * Cin * c.Cout * c.N * c.D * c.H * c.W)

    def _split2d_counts(self, C0: int, C1: int, Cout: int) -> bool:
        """THE rule for a UNet2D under `native_2d_fp32_split` (and for conv2 / conv3 of a ResidualUNet2D's blocks under
        `native_2d_residual_fp32_split`: always a single source), stated once, on channel counts: a 3x3 layer of the `conv2d` family runs
        forward, data gradient and weight gradient on the six-product kernels of the extension library (csrc/u3d_conv2d_f32s.h) when the key
        is on and — a single source (C1 == 0) — both channel counts are multiples of 32, or — a decoder's virtual concat — C0, C1 and Cout
        all are.  A 16 -> 32 layer, the first layer and odd counts keep the fp32 `conv2d` kernels.  Asked by `_split2d` (forward; backward
        reads the record's `f32s`), `_split2d_weights` (which weights get F32S_*2D instead of FWD2D / DGRAD2D images) and
        `_layer_ws_floats`; with the key off the extension library is not loaded."""
        if not self.split2d or Cout <= 0 or Cout % 32 != 0 or C0 <= 0 or C0 % 32 != 0:
            return False
        return C1 == 0 or (C1 > 0 and C1 % 32 == 0)

    def _split2d(self, src: VSrc, Cout: int) -> bool:
        """`_split2d_counts` for a layer about to run on `src`, whose tensors must be fp32 (every activation of a 2-D net is)"""
        return bool(self.split2d) and src.t0.dtype == _F32 and (src.t1 is None or src.t1.dtype == _F32) and \
            self._split2d_counts(src.C0, src.C1, Cout)

    @staticmethod
    def _f32s_src(src: VSrc):
        """the flat source arguments of the u3d_conv2d_*_f32s entry points: (p0, p1, ymap, xmap, C0, C1, H1, W1)"""
        if src.t1 is None:
            return _p(src.t0), None, None, None, src.C0, 0, 0, 0
        return _p(src.t0), _p(src.t1), _p(src.maps[1]), _p(src.maps[2]), src.C0, src.C1, src.H1, src.W1

    def _convtr_t8(self, Cl: int, Cs: int) -> bool:
        """the transposed convolution and its gradients run in space-to-depth form on the bf16 MFMA kernels"""
        return self.bf16 and not self.is2d and nat.get_lib().u3d_convtr3d_t8_supported(Cl, Cs) == 1

    # ---- up-sampling families: a decoder's transposed convolution (csrc file; what selects it) ---------------------------------------
    # (forward launcher (dev, ct, cur) -> up-sampled tensor; backward launcher (cx, up, dt, mk) -> dL/d(x_low), dw written into cx.gview;
    # space-to-depth: between launchers and joining lies T8[i][parity * Ct + c] = t[2i + parity], which the `*_t8` joining kernels take)
    _UP_KERNELS = {
        "t8": ("_up_fwd_t8", "_up_bwd_t8", True),  # u3d_bf16.hip: compute_dtype bf16, summation joining, channels the library takes
        "convtr2d_bf16": ("_up_fwd_convtr2d_bf16", "_up_bwd_convtr2d_bf16", False),  # u3d_conv2d_bf16.hip: `_bf16_convtr2d`
        "convtr2d": ("_up_fwd_convtr2d", "_up_bwd_convtr2d", False),  # u3d_res.hip: every other ConvTranspose2d of a 2-D net
        "convtr3d_subpixel": ("_up_fwd_convtr3d_subpixel", "_up_bwd_convtr3d", False),  # u3d_subpix.hip: both channel counts % 4 == 0
        "convtr3d": ("_up_fwd_convtr3d", "_up_bwd_convtr3d", False),  # u3d_res.hip: the generic gather
    }

    def _up_family(self, Cl: int, Ct: int, concat: bool) -> str:
        """THE rule for a decoder's ConvTranspose (Cl -> Ct, k3 s2 p1), stated once; `concat`: the joining is a concat (the DoubleConv
        executor's virtual one, a residual net's explicit upsample='deconv'), not the sum.  Forward asks and records the answer in
        `UpRec.family`; backward reads the record.  (`_convtr_t8` holds on 3-D nets only: the 2-D rows cannot come before it.)"""
        if self._convtr_t8(Cl, Ct) and not concat:
            return "t8"
        if self.is2d:
            return "convtr2d_bf16" if self._bf16_convtr2d(Cl, Ct) else "convtr2d"
        return "convtr3d_subpixel" if self.subpixel and Cl % 4 == 0 and Ct % 4 == 0 else "convtr3d"

    @staticmethod
    def _up_flops3d(xl, Ct: int) -> float:
        """one pass of a ConvTranspose3d over x_low `xl` (forward; each of the two gradients)"""
        N, D1, H1, W1, Cl = xl.shape
        return 2.0 * 27 * Cl * Ct * N * D1 * H1 * W1

    @staticmethod
    def _up_flops2d(xl, Ct: int) -> float:
        """... of a ConvTranspose2d: 9 taps over the four parity classes of the (2 H1 - 1) x (2 W1 - 1) outputs"""
        N, _, H1, W1, Cl = xl.shape
        return 4.5 * Cl * Ct * N * (2 * H1 - 1) * (2 * W1 - 1)

    def _up_fwd_t8(self, dev, ct, cur):
        # 2x2x2 convolution on the low-res grid into the space-to-depth layout; the resize + join reads that layout directly
        N, D1, H1, W1, Cl = cur.shape
        Ct = ct.out_channels
        t = _empty((N, D1, H1, W1, 8 * Ct), dtype=self.adt, device=dev)
        pk = self.images.get(ct.weight, Kind.T8_FWD, dev)
        need = nat.get_lib().u3d_convtr3d_fwd_t8_workspace_floats(N, D1, H1, W1, Cl, Ct) if self.act_bf16 else 0
        if need > 0:  # small grid, many channels: the flat tile with a split channel reduction (csrc/u3d_bf16.hip)
            kws = _empty(need, dtype=_F32, device=dev)
            nat.call("u3d_convtr3d_fwd_t8_b16_ex", dev.index, _stream(dev), _p(cur), _p(pk), _p(t), N, D1, H1, W1, Cl, Ct, _p(kws), need,
                     flops=self._up_flops3d(cur, Ct))
        else:
            nat.call("u3d_convtr3d_fwd_t8" + ("_b16" if self.act_bf16 else ""), dev.index, _stream(dev), _p(cur), _p(pk), _p(t), N, D1, H1,
                     W1, Cl, Ct, flops=self._up_flops3d(cur, Ct))
        return t

    def _up_fwd_convtr2d(self, dev, ct, cur, entry="u3d_convtr2d_fwd", kind=Kind.CONVTR2D_FWD):
        # four parity-class gather GEMMs (D1 = Dt = 1)
        N, _, H1, W1, Cl = cur.shape
        Ct = ct.out_channels
        t = _empty((N, 1, 2 * H1 - 1, 2 * W1 - 1, Ct), dtype=_F32, device=dev)
        nat.call(entry, dev.index, _stream(dev), _p(cur), _p(self.images.get(ct.weight, kind, dev)), _p(t), N, H1, W1, Cl, Ct,
                 flops=self._up_flops2d(cur, Ct))
        return t

    def _up_fwd_convtr2d_bf16(self, dev, ct, cur):
        # ... on the bf16 matrix pipe, one sub-pixel launch: the same argument list
        return self._up_fwd_convtr2d(dev, ct, cur, "u3d_convtr2d_fwd_bf16", Kind.CONVTR2D_BF16_FWD)

    def _up_fwd_convtr3d_subpixel(self, dev, ct, cur):
        # 8 output parity classes accumulated from one staged input halo tile (scheme Deconv3s2)
        N, D1, H1, W1, Cl = cur.shape
        Ct = ct.out_channels
        t = _empty((N, 2 * D1 - 1, 2 * H1 - 1, 2 * W1 - 1, Ct), dtype=_F32, device=dev)
        nat.call("u3d_convtr3d_fwd_subpixel", dev.index, _stream(dev), _p(cur), _p(self.images.get(ct.weight, Kind.CONVTR_SUBPIXEL, dev)),
                 _p(t), N, D1, H1, W1, Cl, Ct, flops=self._up_flops3d(cur, Ct))
        return t

    def _up_fwd_convtr3d(self, dev, ct, cur):
        N, D1, H1, W1, Cl = cur.shape
        Ct = ct.out_channels
        t = _empty((N, 2 * D1 - 1, 2 * H1 - 1, 2 * W1 - 1, Ct), dtype=_F32, device=dev)
        nat.call("u3d_convtr3d_fwd", dev.index, _stream(dev), _p(cur), _p(ct.weight.detach()), _p(t), N, D1, H1, W1, Cl, Ct,
                 _p(self.images.get(ct.weight, Kind.CONVTR_FWD, dev)), flops=self._up_flops3d(cur, Ct))
        return t

    def _up_bwd_t8(self, cx, up, dt, mk):
        """`dt` in space-to-depth form; dw through the shared fp32 scratch, then dx (ReLU blocks: masked by x_low > 0)"""
        dev, xl = cx.dev, up.x_low
        N, D1, H1, W1, Cl = xl.shape
        Ct = up.weight.shape[1]
        sfx = "_b16" if self.act_bf16 else ""
        lib = nat.get_lib()
        need = max(lib.u3d_convtr3d_wgrad_t8_workspace_floats(N, D1, H1, W1, Cl, Ct),
                   lib.u3d_convtr3d_dgrad_t8_workspace_floats(N, D1, H1, W1, Cl, Ct))  # (both kernels: same stream, one after the other)
        wsb = cx.ensure_ws(need)
        nat.call("u3d_convtr3d_wgrad_t8" + sfx, dev.index, _stream(dev), _p(xl), _p(dt), _p(cx.gview(self._pindex[id(up.weight)])), N, D1,
                 H1, W1, Cl, Ct, _p(wsb), wsb.numel(), flops=self._up_flops3d(xl, Ct))
        dxl = _empty_like(xl)
        nat.call("u3d_convtr3d_dgrad_t8" + sfx + "_ex", dev.index, _stream(dev), _p(dt), _p(self.images.get(up.weight, Kind.T8_DGRAD, dev)),
                 _p(xl) if mk else None, _p(dxl), N, D1, H1, W1, Cl, Ct, _p(wsb), wsb.numel(), flops=self._up_flops3d(xl, Ct))
        return dxl

    def _up_bwd_convtr2d(self, cx, up, dt, mk, bf16=False):
        """dw (double sums in the pool's scratch, written into the flat gradient), then dx masked by x_low > 0"""
        dev, xl = cx.dev, up.x_low
        N, _, H1, W1, Cl = xl.shape
        Ct = up.weight.shape[1]
        sfx = "_bf16" if bf16 else ""
        if bf16:
            scr = cx.ensure_ws(nat.get_lib().u3d_convtr2d_wgrad_bf16_workspace_floats(N, H1, W1, Cl, Ct))
        else:
            scr = cx.pool.take(up.weight.numel())
        nat.call("u3d_convtr2d_wgrad" + sfx, dev.index, _stream(dev), _p(xl), _p(dt), _p(cx.gview(self._pindex[id(up.weight)])), N, H1, W1,
                 Cl, Ct, 0, _p(scr), scr.numel(), flops=self._up_flops2d(xl, Ct))
        dxl = _empty_like(xl)
        kind = Kind.CONVTR2D_BF16_DGRAD if bf16 else Kind.CONVTR2D_DGRAD
        nat.call("u3d_convtr2d_dgrad" + sfx, dev.index, _stream(dev), _p(dt), _p(self.images.get(up.weight, kind, dev)),
                 _p(xl) if mk else None, _p(dxl), N, H1, W1, Cl, Ct, flops=self._up_flops2d(xl, Ct))
        return dxl

    def _up_bwd_convtr2d_bf16(self, cx, up, dt, mk):
        """... with bf16 operands: dw through the shared fp32 scratch in a fixed order; the same argument lists"""
        return self._up_bwd_convtr2d(cx, up, dt, mk, True)

    def _up_bwd_convtr3d(self, cx, up, dt, mk):
        """both gradients in one launch (dx masked by x_low > 0 under `mk`), dw from its double accumulator"""
        dev, xl = cx.dev, up.x_low
        N, D1, H1, W1, Cl = xl.shape
        Ct = up.weight.shape[1]
        acc = cx.pool.take(up.weight.numel())
        dxl = _empty_like(xl)
        nat.call("u3d_convtr3d_bwd", dev.index, _stream(dev), _p(dt), _p(xl), _p(up.weight.detach()), N, D1, H1, W1, Cl, Ct, mk, _p(dxl),
                 _p(acc), _p(self.images.get(up.weight, Kind.CONVTR_DGRAD, dev)), flops=2 * self._up_flops3d(xl, Ct))
        nat.call("u3d_cvt_f64_f32", dev.index, _stream(dev), _p(acc), _p(cx.gview(self._pindex[id(up.weight)])), up.weight.numel())
        return dxl

    # ---- forward kernel families (csrc file; what selects it) -------------------------------------------------------------------
    _FWD_KERNELS = {
        "small": "_fwd_small",        # u3d_smallc.hip: first layer, Cin <= 4
        "subpixel": "_fwd_subpixel",  # u3d_subpix.hip + u3d_conv.hip: cat(skip, nearest2x(low)) on the low-res grid, 8/27 of the MACs
        "f32s": "_fwd_f32s",          # u3d_bf16.hip: compute_dtype fp32_split
        "bf16": "_fwd_bf16",          # u3d_bf16.hip: compute_dtype bf16 (fp32 or bf16 activation storage)
        "fp32": "_fwd_fp32",          # u3d_conv.hip: fp32 MFMA (persistent / generic / split-K chosen by the library)
        "conv2d": "_fwd_conv2d",      # u3d_conv2d.hip: 3x3 convolutions of a 2-D net (native_2d), every layer and only those ...
        "conv2d_bf16": "_fwd_conv2d_bf16",  # u3d_conv2d_bf16.hip: ... except, in bf16, the single-source layers that fit (`_bf16_routed`)
        "small2d": "_fwd_small2d",    # u3d_conv2d.hip: ... and, under `native_2d_stem`, the first layer, Cin <= 4 (the 3-D `small` rule)
        "subpixel2d": "_fwd_subpixel2d",  # u3d_subpix2d.hip + u3d_conv2d.hip: `native_2d_subpixel`, cat(skip, nearest2x(low)), 4/9 of the MACs
        "subpixel2d_bf16": "_fwd_subpixel2d_bf16",  # u3d_conv2d_bf16.hip: `native_2d_bf16_subpixel`, the same on bf16 MFMA (`_bf16_subpixel`)
        "conv2d_bf16_src": "_fwd_conv2d_bf16_src",  # u3d_conv2d_bf16.hip: `native_2d_bf16_vcat`, a decoder's virtual concat read in place
    }

    # ---- a 2-D net (`is2d`): small2d -> subpixel2d | subpixel2d_bf16 (the table's) -> conv2d_bf16 | conv2d_bf16_src | conv2d ----------
    def _fwd_family_2d(self, c: "_ConvCall", residual) -> str:
        if self._small2d(c.Ctot, c.Cout, c.src.t1 is not None) and residual is None:
            return "small2d"
        if c.src.t1 is not None and residual is None and id(c.conv.weight) in c.sub:
            return c.sub.family
        # (a decoder's first conv reaches here on its materialised concat when it fits: `_cat_bf16`; forward and data gradient
        # are covered together by the one channel rule; a residual rides in either family's epilogue)
        if not self._bf16_routed(c.src, c.Cout):
            return "conv2d"
        return "conv2d_bf16" if c.src.t1 is None else "conv2d_bf16_src"  # (`_bf16_vcat`: the `_src` entry points)

    def _fwd_family(self, c: "_ConvCall", residual) -> str:
        if self.is2d:
            return self._fwd_family_2d(c, residual)
        if self.small_cin and c.src.t1 is None and c.Ctot <= 4 and c.Cout <= 32 and residual is None and not c.b16:
            return "small"
        if c.src.t1 is not None and residual is None and id(c.conv.weight) in c.sub:
            return c.sub.family_of(id(c.conv.weight))
        if c.src.t1 is None and self._split_fwd(c.Ctot, c.Cout):
            return "f32s"
        # (`_bf16_routed_weight`: under `bf16_stem` a 16-channel layer too — `c16` in its record — unless it carries a residual or bf16 tensors)
        if c.src.t1 is None and self._bf16_routed_weight(c.Ctot, c.Cout, False) and (
                self._bf16_layer(c.Ctot, c.Cout) or (residual is None and not c.b16)):
            return "bf16"
        return "fp32"

    def _fwd_small(self, c: "_ConvCall"):
        # first layer of the network: K = 27*Cin is too small for the MFMA tiling (csrc/u3d_smallc.hip)
        ystats = c.take_stats(self.stat_reps)
        nat.call("u3d_conv3d_small_cin_fwd_reps", c.dev.index, _stream(c.dev), _p(c.src.t0), _p(c.affine), _p(c.conv.weight.detach()),
                 _p(c.y), c.N, c.D, c.H, c.W, c.Ctot, c.Cout, c.relu, *_tab(ystats), flops=c.flops)
        return ystats

    def _small2d(self, Cin: int, Cout: int, virtual: bool) -> bool:
        """THE rule for the small-Cin family of a 2-D net under `native_2d_stem`, the 3-D `small` rule: a single real source with
        Cin <= 4 and Cout <= 32 (no residual: DoubleConv nets have none).  Asked by `_fwd_family` and `_weight_images` (such a layer gets no
        packed image up front)."""
        return self.stem and self.small_cin and not virtual and Cin <= 4 and Cout <= 32

    def _fwd_small2d(self, c: "_ConvCall"):
        # first layer of a 2-D net under `native_2d_stem`: direct / 16x16x4-MFMA kernels on the reference weight layout (csrc/u3d_conv2d.hip)
        assert c.D == 1 and c.src.t1 is None
        ystats = c.take_stats(self.stat_reps)
        nat.call("u3d_conv2d_small_cin_fwd_reps", c.dev.index, _stream(c.dev), _p(c.src.t0), _p(c.affine), _p(c.conv.weight.detach()),
                 _p(c.y), c.N, c.H, c.W, c.Ctot, c.Cout, c.relu, *_tab(ystats), flops=18.0 * c.Ctot * c.Cout * c.N * c.H * c.W)
        return ystats

    def _fwd_subpixel(self, c: "_ConvCall"):
        # cat(skip, nearest2x(low)): the upsampled half as 8 parity-class 2x2x2 convolutions over the low-res tensor
        # (8/27 of the multiply-adds), then the skip half, whose epilogue adds the partial sums before ReLU / statistics
        dev, conv, src, N, D, H, W, Cout = c.dev, c.conv, c.src, c.N, c.D, c.H, c.W, c.Cout
        pair = C0, C1 = c.sub[id(conv.weight)]
        ystats = c.take_stats(1 if self._split_fwd(C0, Cout) else self.stat_reps)
        part = _empty((N, D, H, W, Cout), dtype=_F32, device=dev)
        D1, H1, W1 = src.D1, src.H1, src.W1
        plus = c.plus
        if any(plus):
            # n -> 2n + 1 along the axes with plus = 1: the sub-pixel kernel writes the window d = u + plus, the general kernel the slab
            # d < 2 of those axes (overwriting the window's first plane, which misses the extra copy of low[0])
            win = (ctypes.c_int * 6)(D, H, W, *plus)
            nat.call("u3d_subpixel_conv_fwd_win", dev.index, _stream(dev), _p(src.t1), _p(c.affine.view(-1)[2 * C0:]), c.Ctot * 2,
                     _p(self.images.get(conv.weight, Kind.UP_FWD, dev, pair)), _p(part), N, D1, H1, W1, C1, Cout, win,
                     flops=128.0 * C1 * Cout * N * D1 * H1 * W1)
            a_hi = c.affine_hi if c.affine_hi is not None else c.affine[:, C0:].contiguous()  # (held: the struct keeps only its pointer)
            s_up = src.up_only_struct(a_hi)
            wp1 = self.images.get(conv.weight, Kind.SLAB_FWD, dev, pair)  # 27-tap forward image of the upsampled channels (slab launches)
            for box in slab_boxes((D, H, W), plus, 2):
                nat.call("u3d_conv3d_box", dev.index, _stream(dev), ctypes.byref(s_up), _p(wp1), _p(part), N, D, H, W, Cout,
                         (ctypes.c_int * 6)(*box), None,
                         flops=54.0 * C1 * Cout * N * (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]))
        else:
            need = nat.get_lib().u3d_subpixel_fwd_workspace_floats(N, D1, H1, W1, C1, Cout)  # split-K scratch, small levels only
            kws = _empty(need, dtype=_F32, device=dev) if need > 0 else None
            nat.call("u3d_subpixel_conv_fwd", dev.index, _stream(dev), _p(src.t1), _p(c.affine.view(-1)[2 * C0:]), c.Ctot * 2,
                     _p(self.images.get(conv.weight, Kind.UP_FWD, dev, pair)), _p(part), N, D1, H1, W1, C1, Cout, _p(kws), need,
                     flops=128.0 * C1 * Cout * N * D1 * H1 * W1)
        a0 = c.affine_lo if c.affine_lo is not None else c.affine[:, :C0].contiguous()
        yp, yr = _tab(ystats)
        if self._split_fwd(C0, Cout):
            nat.call("u3d_conv3d_f32s", dev.index, _stream(dev), _p(src.t0), _p(a0), _p(self.images.get(conv.weight, Kind.F32S_FWD, dev, pair)),
                     _p(c.y), N, D, H, W, C0, Cout, c.relu, yp, None, None, _p(part), None, 0,
                     flops=54.0 * C0 * Cout * N * D * H * W)
        else:
            s0 = VSrc(src.t0).struct(a0)
            nat.call("u3d_conv3d_ex_reps", dev.index, _stream(dev), ctypes.byref(s0), _p(self.images.get(conv.weight, Kind.SKIP_FWD, dev, pair)),
                     _p(c.y), N, D, H, W, Cout, c.relu, yp, None, None, _p(part), None, 0, yr,
                     flops=54.0 * C0 * Cout * N * D * H * W)
        return ystats

    def _fwd_subpixel_bf16(self, c: "_ConvCall"):
        # `bf16_subpixel`: the same two launches on the bf16 MFMA — the upsampled half as 8 parity-class 2x2x2 convolutions with taps
        # pre-summed in fp32 and rounded once (csrc/u3d_subpix_bf16.hip), then the skip half on its sliced 27-tap image, whose epilogue adds
        # the fp32 partial sums before ReLU / statistics (u3d_conv3d_bf16_ex, residual = part).  The concat is never written.
        dev, conv, src, N, D, H, W, Cout = c.dev, c.conv, c.src, c.N, c.D, c.H, c.W, c.Cout
        assert D == 2 * src.D1 and H == 2 * src.H1 and W == 2 * src.W1 and not any(c.plus) and not c.b16
        pair = C0, C1 = c.sub[id(conv.weight)]
        ystats = c.take_stats()
        part = _empty((N, D, H, W, Cout), dtype=_F32, device=dev)
        nat.call("u3d_subpixel_conv_fwd_bf16", dev.index, _stream(dev), _p(src.t1), _p(c.affine.view(-1)[2 * C0:]), c.Ctot * 2,
                 _p(self.images.get(conv.weight, Kind.UP_BF16_FWD, dev, pair)), _p(part), N, src.D1, src.H1, src.W1, C1, Cout,
                 flops=128.0 * C1 * Cout * N * src.D1 * src.H1 * src.W1)
        a0 = c.affine_lo if c.affine_lo is not None else c.affine[:, :C0].contiguous()
        need = nat.get_lib().u3d_conv3d_bf16_workspace_floats(N, D, H, W, C0, Cout)  # split-K scratch on small grids
        kws = _empty(need, dtype=_F32, device=dev) if need > 0 else None
        nat.call("u3d_conv3d_bf16_ex", dev.index, _stream(dev), _p(src.t0), _p(a0), _p(self.images.get(conv.weight, Kind.SKIP_BF16_FWD, dev, pair)),
                 _p(c.y), N, D, H, W, C0, Cout, c.relu, _tab(ystats)[0], None, None, _p(part), _p(kws), need,
                 flops=54.0 * C0 * Cout * N * D * H * W)
        return ystats

    def _fwd_subpixel2d(self, c: "_ConvCall"):
        # `native_2d_subpixel`: the upsampled half as 4 parity-class 2x2 convolutions over the low-res tensor (4/9 of the multiply-adds,
        # csrc/u3d_subpix2d.hip), then the skip half, whose epilogue adds the partial sums before ReLU / statistics (u3d_conv2d_res_reps)
        dev, conv, src, N, H, W, Cout = c.dev, c.conv, c.src, c.N, c.H, c.W, c.Cout
        plus = c.plus
        assert c.D == 1 and H == 2 * src.H1 + plus[1] and W == 2 * src.W1 + plus[2]
        pair = C0, C1 = c.sub[id(conv.weight)]
        ystats = c.take_stats(self.stat_reps)
        part = _empty((N, 1, H, W, Cout), dtype=_F32, device=dev)
        if any(plus):
            # `native_2d_subpixel_plus`, n -> 2n + 1 along the axes with plus = 1: the sub-pixel kernel writes the window d = u + plus, the 3x3
            # kernel the slab d < 2 of those axes (overwriting the window's first row / column, which misses the extra copy of low[0])
            nat.call("u3d_subpixel2d_conv_fwd_win", dev.index, _stream(dev), _p(src.t1), _p(c.affine.view(-1)[2 * C0:]), c.Ctot * 2,
                     _p(self.images.get(conv.weight, Kind.UP_FWD2D, dev, pair)), _p(part), N, src.H1, src.W1, C1, Cout,
                     (ctypes.c_int * 4)(H, W, *plus[1:]), flops=32.0 * C1 * Cout * N * src.H1 * src.W1)
            a_hi = c.affine_hi if c.affine_hi is not None else c.affine[:, C0:].contiguous()  # (held: the struct keeps only its pointer)
            s_up = src.up_only_struct(a_hi)
            wp1 = self.images.get(conv.weight, Kind.SLAB_FWD2D, dev, pair)
            for box in slab_boxes((1, H, W), plus, 2):
                nat.call("u3d_conv2d_box", dev.index, _stream(dev), ctypes.byref(s_up), _p(wp1), _p(part), N, H, W, Cout,
                         (ctypes.c_int * 4)(box[1], box[2], box[4], box[5]), None, None,
                         flops=18.0 * C1 * Cout * N * (box[4] - box[1]) * (box[5] - box[2]))
        else:
            nat.call("u3d_subpixel2d_conv_fwd", dev.index, _stream(dev), _p(src.t1), _p(c.affine.view(-1)[2 * C0:]), c.Ctot * 2,
                     _p(self.images.get(conv.weight, Kind.UP_FWD2D, dev, pair)), _p(part), N, src.H1, src.W1, C1, Cout, None, 0,
                     flops=32.0 * C1 * Cout * N * src.H1 * src.W1)
        a0 = c.affine_lo if c.affine_lo is not None else c.affine[:, :C0].contiguous()
        s0 = VSrc(src.t0).struct(a0)
        need = nat.get_lib().u3d_conv2d_workspace_floats(N, H, W, C0, Cout)  # split-K scratch on small grids
        kws = _empty(need, dtype=_F32, device=dev) if need > 0 else None
        yp, yr = _tab(ystats)
        nat.call("u3d_conv2d_res_reps", dev.index, _stream(dev), ctypes.byref(s0), _p(self.images.get(conv.weight, Kind.SKIP_FWD2D, dev, pair)),
                 _p(c.y), N, H, W, Cout, c.relu, yp, None, None, _p(kws), need, yr, _p(part), flops=18.0 * C0 * Cout * N * H * W)
        return ystats

    def _fwd_subpixel2d_bf16(self, c: "_ConvCall"):
        # `native_2d_bf16_subpixel`: the same two launches on the bf16 MFMA (csrc/u3d_conv2d_bf16.hip) — the upsampled half as 4 parity-class
        # 2x2 convolutions with taps pre-summed in fp32 and rounded once, then the skip half on its sliced image, whose epilogue adds the fp32
        # partial sums before ReLU / statistics (u3d_conv2d_bf16_res).  The concat is never written.
        dev, conv, src, N, H, W, Cout = c.dev, c.conv, c.src, c.N, c.H, c.W, c.Cout
        assert c.D == 1 and H == 2 * src.H1 and W == 2 * src.W1 and not any(c.plus)
        pair = C0, C1 = c.sub[id(conv.weight)]
        ystats = c.take_stats(self.stat_reps)
        part = _empty((N, 1, H, W, Cout), dtype=_F32, device=dev)
        nat.call("u3d_subpixel2d_conv_fwd_bf16", dev.index, _stream(dev), _p(src.t1), _p(c.affine.view(-1)[2 * C0:]), c.Ctot * 2,
                 _p(self.images.get(conv.weight, Kind.UP_BF16_FWD2D, dev, pair)), _p(part), N, src.H1, src.W1, C1, Cout,
                 flops=32.0 * C1 * Cout * N * src.H1 * src.W1)
        a0 = c.affine_lo if c.affine_lo is not None else c.affine[:, :C0].contiguous()
        need = nat.get_lib().u3d_conv2d_bf16_workspace_floats(N, H, W, C0, Cout)  # split-K scratch on small grids
        kws = _empty(need, dtype=_F32, device=dev) if need > 0 else None
        yp, yr = _tab(ystats)
        nat.call("u3d_conv2d_bf16_res", dev.index, _stream(dev), _p(src.t0), _p(a0), _p(self.images.get(conv.weight, Kind.SKIP_BF16_FWD2D, dev, pair)),
                 _p(c.y), N, H, W, C0, Cout, c.relu, yp, None, None, _p(kws), need, yr, _p(part), flops=18.0 * C0 * Cout * N * H * W)
        return ystats

    def _fwd_f32s(self, c: "_ConvCall"):
        # fp32 operands split into three bf16 values each, six partial products on the bf16 MFMA pipe (csrc/u3d_bf16.hip)
        ystats = c.take_stats()
        need = nat.get_lib().u3d_conv3d_bf16_workspace_floats(c.N, c.D, c.H, c.W, c.Ctot, c.Cout)
        kws = _empty(need, dtype=_F32, device=c.dev) if need > 0 else None
        nat.call("u3d_conv3d_f32s", c.dev.index, _stream(c.dev), _p(c.src.t0), _p(c.affine), _p(self.images.get(c.conv.weight, Kind.F32S_FWD, c.dev)),
                 _p(c.y), c.N, c.D, c.H, c.W, c.Ctot, c.Cout, c.relu, _tab(ystats)[0], None, None, _p(c.residual), _p(kws), need,
                 flops=c.flops)
        return ystats

    def _fwd_bf16(self, c: "_ConvCall"):
        # bf16 MFMA operands, fp32 accumulation / epilogue (csrc/u3d_bf16.hip); with bf16 activation storage the input, the
        # output and the residual are bf16 tensors (`_b16` entry point)
        ystats = c.take_stats()
        if c.c16:  # (`bf16_stem`: a 16-channel layer on the extension library's kernel, csrc/u3d_c16_bf16.hip: no residual, no split-K)
            assert c.residual is None and not c.b16
            nat.call("u3d_conv3d_bf16_c16", c.dev.index, _stream(c.dev), _p(c.src.t0), _p(c.affine),
                     _p(self.images.get(c.conv.weight, Kind.BF16_FWD_C16, c.dev)), _p(c.y), c.N, c.D, c.H, c.W, c.Ctot, c.Cout, c.relu,
                     _tab(ystats)[0], None, None, None, 0, flops=c.flops)
            return ystats
        need = nat.get_lib().u3d_conv3d_bf16_workspace_floats(c.N, c.D, c.H, c.W, c.Ctot, c.Cout)  # split-K scratch at the bottom of the U
        kws = _empty(need, dtype=_F32, device=c.dev) if need > 0 else None
        nat.call("u3d_conv3d_bf16_ex" + ("_b16" if c.b16 else ""), c.dev.index, _stream(c.dev), _p(c.src.t0), _p(c.affine),
                 _p(self.images.get(c.conv.weight, Kind.BF16_FWD, c.dev)), _p(c.y), c.N, c.D, c.H, c.W, c.Ctot, c.Cout, c.relu, _tab(ystats)[0], None, None,
                 _p(c.residual), _p(kws), need, flops=c.flops)
        return ystats

    def _fwd_conv2d(self, c: "_ConvCall"):
        # fp32 MFMA 3x3 implicit GEMM on the D = 1 tensors (virtual concat, fused affine, ReLU and statistics as the 3-D kernels);
        # with a residual (ResidualUNet2D's conv3): out = [relu](conv + residual) in the epilogue (u3d_conv2d_res_reps)
        assert c.D == 1
        if c.f32s:  # (`native_2d_fp32_split`, `_split2d`: six bf16 products of split operands, csrc/u3d_conv2d_f32s.h; no split-K scratch)
            wp = self.images.get(c.conv.weight, Kind.F32S_FWD2D, c.dev)
            ystats = c.take_stats(self.stat_reps)
            if c.residual is not None:  # (`native_2d_residual_fp32_split`: a ResNetBlock's conv3 in a pre-norm order, one real source)
                assert c.src.t1 is None
                nat.call("u3d_conv2d_f32s_res", c.dev.index, _stream(c.dev), _p(c.src.t0), _p(c.affine), _p(wp), _p(c.y), c.N, c.H, c.W,
                         c.Ctot, c.Cout, c.relu, *_tab(ystats), _p(c.residual), flops=18.0 * c.Ctot * c.Cout * c.N * c.H * c.W)
                return ystats
            nat.call("u3d_conv2d_f32s", c.dev.index, _stream(c.dev), *self._f32s_src(c.src), _p(c.affine), _p(wp), _p(c.y), c.N, c.H, c.W,
                     c.Cout, c.relu, *_tab(ystats), flops=18.0 * c.Ctot * c.Cout * c.N * c.H * c.W)
            return ystats
        wp = self.images.get(c.conv.weight, Kind.FWD2D, c.dev)
        ystats = c.take_stats(self.stat_reps)
        s = c.src.struct(c.affine)
        need = nat.get_lib().u3d_conv2d_workspace_floats(c.N, c.H, c.W, c.Ctot, c.Cout)  # split-K scratch on small grids
        kws = _empty(need, dtype=_F32, device=c.dev) if need > 0 else None
        yp, yr = _tab(ystats)
        if c.residual is not None:
            nat.call("u3d_conv2d_res_reps", c.dev.index, _stream(c.dev), ctypes.byref(s), _p(wp), _p(c.y), c.N, c.H, c.W, c.Cout, c.relu,
                     yp, None, None, _p(kws), need, yr, _p(c.residual), flops=18.0 * c.Ctot * c.Cout * c.N * c.H * c.W)
        else:
            nat.call("u3d_conv2d_ex_reps", c.dev.index, _stream(c.dev), ctypes.byref(s), _p(wp), _p(c.y), c.N, c.H, c.W, c.Cout, c.relu,
                     yp, None, None, _p(kws), need, yr, flops=18.0 * c.Ctot * c.Cout * c.N * c.H * c.W)
        return ystats

    def _fwd_conv2d_bf16(self, c: "_ConvCall"):
        # bf16 MFMA operands, fp32 accumulation / epilogue on the D = 1 tensors (csrc/u3d_conv2d_bf16.hip): fused affine (rounded once
        # after it), ReLU and statistics as the fp32 kernel; with a residual (ResidualUNet2D's conv3 in a pre-norm order): out =
        # [relu](conv + residual), the fp32 residual added to the fp32 sum in the epilogue (u3d_conv2d_bf16_res)
        c16 = c.c16  # (a 16-channel stem layer under `native_2d_stem`: same kernels, `_c16` envelope)
        assert c.D == 1 and c.src.t1 is None and not (c16 and c.residual is not None)
        wp = self.images.get(c.conv.weight, Kind.BF16_FWD2D_C16 if c16 else Kind.BF16_FWD2D, c.dev)
        ystats = c.take_stats(self.stat_reps)
        lib = nat.get_lib()
        need = (lib.u3d_conv2d_bf16_c16_workspace_floats if c16 else lib.u3d_conv2d_bf16_workspace_floats)(
            c.N, c.H, c.W, c.Ctot, c.Cout)  # split-K scratch on small grids
        kws = _empty(need, dtype=_F32, device=c.dev) if need > 0 else None
        yp, yr = _tab(ystats)
        args = [c.dev.index, _stream(c.dev), _p(c.src.t0), _p(c.affine), _p(wp), _p(c.y), c.N, c.H, c.W, c.Ctot, c.Cout, c.relu, yp, None,
                None, _p(kws), need, yr]
        if c.residual is not None:  # (the `_res` entry point: the same arguments plus the residual)
            args.append(_p(c.residual))
        nat.call("u3d_conv2d_bf16_res" if c.residual is not None else ("u3d_conv2d_bf16_c16" if c16 else "u3d_conv2d_bf16"), *args,
                 flops=18.0 * c.Ctot * c.Cout * c.N * c.H * c.W)
        return ystats

    def _fwd_conv2d_bf16_src(self, c: "_ConvCall"):
        # ... on a decoder's virtual concat (`_bf16_vcat`): same plan, image and scratch, `_src` entry point
        assert c.D == 1 and c.residual is None and not c.c16
        wp = self.images.get(c.conv.weight, Kind.BF16_FWD2D, c.dev)
        ystats = c.take_stats(self.stat_reps)
        need = nat.get_lib().u3d_conv2d_bf16_workspace_floats(c.N, c.H, c.W, c.Ctot, c.Cout)
        kws = _empty(need, dtype=_F32, device=c.dev) if need > 0 else None
        yp, yr = _tab(ystats)
        s = c.src.struct(c.affine)
        nat.call("u3d_conv2d_bf16_src", c.dev.index, _stream(c.dev), ctypes.byref(s), _p(wp), _p(c.y), c.N, c.H, c.W, c.Cout, c.relu,
                 yp, _p(kws), need, yr, flops=18.0 * c.Ctot * c.Cout * c.N * c.H * c.W)
        return ystats

    def _fwd_fp32(self, c: "_ConvCall"):
        wp = self.images.get(c.conv.weight, Kind.FWD, c.dev)
        ystats = c.take_stats(self.stat_reps)  # (replica rows: the persistent kernel's blocks spread their same-address f64 atomics)
        s = c.src.struct(c.affine)
        # bottom-of-the-U shapes split the channel reduction over blocks through a scratch buffer (0 floats otherwise)
        need = nat.get_lib().u3d_conv3d_workspace_floats(c.N, c.D, c.H, c.W, c.Ctot, c.Cout)
        kws = _empty(need, dtype=_F32, device=c.dev) if need > 0 else None
        yp, yr = _tab(ystats)
        nat.call("u3d_conv3d_ex_reps", c.dev.index, _stream(c.dev), ctypes.byref(s), _p(wp), _p(c.y), c.N, c.D, c.H, c.W, c.Cout, c.relu,
                 yp, None, None, _p(c.residual), _p(kws), need, yr, flops=c.flops)
        return ystats

    def _single_conv_fwd(self, sc, name, src: VSrc, st_in, pool: _StatPool, tape: Optional[Tape], want_stats=True,
                         residual: Optional[torch.Tensor] = None, sub=(), y_out: Optional[torch.Tensor] = None, act=None,
                         record_only: bool = False):
        """One SingleConv (buildingblocks.py:99-135) in any native order (parse_order): 'gcr' = GroupNorm -> Conv3d -> ReLU fully
        fused; other non-linearities / GroupNorm after the conv add one bandwidth pass (csrc/u3d_act.hip).  With `residual`:
        f(conv(GN(x)) + residual), the tail of ResNetBlock.forward (buildingblocks.py:277-288; `act` = the block's f)."""
        dev = src.t0.device
        conv = sc.conv
        spec = layer_spec(sc.order)
        gn = getattr(sc, "groupnorm", None) if spec.norm == "g" else (getattr(sc, "batchnorm", None) if spec.norm == "b" else None)
        N, D, H, W = src.N, src.D, src.H, src.W
        Ctot, Cout = src.C, conv.out_channels
        G = gn.num_groups if spec.norm == "g" else 1
        post = not spec.pre  # the conv input has no norm of its own (post-norm and norm-free layers)
        act, slope = (spec.act, spec.slope) if act is None else act
        inner, islope = spec.inner, spec.islope  # 'crg' family: non-linearity on the conv output BEFORE its norm
        assert conv.in_channels == Ctot and (gn is None or getattr(gn, "num_channels", getattr(gn, "num_features", None)) == (Cout if post else Ctot))
        relu = 1 if ((act == ACT_RELU and not post) or inner == ACT_RELU) else 0
        # `out += residual` follows the block's last GroupNorm: inside the conv epilogue for pre-norm orders, in the
        # GroupNorm-apply pass for post-norm orders
        conv_res = None if post else residual
        # the conv epilogue's statistics describe the conv OUTPUT: they are the next GroupNorm's input only when nothing
        # else transforms it (ReLU is in the epilogue); a post-norm layer needs them for its own GroupNorm
        want_stats = ((post and spec.norm is not None and inner in (ACT_NONE, ACT_RELU))
                      or (not post and want_stats and act in (ACT_NONE, ACT_RELU)))
        # ONE flag for the finalize call (batch vs running statistics) and for backward (mean / rstd functions of x vs constants): a
        # BatchNorm3d without running estimates normalises with batch statistics in eval mode too (_norm_finalize)
        bn_training = (bool(gn.training) or gn.running_mean is None) if spec.norm == "b" else True
        split = None  # sub-pixel layers: compact (N,C0,2) / (N,C1,2) copies of the affine rows, written by the finalize launch
        pair = sub.get(id(conv.weight)) if (sub and src.t1 is not None and residual is None) else None  # (C0, C1) of a sub-pixel layer
        plus = self._src_plus(src) if pair is not None else (0, 0, 0)
        if post:
            affine, mean_rstd = self._identity_affine(N, Ctot, dev), None
        else:
            affine = _empty((N, Ctot, 2), dtype=_F32, device=dev)
            if spec.norm == "g" and pair is not None:
                # sub-pixel layer: its two halves are read by different kernels as plain tensors
                Cs0, Cs1 = pair
                split = (Cs0, _empty((N, Cs0, 2), dtype=_F32, device=dev),
                         _empty((N, Cs1, 2), dtype=_F32, device=dev) if any(plus) else None)
            mean_rstd = self._norm_finalize(spec.norm, gn, *st_in, G, float(D * H * W), affine, dev, split)
        # y_out: recomputation under activation checkpointing rewrites the (still alive) block output in place with the
        # bit-identical values instead of allocating a second copy
        b16 = src.t0.dtype == torch.bfloat16  # bf16 activation storage: only the bf16-operand branch below handles it
        if b16:
            assert self.act_bf16 and src.t1 is None and not post and self._bf16_layer(Ctot, Cout) and act == ACT_RELU, \
                "bf16 activation storage reached a layer outside its envelope"
        y = y_out if (y_out is not None and not post) else _empty((N, D, H, W, Cout), dtype=src.t0.dtype if b16 else _F32, device=dev)
        # ---- the convolution itself: ONE decision (which kernel family), then the family's launcher from the table
        call = _ConvCall(dev, conv, src, affine, y, N, D, H, W, Ctot, Cout, relu, bool(want_stats and self.fused_stats), pool, conv_res,
                         sub, b16, *(split[1:] if split is not None else (None, None)), plus)
        family = self._fwd_family(call, residual)
        call.c16 = family in ("conv2d_bf16", "bf16") and self._c16(Ctot, Cout)
        call.f32s = family == "conv2d" and self._split2d(src, Cout)  # (a residual rides in `u3d_conv2d_f32s_res`'s epilogue)
        dmod = getattr(sc, "dropout", None) if spec.drop == "d" else (getattr(sc, "dropout2d", None) if spec.drop == "D" else None)
        rec = None
        if tape is not None:
            # (the routing above included; the normal path completes it at the end: a post-norm layer's output and statistics, the dropout)
            rec = ConvRec(name=name, src=src, affine=affine, mean_rstd=mean_rstd, y=y, gn_w=gn.weight if gn is not None else None,
                          conv_w=conv.weight, G=G, idx_gw=self._pindex[id(gn.weight)] if gn is not None else -1,
                          idx_gb=self._pindex[id(gn.bias)] if gn is not None else self._pindex[id(conv.bias)],
                          idx_w=self._pindex[id(conv.weight)], family=family, sub=pair, plus=plus, c16=call.c16, f32s=call.f32s, pre_norm=not post,
                          norm=spec.norm, bn_training=bn_training, affine_lo=call.affine_lo, affine_hi=call.affine_hi)
            tape.convs.append(rec)
        # record_only (recomputation under activation checkpointing, the block's LAST convolution): y_out still holds this layer's final
        # output — the block output the forward pass kept — so only what backward needs beside it is rebuilt (the GroupNorm tables of
        # the layer's input, above): no convolution launch, no in-place activation pass.  Not for post-norm orders (backward wants the
        # pre-norm tensor z) and not under dropout (its mask belongs to the record).
        if record_only and y_out is not None and not post and not (dmod is not None and dmod.training and dmod.p > 0.0):
            return y, None
        ystats = self._launcher(0, family)(call)
        post_rec = None
        if post:
            # GroupNorm over the conv output z (statistics from the conv epilogue), then the non-linearity: y = f(a*z + b);
            # 'crg' family: z is already f_inner(conv) (ReLU in the epilogue, LeakyReLU / ELU in place here)
            if inner in (ACT_LEAKY, ACT_ELU):
                nat.call("u3d_act_fwd", dev.index, _stream(dev), _p(y), y.numel(), inner, islope, _p(y))
            z, zst = y, ystats
            aff2 = _empty((N, Cout, 2), dtype=_F32, device=dev)
            if spec.norm is None:
                # no norm: the conv's bias (buildingblocks.py:54-55) is the constant affine (1, bias)
                nat.call("u3d_bias_table", dev.index, _stream(dev), _p(conv.bias.detach()), N, Cout, _p(aff2))
            else:
                if zst is None and (spec.norm == "g" or bn_training):
                    zst = self._stats_of(VSrc(z), None, None, pool, dev)[0]
                mean_rstd = self._norm_finalize(spec.norm, gn, zst, None, G, float(D * H * W), aff2, dev)
            y = y_out if y_out is not None else _empty_like(z)
            nat.call("u3d_affine_add_act_fwd", dev.index, _stream(dev), _p(z), _p(aff2), _p(residual), N, D * H * W, Cout, act,
                     slope, _p(y))
            post_rec, ystats = (z, aff2, inner, islope), None
        elif act in (ACT_LEAKY, ACT_ELU):
            nat.call("u3d_act_fwd", dev.index, _stream(dev), _p(y), y.numel(), act, slope, _p(y))
            ystats = None
        drop_rec = None
        if dmod is not None and dmod.training and dmod.p > 0.0:
            # The MASK comes from torch's generator exactly as the reference draws it (F.dropout on an NCDHW tensor of this
            # shape / feature_dropout's (N,C,1,1,1) noise: same Philox consumption, same element order), applied natively.
            if spec.drop == "d":
                m = F.dropout(torch.ones((N, Cout, D, H, W), dtype=_F32, device=dev), dmod.p, True)
                if Cout == 1:
                    mask = m.view(N, D, H, W, 1)
                else:
                    mask = _empty((N, D, H, W, Cout), dtype=_F32, device=dev)
                    nat.call("u3d_ncdhw_to_ndhwc", dev.index, _stream(dev), _p(m), _p(mask), N, Cout, D * H * W)
                nat.call("u3d_mul", dev.index, _stream(dev), _p(y), _p(mask), y.numel(), _p(y))
                drop_rec = ("d", mask)
            else:
                m = torch.feature_dropout(torch.ones((N, Cout, 1, 1, 1), dtype=_F32, device=dev), dmod.p, True).view(N, Cout)
                table = torch.stack((m, torch.zeros_like(m)), dim=-1).contiguous()
                nat.call("u3d_affine_act_fwd", dev.index, _stream(dev), _p(y), _p(table), N, D * H * W, Cout, ACT_NONE, 0.0, _p(y))
                drop_rec = ("D", table)
            ystats = None  # the epilogue's sums describe the tensor before the dropout
        if rec is not None:
            rec.mean_rstd, rec.y, rec.post, rec.drop = mean_rstd, y, post_rec, drop_rec
        return y, ystats

    # ---- backward kernel families ---------------------------------------------------------------------------------------------------
    _WGRAD_KERNELS = {
        "bf16": "_wgrad_bf16",          # u3d_bf16.hip (Cin % 32 == 0 and Cout % 32 == 0: every layer the bf16 forward covers)
        "subpixel": "_wgrad_subpixel",  # u3d_subpix.hip (upsampled channels) + u3d_conv.hip strided (skip channels)
        "fp32_side": "_wgrad_fp32_side",  # u3d_conv.hip on the side stream (U3D_SIDE_VOXELS, off by default)
        "fp32": "_wgrad_fp32",          # u3d_conv.hip
        "conv2d": "_wgrad_conv2d",      # u3d_conv2d.hip (2-D nets)
        "conv2d_bf16": "_wgrad_conv2d_bf16",  # u3d_conv2d_bf16.hip (2-D nets in bf16: every layer the bf16 forward covers)
        "subpixel2d": "_wgrad_subpixel2d",  # u3d_subpix2d.hip (upsampled channels) + u3d_conv2d.hip strided (skip channels)
        "subpixel2d_bf16": "_wgrad_subpixel2d_bf16",  # u3d_conv2d_bf16.hip: both channel slices on bf16 MFMA
    }
    _DGRAD_KERNELS = {
        "subpixel": "_dgrad_subpixel",  # skip half at full resolution + upsampled half directly at LOW resolution
        "f32s": "_dgrad_f32s",
        "bf16": "_dgrad_bf16",
        "fp32": "_dgrad_fp32",
        "conv2d": "_dgrad_conv2d",  # u3d_conv2d.hip (2-D nets)
        "conv2d_bf16": "_dgrad_conv2d_bf16",  # u3d_conv2d_bf16.hip
        "subpixel2d": "_dgrad_subpixel2d",  # u3d_conv2d.hip (skip half) + u3d_subpix2d.hip (upsampled half at LOW resolution)
        "subpixel2d_bf16": "_dgrad_subpixel2d_bf16",  # u3d_conv2d_bf16.hip: both halves on bf16 MFMA
    }

    # `bf16_subpixel` (a UNet3D's levels `_bf16_subpixel3d` accepts): the family `subpixel_bf16`, its three launchers in a table of its own.
    # The three tables above hold the families that replaced a by-shape ladder of backward, and each of their rows is held against that
    # ladder; this family was never chosen by shape — only `_subpixel_layers` names it, forward records it, backward reads the record.
    _RECORDED_ONLY = {
        "subpixel_bf16": ("_fwd_subpixel_bf16",    # u3d_subpix_bf16.hip + u3d_bf16.hip: the upsampled half on the low-res grid, then the skip half
                          "_dgrad_subpixel_bf16",  # u3d_bf16.hip (skip half) + u3d_subpix_bf16.hip (upsampled half at LOW resolution)
                          "_wgrad_subpixel_bf16"),  # u3d_subpix_bf16.hip + u3d_bf16.hip strided: both channel slices on bf16 MFMA
    }

    def _launcher(self, which: int, family: str):
        """the bound launcher of `family`: which = 0 forward (`_FWD_KERNELS`), 1 data gradient, 2 weight gradient; or its `_RECORDED_ONLY` row"""
        table = (self._FWD_KERNELS, self._DGRAD_KERNELS, self._WGRAD_KERNELS)[which]
        return getattr(self, table[family] if family in table else self._RECORDED_ONLY[family][which])

    # the family forward recorded (`ConvRec.family`, a row of _FWD_KERNELS) -> the family of its two gradients, where the name differs: the
    # small families when a data gradient is needed, the split forward, the `_src` entry points (which the `conv2d_bf16` launchers call)
    _BWD_FAMILY = {"small": "fp32", "f32s": "fp32", "small2d": "conv2d", "conv2d_bf16_src": "conv2d_bf16"}

    def _bwd_families(self, cx, rec: ConvRec, need_dg=True):
        """(data-gradient family, weight-gradient family) of a recorded layer: the table's answer, but for the decisions that are backward's
        own.  (None, None): the small families' one-pass backward (dw and the GroupNorm-backward sums, no data gradient)."""
        if rec.small and not need_dg:
            return None, None
        dgrad = wgrad = self._BWD_FAMILY.get(rec.family, rec.family)
        src, Cout = rec.src, rec.y.shape[-1]
        if rec.family in ("f32s", "fp32") and src.t1 is None and self._split_dgrad(src.C, Cout):
            dgrad = "f32s"  # (the forward's channel rule with the roles swapped: 16 -> 32 is split forward only, 32 -> 16 backward only)
        if wgrad == "bf16" and Cout % 32 != 0 and not rec.c16:  # (Cout % 64 == 32 since round 4: 64-column blocks with a zero upper half;
            # a `c16` record's weight gradient is the extension library's, whose envelope is % 16)
            wgrad = "fp32"
        if wgrad == "fp32" and self.overlap_small_wgrad and src.N * src.D * src.H * src.W <= cx.SIDE_MAX_VOXELS and self.debug is None:
            wgrad = "fp32_side"  # (U3D_SIDE_VOXELS, off by default)
        return dgrad, wgrad

    def _wgrad_bf16(self, c: "_BwdCall"):
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        if rec.c16:  # (`bf16_stem`: takes no GroupNorm-backward job — c.job stays set and _conv_bwd runs the reduction on its own)
            ws = cx.ensure_ws(nat.get_ext_lib().u3d_wgrad_bf16_c16_workspace_floats(c.N, c.D, c.H, c.W, src.C, c.Cout))
            nat.call("u3d_conv3d_wgrad_bf16_c16", dev.index, _stream(dev), _p(src.t0), _p(rec.affine), _p(c.dz), _p(cx.gview(rec.idx_w)),
                     c.N, c.D, c.H, c.W, src.C, c.Cout, _p(ws), ws.numel(), flops=c.flops)
            return
        need = nat.get_lib().u3d_wgrad_bf16_workspace_floats(c.N, c.D, c.H, c.W, src.C, c.Cout)
        ws = cx.ensure_ws(need)
        dw = cx.gview(rec.idx_w)
        job = c.job
        # the GroupNorm-backward reduction of the layer's input rides in the launch that adds the splits — where there is one
        if job is not None and nat.get_lib().u3d_conv3d_wgrad_bf16_job_supported(c.N, c.D, c.H, c.W, src.C, c.Cout, 1 if c.b16 else 0, _p(dw),
                                                                                  job.N, job.C0 + job.C1, job.G) != 1:
            job = None
        nat.call("u3d_conv3d_wgrad_bf16" + ("_b16" if c.b16 else "") + "_job", dev.index, _stream(dev), _p(src.t0), _p(rec.affine), _p(c.dz),
                 _p(dw), c.N, c.D, c.H, c.W, src.C, c.Cout, _p(ws), ws.numel(), ctypes.byref(job) if job is not None else None,
                 flops=c.flops)
        if job is not None:
            c.job = None

    def _wgrad_subpixel(self, c: "_BwdCall"):
        # weight gradient in two channel slices of the same (Cout, Ctot, 27) buffer: upsampled channels from the 64
        # (parity class, tap half) matrices over the low-res grid, skip channels from the standard kernel
        cx, dev, src, rec, ws = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws
        C0, C1 = rec.sub
        Ct = src.C
        dwv = cx.gview(rec.idx_w)
        plus = rec.plus
        if any(plus):
            # n -> 2n + 1: outputs d >= 2 of the shifted axes through the windowed sub-pixel kernel, the slab d < 2 through the general
            # kernel on disjoint boxes of dz (each into scratch, added to the same channel slice)
            win = (ctypes.c_int * 9)(c.D, c.H, c.W, *plus, *plus)
            nat.call("u3d_subpixel_conv_wgrad_win", dev.index, _stream(dev), _p(src.t1), _p(rec.affine.view(-1)[2 * C0:]), Ct * 2,
                     _p(c.dz), _p(dwv[C0 * 27:]), Ct, c.N, src.D1, src.H1, src.W1, C1, c.Cout, _p(ws), ws.numel(), win,
                     flops=128.0 * C1 * c.Cout * c.N * src.D1 * src.H1 * src.W1)
            a_hi = rec.affine_hi if rec.affine_hi is not None else rec.affine[:, C0:].contiguous()  # (held across the loop, as above)
            s_up = src.up_only_struct(a_hi)
            slice_view = dwv.view(c.Cout, Ct, 27)[:, C0:, :]
            for box in slab_boxes((c.D, c.H, c.W), plus, 2):
                tmp = _empty((c.Cout, C1, 27), dtype=_F32, device=dev)
                nat.call("u3d_conv3d_wgrad_box", dev.index, _stream(dev), ctypes.byref(s_up), _p(c.dz), _p(tmp), c.N, c.D, c.H, c.W,
                         c.Cout, _p(ws), ws.numel(), (ctypes.c_int * 6)(*box),
                         flops=54.0 * C1 * c.Cout * c.N * (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]))
                slice_view += tmp
        else:
            nat.call("u3d_subpixel_conv_wgrad", dev.index, _stream(dev), _p(src.t1), _p(rec.affine.view(-1)[2 * C0:]), Ct * 2,
                     _p(c.dz), _p(dwv[C0 * 27:]), Ct, c.N, src.D1, src.H1, src.W1, C1, c.Cout, _p(ws), ws.numel(),
                     flops=128.0 * C1 * c.Cout * c.N * src.D1 * src.H1 * src.W1)
        a0 = rec.affine_lo if rec.affine_lo is not None else rec.affine[:, :C0].contiguous()
        if self._split_wgrad(C0, c.Cout):  # (`fp32_split_wgrad`: the skip slice alone; no job — c.job stays set for _conv_bwd's finalize)
            self._split_wgrad_call(c, src.t0, a0, C0, dwv, Ct)
            return
        s0 = VSrc(src.t0).struct(a0)
        nat.call("u3d_conv3d_wgrad_job", dev.index, _stream(dev), ctypes.byref(s0), _p(c.dz), _p(dwv), Ct, c.N, c.D, c.H, c.W,
                 c.Cout, _p(ws), ws.numel(), ctypes.byref(c.job) if c.job is not None else None,
                 flops=54.0 * C0 * c.Cout * c.N * c.D * c.H * c.W)
        c.job = None

    def _wgrad_fp32_side(self, c: "_BwdCall"):
        # small layer: neither kernel fills the chip on its own -> weight gradient on the side stream, data gradient
        # on the caller's stream; joined before anything consumes the flat gradient buffer
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        s_aff = src.struct(rec.affine)
        need = nat.get_lib().u3d_wgrad_workspace_floats(c.N, c.D, c.H, c.W, src.C, c.Cout)
        side = cx.side_stream(need)
        side.wait_stream(torch.cuda.current_stream(dev))  # dz (and the flat buffer) are ready
        with torch.cuda.stream(side):
            nat.call("u3d_conv3d_wgrad", dev.index, _stream(dev), ctypes.byref(s_aff), _p(c.dz), _p(cx.gview(rec.idx_w)), c.N,
                     c.D, c.H, c.W, c.Cout, _p(cx.ws_side), cx.ws_side.numel(), flops=c.flops)
        c.dz.record_stream(side)  # dz is released on the main stream while the side stream may still read it
        cx.side_used = True

    def _wgrad_fp32(self, c: "_BwdCall"):
        cx, dev, src, rec, ws = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws
        if src.t1 is None and self._split_wgrad(src.C, c.Cout):
            # (`fp32_split_wgrad`: takes no GroupNorm-backward job — c.job stays set and _conv_bwd runs the reduction on its own)
            self._split_wgrad_call(c, src.t0, rec.affine, src.C, cx.gview(rec.idx_w), src.C)
            return
        s_aff = src.struct(rec.affine)
        nat.call("u3d_conv3d_wgrad_job", dev.index, _stream(dev), ctypes.byref(s_aff), _p(c.dz), _p(cx.gview(rec.idx_w)), 0, c.N, c.D,
                 c.H, c.W, c.Cout, _p(ws), ws.numel(), ctypes.byref(c.job) if c.job is not None else None, flops=c.flops)
        c.job = None

    def _dgrad_subpixel(self, c: "_BwdCall"):
        # skip half at full resolution; upsampled half directly at LOW resolution (the children sum of the nearest
        # upsampling is folded into the 4x4x4-tap stride-2 gather).  dg = (dg_skip, dlow)
        cx, dev, src, rec, ws, pool = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws, c.cx.pool
        Nn, Dd, Hh, Ww, Cout = c.N, c.D, c.H, c.W, c.Cout
        C0, C1 = rec.sub
        w, pair = rec.conv_w, tuple(rec.sub)
        dg0 = _empty((Nn, Dd, Hh, Ww, C0), dtype=_F32, device=dev)
        dlow = _empty_like(src.t1)
        split0 = self._split_dgrad(C0, Cout)
        plus = rec.plus
        gst0 = pool.table(Nn, C0, 1 if split0 else c.greps)
        gst1 = pool.table(Nn, C1, 1 if any(plus) else c.greps)  # (the windowed form of an n -> 2n + 1 level keeps one row)
        if split0:
            need = nat.get_lib().u3d_conv3d_bf16_workspace_floats(Nn, Dd, Hh, Ww, Cout, C0)
            kws = cx.ensure_ws(need) if need > 0 else None
            nat.call("u3d_conv3d_f32s", dev.index, _stream(dev), _p(c.dz), None, _p(self.images.get(w, Kind.F32S_DGRAD, dev, pair)),
                     _p(dg0), Nn, Dd, Hh, Ww, Cout, C0, 0, None, _p(src.t0), _p(gst0.t), None, _p(kws), need,
                     flops=54.0 * C0 * Cout * Nn * Dd * Hh * Ww)
        else:
            s_dz = VSrc(c.dz).struct()
            s_x0 = VSrc(src.t0).struct()
            nat.call("u3d_conv3d_ex_reps", dev.index, _stream(dev), ctypes.byref(s_dz), _p(self.images.get(w, Kind.SKIP_DGRAD, dev, pair)), _p(dg0),
                     Nn, Dd, Hh, Ww, C0, 0, None, ctypes.byref(s_x0), _p(gst0.t), None, _p(ws), ws.numel(), gst0.reps,
                     flops=54.0 * C0 * Cout * Nn * Dd * Hh * Ww)
        if any(plus):
            # n -> 2n + 1: the share of the outputs d >= 2 from the windowed sub-pixel kernel; the slab's share as a full-resolution
            # gradient of the upsampled channels inside the slab's dilation (general kernel on dz masked to the slab), folded into the
            # first low-res cells of the shifted axes together with its part of the GroupNorm-backward sums
            win = (ctypes.c_int * 9)(Dd, Hh, Ww, *plus, *plus)
            nat.call("u3d_subpixel_conv_dgrad_win", dev.index, _stream(dev), _p(c.dz), _p(self.images.get(w, Kind.UP_DGRAD, dev, pair)), _p(src.t1),
                     _p(dlow), _p(gst1.t), Nn, src.D1, src.H1, src.W1, C1, Cout, win,
                     flops=128.0 * C1 * Cout * Nn * src.D1 * src.H1 * src.W1)
            dv = _empty((Nn, Dd, Hh, Ww, C1), dtype=_F32, device=dev)
            s_dz2 = VSrc(c.dz).struct()
            wpd1 = self.images.get(w, Kind.SLAB_DGRAD, dev, pair)
            mask = (ctypes.c_int * 3)(*(2 * e for e in plus))
            # (the two slab launches are one tile-time each on less than half of the chip's block slots — a 2-voxel slab in 4 x 8 x 8
            # tiles — but running them side by side on two streams was measured in round 6: each takes twice as long, 192 + 214 us
            # against 114 + 113; the waste is MFMA work on dead tile rows, not idle slots)
            for box in slab_boxes((Dd, Hh, Ww), plus, 3):
                nat.call("u3d_conv3d_box", dev.index, _stream(dev), ctypes.byref(s_dz2), _p(wpd1), _p(dv), Nn, Dd, Hh, Ww, C1,
                         (ctypes.c_int * 6)(*box), mask,
                         flops=54.0 * C1 * Cout * Nn * (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]))
            lz, ly, lx = src.los
            nat.call("u3d_nearest_childsum_add", dev.index, _stream(dev), _p(dv), _p(src.t1), _p(dlow), _p(gst1.t), Nn, Dd, Hh, Ww,
                     src.D1, src.H1, src.W1, C1, _p(lz), _p(ly), _p(lx), *plus)
            del dv
        else:
            nat.call("u3d_subpixel_conv_dgrad_reps", dev.index, _stream(dev), _p(c.dz), _p(self.images.get(w, Kind.UP_DGRAD, dev, pair)), _p(src.t1),
                     _p(dlow), _p(gst1.t), Nn, src.D1, src.H1, src.W1, C1, Cout, gst1.reps,
                     flops=128.0 * C1 * Cout * Nn * src.D1 * src.H1 * src.W1)
        return (dg0, dlow), (gst0, gst1)

    def _dgrad_f32s(self, c: "_BwdCall"):
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        dg = _empty((c.N, c.D, c.H, c.W, src.C), dtype=_F32, device=dev)
        gst = cx.pool.table(c.N, src.C)
        need = nat.get_lib().u3d_conv3d_bf16_workspace_floats(c.N, c.D, c.H, c.W, c.Cout, src.C)
        kws = cx.ensure_ws(need) if need > 0 else None
        nat.call("u3d_conv3d_f32s", dev.index, _stream(dev), _p(c.dz), None, _p(self.images.get(rec.conv_w, Kind.F32S_DGRAD, dev)), _p(dg),
                 c.N, c.D, c.H, c.W, c.Cout, src.C, 0, None, _p(src.t0), _p(gst.t), None, _p(kws), need, flops=c.flops)
        return dg, (gst, None)

    def _dgrad_bf16(self, c: "_BwdCall"):
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        dg = _empty((c.N, c.D, c.H, c.W, src.C), dtype=c.dz.dtype if c.b16 else _F32, device=dev)
        gst = cx.pool.table(c.N, src.C)
        if rec.c16:  # (`bf16_stem`: the same kernel with the mode-1 image, roles swapped)
            nat.call("u3d_conv3d_bf16_c16", dev.index, _stream(dev), _p(c.dz), None, _p(self.images.get(rec.conv_w, Kind.BF16_DGRAD_C16, dev)),
                     _p(dg), c.N, c.D, c.H, c.W, c.Cout, src.C, 0, None, _p(src.t0), _p(gst.t), None, 0, flops=c.flops)
            return dg, (gst, None)
        need = nat.get_lib().u3d_conv3d_bf16_workspace_floats(c.N, c.D, c.H, c.W, c.Cout, src.C)
        kws = cx.ensure_ws(need) if need > 0 else None
        nat.call("u3d_conv3d_bf16_ex" + ("_b16" if c.b16 else ""), dev.index, _stream(dev), _p(c.dz), None,
                 _p(self.images.get(rec.conv_w, Kind.BF16_DGRAD, dev)), _p(dg), c.N, c.D, c.H, c.W, c.Cout, src.C, 0, None, _p(src.t0), _p(gst.t),
                 None, _p(kws), need, flops=c.flops)
        return dg, (gst, None)

    def _wgrad_conv2d(self, c: "_BwdCall"):
        # (takes no GroupNorm-backward job: c.job stays set and _conv_bwd runs the reduction on its own)
        cx, dev, src, rec, ws = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws
        if rec.f32s:  # (`_split2d`, read off the record: slots added in slot order, no atomics; takes no job either)
            ws = cx.ensure_ws(nat.get_ext_lib().u3d_wgrad2d_f32s_workspace_floats(c.N, c.H, c.W, src.C, c.Cout))
            nat.call("u3d_conv2d_wgrad_f32s", dev.index, _stream(dev), *self._f32s_src(src), _p(rec.affine), _p(c.dz),
                     _p(cx.gview(rec.idx_w)), c.N, c.H, c.W, c.Cout, _p(ws), ws.numel(), flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)
            return
        s_aff = src.struct(rec.affine)
        nat.call("u3d_conv2d_wgrad", dev.index, _stream(dev), ctypes.byref(s_aff), _p(c.dz), _p(cx.gview(rec.idx_w)), c.N, c.H, c.W,
                 c.Cout, _p(ws), ws.numel(), flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)

    def _dgrad_conv2d(self, c: "_BwdCall"):
        cx, dev, src, rec, ws = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws
        dg = _empty((c.N, c.D, c.H, c.W, src.C), dtype=_F32, device=dev)
        gst = cx.pool.table(c.N, src.C, c.greps)
        if rec.f32s:  # (`_split2d`, read off the record: the mode-1 images, gx the layer's — single or virtual — forward input)
            wpd = self.images.get(rec.conv_w, Kind.F32S_DGRAD2D, dev)
            nat.call("u3d_conv2d_f32s_dgrad", dev.index, _stream(dev), _p(c.dz), _p(wpd), _p(dg), c.N, c.H, c.W, c.Cout,
                     *self._f32s_src(src), _p(gst.t), gst.reps, flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)
            return dg, (gst, None)
        wpd = self.images.get(rec.conv_w, Kind.DGRAD2D, dev)
        s_dz = VSrc(c.dz).struct()
        s_x = src.struct()
        nat.call("u3d_conv2d_ex_reps", dev.index, _stream(dev), ctypes.byref(s_dz), _p(wpd), _p(dg), c.N, c.H, c.W, src.C, 0, None,
                 ctypes.byref(s_x), _p(gst.t), _p(ws), ws.numel(), gst.reps, flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)
        return dg, (gst, None)

    def _wgrad_subpixel2d(self, c: "_BwdCall"):
        # `native_2d_subpixel`: the weight gradient in two channel slices of the same (Cout, Ctot, 9) buffer — upsampled channels from the
        # 16 (parity class, tap half) matrices over the low-res grid, skip channels from the standard kernel (takes no job, as `conv2d`)
        cx, dev, src, rec, ws = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws
        C0, C1 = rec.sub
        Ct = src.C
        dwv = cx.gview(rec.idx_w)
        plus = rec.plus
        if any(plus):
            # `native_2d_subpixel_plus`: outputs d >= 2 of the shifted axes through the windowed sub-pixel kernel, the slab d < 2 through the
            # 3x3 kernel on disjoint boxes of dz (each into scratch, added to the same channel slice)
            win = (ctypes.c_int * 6)(c.H, c.W, *plus[1:], *plus[1:])
            nat.call("u3d_subpixel2d_conv_wgrad_win", dev.index, _stream(dev), _p(src.t1), _p(rec.affine.view(-1)[2 * C0:]), Ct * 2,
                     _p(c.dz), _p(dwv[C0 * 9:]), Ct, c.N, src.H1, src.W1, C1, c.Cout, _p(ws), ws.numel(), win,
                     flops=32.0 * C1 * c.Cout * c.N * src.H1 * src.W1)
            # (a_hi is held across the loop: the struct keeps only its pointer, and `tmp` below must not be carved out of a freed copy)
            a_hi = rec.affine_hi if rec.affine_hi is not None else rec.affine[:, C0:].contiguous()
            s_up = src.up_only_struct(a_hi)
            slice_view = dwv.view(c.Cout, Ct, 9)[:, C0:, :]
            for box in slab_boxes((1, c.H, c.W), plus, 2):
                tmp = _empty((c.Cout, C1, 9), dtype=_F32, device=dev)
                nat.call("u3d_conv2d_wgrad_box", dev.index, _stream(dev), ctypes.byref(s_up), _p(c.dz), _p(tmp), c.N, c.H, c.W, c.Cout,
                         _p(ws), ws.numel(), (ctypes.c_int * 4)(box[1], box[2], box[4], box[5]),
                         flops=18.0 * C1 * c.Cout * c.N * (box[4] - box[1]) * (box[5] - box[2]))
                slice_view += tmp
        else:
            nat.call("u3d_subpixel2d_conv_wgrad", dev.index, _stream(dev), _p(src.t1), _p(rec.affine.view(-1)[2 * C0:]), Ct * 2, _p(c.dz),
                     _p(dwv[C0 * 9:]), Ct, c.N, src.H1, src.W1, C1, c.Cout, _p(ws), ws.numel(),
                     flops=32.0 * C1 * c.Cout * c.N * src.H1 * src.W1)
        a0 = rec.affine_lo if rec.affine_lo is not None else rec.affine[:, :C0].contiguous()
        s0 = VSrc(src.t0).struct(a0)
        nat.call("u3d_conv2d_wgrad_strided", dev.index, _stream(dev), ctypes.byref(s0), _p(c.dz), _p(dwv), Ct, c.N, c.H, c.W, c.Cout,
                 _p(ws), ws.numel(), flops=18.0 * C0 * c.Cout * c.N * c.H * c.W)

    def _wgrad_subpixel2d_bf16(self, c: "_BwdCall"):
        # `native_2d_bf16_subpixel`: the two slices of the same (Cout, Ctot, 9) buffer on the bf16 MFMA — both operands rounded once while
        # staged, fp32 sums added in a fixed order (takes no job, as `conv2d_bf16`)
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        C0, C1 = rec.sub
        Ct = src.C
        lib = nat.get_lib()
        ws = cx.ensure_ws(max(lib.u3d_subpixel2d_wgrad_bf16_workspace_floats(c.N, src.H1, src.W1, C1, c.Cout),
                              lib.u3d_wgrad2d_bf16_workspace_floats(c.N, c.H, c.W, C0, c.Cout)))
        dwv = cx.gview(rec.idx_w)
        nat.call("u3d_subpixel2d_conv_wgrad_bf16", dev.index, _stream(dev), _p(src.t1), _p(rec.affine.view(-1)[2 * C0:]), Ct * 2, _p(c.dz),
                 _p(dwv[C0 * 9:]), Ct, c.N, src.H1, src.W1, C1, c.Cout, _p(ws), ws.numel(), flops=32.0 * C1 * c.Cout * c.N * src.H1 * src.W1)
        a0 = rec.affine_lo if rec.affine_lo is not None else rec.affine[:, :C0].contiguous()
        nat.call("u3d_conv2d_wgrad_bf16_strided", dev.index, _stream(dev), _p(src.t0), _p(a0), _p(c.dz), _p(dwv), Ct, c.N, c.H, c.W, C0, c.Cout,
                 _p(ws), ws.numel(), flops=18.0 * C0 * c.Cout * c.N * c.H * c.W)

    def _wgrad_subpixel_bf16(self, c: "_BwdCall"):
        # `bf16_subpixel`: the two slices of the same (Cout, Ctot, 27) buffer on the bf16 MFMA — both operands rounded once while staged,
        # fp32 sums added in a fixed order.  Takes no job: the GroupNorm-backward reduction of the layer's input stays the separate
        # u3d_gn_bwd_finalize_split launch (`_conv_bwd` runs it when c.job comes back set; same bits by the header's contract)
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        C0, C1 = rec.sub
        Ct = src.C
        lib = nat.get_lib()
        ws = cx.ensure_ws(max(lib.u3d_subpixel_wgrad_bf16_workspace_floats(c.N, src.D1, src.H1, src.W1, C1, c.Cout),
                              lib.u3d_wgrad_bf16_workspace_floats(c.N, c.D, c.H, c.W, C0, c.Cout)))
        dwv = cx.gview(rec.idx_w)
        nat.call("u3d_subpixel_conv_wgrad_bf16", dev.index, _stream(dev), _p(src.t1), _p(rec.affine.view(-1)[2 * C0:]), Ct * 2, _p(c.dz),
                 _p(dwv[C0 * 27:]), Ct, c.N, src.D1, src.H1, src.W1, C1, c.Cout, _p(ws), ws.numel(),
                 flops=128.0 * C1 * c.Cout * c.N * src.D1 * src.H1 * src.W1)
        a0 = rec.affine_lo if rec.affine_lo is not None else rec.affine[:, :C0].contiguous()
        nat.call("u3d_conv3d_wgrad_bf16_strided", dev.index, _stream(dev), _p(src.t0), _p(a0), _p(c.dz), _p(dwv), Ct, c.N, c.D, c.H, c.W, C0,
                 c.Cout, _p(ws), ws.numel(), flops=54.0 * C0 * c.Cout * c.N * c.D * c.H * c.W)

    def _dgrad_subpixel_bf16(self, c: "_BwdCall"):
        # `bf16_subpixel`: the skip half at full resolution (u3d_conv3d_bf16_ex on dz with the mode-1 image of channels [0, C0), gx = skip);
        # the upsampled half directly at LOW resolution.  dg = (dg_skip, dlow) and two statistics tables, as `_dgrad_subpixel`
        cx, dev, src, rec, pool = c.cx, c.cx.dev, c.src, c.rec, c.cx.pool
        C0, C1 = rec.sub
        w, pair = rec.conv_w, tuple(rec.sub)
        dg0 = _empty((c.N, c.D, c.H, c.W, C0), dtype=_F32, device=dev)
        dlow = _empty_like(src.t1)
        gst0 = pool.table(c.N, C0)
        gst1 = pool.table(c.N, C1, c.greps)
        need = nat.get_lib().u3d_conv3d_bf16_workspace_floats(c.N, c.D, c.H, c.W, c.Cout, C0)  # roles swapped
        kws = cx.ensure_ws(need) if need > 0 else None
        nat.call("u3d_conv3d_bf16_ex", dev.index, _stream(dev), _p(c.dz), None, _p(self.images.get(w, Kind.SKIP_BF16_DGRAD, dev, pair)), _p(dg0),
                 c.N, c.D, c.H, c.W, c.Cout, C0, 0, None, _p(src.t0), _p(gst0.t), None, _p(kws), need,
                 flops=54.0 * C0 * c.Cout * c.N * c.D * c.H * c.W)
        nat.call("u3d_subpixel_conv_dgrad_bf16", dev.index, _stream(dev), _p(c.dz), _p(self.images.get(w, Kind.UP_BF16_DGRAD, dev, pair)),
                 _p(src.t1), _p(dlow), _p(gst1.t), c.N, src.D1, src.H1, src.W1, C1, c.Cout, gst1.reps,
                 flops=128.0 * C1 * c.Cout * c.N * src.D1 * src.H1 * src.W1)
        return (dg0, dlow), (gst0, gst1)

    def _dgrad_subpixel2d_bf16(self, c: "_BwdCall"):
        # `native_2d_bf16_subpixel`: the skip half at full resolution (u3d_conv2d_bf16 on dz with the mode-1 image of channels [0, C0), gx =
        # skip); the upsampled half directly at LOW resolution.  dg = (dg_skip, dlow) and two statistics tables, as `_dgrad_subpixel2d`
        cx, dev, src, rec, pool = c.cx, c.cx.dev, c.src, c.rec, c.cx.pool
        C0, C1 = rec.sub
        w, pair = rec.conv_w, tuple(rec.sub)
        dg0 = _empty((c.N, 1, c.H, c.W, C0), dtype=_F32, device=dev)
        dlow = _empty_like(src.t1)
        gst0 = pool.table(c.N, C0, c.greps)
        gst1 = pool.table(c.N, C1, c.greps)
        need = nat.get_lib().u3d_conv2d_bf16_workspace_floats(c.N, c.H, c.W, c.Cout, C0)  # roles swapped
        kws = cx.ensure_ws(need) if need > 0 else None
        nat.call("u3d_conv2d_bf16", dev.index, _stream(dev), _p(c.dz), None, _p(self.images.get(w, Kind.SKIP_BF16_DGRAD2D, dev, pair)), _p(dg0),
                 c.N, c.H, c.W, c.Cout, C0, 0, None, _p(src.t0), _p(gst0.t), _p(kws), need, gst0.reps,
                 flops=18.0 * C0 * c.Cout * c.N * c.H * c.W)
        nat.call("u3d_subpixel2d_conv_dgrad_bf16", dev.index, _stream(dev), _p(c.dz), _p(self.images.get(w, Kind.UP_BF16_DGRAD2D, dev, pair)),
                 _p(src.t1), _p(dlow), _p(gst1.t), c.N, src.H1, src.W1, C1, c.Cout, gst1.reps,
                 flops=32.0 * C1 * c.Cout * c.N * src.H1 * src.W1)
        return (dg0, dlow), (gst0, gst1)

    def _dgrad_subpixel2d(self, c: "_BwdCall"):
        # skip half at full resolution (mode-1 image of channels [0, C0)); upsampled half directly at LOW resolution, the children sum
        # of the nearest upsampling folded into the 4x4-tap stride-2 gather.  dg = (dg_skip, dlow)
        cx, dev, src, rec, ws, pool = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws, c.cx.pool
        C0, C1 = rec.sub
        w, pair = rec.conv_w, tuple(rec.sub)
        dg0 = _empty((c.N, 1, c.H, c.W, C0), dtype=_F32, device=dev)
        dlow = _empty_like(src.t1)
        gst0 = pool.table(c.N, C0, c.greps)
        gst1 = pool.table(c.N, C1, c.greps)
        s_dz = VSrc(c.dz).struct()
        s_x0 = VSrc(src.t0).struct()
        nat.call("u3d_conv2d_ex_reps", dev.index, _stream(dev), ctypes.byref(s_dz), _p(self.images.get(w, Kind.SKIP_DGRAD2D, dev, pair)), _p(dg0),
                 c.N, c.H, c.W, C0, 0, None, ctypes.byref(s_x0), _p(gst0.t), _p(ws), ws.numel(), gst0.reps,
                 flops=18.0 * C0 * c.Cout * c.N * c.H * c.W)
        plus = rec.plus
        if any(plus):
            # `native_2d_subpixel_plus`: the share of the outputs d >= 2 from the windowed sub-pixel kernel; the slab's share as a
            # full-resolution gradient of the upsampled channels on the three rows / columns it reaches (3x3 kernel on dz masked to the
            # slab, into a scratch the size of each box — never a full-resolution tensor), folded into the first low-res cells of the
            # shifted axes together with its part of the GroupNorm-backward sums (replica row 0)
            win = (ctypes.c_int * 6)(c.H, c.W, *plus[1:], *plus[1:])
            nat.call("u3d_subpixel2d_conv_dgrad_win", dev.index, _stream(dev), _p(c.dz), _p(self.images.get(w, Kind.UP_DGRAD2D, dev, pair)),
                     _p(src.t1), _p(dlow), _p(gst1.t), c.N, src.H1, src.W1, C1, c.Cout, gst1.reps, win,
                     flops=32.0 * C1 * c.Cout * c.N * src.H1 * src.W1)
            wpd1 = self.images.get(w, Kind.SLAB_DGRAD2D, dev, pair)
            mask = (ctypes.c_int * 2)(2 * plus[1], 2 * plus[2])
            for box in slab_boxes((1, c.H, c.W), plus, 3):
                y0, x0, y1, x1 = box[1], box[2], box[4], box[5]
                dv = _empty((c.N, y1 - y0, x1 - x0, C1), dtype=_F32, device=dev)
                nat.call("u3d_conv2d_box", dev.index, _stream(dev), ctypes.byref(s_dz), _p(wpd1), _p(dv), c.N, c.H, c.W, C1,
                         (ctypes.c_int * 4)(y0, x0, y1, x1), mask, (ctypes.c_int * 4)(y1 - y0, x1 - x0, y0, x0),
                         flops=18.0 * C1 * c.Cout * c.N * (y1 - y0) * (x1 - x0))
                nat.call("u3d_nearest_childsum_add2d", dev.index, _stream(dev), _p(dv), _p(src.t1), _p(dlow), _p(gst1.t), c.N, src.H1,
                         src.W1, C1, *plus[1:], (ctypes.c_int * 4)(y0, x0, y1, x1))
                del dv
        else:
            nat.call("u3d_subpixel2d_conv_dgrad_reps", dev.index, _stream(dev), _p(c.dz), _p(self.images.get(w, Kind.UP_DGRAD2D, dev, pair)),
                     _p(src.t1), _p(dlow), _p(gst1.t), c.N, src.H1, src.W1, C1, c.Cout, gst1.reps,
                     flops=32.0 * C1 * c.Cout * c.N * src.H1 * src.W1)
        return (dg0, dlow), (gst0, gst1)

    def _wgrad_conv2d_bf16(self, c: "_BwdCall"):
        # both operands rounded to bf16 while staged (g = a*x + b and dz), fp32 sums added in a fixed order; takes no GroupNorm-backward
        # job, like the fp32 2-D kernel
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        sfx = "_c16" if rec.c16 else ""
        need = getattr(nat.get_lib(), f"u3d_wgrad2d_bf16{sfx}_workspace_floats")(c.N, c.H, c.W, src.C, c.Cout)
        ws = cx.ensure_ws(need)
        if rec.family == "conv2d_bf16_src":  # (`_bf16_vcat`: the same plan on the virtual concat)
            s = src.struct(rec.affine)
            nat.call("u3d_conv2d_wgrad_bf16_src", dev.index, _stream(dev), ctypes.byref(s), _p(c.dz), _p(cx.gview(rec.idx_w)), c.N, c.H,
                     c.W, c.Cout, _p(ws), ws.numel(), flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)
            return
        nat.call("u3d_conv2d_wgrad_bf16" + sfx, dev.index, _stream(dev), _p(src.t0), _p(rec.affine), _p(c.dz), _p(cx.gview(rec.idx_w)), c.N,
                 c.H, c.W, src.C, c.Cout, _p(ws), ws.numel(), flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)

    def _dgrad_conv2d_bf16(self, c: "_BwdCall"):
        cx, dev, src, rec = c.cx, c.cx.dev, c.src, c.rec
        sfx = "_c16" if rec.c16 else ""
        wpd = self.images.get(rec.conv_w, Kind.BF16_DGRAD2D_C16 if rec.c16 else Kind.BF16_DGRAD2D, dev)
        dg = _empty((c.N, c.D, c.H, c.W, src.C), dtype=_F32, device=dev)
        gst = cx.pool.table(c.N, src.C, c.greps)
        need = getattr(nat.get_lib(), f"u3d_conv2d_bf16{sfx}_workspace_floats")(c.N, c.H, c.W, c.Cout, src.C)  # roles swapped
        kws = cx.ensure_ws(need) if need > 0 else None
        if rec.family == "conv2d_bf16_src":  # (`_bf16_vcat`: gx is the virtual concat; dz and dg are plain tensors of the full width)
            s = src.struct()
            nat.call("u3d_conv2d_bf16_dgrad_src", dev.index, _stream(dev), _p(c.dz), _p(wpd), _p(dg), c.N, c.H, c.W, c.Cout,
                     ctypes.byref(s), _p(gst.t), _p(kws), need, gst.reps, flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)
            return dg, (gst, None)
        nat.call("u3d_conv2d_bf16" + sfx, dev.index, _stream(dev), _p(c.dz), None, _p(wpd), _p(dg), c.N, c.H, c.W, c.Cout, src.C, 0, None,
                 _p(src.t0), _p(gst.t), _p(kws), need, gst.reps, flops=18.0 * src.C * c.Cout * c.N * c.H * c.W)
        return dg, (gst, None)

    def _dgrad_fp32(self, c: "_BwdCall"):
        cx, dev, src, rec, ws = c.cx, c.cx.dev, c.src, c.rec, c.cx.ws
        wpd = self.images.get(rec.conv_w, Kind.DGRAD, dev)
        dg = _empty((c.N, c.D, c.H, c.W, src.C), dtype=_F32, device=dev)
        gst = cx.pool.table(c.N, src.C, c.greps)
        s_dz = VSrc(c.dz).struct()
        s_x = src.struct()
        nat.call("u3d_conv3d_ex_reps", dev.index, _stream(dev), ctypes.byref(s_dz), _p(wpd), _p(dg), c.N, c.D, c.H, c.W, src.C, 0, None,
                 ctypes.byref(s_x), _p(gst.t), None, _p(ws), ws.numel(), gst.reps, flops=c.flops)
        return dg, (gst, None)

    # -- backward building blocks (shared by the DoubleConv and the residual executors) -----------------------
    def _conv_bwd(self, cx, rec: ConvRec, dz_, need_dg=True):
        """wgrad + dgrad + GroupNorm-backward reductions of one SingleConv; returns (dg, coef, coef_hi): coef_hi is the compact
        (p, 8q, 8r) table of a sub-pixel layer's upsampled channels when a finalize wrote one (_norm_bwd_job), else None"""
        dev, pool, ws, gview = cx.dev, cx.pool, cx.ws, cx.gview
        src = rec.src
        Nn, Dd, Hh, Ww = src.N, src.D, src.H, src.W
        Cout = rec.y.shape[-1]
        if rec.drop is not None:
            # trailing dropout: the consumers already removed f through the (rescaled, sign-preserving) layer output
            kind, mask = rec.drop
            g = _empty_like(dz_)
            if kind == "d":
                nat.call("u3d_mul", dev.index, _stream(dev), _p(dz_), _p(mask), dz_.numel(), _p(g))
            else:
                nat.call("u3d_affine_act_fwd", dev.index, _stream(dev), _p(dz_), _p(mask), Nn, Dd * Hh * Ww, Cout, ACT_NONE, 0.0, _p(g))
            dz_ = g
        if rec.post is not None:
            # post-norm layer: dz_ is the gradient w.r.t. n = a*z + b (the caller removed the non-linearity): norm backward
            # over the conv output z first — sums (sum dn, sum dn*z), parameter gradients, dz = p*dn + q*z + r
            z, _, inner, islope = rec.post
            Vz = Dd * Hh * Ww
            gst2 = pool.table(Nn, Cout)
            nat.call("u3d_pair_stats", dev.index, _stream(dev), _p(dz_), _p(z), Nn, Vz, Cout, _p(gst2.t))
            if rec.norm is None:
                # norm-free layer: n = z + bias -> dbias = sum dn, dz = dn
                nat.call("u3d_bias_grad", dev.index, _stream(dev), _p(gst2.t), Nn, Cout, _p(gview(rec.idx_gb)))
            else:
                coef2 = _empty((Nn, 3, Cout), dtype=_F32, device=dev)
                self._norm_bwd_finalize(cx, rec, (gst2, None), float(Vz), coef2)
                dz_ = self._plain_apply(cx, dz_, coef2, z, 1 if inner == ACT_RELU else 0)  # ('crg': z = relu(conv), mask fused)
                if inner in (ACT_LEAKY, ACT_ELU):
                    nat.call("u3d_act_bwd", dev.index, _stream(dev), _p(dz_), _p(z), dz_.numel(), inner, islope, _p(dz_))
        if self.debug is not None:
            self.debug[rec.name + ".dz"] = dz_.clone()
        # ---- ONE decision, read off the record: the (data-gradient, weight-gradient) families
        dgrad, wgrad = self._bwd_families(cx, rec, need_dg)
        if wgrad is None:
            # one pass gives dw and the GroupNorm-backward sums; no data gradient needed (csrc/u3d_smallc.hip)
            gst = pool.table(Nn, src.C)
            if self.is2d:  # (D = 1: the 2-D twin, csrc/u3d_conv2d.hip)
                nat.call("u3d_conv2d_small_cin_bwd", dev.index, _stream(dev), _p(src.t0), _p(rec.affine), _p(dz_),
                         _p(rec.conv_w.detach()), _p(gview(rec.idx_w)), _p(gst.t), Nn, Hh, Ww, src.C, Cout, _p(ws), ws.numel(),
                         flops=2 * 18.0 * src.C * Cout * Nn * Hh * Ww)
            else:
                nat.call("u3d_conv3d_small_cin_bwd", dev.index, _stream(dev), _p(src.t0), _p(rec.affine), _p(dz_),
                         _p(rec.conv_w.detach()), _p(gview(rec.idx_w)), _p(gst.t), Nn, Dd, Hh, Ww, src.C, Cout, _p(ws), ws.numel(),
                         flops=2 * 54.0 * src.C * Cout * Nn * Dd * Hh * Ww)
            if not rec.pre_norm:
                return None, self._identity_coef(Nn, src.C, dev), None
            coef = _empty((Nn, 3, src.C), dtype=_F32, device=dev)
            return None, coef, self._norm_bwd_finalize(cx, rec, (gst, None), float(Dd * Hh * Ww), coef)
        b16 = src.t0.dtype == torch.bfloat16  # bf16 activation storage
        assert not b16 or (rec.family == "bf16" and Cout % 64 == 0 and dz_.dtype == torch.bfloat16)
        call = _BwdCall(cx, rec, dz_, src, Nn, Dd, Hh, Ww, Cout, b16)
        # ---- data gradient (+ the GroupNorm-backward sums of the conv input), then weight gradient.  The one-block reduction of those
        # sums rides in the weight gradient's reduce launch where the family takes a job (round 6)
        # (replica rows for the sums only where the weight-gradient launch will take the reduction as a job: it reads them in that form)
        # (`fp32_split_wgrad`: the split launch takes no job — `_wgrad_fp32` / `_wgrad_subpixel` ask the same predicate)
        split_w = (wgrad == "fp32" and src.t1 is None and self._split_wgrad(src.C, Cout)) or (
            wgrad == "subpixel" and self._split_wgrad(rec.sub[0], Cout))
        if (self.stat_reps > 1 and rec.pre_norm and rec.norm == "g" and wgrad in ("fp32", "subpixel") and not split_w
                and nat.get_lib().u3d_conv3d_wgrad_job_supported(Nn, src.C, rec.G) == 1):
            call.greps = self.stat_reps
        dg, gst = self._launcher(1, dgrad)(call)
        if self.debug is not None and rec.sub is None:
            self.debug[rec.name + ".dg"] = dg.clone()
        coef = coef_hi = None
        if rec.pre_norm:
            coef = _empty((Nn, 3, src.C), dtype=_F32, device=dev)
            call.job, coef_hi = self._norm_bwd_job(cx, rec, gst, float(Dd * Hh * Ww), coef)
        had_job = call.job is not None
        self._launcher(2, wgrad)(call)
        if not rec.pre_norm:
            return dg, self._identity_coef(Nn, src.C, dev), None  # no GroupNorm on the conv input: dx = dg
        if not had_job or call.job is not None:  # (no job, or a weight-gradient family without a reduce launch to carry it)
            coef_hi = self._norm_bwd_finalize(cx, rec, gst, float(Dd * Hh * Ww), coef)
        return dg, coef, coef_hi

    def _plain_apply(self, cx, dg, coef, x, relu_mask, add=None):
        """GroupNorm backward, elementwise part: (p*dg + q*x + r [+ add]) * (relu_mask ? x > 0 : 1)"""
        dev = cx.dev
        out = _empty_like(x)
        Nn = x.shape[0]
        C = x.shape[-1]
        if x.dtype == torch.bfloat16:  # bf16 activation storage (dg, x, add, out all bf16)
            nat.call("u3d_gn_bwd_apply_b16", dev.index, _stream(dev), _p(dg), C, 0, _p(x), C, _p(coef), C, x.numel() // (Nn * C), Nn,
                     relu_mask, _p(add), _p(out))
            return out
        if add is None:
            nat.call("u3d_gn_bwd_apply", dev.index, _stream(dev), _p(dg), C, 0, _p(x), C, _p(coef), C, x.numel() // (Nn * C), Nn,
                     relu_mask, _p(out))
        else:
            nat.call("u3d_gn_bwd_apply_add", dev.index, _stream(dev), _p(dg), C, 0, _p(x), C, _p(coef), C,
                     x.numel() // (Nn * C), Nn, relu_mask, _p(add), _p(out))
        return out

    def _wgrad_workspace(self, tape, dev):
        return _empty(max(self._wgrad_workspace_floats(tape.convs), 4), dtype=_F32, device=dev)

    def _family_ws_floats(self, family, N, D, H, W, Cin, Cout, sub=None, plus=(0, 0, 0), c16=False, f32s=False):
        """scratch floats the backward of one layer of forward family `family` needs from the shared buffer: its weight gradient + its
        data gradient's split-K scratch (roles swapped); `sub`, `plus`, `c16`, `f32s` as the layer's record holds them"""
        lib = nat.get_lib()
        if family == "conv2d" and f32s:  # (`native_2d_fp32_split`: the extension library's plan; its convolutions never split)
            return nat.get_ext_lib().u3d_wgrad2d_f32s_workspace_floats(N, H, W, Cin, Cout)
        if family == "small":
            return lib.u3d_small_cin_bwd_workspace_floats(N, D, H, W, Cin, Cout)
        if family == "subpixel":  # skip slice (fp32 kernels) + sub-pixel slice + the slab boxes of an n -> 2n + 1 level
            boxes = slab_boxes((D, H, W), plus, 2)
            return max([lib.u3d_wgrad_workspace_floats(N, D, H, W, sub[0], Cout), self._split_wgrad_ws_floats(N, D, H, W, sub[0], Cout),
                        lib.u3d_subpixel_wgrad_workspace_floats(N, D // 2, H // 2, W // 2, sub[1], Cout),
                        lib.u3d_conv3d_workspace_floats(N, D, H, W, Cout, sub[0])] +
                       [lib.u3d_wgrad_workspace_floats(N, b[3] - b[0], b[4] - b[1], b[5] - b[2], sub[1], Cout) for b in boxes])
        if family == "subpixel_bf16":  # (`bf16_subpixel`: skip slice + sub-pixel slice on the bf16 kernels' plans, the skip data gradient's split-K)
            return max(lib.u3d_wgrad_bf16_workspace_floats(N, D, H, W, sub[0], Cout),
                       lib.u3d_subpixel_wgrad_bf16_workspace_floats(N, D // 2, H // 2, W // 2, sub[1], Cout),
                       lib.u3d_conv3d_bf16_workspace_floats(N, D, H, W, Cout, sub[0]))
        if family == "bf16" and c16:  # (`bf16_stem`: the extension library's plans; its convolution never splits)
            return nat.get_ext_lib().u3d_wgrad_bf16_c16_workspace_floats(N, D, H, W, Cin, Cout)
        if family == "bf16":
            return max(lib.u3d_conv3d_bf16_workspace_floats(N, D, H, W, Cout, Cin), lib.u3d_wgrad_bf16_workspace_floats(N, D, H, W, Cin, Cout))
        if family in ("fp32", "f32s"):  # (the split data gradient grows the buffer itself, `_BwdCtx.ensure_ws`)
            return max(lib.u3d_wgrad_workspace_floats(N, D, H, W, Cin, Cout), lib.u3d_conv3d_workspace_floats(N, D, H, W, Cout, Cin),
                       self._split_wgrad_ws_floats(N, D, H, W, Cin, Cout))
        if family == "subpixel2d_bf16":  # (`native_2d_bf16_subpixel`: the three of `subpixel2d` below on the bf16 kernels' plans)
            return max(lib.u3d_wgrad2d_bf16_workspace_floats(N, H, W, sub[0], Cout),
                       lib.u3d_subpixel2d_wgrad_bf16_workspace_floats(N, H // 2, W // 2, sub[1], Cout),
                       lib.u3d_conv2d_bf16_workspace_floats(N, H, W, Cout, sub[0]))
        if family == "subpixel2d":  # (`native_2d_subpixel`: skip slice on the conv2d kernels + the sub-pixel slice's block slots)
            boxes = slab_boxes((1, H, W), plus, 2)  # (`native_2d_subpixel_plus`: the slab's weight-gradient launches)
            return max(lib.u3d_wgrad2d_workspace_floats(N, H, W, sub[0], Cout),
                       lib.u3d_subpixel2d_wgrad_workspace_floats(N, H // 2, W // 2, sub[1], Cout),
                       lib.u3d_conv2d_workspace_floats(N, H, W, Cout, sub[0]),
                       *(lib.u3d_wgrad2d_workspace_floats(N, b[4] - b[1], b[5] - b[2], sub[1], Cout) for b in boxes))
        if family in ("conv2d_bf16", "conv2d_bf16_src"):  # (the bf16 kernels' plans, csrc/u3d_conv2d_bf16.hip)
            sfx = "_c16" if c16 else ""
            return max(getattr(lib, f"u3d_wgrad2d_bf16{sfx}_workspace_floats")(N, H, W, Cin, Cout),
                       getattr(lib, f"u3d_conv2d_bf16{sfx}_workspace_floats")(N, H, W, Cout, Cin))
        need = max(lib.u3d_wgrad2d_workspace_floats(N, H, W, Cin, Cout), lib.u3d_conv2d_workspace_floats(N, H, W, Cout, Cin))
        if family == "small2d":  # (the one-pass backward, or — when a data gradient is needed — the fall-through to the fp32 family)
            return max(need, lib.u3d_small_cin2d_bwd_workspace_floats(N, H, W, Cin, Cout))
        assert family == "conv2d", family
        return need

    def _split_wgrad_ws_floats(self, N, D, H, W, Cin, Cout):
        """the split weight gradient's plan under `fp32_split_wgrad` (0 with the key off or outside `_split_wgrad`: the extension library is
        not loaded then)"""
        return nat.get_ext_lib().u3d_wgrad_f32s_workspace_floats(N, D, H, W, Cin, Cout) if self._split_wgrad(Cin, Cout) else 0

    def _layer_ws_floats(self, N, D, H, W, Cin, Cout, small=False):
        """... by shape, of a single-source (Cin -> Cout) layer no forward has recorded yet (a checkpointed block that backward will
        recompute): the family it will take, from the rules forward asks"""
        if self.is2d:
            family = "small2d" if small else ("conv2d_bf16" if self._bf16_routed_weight(Cin, Cout, False) else "conv2d")
        else:
            family = "small" if small else ("bf16" if self._bf16_routed_weight(Cin, Cout, False) else "fp32")
        return self._family_ws_floats(family, N, D, H, W, Cin, Cout, c16=family in ("conv2d_bf16", "bf16") and self._c16(Cin, Cout),
                                      f32s=family == "conv2d" and self._split2d_counts(Cin, 0, Cout))

    def _wgrad_workspace_floats(self, convs):
        """scratch floats the backward kernels of these recorded layers need (one shared buffer, sized once per backward)"""
        return int(max((self._family_ws_floats(r.family, r.src.N, r.src.D, r.src.H, r.src.W, r.src.C, r.y.shape[-1], r.sub, r.plus, r.c16, r.f32s)
                        for r in convs), default=0))
