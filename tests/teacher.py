"""Teacher-forced float64 step of the bf16 modes (`compute_dtype: bf16`, and `activation_dtype: bf16` on the residual nets).

A network of bf16 layers is chaotic in the last bit: a 1e-6 change in a layer's input flips operand roundings in the next layer, so a
whole-step comparison with an emulation of the same arithmetic can only use global, flip-tolerant bars (tests/test_gpu_bf16.py,
test_gpu_b16.py).  Here every layer is instead fed the native run's OWN tensors and compared with a float64 restatement of the same
bf16 arithmetic (oracle.BF16_OPERANDS / BF16_STORAGE rounding points) on the same operands; only accumulation order is left.

Forward, per 3x3x3 conv (GroupNorm -> conv -> ReLU, 'gcr'):
  * the normalised operand is the fp32-affine restatement (x * a + b, rounded once to fp32, as the kernels' fmaf) built on the NATIVE
    table (a, b), in straight-through form g64 + (g_emul - g64).detach(), so gradients still flow through the float64 GroupNorm;
  * the native table itself is checked against a float64 GroupNorm finalize of the native input ("affine");
  * the layer output is compared with the native `y`, then replaced by it (straight-through again); ReLU masks and max-pool
    arg-maxes are the native run's (decided.decisions_from_tape).
Backward, per conv: the float64 gradient reaching the conv output is compared with the native `dz` (everything between this conv
and its consumers: apply passes, coefficient tables, pool / upsample merges, residual adds, SE and head backward) and the native `dz`
is passed on; the conv's input gradient is compared with the native `dg` and the native `dg` is passed on.  Each parameter's float64
gradient then depends on native inputs only and is compared one by one (decided.gate_failures).

Records are keyed by the module prefixes of the product's module tree: `encoders.{i}.basic_module.SingleConv{k}` / `.conv2` / `.conv3`
(conv records: x, affine, y, dz, dg) and `encoders.{i}.basic_module` (residual block records: r, and `out` after an SE gate).
`native_records` builds them from a native step (its tape and `eng.debug`); `run(..., force=False)` builds the same records from a
CPU run of the emulation itself (the fake native run of the self-tests)."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

import decided as dcd
import unet3d_oracle as orc

# ---- bars (measured on one MI355X by tests/test_gpu_bf16_teacher.py, profiles/r11_bf16_teacher_gate.jsonl) ------------------------------
# fp32-stored tensors (x, y, dz, dg, r, out, logits under `activation_dtype: fp32`): max|native - ref| / max|ref| per layer and per
# (sample, channel) slice, the slice's range floored at SLICE_FLOOR x the layer's.  Never looser than decided.GRAD_REL.
# Measured worst: y 5.2e-6 (ragged ResidualUNet3D, encoders.1 conv2), dg 5.4e-7, conv2 / SingleConv dz 4.1e-7, logits 1.8e-7.
F32_REL = 2e-5
SLICE_FLOOR = 1e-2
# the native GroupNorm table (a, b) against a float64 finalize of the native input, per element.  Measured worst 1.3e-6.
AFFINE_REL = 5e-6
# The gradient of a block output (each `.conv3` dz) is fed through a bf16 rounding no forcing site replaces: the transposed
# convolution's bf16 dt operand (both modes), and under storage the stored gradients of the joined and pooled tensors.  Their rare
# 1-ulp flips reach it, so it takes LINK_REL in place of F32_REL.  Measured worst 2.3e-4 (ragged ResidualUNet3D, encoders.1 conv3).
LINK_REL = 1e-3
# bf16-stored tensors (`activation_dtype: bf16`): every element within B16_ULP bf16 ulp of _r16(ref) or within B16_ABS of its
# (sample, channel) slice's range (an element that is the small result of a cancelling sum carries the fp32 rounding of its large
# terms, many of ITS ulps), and at most B16_FRAC of them differing from _r16(ref) at all (the bar of
# tests/test_gpu_b16.py::test_conv1x1_on_the_bf16_matrix_pipe, 2e-3, tightened).  Measured worst of y, dg, conv2 dz, r and out:
# 1.0 ulp, 2.0e-4 of the elements differing (decoders.0 conv3 dg on the config-4 ladder).
B16_ULP = 1.0
B16_ABS = 5e-4
B16_FRAC = 6e-4
# bf16 link sites (every `.conv3` dz, and a decoder block's residual = the joined tensor, which reads the transposed convolution's
# stored output): measured worst 3.1e-3 of the slice range beyond one ulp (ResidualUNetSE3D, decoders.0 conv3 dz; 3.1 ulp on the
# config-4 ladder) and 1.2e-3 of the elements differing (config-4 ladder, decoders.1 conv3 dz)
B16_LINK_ABS = 1e-2
B16_LINK_FRAC = 4e-3
# parameter gradients: decided.gate_failures (GRAD_REL; FIRST_NORM_REL for the first norm weight, measured worst 5.2e-4 on the bf16
# UNet3D).  Measured worst of the rest 5.6e-6 (UNet3D encoders.0 SingleConv1 GroupNorm bias).  The parameters
# `behind_unforced_rounding` take STORED_GRAD_REL: measured worst 2.9e-4 (ResidualUNetSE3D storage, decoders.0 sSE conv bias).
STORED_GRAD_REL = 2e-3


@contextlib.contextmanager
def bf16_modes(storage: bool):
    """the oracle's bf16-operand (and, with `storage`, bf16-storage) rounding points switched on for the block"""
    old = orc.BF16_OPERANDS, orc.BF16_STORAGE
    orc.BF16_OPERANDS, orc.BF16_STORAGE = True, storage
    try:
        yield
    finally:
        orc.BF16_OPERANDS, orc.BF16_STORAGE = old


def trunc16(t):
    """bf16 by truncation (the planted rounding error of the self-tests)"""
    return (t.float().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def _ulp16(t):
    """one bf16 ulp at |t| (t double)"""
    _, e = torch.frexp(t.abs().clamp(min=1e-38))
    return torch.ldexp(torch.ones_like(t), (e - 8).to(torch.int32))


class _OperandConv3d(torch.autograd.Function):
    """oracle._BF16OperandConv3d (both operands of each of the three GEMMs rounded with `r`), with the self-tests' plants: the dz
    operand rounded with `rdz`, and the data gradient computed without the last D-plane of dz (`drop_last`)"""

    @staticmethod
    def forward(ctx, g, w, r, rdz, drop_last):
        ctx.save_for_backward(g, w)
        ctx.r, ctx.rdz, ctx.drop_last = r, rdz, drop_last
        return F.conv3d(r(g), r(w), None, stride=1, padding=1)

    @staticmethod
    def backward(ctx, dz):
        g, w = ctx.saved_tensors
        dzr = ctx.rdz(dz)
        dzd = dzr
        if ctx.drop_last:
            dzd = dzr.clone()
            dzd[:, :, -1] = 0
        dg = torch.nn.grad.conv3d_input(g.shape, ctx.r(w), dzd, padding=1)
        dw = torch.nn.grad.conv3d_weight(ctx.r(g), w.shape, dzr, padding=1)
        return dg, dw, None, None, None


class _Replace(torch.autograd.Function):
    """straight-through replacement: forward returns `new` (bit for bit), backward hands the gradient to `value`"""

    @staticmethod
    def forward(ctx, value, new):
        return new.detach().clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class _GradSite(torch.autograd.Function):
    """identity forward; backward hands the incoming gradient to hook(g) and passes on what it returns"""

    @staticmethod
    def forward(ctx, x, hook):
        ctx.hook = hook
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.hook(g), None


def _identity(t):
    return t


def affine_table(x, gamma, beta, G, eps=1e-5):
    """(N, C, 2) GroupNorm table (a, b) with normalised = x * a + b, finalized in float64 from x (N, C, ...)"""
    N, C = x.shape[:2]
    xg = x.double().reshape(N, G, -1)
    mean = xg.mean(-1)
    var = (xg - mean[..., None]).square().mean(-1)
    rstd = (var + eps).rsqrt()
    rep = C // G
    a = gamma.double()[None] * rstd.repeat_interleave(rep, 1)
    b = beta.double()[None] - mean.repeat_interleave(rep, 1) * a
    return torch.stack((a, b), -1)


def _bc(t):
    return t[:, :, None, None, None]


@dataclass
class Report:
    figures: Dict[str, Dict[str, float]] = field(default_factory=dict)  # "key:q" -> metrics
    failures: List[str] = field(default_factory=list)
    skipped: Dict[str, str] = field(default_factory=dict)  # "key:q" -> why no native value was forced there
    grads: Dict[str, torch.Tensor] = field(default_factory=dict)  # float64 parameter gradients
    logits: Optional[torch.Tensor] = None

    def worst(self, kind):
        """(site, value) of the largest metric `kind` over all figures"""
        vals = [(k, f[kind]) for k, f in self.figures.items() if kind in f]
        return max(vals, key=lambda t: t[1]) if vals else (None, 0.0)


def compare(native, ref, b16: bool, link: bool = False) -> Dict[str, float]:
    """error figures of one native tensor against the float64 reference: fp32-stored -> rel (layer) and slice (per (n, c), floored);
    bf16-stored -> ulp (max distance from _r16(ref) in bf16 ulp) and frac (fraction of elements differing from it)"""
    a, b = native.double(), ref.detach().double()
    if b16:
        b = orc._r16(b)
        d = (a - b).abs()
        rng = b.abs().amax(dim=tuple(range(2, b.dim())), keepdim=True) if b.dim() >= 3 else b.abs().max()
        rng = rng.clamp(min=SLICE_FLOOR * b.abs().max().item())
        u = _ulp16(torch.maximum(a.abs(), b.abs()))
        ulp = (d / torch.maximum(u, (B16_LINK_ABS if link else B16_ABS) * rng)).max().item() if d.numel() else 0.0
        over = d > u  # (the measurement of B16_ABS: the worst |native - _r16(ref)| / slice range beyond one ulp)
        beyond = (d / rng)[over].max().item() if over.any() else 0.0
        return {"ulp": ulp, "frac": (d > 0).double().mean().item(), "beyond_ulp": beyond}
    d = (a - b).abs()
    top = b.abs().max().item()
    top = top if top > 0 else 1.0
    if b.dim() >= 3:
        dims = tuple(range(2, b.dim()))
        err, rng = d.amax(dim=dims), b.abs().amax(dim=dims)
    else:
        err, rng = d, b.abs()
    return {"rel": d.max().item() / top, "slice": (err / rng.clamp(min=SLICE_FLOOR * top)).max().item()}


_B16_QS = ("y", "dz", "dg", "r", "out")  # the quantities a bf16-storage step keeps as bf16 (conv inputs `x`: UNet3D only, fp32)


def _bad(fig, bar, link=False) -> bool:
    if "ulp" in fig:
        return not (fig["ulp"] <= B16_ULP and fig["frac"] < (B16_LINK_FRAC if link else B16_FRAC))
    return not (fig["rel"] < bar and fig["slice"] < bar)


class _Run:
    """one pass of the functional step: force=True -> teacher-forced against `records`; force=False -> capture `records` (and the
    decisions) from the step itself, with the self-tests' `plant`s applied"""

    def __init__(self, records, decisions, force, storage, plant, sites, dtype):
        self.rec = records
        self.dec = decisions
        self.force = force
        self.storage = storage
        self.plant = plant or {}
        self.sites = sites  # decision sites of the module tree (decided.decision_sites)
        self.dtype = dtype
        self.used: Dict[str, int] = {}
        self.dec_used: Dict[str, int] = {}
        self.report = Report()

    # -- bookkeeping
    def _native(self, key, q):
        r = self.rec.get(key)
        if r is None or q not in r:
            raise KeyError(f"no native record {key}:{q}")
        self.used[f"{key}:{q}"] = self.used.get(f"{key}:{q}", 0) + 1
        return r[q]

    def _check(self, key, q, native, ref, b16, link=False):
        fig = compare(native, ref, b16, link)
        self.report.figures[f"{key}:{q}"] = fig
        bar = LINK_REL if link else F32_REL
        if _bad(fig, bar, link):
            lim = f"<= {B16_ULP} ulp, frac < {B16_LINK_FRAC if link else B16_FRAC}" if b16 else f"< {bar}"
            self.report.failures.append(f"{key}: {q} " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()) + f" (bar {lim})")

    def _store(self, key, q, value):
        slot = self.rec.setdefault(key, {})
        assert q not in slot, f"{key}:{q} captured twice"
        slot[q] = value.detach().clone()

    def decision(self, name, make):
        assert name in self.sites, f"no decision site {name}"
        self.dec_used[name] = self.dec_used.get(name, 0) + 1
        if self.force:
            return self.dec[name]
        d = make()
        assert name not in self.dec, name
        self.dec[name] = d
        return d

    # -- forcing sites
    def fwd(self, key, q, value, b16, link=False):
        """a forward tensor: compared with the native one, then replaced by it (straight-through)"""
        p = self.plant.get((key, q))
        if not self.force:
            if p is not None:
                value = p(value)
            self._store(key, q, value)
            return value
        nat = self._native(key, q).to(value.dtype)
        self._check(key, q, nat, value, b16, link)
        return _Replace.apply(value, nat)

    def bwd(self, key, q, value, b16, link=False):
        """a gradient: the one reaching `value` is compared with the native one, and the native one is passed on"""
        p = self.plant.get((key, q))

        def hook(g):
            if not self.force:
                if p is not None:
                    g = p(g)
                self._store(key, q, g)
                return g
            r = self.rec.get(key, {})
            if q not in r and f"{q}_skip" in r:
                self.report.skipped[f"{key}:{q}"] = r[f"{q}_skip"]
                return g
            nat = self._native(key, q).to(g.dtype)
            self._check(key, q, nat, g, b16, link)
            return nat

        return _GradSite.apply(value, hook)

    # -- layers
    def conv_layer(self, h, key, L, num_groups, residual=None, in_res=False, mask_name=None, stored_out=False):
        """GroupNorm -> 3x3x3 conv [+ residual] -> ReLU with the forcing sites of one conv record"""
        gw, gb, w = L[f"{key}.groupnorm.weight"], L[f"{key}.groupnorm.bias"], L[f"{key}.conv.weight"]
        G = orc.groups_for(h.shape[1], num_groups)
        g64 = F.group_norm(h, G, gw, gb, 1e-5)
        if self.force:
            tab = self._native(key, "affine").double()
            ref = affine_table(h.detach(), gw.detach(), gb.detach(), G)
            fa, fb = compare(tab[..., 0], ref[..., 0], False), compare(tab[..., 1], ref[..., 1], False)
            fig = {k: max(fa[k], fb[k]) for k in fa}
            self.report.figures[f"{key}:affine"] = fig
            if _bad(fig, AFFINE_REL):
                self.report.failures.append(f"{key}: affine rel {fig['rel']:.3g}, slice {fig['slice']:.3g} (bar < {AFFINE_REL})")
        else:
            tab = affine_table(h.detach(), gw.detach(), gb.detach(), G).float()
            self._store(key, "affine", tab)
            tab = tab.double()
        # the kernels stage (__bf16)fmaf(x, a, b): one rounding to fp32 of the exact x*a + b, then the operand rounding
        g_emul = (h.detach().double() * _bc(tab[..., 0]) + _bc(tab[..., 1])).float().to(h.dtype)
        g = _Replace.apply(g64, g_emul)
        b16 = self.storage and in_res
        g = self.bwd(key, "dg", g, b16)
        if in_res:
            g = orc.grad_stored(g)
        bf16 = orc.BF16_OPERANDS and w.shape[0] % 32 == 0 and w.shape[1] % 32 == 0
        r = orc._r16 if bf16 else _identity
        rdz = trunc16 if self.plant.get((key, "trunc_dz")) else r
        z = _OperandConv3d.apply(g, w, r, rdz, bool(self.plant.get((key, "drop_last_dg"))))
        s = z if residual is None else z + residual
        s = self.bwd(key, "dz", s, b16, link=key.endswith(".conv3"))
        m = self.decision(mask_name, lambda: s.detach() > 0)
        y = s * m.to(s.dtype)
        if stored_out:
            y = orc.stored(y)
        return self.fwd(key, "y", y, b16)

    def pool(self, h, name):
        win = dcd._windows(h, False)
        idx = self.decision(name, lambda: win.detach().argmax(-1).to(torch.uint8))
        return win.gather(-1, idx.long().unsqueeze(-1)).squeeze(-1)

    def mask_of(self, prefix):
        names = [k for k in self.sites if k.startswith(prefix + ".")]
        assert len(names) == 1, (prefix, names)
        return names[0]

    def res_block(self, x, base, L, num_groups):
        if f"{base}.conv1.weight" in L:
            r = orc.conv1x1_bias(x, L[f"{base}.conv1.weight"], L[f"{base}.conv1.bias"])
        else:
            r = x
        r = orc.stored(r)
        r = self.fwd(base, "r", r, self.storage, link=self.storage and base.startswith("decoders."))
        if self.plant.get((base, "r_split_round")):
            # planted: the gradient of r rounded per consumer, then the sum rounded again
            r2, r3 = orc._BF16GradStore.apply(r), orc._BF16GradStore.apply(r)
        else:
            r2 = r3 = r
        o2 = self.conv_layer(r2, f"{base}.conv2", L, num_groups, in_res=True, mask_name=self.mask_of(f"{base}.conv2"),
                             stored_out=True)
        y = self.conv_layer(o2, f"{base}.conv3", L, num_groups, residual=r3, in_res=True, mask_name=f"{base}.non_linearity",
                            stored_out=True)
        if f"{base}.se_module.cSE.fc1.weight" in L or f"{base}.se_module.fc1.weight" in L or f"{base}.se_module.conv.weight" in L:
            y = self.fwd(base, "out", orc.se_gate(y, L, base), self.storage)
        return y

    def double_conv(self, h, base, L, num_groups):
        k1, k2 = f"{base}.SingleConv1", f"{base}.SingleConv2"
        h = self.fwd(k1, "x", h, False)
        h = self.conv_layer(h, k1, L, num_groups, mask_name=self.mask_of(k1))
        return self.conv_layer(h, k2, L, num_groups, mask_name=self.mask_of(k2))


def run(cfg, sd, x, target, loss_fn: Callable, records, decisions, storage=False, force=True, dtype=torch.float64,
        plant=None, native_logits=None) -> Report:
    """One teacher-forced (force=True: `records` / `decisions` are the native run's) or capturing (force=False: `records` and
    `decisions` are filled) step of the gcr UNet3D / ResidualUNet3D / ResidualUNetSE3D in `cfg` under the oracle's bf16 rounding
    points.  Returns a Report: per-site error figures and failures (force), the parameter gradients, the logits."""
    num_groups = cfg.get("num_groups", 8)
    assert cfg.get("layer_order", "gcr") == "gcr" and cfg.get("is_segmentation", True), cfg
    from pytorch3dunet_amd.unet3d.model import get_model

    R = _Run(records, decisions, force, storage, plant, dcd.decision_sites(get_model(dict(cfg))), dtype)
    L = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    h = x.to(dtype)
    residual_net = orc.is_residual(sd)
    n_enc, n_dec = orc._count(sd, "encoders"), orc._count(sd, "decoders")
    with bf16_modes(storage):
        feats = []
        for i in range(n_enc):
            if i > 0:
                h = R.pool(h, f"encoders.{i}.pooling")
                if residual_net:
                    # (bf16 storage) the pooled tensor is stored, and so is its gradient: the 1x1x1 conv's backward writes it as bf16
                    # before the pool's backward merges it with the skip gradient, a rounding of its own the oracle does not restate
                    h = orc.grad_stored(h)
            base = f"encoders.{i}.basic_module"
            h = R.res_block(h, base, L, num_groups) if residual_net else R.double_conv(h, base, L, num_groups)
            feats.insert(0, h)
        feats = feats[1:]
        for j in range(n_dec):
            skip, base = feats[j], f"decoders.{j}.basic_module"
            if residual_net:
                up = orc.stored(orc.conv_transpose_up(h, L[f"decoders.{j}.upsampling.upsample.conv_transposed.weight"]))
                h = R.res_block(orc.stored(skip + F.interpolate(up, size=skip.shape[2:])), base, L, num_groups)
            else:
                h = R.double_conv(torch.cat((skip, orc.nearest_to(h, skip.shape[2:])), dim=1), base, L, num_groups)
        # (the native head accumulates its gradients in double: so does the fake run)
        logits = F.conv3d(h.double(), L["final_conv.weight"].double(), L["final_conv.bias"].double())
        if force and native_logits is not None:
            R._check("final_conv", "logits", native_logits.double(), logits, False)
        probs = torch.sigmoid(logits) if cfg.get("final_sigmoid", True) else torch.softmax(logits, dim=1)
        loss = loss_fn(probs, logits, target.double())
        grads = torch.autograd.grad(loss, list(L.values()))
    rep = R.report
    rep.grads = dict(zip(L.keys(), grads))
    rep.logits = logits.detach()
    bad = {k: n for k, n in R.dec_used.items() if n != 1}
    missing = sorted(set(R.sites) - set(R.dec_used))
    assert not bad and not missing, f"decision sites not used exactly once: {bad}; unused: {missing}"
    if force:
        assert set(decisions) == set(R.sites), sorted(set(decisions) ^ set(R.sites))
        given = {f"{k}:{q}" for k, r in records.items() for q in r if not q.endswith("_skip")}
        wrong = {k: R.used.get(k, 0) for k in given if R.used.get(k, 0) != 1}
        assert not wrong, f"forcing sites not used exactly once: {wrong}"
    return rep


def behind_unforced_rounding(name: str, storage: bool) -> bool:
    """a parameter whose gradient reads a bf16-rounded gradient that no forcing site replaces, and so carries its rare 1-ulp flips: the
    transposed convolution's (its dt operand); under storage also the 1x1x1 conv's (the stored residual gradient) and the SE gate's
    (the stored block-output gradient)"""
    return "conv_transposed" in name or (storage and (".conv1." in name or ".se_module." in name))


def gate(cfg, sd, x, target, loss_fn, records, decisions, native_grads, storage, native_logits=None):
    """teacher-forced step + every check: (report, failures) where failures list the layer sites, then the parameters outside
    decided.gate_failures (STORED_GRAD_REL for the parameters `behind_unforced_rounding`)"""
    rep = run(cfg, sd, x, target, loss_fn, records, decisions, storage=storage, native_logits=native_logits)
    first = dcd.first_norm_weight(rep.grads)
    for k in rep.grads:
        rep.figures[f"param:{k}"] = {"grad_rel": dcd.rel_err(native_grads[k], rep.grads[k])}
    fails = list(rep.failures)
    for k, e, bar in dcd.gate_failures(native_grads, rep.grads, first):
        if behind_unforced_rounding(k, storage):
            if e < STORED_GRAD_REL:
                continue
            bar = STORED_GRAD_REL
        fails.append(f"param {k}: rel {e:.3g} (bar < {bar})")
    return rep, fails


def capture(cfg, sd, x, target, loss_fn, storage, dtype=torch.float32, plant=None):
    """the fake native run: the emulation itself in `dtype`, unforced -> (records, decisions, grads, logits)"""
    records, decisions = {}, {}
    rep = run(cfg, sd, x, target, loss_fn, records, decisions, storage=storage, force=False, dtype=dtype, plant=plant)
    return records, decisions, {k: g.float() for k, g in rep.grads.items()}, rep.logits.float()


def compare_records(native, ref, storage):
    """[(site, figure)] of every forced quantity of two captured record sets (the chaos measurement of the self-tests)"""
    out = []
    for key, r in ref.items():
        for q, v in r.items():
            if q.endswith("_skip"):
                continue
            b16 = storage and q in _B16_QS
            fig = compare(native[key][q].double(), v.double(), b16)
            out.append((f"{key}:{q}", fig, _bad(fig, AFFINE_REL if q == "affine" else F32_REL)))  # (the direct-site bars)
    return out


# ---- the converter: a native step's tape and eng.debug -> records -----------------------------------------------------------------------
def _nc(t):
    return t.permute(0, 4, 1, 2, 3).contiguous().cpu()


def _materialised(src):
    """NCDHW float tensor of a (virtual) conv input: t0, or torch.cat((t0, nearest(t1))) for a virtual concat"""
    t0 = _nc(src.t0).float()
    if src.t1 is None:
        return t0
    up = F.interpolate(_nc(src.t1).float(), size=tuple(t0.shape[2:]), mode="nearest")
    return torch.cat((t0, up), dim=1)


def native_records(model, tape):
    """forward records of a native step (call right after the forward: backward may reuse the tape's buffers) -> (records, names)
    with names = {tape conv name: record key}; the dtype of every stored tensor is kept in records[key]["<q>_dtype"]"""
    mods = dict(model.named_modules())
    records: Dict[str, dict] = {}
    names = {}
    for rec in tape.convs:
        assert rec.post is None and rec.pre_norm and rec.norm == "g" and rec.drop is None, f"{rec.name}: not a gcr layer"
        _, key = dcd.record_module(mods, rec.name)
        assert key not in records, f"two tape records for {key}"
        names[rec.name] = key
        r = records[key] = {"affine": rec.affine.detach().cpu().clone(), "y": _nc(rec.y).float(), "y_dtype": rec.y.dtype}
        if key.endswith("SingleConv1"):
            r["x"] = _materialised(rec.src)
        if rec.small:
            r["dg_skip"] = "first layer: the native backward computes no input gradient there (small-Cin kernel)"
        elif rec.sub is not None:
            r["dg_skip"] = "sub-pixel layer: its data gradient is never materialised"
    for b in tape.blocks:
        assert hasattr(b, "rec2"), f"{b.name}: checkpointed blocks are outside the teacher-forced gate"
        base = dcd.block_module(mods, b.name)
        assert base not in records, base
        records[base] = {"r": _nc(b.r).float(), "r_dtype": b.r.dtype}
        if b.se is not None:
            records[base]["out"] = _nc(b.se["out"]).float()
            records[base]["out_dtype"] = b.se["out"].dtype
    return records, names


def attach_gradients(records, names, debug):
    """add the backward's `dz` / `dg` clones of eng.debug (every one must belong to a tape conv)"""
    for k, v in debug.items():
        if k == "tape":
            continue
        name, _, q = k.rpartition(".")
        assert q in ("dz", "dg") and name in names, f"eng.debug entry {k!r} without a tape conv"
        slot = records[names[name]]
        assert q not in slot and f"{q}_skip" not in slot, k
        slot[q] = _nc(v).float()
        slot[f"{q}_dtype"] = v.dtype
    for key, r in records.items():
        if ".conv" in key or ".SingleConv" in key:
            assert "dz" in r and ("dg" in r or "dg_skip" in r), f"{key}: no native dz / dg recorded"


def strip_dtypes(records, storage):
    """drop the `<q>_dtype` entries after checking them: under bf16 storage exactly the tensors the teacher compares as bf16 are bf16"""
    out = {}
    for key, r in records.items():
        out[key] = {}
        for q, v in r.items():
            if q.endswith("_dtype"):
                want = torch.bfloat16 if (storage and q[:-6] in _B16_QS) else torch.float32
                assert v == want, f"{key}:{q[:-6]} is {v}, the teacher compares it as {want}"
                continue
            out[key][q] = v
    return out
