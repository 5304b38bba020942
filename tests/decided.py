"""Decision-consistent float64 step of any model the native executor runs.

A ReLU / LeakyReLU network's gradient is discontinuous in its pre-activations, and so is a max-pool's in the gap between the two
largest window candidates: two correct fp32 implementations take different decisions where those sit within round-off of zero, and
each flip is an O(1) local change of the gradient.  The loose whole-model bars of the suite exist to absorb that.  Here the DISCRETE
decisions a native forward took (its activation tape, `eng.debug = {}` -> `eng.debug["tape"]`) are imposed on the product's own CPU
module tree in float64; what is left is smooth arithmetic, so logits, loss, the input gradient and every parameter gradient must agree
with the kernels to rounding.

The module tree is the one `get_model(cfg)` builds (pinned to the reference's records by tests/test_native2d.py,
test_native2d_residual.py and test_oracle.py).  Decisions are imposed with forward hooks:
  * every ReLU / LeakyReLU outside a squeeze-and-excitation gate: output = pre * mask (ReLU) or pre * where(mask, 1, slope);
    the copies run with `inplace=False`, which keeps the pre-activation the mask multiplies.  ELU (and sigmoid) take no decision.
  * every MaxPool2d / MaxPool3d: output = the window candidate the tape names (3-D byte dz*4 + dy*2 + dx, 2-D 2*dy + dx).
The squeeze-and-excitation gates (ResNetBlockSE) run un-hooked, as in oracle.forward_backward_decided: their ReLU acts on a handful
of pooled channel means and the native executor records no decision for it.

Tape records map to modules by name: `enc{i}.c{k}` / `dec{j}.c{k}` -> `encoders.{i}.basic_module.SingleConv{k}` (DoubleConv),
`enc{i}.c2` -> `.conv2` and `enc{i}.c3` -> `.non_linearity` (ResNetBlock: rec3.y = f(conv3 + r)), the pools of `tape.pools` ->
`encoders.{i}.pooling` for i >= 1.  A record whose module does not exist, a decision-taking module without a decision, or a decision
not consumed exactly once raises."""
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import torch
import torch.nn as nn

_ACTS = (nn.ReLU, nn.LeakyReLU, nn.ELU)
_DECIDING = (nn.ReLU, nn.LeakyReLU)
_POOLS = (nn.MaxPool2d, nn.MaxPool3d)
_NORM_CHARS = "gb"
_ACT_CHARS = "rle"


def build_model(cfg, sd, dtype=torch.float64, train=True):
    """the product's CPU module tree for `cfg` with `sd` loaded, in `dtype`, activations out of place"""
    from pytorch3dunet_amd.unet3d.model import get_model

    m = get_model(dict(cfg))
    m.load_state_dict(sd, strict=True)
    m = m.to(dtype).train(train)
    for mod in m.modules():
        if isinstance(mod, _ACTS):
            mod.inplace = False
    return m


def decision_sites(model) -> Dict[str, nn.Module]:
    """name -> module of every module whose output depends on a discrete decision the native executor records"""
    out = {}
    for name, mod in model.named_modules():
        if ".se_module" in name:
            continue
        if isinstance(mod, _DECIDING) or (isinstance(mod, _POOLS) and name.endswith(".pooling")):
            out[name] = mod
    return out


def _to_nc(t, is2d):
    """NDHWC (2-D: D = 1) device tensor -> NCDHW / NCHW CPU tensor"""
    t = t.permute(0, 4, 1, 2, 3).contiguous().cpu()
    return t.squeeze(2) if is2d else t


def _act_of(sc: nn.Module) -> Optional[str]:
    """name of the activation child of a SingleConv, None without one"""
    names = [n for n, m in sc.named_children() if isinstance(m, _ACTS)]
    assert len(names) <= 1, names
    return names[0] if names else None


def _inner_act(order: str) -> bool:
    """'c A N' orders ('crg', 'clb', ...): the non-linearity sits between the conv and its norm"""
    ci = order.index("c")
    acts = [i for i, ch in enumerate(order) if ch in _ACT_CHARS]
    norms = [i for i, ch in enumerate(order) if ch in _NORM_CHARS]
    return bool(acts and norms and ci < acts[0] < norms[0])


def block_module(mods: Dict[str, nn.Module], block: str) -> str:
    """`enc{i}` / `dec{j}` (a tape block name) -> `encoders.{i}.basic_module` / `decoders.{j}.basic_module`; raises without one"""
    side, idx = ("encoders", block[3:]) if block.startswith("enc") else ("decoders", block[3:])
    assert block[:3] in ("enc", "dec") and idx.isdigit(), block
    base = f"{side}.{idx}.basic_module"
    assert base in mods, f"{block}: no module {base}"
    return base


def record_module(mods: Dict[str, nn.Module], name: str):
    """(basic module, SingleConv module) names of a tape conv record: `enc{i}.c{k}` -> `encoders.{i}.basic_module.SingleConv{k}`
    (DoubleConv), `.c2` -> `.conv2` and `.c3` -> `.conv3` (ResNetBlock); raises for a record without its module"""
    blk, _, conv = name.partition(".")
    base = block_module(mods, blk)
    if hasattr(mods[base], "conv2"):  # ResNetBlock: c2 = conv2 (the block's order), c3 = conv3 + `out += residual` + non_linearity
        assert conv in ("c2", "c3"), f"{name}: unknown residual record"
        sc_name = f"{base}.conv{conv[1]}"
    else:
        assert conv in ("c1", "c2"), name
        sc_name = f"{base}.SingleConv{conv[1]}"
    assert sc_name in mods, f"{name}: no module {sc_name}"
    return base, sc_name


def decisions_from_tape(model, tape) -> Dict[str, torch.Tensor]:
    """{module name: decision} from a native forward's tape: bool masks (N,C,...) for activations, window indices (uint8) for pools.
    Must be called right after the forward (backward may reuse the tape's buffers)."""
    is2d = not model._is3d
    mods = dict(model.named_modules())
    out: Dict[str, torch.Tensor] = {}

    def put(key, val):
        assert key in mods, f"tape decision for {key!r}: no such module"
        assert key not in out, f"two tape records decide {key!r}"
        out[key] = val

    for rec in tape.convs:
        assert rec.drop is None, f"{rec.name}: dropout records are outside the decided harness"
        base, sc_name = record_module(mods, rec.name)
        if sc_name.endswith(".conv3"):
            bm = mods[base]
            assert _act_of(bm.conv3) is None, f"{rec.name}: conv3 carries an activation"
            if isinstance(bm.non_linearity, _DECIDING):
                put(f"{base}.non_linearity", _to_nc(rec.y, is2d) > 0)
            continue
        sc = mods.get(sc_name)
        assert sc is not None, f"{rec.name}: no module {sc_name}"
        act = _act_of(sc)
        if act is None or not isinstance(getattr(sc, act), _DECIDING):
            continue
        if _inner_act(sc.order):
            assert rec.post is not None, f"{rec.name}: inner activation without a post-norm record"
            pre = rec.post[0]
        else:
            pre = rec.y
        put(f"{sc_name}.{act}", _to_nc(pre, is2d) > 0)
    pools = [n for n, m in mods.items() if isinstance(m, _POOLS) and n.endswith(".pooling")]
    pools.sort(key=lambda n: int(n.split(".")[1]))
    assert len(pools) == len(tape.pools), (pools, len(tape.pools))
    for name, (_, am, _) in zip(pools, tape.pools):
        put(name, _to_nc(am, is2d))
    return out


def _windows(h, is2d):
    """candidates of every 2x2(x2) window (floor sizes), last axis = dz*4 + dy*2 + dx (2-D: 2*dy + dx)"""
    if is2d:
        n, c, hh, w = h.shape
        h2, w2 = hh // 2, w // 2
        win = h[:, :, : 2 * h2, : 2 * w2].reshape(n, c, h2, 2, w2, 2).permute(0, 1, 2, 4, 3, 5)
        return win.reshape(n, c, h2, w2, 4)
    n, c, d, hh, w = h.shape
    d2, h2, w2 = d // 2, hh // 2, w // 2
    win = h[:, :, : 2 * d2, : 2 * h2, : 2 * w2].reshape(n, c, d2, 2, h2, 2, w2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7)
    return win.reshape(n, c, d2, h2, w2, 8)


def own_decisions(cfg, sd, x, dtype=torch.float64, train=True) -> Dict[str, torch.Tensor]:
    """the decisions the module tree itself takes on x in `dtype` (a plain forward of a fresh copy): the fake tape of the harness's
    self-tests"""
    model = build_model(cfg, sd, dtype, train)
    is2d = not model._is3d
    sites = decision_sites(model)
    out, hooks = {}, []

    def mk(name, mod):
        def hook(m, inp, outp):
            h = inp[0].detach()
            if isinstance(mod, _POOLS):
                out[name] = _windows(h, is2d).argmax(-1).to(torch.uint8)
            else:
                out[name] = h > 0
        return hook

    for name, mod in sites.items():
        hooks.append(mod.register_forward_hook(mk(name, mod)))
    try:
        with torch.no_grad():
            model(x.to(dtype))
    finally:
        for h in hooks:
            h.remove()
    return out


@dataclass
class Decided:
    """the float64 step with the decisions imposed"""

    probs: torch.Tensor
    logits: torch.Tensor
    loss: float
    dx: torch.Tensor
    grads: Dict[str, torch.Tensor]
    buffers: Dict[str, torch.Tensor] = field(default_factory=dict)  # BatchNorm running statistics after the training forward


def decided_step(cfg, sd, x, target, loss_fn: Callable, decisions: Dict[str, torch.Tensor], dtype=torch.float64,
                 train=True) -> Decided:
    """One forward + backward of the module tree for `cfg` / `sd` in `dtype`, every decision of `decision_sites` replaced by
    `decisions` (decisions_from_tape / own_decisions).  loss_fn(probs, logits, target) -> scalar.  Raises unless every
    decision-taking module consumed exactly one decision and every decision was consumed."""
    model = build_model(cfg, sd, dtype, train)
    is2d = not model._is3d
    sites = decision_sites(model)
    missing, extra = sorted(set(sites) - set(decisions)), sorted(set(decisions) - set(sites))
    assert not missing and not extra, f"decision sites without a decision: {missing}; decisions without a site: {extra}"
    used = {k: 0 for k in sites}
    hooks = []

    def mk(name, mod):
        d = decisions[name]

        def hook(m, inp, outp):
            used[name] += 1
            h = inp[0]
            if isinstance(mod, _POOLS):
                win = _windows(h, is2d)
                assert d.shape == win.shape[:-1], (name, tuple(d.shape), tuple(win.shape))
                return win.gather(-1, d.long().unsqueeze(-1)).squeeze(-1)
            assert d.shape == h.shape and d.dtype == torch.bool, (name, tuple(d.shape), tuple(h.shape), d.dtype)
            if isinstance(mod, nn.LeakyReLU):
                return torch.where(d, h, h * mod.negative_slope)
            return h * d.to(h.dtype)
        return hook

    for name, mod in sites.items():
        hooks.append(mod.register_forward_hook(mk(name, mod)))
    try:
        xl = x.detach().to(dtype).clone().requires_grad_(True)
        probs, logits = model(xl, return_logits=True)
        loss = loss_fn(probs, logits, target.to(dtype))
        params = dict(model.named_parameters())
        grads = torch.autograd.grad(loss, [xl] + list(params.values()))
    finally:
        for h in hooks:
            h.remove()
    bad = {k: n for k, n in used.items() if n != 1}
    assert not bad, f"decision sites not consumed exactly once: {bad}"
    buffers = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    return Decided(probs.detach(), logits.detach(), loss.item(), grads[0], dict(zip(params.keys(), grads[1:])), buffers)


def plain_step(cfg, sd, x, target, loss_fn: Callable, dtype=torch.float64, train=True) -> Decided:
    """the same step through plain autograd of the module tree (no hooks): the harness's self-test reference"""
    model = build_model(cfg, sd, dtype, train)
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    probs, logits = model(xl, return_logits=True)
    loss = loss_fn(probs, logits, target.to(dtype))
    params = dict(model.named_parameters())
    grads = torch.autograd.grad(loss, [xl] + list(params.values()))
    buffers = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    return Decided(probs.detach(), logits.detach(), loss.item(), grads[0], dict(zip(params.keys(), grads[1:])), buffers)


def first_norm_weight(names) -> Optional[str]:
    """the parameter name of the network's first norm weight (GroupNorm or BatchNorm), None in a norm-free net"""
    return next((k for k in names if k.endswith(("groupnorm.weight", "batchnorm.weight"))), None)


GRAD_REL = 1e-4  # every parameter gradient and the input gradient: max|ours - decided| / max|decided|
# The first norm's weight (GroupNorm or BatchNorm, on the input or on the first conv's output) is the one cancellation-dominated
# gradient: the next norm renormalises its scale away, so d/dgamma is a sum of large terms that cancel to ~0 and keeps the round-off
# of every term (tests/test_gpu_model.py::test_gradients_match_decision_consistent_fp64_oracle uses the same bar).  Measured by
# tests/test_gpu_decided.py (profiles/r10_decided_gate.jsonl): 1.1e-4 on the DSB2018 'bcr' UNet2D at 2x1x256x256 (its first
# BatchNorm weight), 1.4e-7 ... 1.7e-5 elsewhere; every other parameter 2.3e-7 ... 5.0e-5 over all 48 configurations.
FIRST_NORM_REL = 1e-3


def rel_err(a, b) -> float:
    """max|a - b| / max|b| (1 when b is all zero)"""
    a, b = a.double(), b.double()
    denom = b.abs().max().item()
    return (a - b).abs().max().item() / (denom if denom > 0 else 1.0)


def gate_failures(grads: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor], first_norm: Optional[str] = None):
    """[(name, rel_err, bar)] of every parameter gradient outside the decided gate: GRAD_REL, FIRST_NORM_REL for `first_norm`"""
    assert set(grads) == set(ref), sorted(set(grads) ^ set(ref))
    out = []
    for k in ref:
        bar = FIRST_NORM_REL if k == first_norm else GRAD_REL
        e = rel_err(grads[k], ref[k])
        if not e < bar:
            out.append((k, e, bar))
    return out
