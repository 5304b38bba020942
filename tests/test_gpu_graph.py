"""-m gpu: the static-shape step runner (engine.GraphStep; `hip_graph: true` / U3D_GRAPH=1) — the reference's training loop
`output, loss = self._forward_pass(...); optimizer.zero_grad(); loss.backward(); optimizer.step()` (unet3d/trainer.py:231-246)
with both directions of the model replayed from captured hipGraphs: bitwise the same trajectory as eager launches, across two
input sizes, with the optimizer changing the weights between replays; misuse raises instead of reading a stale tape."""
import copy
import time

import pytest
import torch

from conftest import diag

import os

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("U3D_POISON", "0") == "1",
                                                  reason="graph capture is refused in poison mode (fills outside the graph's pool)")]

DEV = torch.device("cuda", 0)


def _mk(name, **kw):
    from pytorch3dunet_amd.unet3d.model import get_model

    torch.manual_seed(0)
    m = get_model({**dict(name=name, in_channels=1, out_channels=1, final_sigmoid=True, layer_order="gcr"), **kw})
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "groupnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    return m


def _batches(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp in shapes:
        x = torch.randn(shp, generator=g)
        out.append((x.to(DEV), (x > 0.3).float().to(DEV)))
    return out


def _train(model, batches, lr=1e-2, loss=None, xgrads=None, opt=None):
    """SGD-with-momentum steps over `batches`; `loss(probs, logits, target)` defaults to the fused BCEDiceLoss on the logits.  An input
    that requires grad has its gradient appended to `xgrads` (and cleared) every step; `opt` continues an earlier call's optimizer."""
    from pytorch3dunet_amd.unet3d.losses import BCEDiceLoss

    if loss is None:
        crit = BCEDiceLoss()
        loss = lambda probs, logits, t: crit(logits, t)  # noqa: E731
    if opt is None:
        opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9)
    model.train()
    losses, grads = [], []
    for x, t in batches:
        out, logits = model(x, return_logits=True)
        value = loss(out, logits, t)
        opt.zero_grad()
        value.backward()
        grads.append([p.grad.detach().clone() for p in model.parameters()])
        losses.append(value.detach().clone())
        if x.grad is not None and xgrads is not None:
            xgrads.append(x.grad.detach().clone())
            x.grad = None
        opt.step()
    torch.cuda.synchronize()
    return losses, grads


CASES = [
    ("UNet3D", dict(f_maps=16, num_groups=8), [(1, 1, 32, 64, 64)] * 2 + [(2, 1, 16, 32, 32)] * 2 + [(1, 1, 32, 64, 64)]),  # BASELINE config 1's shape
    ("UNet3D", dict(f_maps=[8, 16, 32], num_groups=4), [(2, 1, 8, 16, 16), (1, 1, 17, 33, 35), (2, 1, 8, 16, 16), (1, 1, 17, 33, 35)]),
    ("ResidualUNet3D", dict(f_maps=[8, 16, 32], num_groups=4, num_levels=3), [(1, 1, 16, 32, 32)] * 3 + [(1, 1, 8, 16, 24)]),
    ("ResidualUNetSE3D", dict(f_maps=[8, 16, 32], num_groups=4, num_levels=3), [(1, 1, 16, 32, 32)] * 3),
    # bf16 mode (round 4): DoubleConv decoders on a materialised concat + the bf16 weight gradient with 32 output channels ...
    ("UNet3D", dict(f_maps=32, num_levels=3, num_groups=8, compute_dtype="bf16"), [(1, 1, 16, 32, 32)] * 3),
    # ... and an SE net with bf16 activation storage (the `_b16` gates)
    ("ResidualUNetSE3D", dict(f_maps=[64, 128], num_groups=8, compute_dtype="bf16"), [(1, 1, 8, 16, 16)] * 3),
]


@pytest.mark.parametrize("name,kw,shapes", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_graph_replay_is_bitwise_the_eager_trajectory(name, kw, shapes):
    from pytorch3dunet_amd import _native as nat

    base = _mk(name, **kw)
    eager = copy.deepcopy(base).to(DEV)
    graphed = copy.deepcopy(base).to(DEV)
    graphed.hip_graph = True
    graphed._get_engine().hip_graph = True
    batches = _batches(shapes, 5)
    l0, g0 = _train(eager, batches)
    l1, g1 = _train(graphed, batches)
    eng = graphed._get_engine()
    assert len(eng._graph_steps) == len(set(shapes)) and eng._graph_off_reason is None
    for step, (a, b) in enumerate(zip(l0, l1)):
        assert torch.equal(a, b), f"loss differs at step {step}: {a.item()} vs {b.item()}"
    for step, (ga, gb) in enumerate(zip(g0, g1)):
        for (k, _), a, b in zip(eager.named_parameters(), ga, gb):
            assert torch.equal(a, b), f"gradient of {k} differs at step {step}"
    for (k, a), (_, b) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.equal(a, b), f"parameter {k} differs after training"
    # a replayed step does not go through the model's C-ABI entry points again: only the fused loss (forward + backward) does
    crit = __import__("pytorch3dunet_amd.unet3d.losses", fromlist=["BCEDiceLoss"]).BCEDiceLoss()
    x, t = batches[0]
    n1 = nat.launch_count
    _, logits = graphed(x, return_logits=True)
    crit(logits, t).backward()
    torch.cuda.synchronize()
    assert nat.launch_count - n1 <= 6, nat.launch_count - n1
    # inference of the same model object stays eager and sees the trained weights
    graphed.eval(), eager.eval()
    with torch.no_grad():
        assert torch.equal(graphed(batches[0][0]), eager(batches[0][0]))


def test_graph_misuse_raises_and_outputs_are_private_copies():
    m = _mk("UNet3D", f_maps=[8, 16], num_groups=4).to(DEV)
    m.hip_graph = True
    m._get_engine().hip_graph = True
    m.train()
    (x, t), (x2, _) = _batches([(1, 1, 8, 16, 16)] * 2, 3)
    p1, l1 = m(x, return_logits=True)
    keep = l1.detach().clone()
    p2, l2 = m(x2, return_logits=True)  # same shape: the one tape now belongs to this forward
    assert torch.equal(l1, keep), "an earlier step's outputs must not alias the graph's static buffers"
    with pytest.raises(RuntimeError, match="overwritten"):
        l1.sum().backward()
    l2.sum().backward(retain_graph=True)
    g = [p.grad.clone() for p in m.parameters()]
    l2.sum().backward()  # the tape is still this forward's: a retained graph can be walked again, gradients accumulate
    for p, a in zip(m.parameters(), g):
        assert torch.equal(p.grad, 2 * a)
    # gradients handed to autograd are copies: a later replay must not change what an earlier .grad tensor holds
    held = [p.grad for p in m.parameters()]
    snap = [h.clone() for h in held]
    m.zero_grad(set_to_none=True)
    _, l3 = m(x, return_logits=True)
    (3.0 * l3.sum()).backward()
    for h, a in zip(held, snap):
        assert torch.equal(h, a)
    m.zero_grad(set_to_none=True)
    _, l4 = m(x2, return_logits=True)
    l4.sum().backward()
    for p, a in zip(m.parameters(), g):
        assert torch.equal(p.grad, a)  # the same step again reproduces the first gradients bit for bit


@pytest.mark.parametrize("name,kw", [("UNet3D", dict(f_maps=[8, 16, 32], num_groups=4)),
                                     ("ResidualUNet3D", dict(f_maps=[64, 128], num_groups=8, num_levels=2, compute_dtype="bf16"))])
def test_graphs_survive_validation_and_empty_cache_between_training_steps(name, kw):
    """the captured forward graph bakes in the device pointer of the pack descriptor table, whose only other
    owner was a one-entry dict that the first EAGER forward with a different stale set (validation between training steps,
    trainer.py:254-262: modes (0,) instead of (0, 1)) cleared — every later replay then ran the pack kernel on freed memory, and
    `torch.cuda.empty_cache()` (the predictor's OOM fallback calls it) or any reuse of the block made it read garbage pointers.
    train -> eval forward -> empty_cache + allocator churn -> train must stay bitwise the eager trajectory."""
    base = _mk(name, **kw)
    eager = copy.deepcopy(base).to(DEV)
    graphed = copy.deepcopy(base).to(DEV)
    graphed.hip_graph = True
    graphed._get_engine().hip_graph = True
    shape = (1, 1, 16, 32, 32)
    batches = _batches([shape] * 6, 11)
    res = {}
    for tag, m in (("eager", eager), ("graph", graphed)):
        out = []
        out.append(_train(m, batches[:3]))
        m.eval()
        with torch.no_grad():
            ev = m(batches[0][0]).clone()
        # drop everything the allocator can drop, then churn: a freed descriptor table / packed image would be handed out again
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        junk = [torch.full((n,), float("nan"), device=DEV) for n in (257, 4099, 65537, 1 << 20, 3 << 20)]
        torch.cuda.synchronize()
        out.append(_train(m, batches[3:]))
        del junk
        res[tag] = (out, ev)
    assert len(graphed._get_engine()._graph_steps) == 1
    assert torch.equal(res["eager"][1], res["graph"][1])
    for phase in range(2):
        (l0, g0), (l1, g1) = res["eager"][0][phase], res["graph"][0][phase]
        for step, (a, b) in enumerate(zip(l0, l1)):
            assert torch.isfinite(b) and torch.equal(a, b), (phase, step, a.item(), b.item())
        for step, (ga, gb) in enumerate(zip(g0, g1)):
            for (k, _), a, b in zip(eager.named_parameters(), ga, gb):
                assert torch.equal(a, b), (phase, step, k)
    for (k, a), (_, b) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.equal(a, b), k


def test_graphed_backward_refuses_weights_changed_since_its_forward():
    """the graphed node gets the parameter-version check of the eager node — an in-place update between forward and
    backward raises like stock autograd instead of mixing old packed images with new raw weights"""
    m = _mk("UNet3D", f_maps=[8, 16], num_groups=4).to(DEV)
    m.hip_graph = True
    m._get_engine().hip_graph = True
    m.train()
    (x, t), = _batches([(1, 1, 8, 16, 16)], 3)
    _, logits = m(x, return_logits=True)
    with torch.no_grad():
        m.final_conv.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        logits.sum().backward()
    _, logits = m(x, return_logits=True)  # a fresh forward -> backward pair works again
    logits.sum().backward()


def test_graph_mode_cuts_host_time_on_the_host_bound_shape():
    """BASELINE config 1's shape (UNet3D f_maps=16, 1x1x32x64x64) is host-bound in eager mode (~3.3 ms of ctypes + allocator work
    per step against ~3 ms of kernels, tools/host_bound_check.py); replaying two graphs must take well under a millisecond of
    host time.  The bound here is loose (shared CI hosts); the measured figures go to gpurun_out/parity_diag.jsonl."""
    from pytorch3dunet_amd.unet3d.losses import BCEDiceLoss

    res = {}
    for mode in ("eager", "graph"):
        m = _mk("UNet3D", f_maps=16, num_groups=8).to(DEV)
        if mode == "graph":
            m.hip_graph = True
            m._get_engine().hip_graph = True
        crit = BCEDiceLoss()
        opt = torch.optim.Adam(m.parameters(), lr=2e-4)
        (x, t), = _batches([(1, 1, 32, 64, 64)], 0)
        m.train()

        def step():
            _, logits = m(x, return_logits=True)
            loss = crit(logits, t)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        K = 20
        t0 = time.perf_counter()
        for _ in range(K):
            step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res[mode] = (1e3 * (t1 - t0) / K, 1e3 * (t2 - t0) / K)
    diag(test="graph_host_time_cfg1_shape", eager_host_ms=res["eager"][0], eager_step_ms=res["eager"][1],
         graph_host_ms=res["graph"][0], graph_step_ms=res["graph"][1])
    assert res["graph"][0] < 0.6 * res["eager"][0], res
    assert res["graph"][1] < res["eager"][1], res
