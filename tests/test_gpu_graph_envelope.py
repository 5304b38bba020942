"""-m gpu: `hip_graph: true` across everything the constructor accepts it for (engine.GraphStep).  A replayed step can be
wrong without any kernel being wrong: a packed image that is not rewritten inside the forward graph, a constant or descriptor table first
built during capture, a buffer a replay reads that nothing keeps alive, a host-side decision the eager path re-takes every step.  Every
case trains the same weights twice — eagerly and replayed — with SGD + momentum over alternating input shapes and demands the SAME BITS:
losses, every parameter gradient of every step, the input gradient where asked for, the final parameters, and an eval forward afterwards.
The eager step is what the rest of the suite holds to the float64 oracles; it is run twice per case, and must reproduce itself bit for bit
before bit-equality with it means anything (`_UNORDERED` names the cases where it does not, gated at 10x their own run-to-run distance).

CASES / FALLBACK_ORDERS are plain data: tests/test_graph_envelope_keys.py (no GPU) imports them and refuses a model key, layer order or
upsample value that is neither replayed here nor refused / declined by the executor."""
import copy
import warnings

import pytest
import torch

import test_gpu_graph as tg
from conftest import diag, loss_by_name

pytestmark = tg.pytestmark
DEV = tg.DEV

# the smallest shapes at which the paths exist: exact-2x levels (sub-pixel decoder kernels) and n -> 2n + 1 levels (general nearest tables);
# two shapes alternate, so steps 3 and 4 return to graphs captured at steps 1 and 2
EXACT = [(1, 1, 8, 16, 16), (2, 1, 8, 16, 16)] * 2
ODD = [(1, 1, 9, 13, 11), (1, 1, 17, 33, 35)] * 2
SMALL = dict(f_maps=[8, 16, 32], num_groups=4)


def _with_channels(shapes, c):
    return [(s[0], c) + tuple(s[2:]) for s in shapes]


def _case(cid, cls, kw, loss="bce_dice", shapes=EXACT, xgrad=False):
    kw = dict(kw, hip_graph=True)
    return (cid, cls, kw, loss, _with_channels(shapes, kw.get("in_channels", 1)), xgrad)


SOFTMAX = dict(in_channels=2, out_channels=3, final_sigmoid=False)
_ORDERS = ["gcl", "gce", "gc", "cgr", "cgl", "cge", "cg", "crg", "clg", "ceg", "cr", "cl", "ce", "c"]

CASES = [
    # compute_dtype fp32_split: the three-part bf16 images must be rewritten inside the forward graph after every optimizer step
    _case("f32s-unet3d", "UNet3D", dict(f_maps=32, num_groups=8, compute_dtype="fp32_split")),
    _case("f32s-se3d-softmax", "ResidualUNetSE3D", dict(f_maps=[32, 64, 128], num_groups=8, compute_dtype="fp32_split", in_channels=3,
                                                       out_channels=2, final_sigmoid=False), "probs_sum", [(1, 1, 9, 13, 11), (1, 1, 8, 16, 16)] * 2),
    # ... next to the slab images of n -> 2n + 1 levels; and bf16 operands under a post-norm order at such levels (a pairing, not an axis)
    _case("f32s-unet3d-odd", "UNet3D", dict(f_maps=32, num_levels=3, num_groups=8, compute_dtype="fp32_split"), shapes=ODD),
    _case("bf16-unet3d-odd-cgr", "UNet3D", dict(f_maps=32, num_levels=3, num_groups=8, compute_dtype="bf16", layer_order="cgr"), shapes=ODD),
    # every layer order the executor runs besides 'gcr' (post-norm passes, pair statistics, bias tables, identity tables), exact and odd
    # sizes in turn
    *[_case(f"order-{o}", "UNet3D", dict(SMALL, layer_order=o), shapes=(EXACT if i % 2 == 0 else ODD)) for i, o in enumerate(_ORDERS)],
    # ... and the residual executor's own forms of a post-norm, a pre-norm LeakyReLU, a norm-last and a norm-free order
    *[_case(f"res-order-{o}", "ResidualUNet3D", dict(SMALL, layer_order=o), shapes=(ODD if i % 2 == 0 else EXACT))
      for i, o in enumerate(["cge", "gcl", "crg", "cr"])],
    # up-sampling: transposed convolutions with their own packed images, the int32 index / weight tables of the resampling kernels
    _case("up-nearest", "UNet3D", dict(SMALL, upsample="nearest"), shapes=ODD),
    _case("up-deconv", "UNet3D", dict(SMALL, upsample="deconv")),
    _case("up-deconv-odd-softmax", "UNet3D", dict(SMALL, upsample="deconv", **SOFTMAX), "probs_sum", ODD),
    _case("up-trilinear", "UNet3D", dict(SMALL, upsample="trilinear"), shapes=ODD),
    _case("up-area", "UNet3D", dict(SMALL, upsample="area")),
    _case("up-deconv-res3d", "ResidualUNet3D", dict(SMALL, upsample="deconv"), shapes=ODD),
    _case("up-deconv-se3d", "ResidualUNetSE3D", dict(SMALL, upsample="deconv")),
    # heads: softmax with a gradient through the probabilities (the softmax branch of the graphed node's backward), softmax under a
    # class-index loss, and a regression model (no probabilities at all)
    _case("head-softmax-probs", "UNet3D", dict(SMALL, **SOFTMAX), "probs_sum"),
    _case("head-softmax-ce", "ResidualUNet3D", dict(SMALL, **SOFTMAX), "ce", ODD),
    _case("head-regression", "UNet3D", dict(SMALL, is_segmentation=False, out_channels=2), "mse", ODD),
    _case("head-regression-res3d", "ResidualUNet3D", dict(SMALL, is_segmentation=False), "mse"),
    # an input that requires grad: need_dx is part of the capture key and of the captured backward
    _case("xgrad-unet3d", "UNet3D", dict(SMALL, in_channels=2), shapes=ODD, xgrad=True),
    _case("xgrad-res3d", "ResidualUNet3D", dict(SMALL), xgrad=True),
    # recomputation inside the captured backward, fp32
    _case("ckpt-encoders", "ResidualUNet3D", dict(SMALL, checkpoint_encoders=True)),
    _case("ckpt-levels-1", "ResidualUNetSE3D", dict(SMALL, checkpoint_encoders=True, checkpoint_levels=1), shapes=ODD),
    # bf16 operands with fp32 activation storage on a net that would qualify for bf16 storage
    _case("bf16-act-fp32", "ResidualUNet3D", dict(f_maps=[64, 128], num_groups=8, compute_dtype="bf16", activation_dtype="fp32")),
    _case("conv-upscale-1", "UNet3D", dict(SMALL, conv_upscale=1), shapes=ODD),
    _case("levels-2", "UNet3D", dict(f_maps=8, num_levels=2, num_groups=4)),
    _case("levels-5", "UNet3D", dict(f_maps=8, num_levels=5, num_groups=4), shapes=[(1, 1, 16, 16, 16), (1, 1, 16, 32, 16)] * 2),
    # sizes that are odd at every level: 7 -> 3 -> 1, 15 -> 7 -> 3, 23 -> 11 -> 5
    _case("odd-every-level", "UNet3D", dict(SMALL), shapes=[(1, 1, 7, 15, 23), (2, 1, 15, 7, 7)] * 2),
]

# layer orders the executor declines to capture (`_graph_blocker`): the step runs eagerly under the flag, with one warning
FALLBACK_ORDERS = ["bcr", "gcrd", "crD", "cbr", "crb", "cbl", "gcrD", "cgld", "crd", "bcrD"]

# cases whose EAGER step does not reproduce itself bit for bit (an unordered floating-point sum in a kernel): gated at 10x their measured
# run-to-run distance instead.  At most two may ever stand here.
_UNORDERED: set = set()


# 'probs_sum' is a SUM over voxels (gradients ~1e4 times those of the mean-reduced losses): a step size that keeps four steps finite
_LR = {"probs_sum": 1e-5}


def _loss(name):
    if name in ("bce_dice", "ce"):  # the fused losses, taken on the logits like the trainer does; 'ce' with a class-index target
        from pytorch3dunet_amd.unet3d.losses import BCEDiceLoss, CrossEntropyLoss

        crit = BCEDiceLoss() if name == "bce_dice" else CrossEntropyLoss()
        return lambda probs, logits, t: crit(logits, t)
    return lambda probs, logits, t: loss_by_name(name, probs, logits, t)


def _data(kw, loss, shapes, xgrad, seed=5):
    """[(x, target)] on the device: a float target of the output's shape, class indices for 'ce'"""
    g = torch.Generator().manual_seed(seed)
    co = kw.get("out_channels", 1)
    out = []
    for shp in shapes:
        x = torch.randn(shp, generator=g)
        if loss == "ce":
            t = torch.randint(0, co, (shp[0],) + tuple(shp[2:]), generator=g)
        else:
            t = (torch.rand((shp[0], co) + tuple(shp[2:]), generator=g) > 0.6).float()
        x = x.to(DEV)
        if xgrad:
            x.requires_grad_()
        out.append((x, t.to(DEV)))
    return out


def _pair(cls, kw):
    """(eager, graphed): two copies of one initialisation; the graphed one keeps the constructor's flag"""
    base = tg._mk(cls, **kw)
    assert base.hip_graph
    eager = copy.deepcopy(base)
    eager.hip_graph = False
    return eager.to(DEV), copy.deepcopy(base).to(DEV)


def _run(model, batches, loss, seed=None, between=None):
    """one trajectory: (losses, per-step gradients, input gradients, final parameters + buffers).  `between(step)` runs before step > 0."""
    if seed is not None:
        torch.manual_seed(seed)
    xg, losses, grads = [], [], []
    opt = torch.optim.SGD(model.parameters(), lr=_LR.get(loss, 1e-2), momentum=0.9)
    for i, b in enumerate(batches):
        if between is not None and i:
            between(i)
        l, g = tg._train(model, [b], loss=_loss(loss), xgrads=xg, opt=opt)
        losses += l
        grads += g
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert all(torch.isfinite(l) for l in losses), losses
    return losses, grads, xg, state


def _flat(run):
    """every figure of a trajectory as one list of (label, tensor)"""
    losses, grads, xg, state = run
    out = [(f"loss of step {i}", l) for i, l in enumerate(losses)]
    out += [(f"gradients of step {i}", torch.cat([t.flatten() for t in g])) for i, g in enumerate(grads)]
    out += [(f"input gradient of step {i}", t) for i, t in enumerate(xg)]
    out += [(f"{k} after training", v) for k, v in state.items()]
    return out


def _distance(a, b):
    """largest relative L2 distance between corresponding figures of two trajectories"""
    worst = 0.0
    for (_, u), (_, v) in zip(_flat(a), _flat(b)):
        u, v = u.double(), v.double()
        worst = max(worst, ((u - v).norm() / u.norm().clamp_min(1e-30)).item())
    return worst


def _assert_same_bits(a, b, names, what):
    la, ga, xa, sa = a
    lb, gb, xb, sb = b
    assert len(la) == len(lb) and len(xa) == len(xb)
    for step, (u, v) in enumerate(zip(la, lb)):
        assert torch.equal(u, v), f"{what}: loss differs at step {step}: {u.item()} vs {v.item()}"
    for step, (gu, gv) in enumerate(zip(ga, gb)):
        for k, u, v in zip(names, gu, gv):
            assert torch.equal(u, v), f"{what}: gradient of {k} differs at step {step}"
    for step, (u, v) in enumerate(zip(xa, xb)):
        assert torch.equal(u, v), f"{what}: input gradient differs at step {step}"
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: {k} differs after training"


def _assert_replayed(graphed, batches, loss):
    """one further step goes through two graph launches: only a fused loss reaches the C-ABI (at most 6 launches, forward + backward)"""
    from pytorch3dunet_amd import _native as nat

    fn = _loss(loss)
    x, t = batches[0]
    graphed.train()
    n1 = nat.launch_count
    probs, logits = graphed(x, return_logits=True)
    fn(probs, logits, t).backward()
    torch.cuda.synchronize()
    assert nat.launch_count - n1 <= 6, nat.launch_count - n1
    x.grad = None


@pytest.mark.parametrize("cid,cls,kw,loss,shapes,xgrad", CASES, ids=[c[0] for c in CASES])
def test_every_accepted_configuration_replays_the_eager_trajectory(cid, cls, kw, loss, shapes, xgrad):
    eager, graphed = _pair(cls, kw)
    again = copy.deepcopy(eager)
    batches = _data(kw, loss, shapes, xgrad)
    names = [k for k, _ in eager.named_parameters()]
    r0 = _run(eager, batches, loss)
    r0b = _run(again, batches, loss)
    r1 = _run(graphed, batches, loss)
    assert len(r0[2]) == (len(shapes) if xgrad else 0)
    eng = graphed._get_engine()
    assert eng._graph_off_reason is None
    assert len(eng._graph_steps) == min(len(set(shapes)), 2)
    if cid in _UNORDERED:
        d_eager, d_graph = _distance(r0, r0b), _distance(r0, r1)
        diag(test="graph_envelope_unordered", case=cid, eager_vs_eager=d_eager, graph_vs_eager=d_graph)
        assert d_graph <= 10.0 * d_eager, (cid, d_graph, d_eager)
    else:
        _assert_same_bits(r0, r0b, names, "eager vs eager")  # the yardstick reproduces itself ...
        _assert_same_bits(r0, r1, names, "graph vs eager")   # ... and the replayed step is it
    _assert_replayed(graphed, batches, loss)
    # inference of the same model object stays eager and sees the trained weights
    graphed.eval(), eager.eval(), again.eval()
    with torch.no_grad():
        x = batches[0][0].detach()
        y1, y0, y0b = graphed(x), eager(x), again(x)
        if cid in _UNORDERED:
            rel = lambda u, v: ((u.double() - v.double()).norm() / v.double().norm()).item()  # noqa: E731
            diag(test="graph_envelope_unordered_eval", case=cid, eager_vs_eager=rel(y0b, y0), graph_vs_eager=rel(y1, y0))
            assert rel(y1, y0) <= 10.0 * rel(y0b, y0), (cid, rel(y1, y0), rel(y0b, y0))
        else:
            assert torch.equal(y1, y0)


def _churn():
    """drop everything the allocator can drop, then fill fresh blocks with NaNs: a freed table or image would be handed out again"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (257, 4099, 65537, 1 << 20, 3 << 20)]
    torch.cuda.synchronize()
    return junk


def test_a_third_shape_evicts_the_oldest_step_and_it_is_captured_again():
    """more input shapes than the executor keeps graphs for (2): A, B, C, A, B — step 3 evicts A's graphs and pool, step 4 captures A again
    (evicting B), step 5 captures B again; then the same cycle with the allocator emptied and churned between steps 3 and 4"""
    from pytorch3dunet_amd import _engine_graph

    assert _engine_graph._GRAPH_MAX_SHAPES == 2
    kw = dict(f_maps=[8, 16], num_groups=4, hip_graph=True)
    A, B, C = (1, 1, 8, 16, 16), (2, 1, 8, 16, 16), (1, 1, 9, 13, 11)
    shapes = [A, B, C, A, B]
    eager, graphed = _pair("UNet3D", kw)
    names = [k for k, _ in eager.named_parameters()]
    batches = _data(kw, "bce_dice", shapes, False)
    seen = []

    def count(step):
        seen.append(len(graphed._get_engine()._graph_steps))

    r0 = _run(eager, batches, "bce_dice")
    r1 = _run(graphed, batches, "bce_dice", between=count)
    seen.append(len(graphed._get_engine()._graph_steps))
    assert seen == [1, 2, 2, 2, 2], seen
    _assert_same_bits(r0, r1, names, "graph vs eager")
    held = []
    more = _data(kw, "bce_dice", shapes, False, seed=6)
    r2 = _run(eager, more, "bce_dice", between=lambda step: held.append(_churn()) if step == 3 else None)
    r3 = _run(graphed, more, "bce_dice", between=lambda step: held.append(_churn()) if step == 3 else None)
    assert len(graphed._get_engine()._graph_steps) == 2 and graphed._get_engine()._graph_off_reason is None
    assert all(torch.isfinite(l) for l in r3[0]), r3[0]
    _assert_same_bits(r2, r3, names, "graph vs eager after allocator churn")
    del held


@pytest.mark.parametrize("cls,kw", [("UNet3D", dict(f_maps=[8, 16], num_groups=4)),
                                    ("UNet3D", dict(f_maps=[32, 64], num_groups=8, compute_dtype="fp32_split"))], ids=["fp32", "fp32_split"])
def test_in_place_load_state_dict_between_replays_is_seen(cls, kw):
    """resume / fine-tune: load_state_dict (in place, the default) of other weights between two training steps — the next replay must read
    them, every packed image of them included (fp32_split: the three-part bf16 images)"""
    kw = dict(kw, hip_graph=True)
    eager, graphed = _pair(cls, kw)
    names = [k for k, _ in eager.named_parameters()]
    batches = _data(kw, "bce_dice", [(1, 1, 8, 16, 16)] * 4, False)
    g = torch.Generator().manual_seed(9)
    other = {k: v.detach().cpu() for k, v in eager.state_dict().items()}
    other = {k: (v + 0.05 * torch.randn(v.shape, generator=g) if v.is_floating_point() else v) for k, v in other.items()}
    runs = []
    for m in (eager, graphed):
        ptr = next(m.parameters()).data_ptr()

        def load(step, m=m):
            if step == 2:
                m.load_state_dict(other)

        runs.append(_run(m, batches, "bce_dice", between=load))
        assert next(m.parameters()).data_ptr() == ptr  # (in place: the graphs' parameter pointers stay valid)
    eng = graphed._get_engine()
    assert len(eng._graph_steps) == 1 and eng._graph_off_reason is None
    _assert_same_bits(runs[0], runs[1], names, "graph vs eager")
    # (the loaded weights did change the step: the trajectory without the load differs)
    plain, _ = _pair(cls, kw)
    assert not torch.equal(_run(plain, batches, "bce_dice")[0][2], runs[0][0][2])


@pytest.mark.parametrize("order", FALLBACK_ORDERS)
def test_orders_that_cannot_be_captured_warn_once_and_run_the_eager_step(order):
    from pytorch3dunet_amd.engine import _graph_blocker

    kw = dict(f_maps=[8, 16], num_groups=4, layer_order=order, dropout_prob=0.25, hip_graph=True)
    eager, flagged = _pair("UNet3D", kw)
    names = [k for k, _ in eager.named_parameters()]
    batches = _data(kw, "bce_dice", EXACT, False)
    r0 = _run(eager, batches, "bce_dice", seed=1234)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r1 = _run(flagged, batches, "bce_dice", seed=1234)
    eng = flagged._get_engine()
    why = _graph_blocker(eng)
    assert why is not None and order in why
    told = [w for w in rec if issubclass(w.category, UserWarning) and "hip_graph" in str(w.message)]
    assert len(told) == 1 and why in str(told[0].message), [str(w.message) for w in rec]
    assert eng._graph_off_reason == why and not eng._graph_steps
    assert eager._get_engine()._graph_off_reason is None
    if "b" in order:
        assert any("running_mean" in k for k in r0[3]) and any(int(v) == len(batches) for k, v in r0[3].items() if k.endswith("num_batches_tracked"))
    _assert_same_bits(r0, r1, names, "flagged vs plain eager")  # (BatchNorm's running estimates are part of the compared state)


def test_a_dropped_model_is_collected_before_the_next_capture_not_during_it():
    """A model and its executor point at each other: a dropped model's captured steps (hipGraphs, their pool, streams, events) wait for
    Python's cycle collector, which fires wherever its counters trip — inside another model's stream capture too (the whole GPU suite in
    one process aborted there, in the collector, under the captured backward of the eviction test above).  GraphStep collects BEFORE it
    captures and holds the collector off until the capture is over.  Here the collector is off for the whole test, so the only thing
    that can free the first model's step is the second model's capture — before it begins."""
    import gc
    import weakref

    kw = dict(f_maps=[8, 16], num_groups=4, hip_graph=True)
    batches = _data(kw, "bce_dice", [(1, 1, 8, 16, 16)] * 2, False)
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        _, old = _pair("UNet3D", kw)
        _run(old, batches, "bce_dice")
        step = weakref.ref(next(iter(old._get_engine()._graph_steps.values())))
        del old
        assert step() is not None  # (the cycle: reference counting alone does not free it)
        _, new = _pair("UNet3D", kw)
        _run(new, batches, "bce_dice")
        assert step() is None, "the dead model's captured step was still waiting for the collector during the next capture"
        assert not gc.isenabled()  # (GraphStep restores what it found)
    finally:
        if was:
            gc.enable()
