"""-m gpu: the fused regression losses (u3d_reg_loss_*) and the factory's loss options inside the kernels (the *_ex entry
points: `skip_last_target` as a strided target, `ignore_index` through MaskingLossWrapper as a compare in the kernel,
a one-element `pos_weight`) against the live reference's golden vectors (tests/golden/l3_losses_reg.npz), against float64
torch at the shipped shapes and odd voxel counts, and for the properties that tell the feature from the wrappers merely
still working: no full-size stock operator and no copy in front of the kernels, no host synchronisation, bitwise
reproducibility, exact zeros at ignored voxels, and unchanged results on the option-free paths."""
import copy
import ctypes

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import unet3d_oracle as orc
from losses_reg_util import CASES, caller_losses, check_case, criterion, spec_of
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.unet3d import losses as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MOD = caller_losses()


@pytest.mark.parametrize("case", CASES)
def test_fused_criterion_matches_reference_golden(case):
    """the bars of test_gpu_losses_mc.py's golden test (loss 1e-5 * max(1, |ref|), gradient 1e-3 * max|grad_ref|)"""
    n0 = nat.launch_count
    check_case(MOD, case, "cuda", 1e-5, 1e-3)
    assert nat.launch_count > n0, "fused loss kernels did not run"


IGN, SKIP = {"ignore_index": -1}, {"skip_last_target": True}
WSL1 = {"name": "WeightedSmoothL1Loss", "threshold": 0.5, "initial_weight": 3.0}
# name: (loss config, target kind)
REG = {
    "mse": ({"name": "MSELoss"}, "real"),
    "l1": ({"name": "L1Loss"}, "real"),
    "smooth_l1": ({"name": "SmoothL1Loss"}, "real"),
    "wsl1_below": ({**WSL1, "apply_below_threshold": True}, "real"),
    "wsl1_above": ({**WSL1, "apply_below_threshold": False}, "real"),
    "mse_ign": ({"name": "MSELoss", **IGN}, "real"),
    "l1_ign": ({"name": "L1Loss", **IGN}, "real"),
    "smooth_l1_ign": ({"name": "SmoothL1Loss", **IGN}, "real"),
    "wsl1_ign": ({**WSL1, **IGN}, "real"),
    "smooth_l1_skip": ({"name": "SmoothL1Loss", **SKIP}, "real"),
    "wsl1_ign_skip": ({**WSL1, **IGN, **SKIP}, "real"),
}
SEG = {
    "bcedice_skip": ({"name": "BCEDiceLoss", **SKIP}, "binary"),
    "bcedice_ign": ({"name": "BCEDiceLoss", **IGN}, "binary"),
    "bcedice_ign_skip": ({"name": "BCEDiceLoss", "alpha": 0.7, **IGN, **SKIP}, "binary"),
    "dice_sigmoid_ign_skip": ({"name": "DiceLoss", **IGN, **SKIP}, "binary"),
    "dice_softmax_ign": ({"name": "DiceLoss", "normalization": "softmax", **IGN}, "onehot"),
    "dice_softmax_skip": ({"name": "DiceLoss", "normalization": "softmax", **SKIP}, "onehot"),
    "dice_none_ign_skip": ({"name": "DiceLoss", "normalization": "none", **IGN, **SKIP}, "onehot"),
    "gdl_ign": ({"name": "GeneralizedDiceLoss", **IGN}, "binary"),
    "gdl_softmax_ign_skip": ({"name": "GeneralizedDiceLoss", "normalization": "softmax", **IGN, **SKIP}, "onehot"),
    "bce_skip": ({"name": "BCEWithLogitsLoss", **SKIP}, "binary"),
    "bce_ign": ({"name": "BCEWithLogitsLoss", **IGN}, "binary"),
    "bce_pw": ({"name": "BCEWithLogitsLoss", "pos_weight": [2.5]}, "binary"),
    "bce_pw_ign_skip": ({"name": "BCEWithLogitsLoss", "pos_weight": [0.375], **IGN, **SKIP}, "binary"),
    "ce_skip_squeeze": ({"name": "CrossEntropyLoss", **SKIP, "squeeze_channel": True}, "label2"),
    "wce_skip_squeeze": ({"name": "WeightedCrossEntropyLoss", **SKIP, "squeeze_channel": True}, "label2"),
}
ALL = {**REG, **SEG}


def _inputs(spec, kind, shape, seed):
    """logits and a target whose values are exact in fp32 (multiples of 1/256, 0/1, -1): the threshold 0.5 and the ignore
    value decide the same way in fp32 and in float64"""
    g = torch.Generator().manual_seed(seed)
    n, c = shape[0], shape[1]
    x = 2.5 * torch.randn(shape, generator=g)
    tc = c + 1 if spec.get("skip_last_target") else c
    tshape = (n, tc) + tuple(shape[2:])
    if kind == "real":
        t = torch.randint(0, 257, tshape, generator=g).float() / 256
    elif kind == "binary":
        t = (torch.rand(tshape, generator=g) > 0.6).float()
    elif kind == "onehot":
        t = torch.nn.functional.one_hot(torch.randint(0, tc, (n,) + tuple(shape[2:]), generator=g), tc).movedim(-1, 1).float()
    else:  # int64 (N, 2, *S): labels in channel 0, the skipped channel behind it
        t = torch.randint(0, c, (n, 2) + tuple(shape[2:]), generator=g)
    if spec.get("ignore_index") is not None and kind != "label2":
        t[torch.rand(tshape, generator=g) < 0.2] = float(spec["ignore_index"])
    return x, t


def _vs_float64(name, shape, seed):
    """the fused criterion on the device against the same criterion object in float64 on the CPU, where every class of the
    tree runs its stock statements (the wrappers' own forward, the losses' torch branch)"""
    spec, kind = ALL[name]
    x, t = _inputs(spec, kind, shape, seed)
    crit = criterion(MOD, spec, "cpu")
    xr = x.double().requires_grad_(True)
    ref = copy.deepcopy(crit).double()(xr, t if t.dtype == torch.int64 else t.double())
    ref.backward()
    n0 = nat.launch_count
    xd = x.to(DEV).requires_grad_(True)
    val = crit.to(DEV)(xd, t.to(DEV))
    val.backward()
    assert nat.launch_count > n0, "fused loss kernels did not run"
    e_loss = abs(val.item() - ref.item())
    scale = xr.grad.abs().max().item()
    e_grad = (xd.grad.cpu().double() - xr.grad).abs().max().item()
    print(f"{name} {shape}: loss {val.item():.8f} float64 {ref.item():.8f}, gradient max err {e_grad:.3e} of scale {scale:.3e}")
    assert e_loss <= 1e-5 * max(1.0, abs(ref.item())), (name, shape, val.item(), ref.item())
    assert e_grad <= 1e-3 * scale, (name, shape, e_grad, scale)


@pytest.mark.parametrize("name", sorted(REG))
def test_regression_vs_float64_denoising_shape(name):
    """the patch of resources/3DUnet_denoising/train_config_regression.yaml: one channel at 128^3"""
    _vs_float64(name, (1, 1, 128, 128, 128), 11)


@pytest.mark.parametrize("name", ["bcedice_skip", "bcedice_ign_skip", "bce_pw_ign_skip", "gdl_ign"])
def test_segmentation_options_vs_float64_shipped_shape(name):
    """BASELINE config 2's logits (2, 1, 64, 128, 128), with the 2-channel target of the configs that skip the last channel"""
    _vs_float64(name, (2, 1, 64, 128, 128), 12)


@pytest.mark.parametrize("name", sorted(ALL))
@pytest.mark.parametrize("shape", [(3, 5, 5, 7, 9), (1, 2, 1, 1, 1)])
def test_vs_float64_odd_voxel_counts(name, shape):
    _vs_float64(name, shape, 13)


@pytest.mark.parametrize("name", ["dice_softmax_ign", "gdl_softmax_ign_skip", "dice_softmax_skip", "dice_none_ign_skip"])
def test_masked_softmax_dice_vs_float64_wide_head(name):
    """C = 20 > 16: the channel-sums pass works in channel chunks and takes the voxel's masked softmax terms from memory"""
    _vs_float64(name, (2, 20, 3, 5, 7), 14)


class _Recorder(TorchDispatchMode):
    """every ATen op with what it allocates or writes: (name, elements of the largest tensor it returns that is not a view of
    an argument, elements of the largest argument it mutates)"""

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        flat_in = [a for a in torch.utils._pytree.tree_leaves((args, kwargs or {})) if isinstance(a, torch.Tensor)]
        flat_out = [o for o in torch.utils._pytree.tree_leaves(out) if isinstance(o, torch.Tensor)]
        held = {a.untyped_storage().data_ptr() for a in flat_in if a.numel()}
        fresh = max([o.numel() for o in flat_out if o.untyped_storage().data_ptr() not in held], default=0)
        written = 0
        if func._schema.is_mutable:
            for arg, a in zip(func._schema.arguments, args):
                if arg.alias_info is not None and arg.alias_info.is_write and isinstance(a, torch.Tensor):
                    written = max(written, a.numel())
        self.ops.append((func._schema.name, fresh, written))
        return out


STACKS = {"skip": SKIP, "ignore": IGN, "ignore+skip": {**IGN, **SKIP}}


@pytest.mark.parametrize("stack", sorted(STACKS))
@pytest.mark.parametrize("loss", ["BCEDiceLoss", "DiceLoss", "GeneralizedDiceLoss", "BCEWithLogitsLoss", "SmoothL1Loss"])
def test_no_copy_and_no_stock_operator_in_front_of_the_kernels(loss, stack):
    """forward + backward of the factory's criterion under a dispatch-mode recorder: no ATen op allocates or writes a tensor
    with as many elements as the logits (the target is larger), except the one `empty_like` that is dlogits.  A real copy of
    the sliced target would show as aten::clone / aten::copy_, the masking wrapper's statements as clone / ne_ / mul."""
    spec = {"name": loss, **STACKS[stack]}
    x, t = _inputs(spec, "binary", (2, 3, 8, 16, 16), 21)
    crit = criterion(MOD, spec, DEV)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV)
    crit(xd, td).backward()  # warm-up: library load, a cached pos_weight
    xd.grad = None
    torch.cuda.synchronize()
    full = xd.numel()
    n0 = nat.launch_count
    with _Recorder() as rec:
        val = crit(xd, td)
        (grad,) = torch.autograd.grad(1.7 * val, xd)
    torch.cuda.synchronize()
    assert nat.launch_count >= n0 + 2, "forward and backward must both be native calls"
    big = [op for op in rec.ops if op[1] >= full or op[2] >= full]
    assert big == [("aten::empty_like", full, 0)], (big, rec.ops)
    assert grad.shape == xd.shape and torch.isfinite(grad).all()


@pytest.mark.parametrize("below", [True, False])
def test_weighted_smooth_l1_has_no_gather_and_no_sync(below):
    """WeightedSmoothL1Loss forward + backward: none of the operators of the stock `l1[mask] = l1[mask] * w` form (nonzero,
    index, index_put_) and no device-to-host read (_local_scalar_dense) is dispatched, and the step also runs under
    torch.cuda.set_sync_debug_mode("error"), which this ROCm build of torch honours (the probe below makes it raise on
    `.item()`; were it not honoured the probe fails the test rather than passing it silently)."""
    spec = {**WSL1, "apply_below_threshold": below}
    x, t = _inputs(spec, "real", (1, 1, 32, 32, 32), 22)
    crit = criterion(MOD, spec, DEV)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV)
    crit(xd, td).backward()
    torch.cuda.synchronize()
    n0 = nat.launch_count
    with _Recorder() as rec:
        (grad,) = torch.autograd.grad(crit(xd, td) * 1.7, xd)
    assert nat.launch_count >= n0 + 2
    names = {op[0] for op in rec.ops}
    assert not names & {"aten::nonzero", "aten::index", "aten::index_put_", "aten::index_put", "aten::_local_scalar_dense",
                        "aten::masked_select", "aten::where"}, names
    probe = torch.ones(1, device=DEV)
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        (grad2,) = torch.autograd.grad(crit(xd, td) * 1.7, xd)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert torch.equal(grad, grad2)


@pytest.mark.parametrize("name", sorted(ALL))
def test_new_native_paths_bitwise_reproducible(name):
    spec, kind = ALL[name]
    x, t = _inputs(spec, kind, (2, 3, 24, 40, 56), 23)
    crit = criterion(MOD, spec, DEV)
    x, t = x.to(DEV), t.to(DEV)
    out = []
    for _ in range(2):
        xd = x.clone().requires_grad_(True)
        n0 = nat.launch_count
        val = crit(xd, t)
        val.backward()
        assert nat.launch_count > n0
        out.append((val.detach().clone(), xd.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("name", sorted(k for k, (s, kind) in ALL.items() if "ignore_index" in s and kind != "label2"))
def test_masked_gradient_is_exactly_zero_and_target_untouched(name):
    spec, kind = ALL[name]
    x, t = _inputs(spec, kind, (2, 3, 5, 7, 9), 24)
    crit = criterion(MOD, spec, DEV)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV)
    before = td.clone()
    (crit(xd, td) * -2.75).backward()
    seen = td[:, :-1] if spec.get("skip_last_target") else td
    ignored = seen == -1
    assert ignored.any() and not ignored.all()
    assert torch.count_nonzero(xd.grad[ignored]).item() == 0
    assert torch.count_nonzero(xd.grad[~ignored]).item() > 0
    assert torch.equal(td, before)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def test_option_free_paths_equal_the_plain_entry_points_bitwise():
    """a contiguous target without options: BCEDiceLoss / DiceLoss(softmax) / CrossEntropyLoss give the bits of the plain
    entry points called directly through the C-ABI"""
    g = torch.Generator().manual_seed(25)
    n, c, sp = 2, 3, (9, 20, 28)
    v = sp[0] * sp[1] * sp[2]
    x = (2.0 * torch.randn((n, c) + sp, generator=g)).to(DEV)
    tb = (torch.rand((n, c) + sp, generator=g) > 0.6).float().to(DEV)
    lab = torch.randint(0, c, (n,) + sp, generator=g).to(DEV)
    lib = nat.get_lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    one = torch.ones(1, device=DEV)

    def via_class(crit, t):
        xd = x.clone().requires_grad_(True)
        val = crit(xd, t)
        val.backward()
        return val.detach().reshape(1), xd.grad

    loss, dl = torch.empty(1, device=DEV), torch.empty_like(x)
    # BCEDiceLoss(alpha = 0.7)
    sums = torch.empty(lib.u3d_bce_dice_scratch_doubles(n, c, v), dtype=torch.float64, device=DEV)
    coef = torch.empty(2 * c + 1, device=DEV)
    nat.call("u3d_bce_dice_fwd", 0, stream, _ptr(x), _ptr(tb), None, n, c, v, 1.0, 0.7, 1e-6, _ptr(sums), _ptr(loss), _ptr(coef))
    nat.call("u3d_bce_dice_bwd", 0, stream, _ptr(x), _ptr(tb), _ptr(coef), _ptr(one), n, c, v, _ptr(dl))
    val, grad = via_class(L.BCEDiceLoss(alpha=0.7), tb)
    assert torch.equal(val, loss) and torch.equal(grad, dl)
    # DiceLoss(softmax)
    sums = torch.empty(lib.u3d_dice_scratch_doubles(n, c, v), dtype=torch.float64, device=DEV)
    coef = torch.empty(3 * c, device=DEV)
    nat.call("u3d_dice_fwd", 0, stream, _ptr(x), _ptr(tb), None, n, c, v, 1, 0, 1e-6, _ptr(sums), _ptr(loss), _ptr(coef))
    nat.call("u3d_dice_bwd", 0, stream, _ptr(x), _ptr(tb), _ptr(coef), _ptr(one), n, c, v, 1, _ptr(dl))
    val, grad = via_class(L.DiceLoss(normalization="softmax"), tb)
    assert torch.equal(val, loss) and torch.equal(grad, dl)
    # CrossEntropyLoss
    sums = torch.empty(lib.u3d_softmax_ce_scratch_doubles(n, c, v), dtype=torch.float64, device=DEV)
    coef = torch.empty(c + 1, device=DEV)
    nat.call("u3d_softmax_ce_fwd", 0, stream, _ptr(x), _ptr(lab), None, n, c, v, -100, 0, _ptr(sums), _ptr(loss), _ptr(coef))
    nat.call("u3d_softmax_ce_bwd", 0, stream, _ptr(x), _ptr(lab), _ptr(coef), _ptr(one), n, c, v, -100, _ptr(dl))
    val, grad = via_class(L._upgrade(torch.nn.CrossEntropyLoss()), lab)
    assert torch.equal(val, loss) and torch.equal(grad, dl)


def test_skipped_channel_view_matches_its_contiguous_copy():
    """the target read in place through its sample stride against the same target copied to a dense tensor, which takes the
    plain entry points.  Both run the same formulas on the same numbers in fp32, in differently compiled kernels (the
    compiler may contract multiply-adds differently), so they agree to a few fp32 roundings: each of the ~20 operations of
    an element rounds to 2^-24 relative (6e-8), bounded here by 1e-6 on the loss and 1e-5 of the gradient's scale."""
    for name in ("bcedice_skip", "dice_softmax_skip", "smooth_l1_skip", "ce_skip_squeeze"):
        spec, kind = ALL[name]
        x, t = _inputs(spec, kind, (2, 3, 6, 10, 12), 26)
        crit = criterion(MOD, spec, DEV)
        inner = crit.loss
        x, t = x.to(DEV), t.to(DEV)
        dense = t[:, :-1].contiguous()
        dense = dense.squeeze(1) if spec.get("squeeze_channel") else dense
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a, b = crit(xa, t), inner(xb, dense)
        a.backward()
        b.backward()
        e_loss = abs(a.item() - b.item())
        e_grad, scale = (xa.grad - xb.grad).abs().max().item(), xb.grad.abs().max().item()
        print(f"{name}: strided against dense: loss diff {e_loss:.3e}, gradient max diff {e_grad:.3e} of scale {scale:.3e}")
        assert e_loss <= 1e-6 * max(1.0, abs(b.item())) and e_grad <= 1e-5 * scale, (name, e_loss, e_grad, scale)


def test_native_regression_step_with_fused_smooth_l1():
    """one whole native step: UNet3D(is_segmentation=False) with the factory's SmoothL1Loss against the same model with
    torch.nn.SmoothL1Loss evaluated on the device output by stock operators.  Only the loss kernel differs: dlogits to the
    gradient bar of the golden test, the parameter gradients to the same relative bar."""
    from pytorch3dunet_amd.unet3d.model import UNet3D

    torch.manual_seed(0)
    model = UNet3D(1, 1, is_segmentation=False, f_maps=[8, 16, 32], num_groups=4)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "groupnorm" in k:
                p.add_(0.2 * torch.randn_like(p))
    model = model.to(DEV).train()
    x = torch.randn(1, 1, 16, 24, 24, device=DEV)
    t = torch.randint(0, 257, (1, 1, 16, 24, 24)).float().div(256).to(DEV)
    crit = criterion(MOD, {"name": "SmoothL1Loss"}, DEV)
    assert type(crit) is L.SmoothL1Loss

    def step(loss_fn):
        model.zero_grad()
        n0 = nat.launch_count
        _, out = model(x, return_logits=True)
        out.retain_grad()
        n1 = nat.launch_count
        loss = loss_fn(out, t)
        n2 = nat.launch_count
        loss.backward()
        torch.cuda.synchronize()
        assert n1 > n0, "the native network did not run"
        return loss.detach(), out.grad.clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}, n2 - n1

    loss_a, dl_a, grads_a, calls_a = step(crit)
    loss_b, dl_b, grads_b, calls_b = step(torch.nn.SmoothL1Loss())
    assert calls_a > 0 and calls_b == 0
    assert abs(loss_a.item() - loss_b.item()) <= 1e-5 * max(1.0, abs(loss_b.item()))
    assert (dl_a - dl_b).abs().max().item() <= 1e-3 * dl_b.abs().max().item()
    worst = max((orc.rel_err(grads_a[k].cpu().double(), grads_b[k].cpu().double()), k) for k in grads_a)
    print(f"SmoothL1 step: loss {loss_a.item():.8f} stock {loss_b.item():.8f}, worst parameter gradient rel err {worst}")
    assert worst[0] < 1e-3, worst
