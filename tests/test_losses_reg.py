"""The regression losses and the factory's loss options (`ignore_index` through MaskingLossWrapper, `skip_last_target`,
`pos_weight`) on the CPU: the criterion `install_fused(caller's module).get_loss_criterion(spec)` builds against golden
vectors of the LIVE reference's factory (tests/golden/l3_losses_reg.npz, make_losses_reg.py), what the patch puts into the
caller's module, and the wrappers around a loss that is not ours.  The kernels are tested by test_gpu_losses_reg.py."""
import importlib.util
import os

import pytest
import torch

from losses_reg_util import CASES, caller_losses, check_case, criterion, foreign_objects, spec_of
from pytorch3dunet_amd.unet3d import losses as L


@pytest.mark.parametrize("case", CASES)
def test_factory_criterion_matches_reference_golden_on_cpu(case):
    """the bars of test_losses_mc.py's CPU check; every object of the returned tree is a class of our module"""
    mod = caller_losses()
    crit = check_case(mod, case, "cpu", 1e-6, 2e-5)
    assert not foreign_objects(crit), [type(m) for m in crit.modules()]


def test_install_patches_regression_losses_and_wrappers():
    plain = caller_losses(fused=False)
    mod = caller_losses()
    assert mod.MSELoss is L.MSELoss and mod.L1Loss is L.L1Loss and mod.SmoothL1Loss is L.SmoothL1Loss
    for name in ("WeightedSmoothL1Loss", "MaskingLossWrapper", "SkipLastTargetChannelWrapper"):
        ours, theirs = getattr(mod, name), getattr(plain, name)
        assert ours.__module__ == L.__name__ and ours.__name__ == name
        # built from the caller's own class, which stays the fallback
        assert [b.__name__ for b in ours.__mro__[1:2]] == [name] and ours.__mro__[1].__module__ != L.__name__, ours.__mro__
        assert theirs.__module__ != L.__name__
    crit = criterion(mod, {"name": "BCEDiceLoss", "ignore_index": -1, "skip_last_target": True}, "cpu")
    assert type(crit) is mod.SkipLastTargetChannelWrapper and type(crit.loss) is mod.MaskingLossWrapper
    assert type(crit.loss.loss) is L.BCEDiceLoss and crit.loss.ignore_index == -1
    w = criterion(mod, {"name": "WeightedSmoothL1Loss", "threshold": 0.5, "initial_weight": 3.0,
                        "apply_below_threshold": False}, "cpu")
    assert type(w) is mod.WeightedSmoothL1Loss and (w.threshold, w.weight, w.apply_below_threshold) == (0.5, 3.0, False)
    pw = criterion(mod, {"name": "BCEWithLogitsLoss", "pos_weight": [2.5]}, "cpu")
    assert type(pw) is L.BCEWithLogitsLoss and pw._pos_weight_value() == 2.5
    assert criterion(mod, {"name": "BCEWithLogitsLoss", "pos_weight": [1.0, 2.0]}, "cpu")._pos_weight_value() is None
    assert L.install_fused(mod) is mod and mod.MaskingLossWrapper is type(crit.loss)  # idempotent: nothing is derived twice


def test_wrappers_around_a_foreign_loss_behave_as_the_callers():
    """a wrapped loss that is not ours (a lambda): the patched wrappers compute what the caller's own wrappers compute"""
    plain, mod = caller_losses(fused=False), caller_losses()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 4, 5, 6), generator=g)
    t = torch.rand((2, 4, 4, 5, 6), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.3] = -1.0
    seen = []

    def foreign(a, b):
        seen.append((a.detach().clone(), b.detach().clone()))
        return ((a - b) ** 2).sum() + a.sum()

    outs = []
    for m in (plain, mod):
        xr = x.clone().requires_grad_(True)
        crit = m.SkipLastTargetChannelWrapper(m.MaskingLossWrapper(foreign, -1))
        val = crit(xr, t)
        val.backward()
        outs.append((val.detach(), xr.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    (a0, b0), (a1, b1) = seen
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and b1.shape == x.shape
    # the masked elements reached the foreign loss as zeros: the caller's statements ran
    assert torch.count_nonzero(b1[t[:, :-1] == -1]).item() == 0 and torch.count_nonzero(a1[t[:, :-1] == -1]).item() == 0
    sq = mod.SkipLastTargetChannelWrapper(lambda a, b: b, squeeze_channel=True)(x, t[:, :2])
    assert sq.shape == (2, 4, 5, 6) and torch.equal(sq, t[:, 0])


def test_sample_stride_of_target_views():
    t = torch.zeros(3, 4, 5, 6, 7)
    assert L._sample_stride(t) == 4 * 210
    assert L._sample_stride(t[:, :-1]) == 4 * 210 and t[:, :-1].numel() // 3 == 3 * 210  # dense samples, 4 channels apart
    assert L._sample_stride(t[:, :-1][:1]) == 3 * 210  # a single sample: its own size
    assert L._sample_stride(torch.zeros(3, 2, 5, 6, 7, dtype=torch.int64)[:, :-1].squeeze(1)) == 2 * 210
    assert L._sample_stride(t[:, 1:]) == 4 * 210  # an offset view: the data pointer carries the offset
    assert L._sample_stride(t[:, :, ::2]) is None and L._sample_stride(t.transpose(1, 2)) is None
    assert L._sample_stride(t[..., :-1]) is None and L._sample_stride(t.expand(3, 4, 5, 6, 7)[::2]) == 8 * 210
    assert L._sample_stride(torch.zeros(1, 4, 5).expand(3, 4, 5)) is None  # samples that overlap are copied


def test_regression_classes_fall_back_to_torch():
    """CPU tensors, other reductions and dtypes compute torch's own values"""
    g = torch.Generator().manual_seed(6)
    x, t = torch.randn((2, 3, 4, 5), generator=g), torch.randn((2, 3, 4, 5), generator=g)
    for ours, theirs in ((L.MSELoss, torch.nn.MSELoss), (L.L1Loss, torch.nn.L1Loss), (L.SmoothL1Loss, torch.nn.SmoothL1Loss)):
        for kw in ({}, {"reduction": "sum"}, {"reduction": "none"}):
            assert torch.equal(ours(**kw)(x, t), theirs(**kw)(x, t))
        assert torch.equal(ours()(x.double(), t.double()), theirs()(x.double(), t.double()))
    assert torch.equal(L.SmoothL1Loss(beta=0.25)(x, t), torch.nn.SmoothL1Loss(beta=0.25)(x, t))


def test_factory_criterion_matches_live_reference():
    """the patched LIVE reference factory against the unpatched one on fresh inputs (skips where the reference is absent);
    a private copy of the reference's module is patched, the shared one stays as it is"""
    from ref_import import REFERENCE_ROOT, import_reference, reference_available

    if not reference_available():
        pytest.skip("the reference checkout is not present")
    import_reference()
    R = importlib.import_module("pytorch3dunet.unet3d.losses")
    spec = importlib.util.spec_from_file_location("_u3d_private_reference_losses",
                                                  os.path.join(REFERENCE_ROOT, "pytorch3dunet", "unet3d", "losses.py"))
    P = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(P)
    L.install_fused(P)
    g = torch.Generator().manual_seed(78)
    for case in CASES:
        s = spec_of(case)
        if s["name"] == "CrossEntropyLoss":
            continue
        c = 3
        x = 2.0 * torch.randn((2, c, 5, 6, 7), generator=g)
        t = torch.rand((2, c + 1 if s.get("skip_last_target") else c, 5, 6, 7), generator=g).round()
        if "ignore_index" in s:
            t[torch.rand(t.shape, generator=g) < 0.2] = -1.0
        ref, ours = criterion(R, s, "cpu"), criterion(P, s, "cpu")
        assert not foreign_objects(ours), case
        xr, xo = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a, b = ref(xr, t), ours(xo, t)
        a.backward()
        b.backward()
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7) and torch.allclose(xr.grad, xo.grad, rtol=1e-5, atol=1e-8), case
