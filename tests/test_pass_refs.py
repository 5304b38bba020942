"""CPU only.  (1) Every float64 restatement of tests/pass_refs.py against torch's own float64 operators and autograd.
(2) The inputs of every case of tests/test_gpu_pass_kernels.py can tell right from wrong: each deliberately wrong restatement
that changes a case's arithmetic lands OUTSIDE that case's tolerance on exactly the inputs the GPU test uses."""
import pytest
import torch
import torch.nn.functional as F

import pass_refs as R

PIN = 1e-11  # float64 against float64: relative to the largest magnitude


def close(a, b, tol=PIN):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def nc(t):  # channels-last -> channels-first, float64
    return t.double().permute(0, 4, 1, 2, 3).contiguous()


def cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


# ---- pins ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.POOL_SIZES + [(8, 12, 16)])
def test_pool_fwd_is_max_pool3d_with_first_max_indices(size):
    D, H, W = size
    e = torch.relu(torch.round(torch.randn(2, D, H, W, 5, generator=torch.Generator().manual_seed(3)) * 2) / 2 - 0.75)
    pooled, am = R.pool_fwd(e)
    ref, idx = F.max_pool3d(nc(e), 2, return_indices=True)
    assert torch.equal(nc(pooled), ref)
    z, y, x = idx // (H * W), (idx // W) % H, idx % W
    assert torch.equal(nc(am).long(), 4 * (z % 2) + 2 * (y % 2) + (x % 2))
    assert not torch.equal(R.pool_fwd(e, last=True)[1], am)


@pytest.mark.parametrize("c", R.pool_merge_cases(), ids=R.case_id)
def test_pool_merge_is_autograd_of_pool_groupnorm_and_concat_consumer(c):
    t = R.pool_merge_inputs(c)
    e = nc(t["e"])
    if c["relu"]:
        leaf = torch.where(e > 0, e, -torch.ones_like(e)).requires_grad_(True)
        ev = F.relu(leaf)
    else:
        leaf = ev = e.clone().requires_grad_(True)
    pooled = F.max_pool3d(ev, 2)
    coef = scoef = None
    if c["coef"]:
        loss = (F.group_norm(pooled, t["G1"], t["gamma1"].double(), None, R.f32_scalar(1e-5)) * nc(t["dg"])).sum()
        coef = R.gn_tables(t["pooled"], t["dg"], t["G1"], t["gamma1"], False)
    else:
        loss = (pooled * nc(t["dg"])).sum()
    if c["skip"] == "plain":
        loss = loss + (ev * nc(t["sdg"])).sum()
    elif c["skip"] == "gn":
        cat = torch.cat((ev, nc(t["other"])), 1)
        loss = loss + (F.group_norm(cat, t["G2"], t["gamma2"].double(), None, R.f32_scalar(1e-5)) * nc(t["sdg"])).sum()
        scoef = R.gn_tables(torch.cat((t["e"], t["other"]), -1), t["sdg"], t["G2"], t["gamma2"], False)
    loss.backward()
    ref, mag = R.pool_merge(t["dg"], t["pooled"], t["argmax"], coef, t["sdg"], scoef, t["e"], c["relu"])
    assert close(ref, cl(leaf.grad))
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    # the fp32-rounded tables the GPU case uses stay within rounding of the float64 ones
    ref32, _ = R.pool_merge_ref(t)
    assert close(ref32, ref, 1e-5)


@pytest.mark.parametrize("e", R.CHILD_SHIFTS)
@pytest.mark.parametrize("size", R.CHILD_SIZES)
def test_children_passes_are_sums_over_the_upsampled_image(size, e):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, *size, 8, generator=g)
    up = R.nearest_up(x.double(), *e)
    assert up.shape[1:4] == tuple(2 * n + s for n, s in zip(size, e))
    ref, mag = R.chan_stats_children(x, *e)
    assert close(ref, torch.stack((up.sum((1, 2, 3)), (up * up).sum((1, 2, 3))), -1))
    assert close(mag[..., 0], up.abs().sum((1, 2, 3)))
    # F.interpolate agrees on what the image is
    assert torch.equal(nc(up), F.interpolate(nc(x), size=up.shape[1:4], mode="nearest"))
    # apply: p dlow + sum over the children of (q x_up + r)
    dlow, coef = torch.randn(2, *size, 8, generator=g), torch.randn(2, 3, 16, generator=g)
    p, q, r = (coef[:, k, 4:12].double().view(2, 1, 1, 1, 8) for k in range(3))
    xv = x.double().clone().requires_grad_(True)
    (R.nearest_up(xv, *e) * (q * up + r)).sum().backward()
    for relu in (0, 1):
        out, mag = R.gn_bwd_apply_children(dlow, x, coef, 4, *e, relu)
        want = (p * dlow.double() + xv.grad) * ((x > 0) if relu else 1)
        assert close(out, want)
        assert bool((mag >= out.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("c", R.bn_finalize_cases(), ids=R.case_id)
def test_bn_finalize_is_batch_norm(c):
    t = R.bn_finalize_inputs(c)
    x = t["x0"].double()
    if t["C1"]:
        x = torch.cat((x, R.nearest_up(t["x1"].double(), 0, 0, 0)), -1)
    rm = t["rm"].double().clone() if t["rm"] is not None else None
    rv = t["rv"].double().clone() if t["rv"] is not None else None
    y = F.batch_norm(nc(x), rm, rv, t["gamma"].double(), t["beta"].double(), bool(t["train"]), R.f32_scalar(t["mom"]), R.f32_scalar(t["eps"]))
    out, mag = R.bn_finalize_ref(t)
    a, b = out["affine"][..., 0], out["affine"][..., 1]
    N, C = a.shape
    assert close(a.view(N, 1, 1, 1, C) * x + b.view(N, 1, 1, 1, C), cl(y), 1e-9)
    if t["train"] and rm is not None:
        assert close(out["running_mean"], rm) and close(out["running_var"], rv)
    else:
        assert "running_mean" not in out and "running_var" not in out
    if t["train"]:
        assert out["mean_rstd"][1, 1].item() == pytest.approx(R.f32_scalar(1e-5) ** -0.5, rel=1e-9)  # the constant channel: var = 0


@pytest.mark.parametrize("c", R.bn_bwd_cases(), ids=R.case_id)
def test_bn_bwd_finalize_is_autograd_of_batch_norm(c):
    t = R.bn_bwd_inputs(c)
    N, C = t["N"], t["C"]
    dx, dgamma, dbeta = R.bn_bwd_autograd(t)
    out, mag = R.bn_bwd_ref(t, exact=True)
    assert close(out["dgamma"], dgamma) and close(out["dbeta"], dbeta)
    p, q, r = (out["coef"][:, k].view(N, 1, C) for k in range(3))
    assert close(p * t["dg"].double() + q * t["x"].double() + r, dx, 1e-10)
    assert all(bool((mag[k] >= out[k].abs() * (1 - 1e-12)).all()) for k in out)


@pytest.mark.parametrize("mode,slope", R.ACT_MODES)
def test_activations_are_torch_on_signed_zeros(mode, slope):
    s = R.f32_scalar(slope)
    f = {0: lambda v: v * 1.0, 1: F.relu, 2: lambda v: F.leaky_relu(v, s), 3: F.elu}[mode]
    x, g = R.act_inputs(4099, mode)
    assert bool((x == 0).sum() >= 6) and bool(torch.signbit(x[x == 0]).any()) and not bool(torch.signbit(x[x == 0]).all())
    xv = x.double().requires_grad_(True)
    y = f(xv)
    y.backward(g.double())
    ref, _ = R.act_fwd(x, mode, slope)
    assert close(ref, y.detach())
    dref, dmag = R.act_bwd(g, y.detach(), mode, slope)
    assert close(dref, xv.grad)
    assert bool((dmag >= dref.abs() * (1 - 1e-12)).all())
    # affine + add form
    c = dict(shape=(2, 33, 24), add=1, mode=mode, slope=slope)
    t = R.affine_inputs(c)
    a, b = t["affine"][..., 0].double().view(2, 1, 24), t["affine"][..., 1].double().view(2, 1, 24)
    ref, mag = R.affine_add_act(t["z"], t["affine"], t["add"], mode, slope)
    assert close(ref, f(a * t["z"].double() + b + t["add"].double()))
    assert bool(((a * t["z"].double() + b)[:, 0, :] == 0).all())  # the exact zeros are there


def test_pair_stats_bias_and_mul_are_plain_sums():
    t = R.pair_stats_inputs(7, 3)
    ref, _ = R.pair_stats(t["a"], t["b"])
    assert close(ref[..., 1], torch.einsum("nvc,nvc->nc", t["a"].double(), t["b"].double()))
    b = R.bias_inputs(3, 300)
    assert torch.equal(R.bias_table(b["bias"], 3)[2, :, 1], b["bias"].double())
    assert close(R.bias_grad(b["stats"])[0], b["stats"][..., 0].sum(0))
    x, m = R.mul_inputs(257)
    assert torch.equal(R.mul(x, m)[0], x.double() * m.double())


def test_launch_geometry_formulas():
    # C = 48: 12 quads, 21 rows (252 live threads); C = 1024: one row; V = 1025: two splits of 513 -> 129 steps per thread
    assert R.chan_stats_children_K(2, 30, 48) == 2 + 21 + 2 and R.chan_stats_children_K(2, 168, 1024) == 16 + 1 + 2  # (11 blocks per sample)
    assert R.chan_stats_children_K(2, 168, 8) == 2 + 128 + 2  # Q = 2, rows = 128, one block per sample
    assert R.pair_stats_K(1025) == 129 + 2 and R.pair_stats_K(1) == 1 + 2 and R.pair_stats_K(5000) == 250 + 2


# ---- the cases reject wrong restatements -------------------------------------------------------------------------------------------
def _pairs(cases, wrongs):
    return [pytest.param(c, w, id=f"{R.case_id(c)}-{w}") for c in cases for w in wrongs(c)]


@pytest.mark.parametrize("c,w", _pairs(R.pool_merge_cases(), R.pool_merge_wrongs))
def test_pool_merge_cases_reject(c, w):
    t = R.pool_merge_inputs(c)
    ref, mag = R.pool_merge_ref(t)
    assert R.outside(R.pool_merge_ref(t, w)[0], ref, mag, R.K_POOL_MERGE)


@pytest.mark.parametrize("c,w", _pairs(R.children_stats_cases(), lambda c: R.children_wrongs(c, False)))
def test_children_stats_cases_reject(c, w):
    t = R.children_stats_inputs(c)
    ref, mag = R.chan_stats_children(t["x"], *c["e"])
    V = c["size"][0] * c["size"][1] * c["size"][2]
    assert R.outside(R.chan_stats_children(t["x"], *c["e"], w)[0], ref, mag, R.chan_stats_children_K(2, V, c["C"]))


@pytest.mark.parametrize("c,w", _pairs(R.children_apply_cases(), lambda c: R.children_wrongs(c, True)))
def test_children_apply_cases_reject(c, w):
    t = R.children_apply_inputs(c)
    ref, mag = R.gn_bwd_apply_children(t["dlow"], t["x"], t["coef"], t["coff"], *c["e"], c["relu"])
    assert R.outside(R.gn_bwd_apply_children(t["dlow"], t["x"], t["coef"], t["coff"], *c["e"], c["relu"], w)[0], ref, mag, R.K_APPLY_CHILDREN)


def _any_outside(wrong, ref, mag, K):
    return any(R.outside(wrong[k], ref[k], mag[k], K) for k in ref)


@pytest.mark.parametrize("c,w", _pairs(R.bn_finalize_cases(), R.bn_finalize_wrongs))
def test_bn_finalize_cases_reject(c, w):
    t = R.bn_finalize_inputs(c)
    ref, mag = R.bn_finalize_ref(t)
    assert _any_outside(R.bn_finalize_ref(t, w)[0], ref, mag, R.K_F64_ROUNDED)


@pytest.mark.parametrize("c,w", _pairs(R.bn_bwd_cases(), R.bn_bwd_wrongs))
def test_bn_bwd_cases_reject(c, w):
    t = R.bn_bwd_inputs(c)
    ref, mag = R.bn_bwd_ref(t)
    assert _any_outside(R.bn_bwd_ref(t, w)[0], ref, mag, R.K_F64_ROUNDED)


@pytest.mark.parametrize("n", R.ACT_SIZES)
@pytest.mark.parametrize("mode,slope", R.ACT_MODES)
def test_activation_cases_reject(mode, slope, n):
    x, g = R.act_inputs(n, mode)
    ref, mag = R.act_fwd(x, mode, slope)
    y = ref.float()
    dref, dmag = R.act_bwd(g, y, mode, slope)
    for w in R.act_wrongs(mode, slope, True):
        if w == "slope_swapped" and n > 1:  # (n = 1 is the single value 0.0: no slope in f(0))
            assert R.outside(R.act_fwd(x, mode, slope, w)[0], ref, mag, R.K_ACT_FWD[mode])
        assert R.outside(R.act_bwd(g, y, mode, slope, w)[0], dref, dmag, R.K_ACT_BWD[mode])


@pytest.mark.parametrize("c,w", _pairs(R.affine_cases(), R.affine_wrongs))
def test_affine_cases_reject(c, w):
    t = R.affine_inputs(c)
    ref, mag = R.affine_add_act(t["z"], t["affine"], t["add"], c["mode"], c["slope"])
    assert R.outside(R.affine_add_act(t["z"], t["affine"], t["add"], c["mode"], c["slope"], w)[0], ref, mag,
                     R.affine_add_act_K(c["mode"], c["add"]))


@pytest.mark.parametrize("V", R.PAIR_V)
@pytest.mark.parametrize("C", R.PAIR_C)
def test_pair_stats_cases_reject(C, V):
    t = R.pair_stats_inputs(C, V)
    ref, mag = R.pair_stats(t["a"], t["b"])
    assert R.outside(R.pair_stats(t["a"], t["b"], "drop_last")[0], ref, mag, R.pair_stats_K(V))


def test_every_listed_wrong_variant_is_exercised_by_some_case():
    used = set()
    for cases, wrongs in ((R.pool_merge_cases(), R.pool_merge_wrongs), (R.children_stats_cases(), lambda c: R.children_wrongs(c, False)),
                          (R.children_apply_cases(), lambda c: R.children_wrongs(c, True)), (R.bn_finalize_cases(), R.bn_finalize_wrongs),
                          (R.bn_bwd_cases(), R.bn_bwd_wrongs), (R.affine_cases(), R.affine_wrongs)):
        for c in cases:
            used.update(wrongs(c))
    for mode, slope in R.ACT_MODES:
        used.update(R.act_wrongs(mode, slope, True))
    assert used >= {"two_children", "ez_dropped", "biased", "count_only", "scale1_ignored", "last_max", "mask_before_add",
                    "coff_ignored", "slope_swapped", "df_one_at_zero", "eval_not_zeroed", "coef_row0"}
