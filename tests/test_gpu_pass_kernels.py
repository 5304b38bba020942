"""-m gpu: the small bandwidth passes around the convolutions, each called through the C-ABI and held to its float64 restatement
(tests/pass_refs.py, pinned to torch by tests/test_pass_refs.py): the 3-D pool-merge on every argument arm, the 3-D children
passes of n -> 2n + 1 levels, BatchNorm finalize / backward in train and eval mode, bias, dropout multiply, and the activation /
post-norm passes on exact zeros.  Every comparison is |got - ref| <= K * 2^-24 * magnitude with K derived in pass_refs next to
each constant; outputs start as NaN, `+=` tables start non-zero.  The observed ratio err / (2^-24 * magnitude) of every case goes to
the parity diagnostics."""
import pytest
import torch

import gpu_utils as U
import pass_refs as R
from conftest import diag
from pytorch3dunet_amd import _native as nat
from pytorch3dunet_amd.engine import _p, _stream

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev(t):
    return None if t is None else t.contiguous().to(U.DEV)


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=U.DEV)


def check(kernel, got, ref, mag, K, **kw):
    r = R.ratio(got, ref, mag)
    diag(test="pass_kernels", kernel=kernel, K=K, ratio=r, **kw)
    assert r <= K, (kernel, kw, r, K)


def S():
    return _stream(U.DEV)


# ---- pool-merge, 3-D ------------------------------------------------------------------------------------------------------------
def _pool_fwd_on_device(t):
    N, D, H, W, C = t["N"], t["D"], t["H"], t["W"], t["C"]
    ed = dev(t["e"])
    pooled = nans(*t["pooled"].shape)
    am = torch.full(t["pooled"].shape, 255, dtype=torch.uint8, device=U.DEV)
    nat.call("u3d_maxpool2_fwd", 0, S(), _p(ed), N, D, H, W, C, _p(pooled), _p(am), None)
    assert torch.equal(pooled.cpu(), t["pooled"]) and torch.equal(am.cpu(), t["argmax"])  # first maximum on ties, as torch
    return ed, pooled, am


@pytest.mark.parametrize("c", R.pool_merge_cases(), ids=R.case_id)
def test_pool_merge_3d(c):
    t = R.pool_merge_inputs(c)
    N, D, H, W, C = t["N"], t["D"], t["H"], t["W"], t["C"]
    ed, pooled, am = _pool_fwd_on_device(t)
    dg, coef, sdg, scoef = dev(t["dg"]), dev(t["coef"]), dev(t["sdg"]), dev(t["scoef"])
    out = nans(N, D, H, W, C)
    pooled_arg = pooled if coef is not None else None
    if c["skip"] == "gn":
        nat.call("u3d_maxpool2_bwd_merge_gn", 0, S(), _p(dg), _p(pooled_arg), _p(am), _p(coef), _p(sdg), t["Cdg"], _p(scoef), t["Ctot"],
                 _p(ed), N, D, H, W, C, c["relu"], _p(out))
    else:
        e_arg = ed if c["relu"] else None  # (e is read only for the mask or the fused skip form)
        nat.call("u3d_maxpool2_bwd_merge", 0, S(), _p(dg), _p(pooled_arg), _p(am), _p(coef), _p(sdg), _p(e_arg), N, D, H, W, C, c["relu"],
                 _p(out))
    ref, mag = R.pool_merge_ref(t)
    check("u3d_maxpool2_bwd_merge" + ("_gn" if c["skip"] == "gn" else ""), out, ref, mag, R.K_POOL_MERGE, **c)


@pytest.mark.parametrize("missing", ["skip_dg", "skip_coef"])
def test_pool_merge_gn_refuses_null_skip_arguments(missing):
    c = dict(size=(4, 6, 2), skip="gn", ch="vec", coef=0, relu=1)
    t = R.pool_merge_inputs(c)
    N, D, H, W, C = t["N"], t["D"], t["H"], t["W"], t["C"]
    ed, pooled, am = _pool_fwd_on_device(t)
    dg, sdg, scoef = dev(t["dg"]), dev(t["sdg"]), dev(t["scoef"])
    out = nans(N, D, H, W, C)
    rc = nat.get_lib().u3d_maxpool2_bwd_merge_gn(0, S(), _p(dg), None, _p(am), None, None if missing == "skip_dg" else _p(sdg), t["Cdg"],
                                                 None if missing == "skip_coef" else _p(scoef), t["Ctot"], _p(ed), N, D, H, W, C, 1, _p(out))
    assert rc == nat.U3D_EINVAL and b"u3d_maxpool2_bwd_merge_gn" in nat.get_lib().u3d_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # nothing was launched


# ---- children passes, 3-D -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.children_stats_cases(), ids=R.case_id)
def test_chan_stats_children_3d(c):
    t = R.children_stats_inputs(c)
    N, (D1, H1, W1), C = 2, c["size"], c["C"]
    x, st = dev(t["x"]), dev(t["init"])
    nat.call("u3d_chan_stats_children", 0, S(), _p(x), N, D1, H1, W1, C, *c["e"], _p(st))
    ref, mag = R.chan_stats_children(t["x"], *c["e"])
    check("u3d_chan_stats_children", st.cpu() - t["init"], ref, mag, R.chan_stats_children_K(N, D1 * H1 * W1, C), **c)


def test_chan_stats_children_refuses_channels_not_a_multiple_of_4():
    x, st = torch.zeros((2, 2, 3, 5, 6), device=U.DEV), torch.ones((2, 6, 2), dtype=torch.float64, device=U.DEV)
    rc = nat.get_lib().u3d_chan_stats_children(0, S(), _p(x), 2, 2, 3, 5, 6, 1, 0, 1, _p(st))
    assert rc == nat.U3D_EINVAL
    torch.cuda.synchronize()
    assert bool((st == 1).all())


@pytest.mark.parametrize("c", R.children_apply_cases(), ids=R.case_id)
def test_gn_bwd_apply_children_3d(c):
    t = R.children_apply_inputs(c)
    N, (D1, H1, W1), C = 2, c["size"], t["C"]
    x, dlow, coef = dev(t["x"]), dev(t["dlow"]), dev(t["coef"])
    out = nans(N, D1, H1, W1, C)
    nat.call("u3d_gn_bwd_apply_children", 0, S(), _p(dlow), _p(x), _p(coef), t["Ctot"], t["coff"], N, D1, H1, W1, C, *c["e"], c["relu"], _p(out))
    ref, mag = R.gn_bwd_apply_children(t["dlow"], t["x"], t["coef"], t["coff"], *c["e"], c["relu"])
    check("u3d_gn_bwd_apply_children", out, ref, mag, R.K_APPLY_CHILDREN, **c)


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.bn_finalize_cases(), ids=R.case_id)
def test_bn_finalize(c):
    t = R.bn_finalize_inputs(c)
    N, C0, C1 = t["N"], t["C0"], t["C1"]
    C = C0 + C1
    st0, st1, gamma, beta, rm, rv = (dev(t[k]) for k in ("stats0", "stats1", "gamma", "beta", "rm", "rv"))
    if not t["train"]:
        st0 = st1 = None  # eval: the table comes from the running statistics alone
    aff, mr = nans(N, C, 2), nans(C, 2)
    nat.call("u3d_bn_finalize", 0, S(), _p(st0), C0, 1.0, _p(st1), C1, 8.0, N, t["count"], _p(gamma), _p(beta), t["eps"], t["train"],
             t["mom"], _p(rm), _p(rv), _p(aff), _p(mr))
    ref, mag = R.bn_finalize_ref(t)
    check("u3d_bn_finalize/affine", aff, ref["affine"], mag["affine"], R.K_F64_ROUNDED, **c)
    check("u3d_bn_finalize/mean_rstd", mr, ref["mean_rstd"], mag["mean_rstd"], R.K_F64_ROUNDED, **c)
    if t["train"] and c["run"]:
        check("u3d_bn_finalize/running_mean", rm, ref["running_mean"], mag["running_mean"], R.K_F64_ROUNDED, **c)
        check("u3d_bn_finalize/running_var", rv, ref["running_var"], mag["running_var"], R.K_F64_ROUNDED, **c)
    elif c["run"]:
        assert torch.equal(rm.cpu(), t["rm"]) and torch.equal(rv.cpu(), t["rv"])  # eval mode leaves the running statistics alone


@pytest.mark.parametrize("c", R.bn_bwd_cases(), ids=R.case_id)
def test_bn_bwd_finalize(c):
    t = R.bn_bwd_inputs(c)
    N, C = t["N"], t["C"]
    gst, mr, gamma = dev(t["gstats"]), dev(t["mean_rstd"]), dev(t["gamma"])
    dgam, dbet, coef = nans(C), nans(C), nans(N, 3, C)
    nat.call("u3d_bn_bwd_finalize", 0, S(), _p(gst), _p(mr), _p(gamma), N, C, t["count"], t["train"], _p(dgam), _p(dbet), _p(coef))
    ref, mag = R.bn_bwd_ref(t)
    check("u3d_bn_bwd_finalize/dgamma", dgam, ref["dgamma"], mag["dgamma"], R.K_F64_ROUNDED, **c)
    check("u3d_bn_bwd_finalize/dbeta", dbet, ref["dbeta"], mag["dbeta"], R.K_F64_ROUNDED, **c)
    check("u3d_bn_bwd_finalize/coef", coef, ref["coef"], mag["coef"], R.K_F64_ROUNDED, **c)  # (every row n)
    if not t["train"]:
        assert bool((coef[:, 1:].cpu() == 0).all())  # eval: q = r = 0
    # dx = p dg + q x + r from the kernel's table against autograd with the exact statistics
    k = coef.cpu().double()
    p, q, r = (k[:, i].view(N, 1, C) for i in range(3))
    mp, mq, mr_ = (mag["coef"][:, i].view(N, 1, C) for i in range(3))
    dg, x = t["dg"].double(), t["x"].double()
    dx, dgamma, dbeta = R.bn_bwd_autograd(t)
    check("u3d_bn_bwd_finalize/dx", p * dg + q * x + r, dx, mp * dg.abs() + mq * x.abs() + mr_, R.K_BN_DX, **c)


# ---- bias and dropout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", R.BIAS_CASES)
def test_bias_table_and_bias_grad(N, C):
    t = R.bias_inputs(N, C)
    bias, st = dev(t["bias"]), dev(t["stats"])
    aff, db = nans(N, C, 2), nans(C)
    nat.call("u3d_bias_table", 0, S(), _p(bias), N, C, _p(aff))
    assert torch.equal(aff.cpu().double(), R.bias_table(t["bias"], N))
    nat.call("u3d_bias_grad", 0, S(), _p(st), N, C, _p(db))
    ref, mag = R.bias_grad(t["stats"])
    check("u3d_bias_grad", db, ref, mag, R.K_F64_ROUNDED, N=N, C=C)


@pytest.mark.parametrize("n", R.MUL_SIZES)
def test_mul(n):
    a, b = R.mul_inputs(n)
    ref, mag = R.mul(a, b)
    ad, bd, out = dev(a), dev(b), nans(n)
    nat.call("u3d_mul", 0, S(), _p(ad), _p(bd), n, _p(out))
    check("u3d_mul", out, ref, mag, R.K_MUL, n=n)
    nat.call("u3d_mul", 0, S(), _p(ad), _p(bd), n, _p(ad))  # in place on a
    check("u3d_mul/in_place", ad, ref, mag, R.K_MUL, n=n)
    assert torch.equal(bd.cpu(), b)


# ---- activations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ACT_SIZES)
@pytest.mark.parametrize("mode,slope", R.ACT_MODES)
def test_act_fwd_and_bwd(mode, slope, n):
    x, g = R.act_inputs(n, mode)
    ref, mag = R.act_fwd(x, mode, slope)
    xd, out = dev(x), nans(n)
    nat.call("u3d_act_fwd", 0, S(), _p(xd), n, mode, slope, _p(out))
    check("u3d_act_fwd", out, ref, mag, R.K_ACT_FWD[mode], mode=mode, slope=slope, n=n)
    nat.call("u3d_act_fwd", 0, S(), _p(xd), n, mode, slope, _p(xd))  # in place
    assert torch.equal(xd, out)
    # the derivative through the OUTPUT (ELU: y + 1, what nn.ELU(inplace=True) leaves to its backward); y = the rounded reference
    y = ref.float()
    dref, dmag = R.act_bwd(g, y, mode, slope)
    yd, gd, dout = dev(y), dev(g), nans(n)
    nat.call("u3d_act_bwd", 0, S(), _p(gd), _p(yd), n, mode, slope, _p(dout))
    check("u3d_act_bwd", dout, dref, dmag, R.K_ACT_BWD[mode], mode=mode, slope=slope, n=n)
    nat.call("u3d_act_bwd", 0, S(), _p(gd), _p(yd), n, mode, slope, _p(gd))  # in place on g
    check("u3d_act_bwd/in_place", gd, dref, dmag, R.K_ACT_BWD[mode], mode=mode, slope=slope, n=n)


@pytest.mark.parametrize("c", R.affine_cases(), ids=R.case_id)
def test_affine_add_act_fwd(c):
    t = R.affine_inputs(c)
    N, V, C = c["shape"]
    z, aff, add = dev(t["z"]), dev(t["affine"]), dev(t["add"])
    out = nans(N, V, C)
    ref, mag = R.affine_add_act(t["z"], t["affine"], t["add"], c["mode"], c["slope"])
    K = R.affine_add_act_K(c["mode"], c["add"])
    if c["add"]:
        nat.call("u3d_affine_add_act_fwd", 0, S(), _p(z), _p(aff), _p(add), N, V, C, c["mode"], c["slope"], _p(out))
        check("u3d_affine_add_act_fwd", out, ref, mag, K, **c)
    else:
        nat.call("u3d_affine_add_act_fwd", 0, S(), _p(z), _p(aff), None, N, V, C, c["mode"], c["slope"], _p(out))
        check("u3d_affine_add_act_fwd/no_add", out, ref, mag, K, **c)
        out2 = nans(N, V, C)
        nat.call("u3d_affine_act_fwd", 0, S(), _p(z), _p(aff), N, V, C, c["mode"], c["slope"], _p(out2))
        check("u3d_affine_act_fwd", out2, ref, mag, K, **c)
        assert bool((out[:, 0, :] == 0).all())  # the pre-activation is exactly 0 there, and f(0) = 0 for every mode


@pytest.mark.parametrize("V", R.PAIR_V)
@pytest.mark.parametrize("C", R.PAIR_C)
def test_pair_stats(C, V):
    t = R.pair_stats_inputs(C, V)
    a, b, st = dev(t["a"]), dev(t["b"]), dev(t["init"])
    nat.call("u3d_pair_stats", 0, S(), _p(a), _p(b), 2, V, C, _p(st))
    ref, mag = R.pair_stats(t["a"], t["b"])
    check("u3d_pair_stats", st.cpu() - t["init"], ref, mag, R.pair_stats_K(V), C=C, V=V)
