"""Plain float64 restatements of the small bandwidth passes around the convolutions (3-D pool-merge, the children passes of
n -> 2n + 1 decoder levels, BatchNorm / bias / dropout, the activation passes of csrc/u3d_act.hip), the inputs of every case
tests/test_gpu_pass_kernels.py runs, and the tolerances those cases are held to.  torch on the CPU only; nothing of the native
library is imported here.  tests/test_pass_refs.py pins every restatement to torch's own float64 operators and shows that each
case's inputs reject a deliberately wrong restatement (the `wrong=` arguments below).

Conventions: tensors are channels-last as the kernels see them ((N, D, H, W, C) / (N, V, C)); every restatement takes the fp32
inputs the kernel gets, upcasts them and returns (expected, magnitude) in float64, `magnitude` being the sum of the absolute
values of the terms that are added to form each output element.  Every comparison is |got - ref| <= K * 2^-24 * magnitude
(so an element whose magnitude is 0 — masked, or a border voxel nothing is scattered to — must be an exact zero).

K of an elementwise pass = the number of fp32 roundings on the longest path from an input term to the output in the kernel as
written (a sum's error is at most depth * 2^-24 * sum |terms|, depth = roundings a term passes through), plus 2.  Contraction
to FMAs only removes roundings.  K of a statistics pass = the longest per-thread fp32 chain of the launch geometry plus the
cross-row adds (functions *_K below repeat the launchers' formulas).  The double-precision finalize kernels round once: K = 2."""
import math

import torch

U32 = 2.0 ** -24
F64 = torch.float64


def f32_scalar(v):
    """the value a C `float` argument carries"""
    return torch.tensor(float(v), dtype=torch.float32).double().item()


def ratio(got, ref, mag):
    """max |got - ref| / (2^-24 * magnitude); inf for a non-finite result or a non-zero where the magnitude is 0"""
    got = got.detach().cpu().double().reshape(ref.shape)
    if not torch.isfinite(got).all():
        return math.inf
    err = (got - ref).abs()
    z = mag == 0
    if bool((err[z] != 0).any()):
        return math.inf
    return (err[~z] / (U32 * mag[~z])).max().item() if bool((~z).any()) else 0.0


def outside(wrong, ref, mag, K):
    """a wrong restatement is REJECTED by a case if some element leaves the case's tolerance"""
    return bool(((wrong - ref).abs() > K * U32 * mag).any())


def _gen(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ---- GroupNorm backward tables (u3d_gn_bwd_finalize, csrc/u3d_gn.h) --------------------------------------------------------
def gn_mean_rstd(x, G, eps=1e-5):
    """x (N, ..., C) float64 -> (N, G, 2) = (mean, rstd) of nn.GroupNorm(G, C, eps)"""
    N, C = x.shape[0], x.shape[-1]
    xg = x.reshape(N, -1, G, C // G)
    return torch.stack((xg.mean(dim=(1, 3)), (xg.var(dim=(1, 3), unbiased=False) + f32_scalar(eps)).rsqrt()), -1)


def gn_bwd_finalize(gstats, mean_rstd, gamma, count):
    """gstats (N, C, 2) = (sum dy, sum dy * x), mean_rstd (N, G, 2), gamma (C) -> dgamma, dbeta, coef (N, 3, C) = (p, q, r)
    of dx = p * dy + q * x + r"""
    N, C, _ = gstats.shape
    G = mean_rstd.shape[1]
    cpg = C // G
    S1, S2 = gstats[..., 0], gstats[..., 1]
    mean, rstd = mean_rstd[..., 0], mean_rstd[..., 1]
    mean_c, rstd_c = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    m = count * cpg
    A = (gamma * S1).view(N, G, cpg).sum(2)
    B = (gamma * rstd_c * (S2 - mean_c * S1)).view(N, G, cpg).sum(2)
    q = -rstd * rstd * B / m
    r = -rstd * A / m + rstd * rstd * mean * B / m
    coef = torch.stack((rstd_c * gamma, q.repeat_interleave(cpg, 1), r.repeat_interleave(cpg, 1)), 1)
    return (rstd_c * (S2 - mean_c * S1)).sum(0), S1.sum(0), coef


def gn_tables(x, dy, G, gamma, round32):
    """coefficient table of GroupNorm(x)'s backward for the output gradient dy (x, dy channels-last).  round32: mean / rstd and the
    table rounded to fp32, as the kernels store them."""
    x, dy, gamma = x.double(), dy.double(), gamma.double()
    N, C = x.shape[0], x.shape[-1]
    mr = gn_mean_rstd(x, G)
    if round32:
        mr = mr.float().double()
    gst = torch.stack((dy.reshape(N, -1, C).sum(1), (dy * x).reshape(N, -1, C).sum(1)), -1)
    coef = gn_bwd_finalize(gst, mr, gamma, float(x[0, ..., 0].numel()))[2]
    return coef.float() if round32 else coef


# ---- MaxPool3d(2) + pool-merge ------------------------------------------------------------------------------------------------
def pool_fwd(e, last=False):
    """e (N, D, H, W, C) -> pooled (N, D/2, H/2, W/2, C), argmax byte k = 4 dz + 2 dy + dx: FIRST maximum in z, y, x scan order
    (last=True: the wrong rule, last maximum on ties)"""
    D2, H2, W2 = e.shape[1] // 2, e.shape[2] // 2, e.shape[3] // 2
    best = bi = None
    for k in range(8):
        cand = e[:, (k >> 2):2 * D2:2, ((k >> 1) & 1):2 * H2:2, (k & 1):2 * W2:2, :]
        if best is None:
            best, bi = cand.clone(), torch.zeros(cand.shape, dtype=torch.uint8)
        else:
            upd = (cand >= best) if last else (cand > best)
            best = torch.where(upd, cand, best)
            bi = torch.where(upd, torch.full_like(bi, k), bi)
    return best, bi


def _scatter(dp, argmax, shape):
    out = torch.zeros(shape, dtype=F64)
    D2, H2, W2 = dp.shape[1:4]
    for k in range(8):
        out[:, (k >> 2):2 * D2:2, ((k >> 1) & 1):2 * H2:2, (k & 1):2 * W2:2, :] += dp * (argmax == k)
    return out


def _rows(coef, C, coff=0, row0=False):
    c = coef.double()
    if row0:
        c = c[0:1].expand_as(c)
    return (c[:, k, coff:coff + C].reshape(c.shape[0], 1, 1, 1, C) for k in range(3))


# dp = p*dg (1) + q*pooled (2) + r (3); skip = ps*sdg (1) + qs*e (2) + rs (3); g = skip + dp (4): longest path 4 roundings
K_POOL_MERGE = 4 + 2


def pool_merge(dg, pooled, argmax, coef, sdg, scoef, e, relu_mask, wrong=None):
    """dz_e = (skip + scatter(dpool)) * [e > 0 if relu_mask]; dpool = p dg + q pooled + r (coef None: dg); skip = 0 (sdg None) |
    sdg[..., :C] (scoef None) | ps sdg[..., :C] + qs e + rs.  wrong: last_max | mask_before_add | coef_row0"""
    e = e.double()
    C = e.shape[-1]
    row0 = wrong == "coef_row0"
    if wrong == "last_max":
        argmax = pool_fwd(e, last=True)[1]
    dp, mdp = dg.double(), dg.double().abs()
    if coef is not None:
        p, q, r = _rows(coef, C, 0, row0)
        dp, mdp = p * dg.double() + q * pooled.double() + r, (p * dg.double()).abs() + (q * pooled.double()).abs() + r.abs()
    skip = mskip = torch.zeros_like(e)
    if sdg is not None:
        s = sdg.double()[..., :C]
        skip, mskip = s, s.abs()
        if scoef is not None:
            ps, qs, rs = _rows(scoef, C, 0, row0)
            skip, mskip = ps * s + qs * e + rs, (ps * s).abs() + (qs * e).abs() + rs.abs()
    sc, msc = _scatter(dp, argmax, e.shape), _scatter(mdp, argmax, e.shape)
    keep = (e > 0).double() if relu_mask else torch.ones_like(e)
    if wrong == "mask_before_add":
        return skip * keep + sc, mskip * keep + msc
    return (skip + sc) * keep, (mskip + msc) * keep


POOL_SIZES = [(9, 13, 11), (4, 6, 2)]
# (C, Cdg of the fused skip form, groups of the pooled tensor's GroupNorm, groups of the consumer's GroupNorm over Cdg channels —
# chosen so that one group spans skip and other channels)
POOL_CHANNELS = {"vec": (8, 24, 2, 2), "scalar": (5, 9, 1, 3), "scalar_cdg": (8, 10, 2, 2)}


def pool_merge_cases():
    out = []
    for size in POOL_SIZES:
        for skip in ("none", "plain", "gn"):
            for ch in (("vec", "scalar", "scalar_cdg") if skip == "gn" else ("vec", "scalar")):  # (Cdg only exists in the fused form)
                for coef in (0, 1):
                    for relu in (0, 1):
                        out.append(dict(size=size, skip=skip, ch=ch, coef=coef, relu=relu))
    return out


def case_id(c):
    return "-".join(f"{k}{'x'.join(map(str, v)) if isinstance(v, (tuple, list)) else v}" for k, v in c.items())


def pool_merge_inputs(c, N=2):
    """e is post-ReLU on a half-integer lattice: windows that are all zero AND windows with tied positive maxima both occur"""
    D, H, W = c["size"]
    C, Cdg, G1, G2 = POOL_CHANNELS[c["ch"]]
    g = _gen(D, H, W, C, Cdg, c["coef"], c["relu"], len(c["skip"]))
    e = torch.relu(torch.round(torch.randn(N, D, H, W, C, generator=g) * 2) / 2 - 0.75)
    pooled, argmax = pool_fwd(e)
    t = dict(N=N, D=D, H=H, W=W, C=C, Cdg=C, Ctot=0, G1=G1, G2=G2, e=e, pooled=pooled, argmax=argmax, coef=None, sdg=None, scoef=None,
             relu=c["relu"])
    t["dg"] = torch.randn(pooled.shape, generator=g)
    t["gamma1"] = torch.randn(C, generator=g)
    if c["coef"]:
        t["coef"] = gn_tables(pooled, t["dg"], G1, t["gamma1"], True)
    if c["skip"] == "plain":
        t["sdg"] = torch.randn(N, D, H, W, C, generator=g)
    elif c["skip"] == "gn":
        t["Cdg"] = t["Ctot"] = Cdg
        t["sdg"] = torch.randn(N, D, H, W, Cdg, generator=g)
        t["other"] = torch.randn(N, D, H, W, Cdg - C, generator=g)
        t["gamma2"] = torch.randn(Cdg, generator=g)
        t["scoef"] = gn_tables(torch.cat((e, t["other"]), -1), t["sdg"], G2, t["gamma2"], True)
    return t


def pool_merge_ref(t, wrong=None):
    return pool_merge(t["dg"], t["pooled"], t["argmax"], t["coef"], t["sdg"], t["scoef"], t["e"], t["relu"], wrong)


def pool_merge_wrongs(c):
    w = ["last_max"]
    if c["relu"]:
        w.append("mask_before_add")
    if c["coef"] or c["skip"] == "gn":
        w.append("coef_row0")
    return w


# ---- children passes of n -> 2n + 1 levels -------------------------------------------------------------------------------------
def children_weights(D1, H1, W1, ez, ey, ex, wrong=None):
    """(D1, H1, W1) children of a low-res voxel = (2 + [ez && z == 0]) (2 + [ey && y == 0]) (2 + [ex && x == 0]).
    wrong: two_children (2 at cell 0 of the last shifted axis) | ez_dropped"""
    e = [ez and wrong != "ez_dropped", ey, ex]
    if wrong == "two_children":
        e[max(i for i in range(3) if e[i])] = 0
    ax = []
    for n, s in zip((D1, H1, W1), e):
        w = torch.full((n,), 2.0, dtype=F64)
        if s:
            w[0] = 3.0
        ax.append(w)
    return ax[0].view(-1, 1, 1) * ax[1].view(1, -1, 1) * ax[2].view(1, 1, -1)


def nearest_up(x, ez, ey, ex):
    """the materialised F.interpolate(mode='nearest') image n -> 2n + e per axis of x (N, D1, H1, W1, C): src = (dst - e) >> 1 clamped"""
    for dim, s in zip((1, 2, 3), (ez, ey, ex)):
        n = x.shape[dim]
        idx = torch.arange(n).repeat_interleave(2)
        if s:
            idx = torch.cat((torch.zeros(1, dtype=idx.dtype), idx))
        x = x.index_select(dim, idx)
    return x


def chan_stats_children(x, ez, ey, ex, wrong=None):
    """the INCREMENT of stats (N, C, 2): (sum w x, sum w x^2) over the low-res grid.  wrong: two_children | ez_dropped | drop_last"""
    x = x.double()
    w = children_weights(*x.shape[1:4], ez, ey, ex, wrong).unsqueeze(-1).expand(x.shape[1:4] + (1,)).clone()
    if wrong == "drop_last":
        w[-1, -1, -1] = 0.0
    return (torch.stack(((w * x).sum((1, 2, 3)), (w * x * x).sum((1, 2, 3))), -1),
            torch.stack(((w * x.abs()).sum((1, 2, 3)), (w * x * x).sum((1, 2, 3))), -1))


def chan_stats_children_K(N, V, C):
    """launcher of csrc/u3d_ops.hip: Q = C / 4 threads per voxel row, rows = 256 / Q, bpn blocks per sample; a thread adds
    ceil(per / rows) products w * (x * x) (2 roundings), then `rows` partials are added in fp32, then float64"""
    Q = C // 4
    rows = 256 // Q
    bpn = max(1, min(-(-V // (rows * 16)), -(-1024 // N)))
    per = -(-V // bpn)
    return -(-per // rows) + rows + 2


# q*x (1) + r (2), * cnt (3), + p*dlow (4): longest path 4 roundings
K_APPLY_CHILDREN = 4 + 2


def gn_bwd_apply_children(dlow, x, coef, coff, ez, ey, ex, relu_mask, wrong=None):
    """out = (p dlow + children (q x + r)) * [x > 0 if relu_mask], (p, q, r) = coef[n][0..2][coff + c].
    wrong: two_children | ez_dropped | coff_ignored | coef_row0"""
    x, dlow = x.double(), dlow.double()
    C = x.shape[-1]
    p, q, r = _rows(coef, C, 0 if wrong == "coff_ignored" else coff, wrong == "coef_row0")
    cnt = children_weights(*x.shape[1:4], ez, ey, ex, wrong).unsqueeze(-1)
    keep = (x > 0).double() if relu_mask else torch.ones_like(x)
    return (p * dlow + cnt * (q * x + r)) * keep, ((p * dlow).abs() + cnt * ((q * x).abs() + r.abs())) * keep


CHILD_SHIFTS = [(0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1)]
CHILD_SIZES = [(2, 3, 5), (4, 6, 7)]
CHILD_STATS_C = [8, 20, 48, 256, 1024]


def children_stats_cases():
    return [dict(size=s, e=e, C=C) for s in CHILD_SIZES for e in CHILD_SHIFTS for C in CHILD_STATS_C]


def children_stats_inputs(c, N=2):
    g = _gen(*c["size"], *c["e"], c["C"])
    return dict(x=torch.randn(N, *c["size"], c["C"], generator=g), init=torch.randn(N, c["C"], 2, generator=g, dtype=F64))


def children_apply_cases():
    return [dict(size=s, e=e, relu=m) for s in CHILD_SIZES for e in CHILD_SHIFTS for m in (0, 1)]


def children_apply_inputs(c, N=2, C=8, Ctot=16):
    g = _gen(*c["size"], *c["e"], c["relu"], 99)
    return dict(x=torch.randn(N, *c["size"], C, generator=g), dlow=torch.randn(N, *c["size"], C, generator=g),
                coef=torch.randn(N, 3, Ctot, generator=g), coff=4, Ctot=Ctot, C=C)


def children_wrongs(c, apply):
    w = ["coff_ignored", "coef_row0"] if apply else ["drop_last"]
    if any(c["e"]):
        w.append("two_children")
    if c["e"][0]:
        w.append("ez_dropped")
    return w


# ---- BatchNorm / bias / dropout (csrc/u3d_norm.hip: double arithmetic, one rounding) --------------------------------------------
K_F64_ROUNDED = 2


def bn_finalize(stats0, sc0, stats1, sc1, N, count, gamma, beta, eps, training, momentum, running_mean, running_var, wrong=None):
    """-> (out, mag) dicts with affine (N, C, 2), mean_rstd (C, 2) and, when training with running buffers, running_mean / running_var
    after the call.  wrong: biased | count_only | scale1_ignored"""
    gamma, beta, eps, mom = gamma.double(), beta.double(), f32_scalar(eps), f32_scalar(momentum)
    out, mag = {}, {}
    if training:
        s = sc0 * stats0.sum(0)
        if stats1 is not None:
            s = torch.cat((s, (1.0 if wrong == "scale1_ignored" else sc1) * stats1.sum(0)), 0)
        m = count if wrong == "count_only" else count * N
        mean = s[:, 0] / m
        var = (s[:, 1] / m - mean * mean).clamp_min(0.0)
        rstd = (var + eps).rsqrt()
        if running_mean is not None and running_var is not None:
            unb = var if (wrong == "biased" or m <= 1.0) else var * m / (m - 1.0)
            out["running_mean"] = (1.0 - mom) * running_mean.double() + mom * mean
            mag["running_mean"] = (1.0 - mom) * running_mean.double().abs() + mom * mean.abs()
            out["running_var"] = (1.0 - mom) * running_var.double() + mom * unb
            mag["running_var"] = (1.0 - mom) * running_var.double().abs() + mom * unb.abs()
    else:
        mean, rstd = running_mean.double(), (running_var.double() + eps).rsqrt()
    a = rstd * gamma
    out["mean_rstd"], mag["mean_rstd"] = torch.stack((mean, rstd), -1), torch.stack((mean.abs(), rstd), -1)
    out["affine"] = torch.stack((a, beta - mean * a), -1).unsqueeze(0).expand(N, -1, -1).contiguous()
    mag["affine"] = torch.stack((a.abs(), beta.abs() + (mean * a).abs()), -1).unsqueeze(0).expand(N, -1, -1).contiguous()
    return out, mag


def bn_bwd_finalize(gstats, mean_rstd, gamma, N, count, training, wrong=None):
    """gstats (N, C, 2), mean_rstd (C, 2) -> (out, mag) with dgamma, dbeta, coef (N, 3, C).  wrong: eval_not_zeroed | count_only"""
    S1, S2 = gstats[..., 0].sum(0), gstats[..., 1].sum(0)
    mean, rstd, gamma = mean_rstd[:, 0].double(), mean_rstd[:, 1].double(), gamma.double()
    m = count if wrong == "count_only" else count * N
    p = rstd * gamma
    q, r, mq, mr = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    if training or wrong == "eval_not_zeroed":
        k = rstd * (S2 - mean * S1) / m
        q, r = -p * k * rstd, -p * S1 / m + p * k * rstd * mean
        mk = rstd * (S2.abs() + (mean * S1).abs()) / m
        mq, mr = (p * rstd).abs() * mk, (p * S1 / m).abs() + (p * rstd * mean).abs() * mk
    ex = lambda t: torch.stack(t, 0).unsqueeze(0).expand(N, -1, -1).contiguous()  # noqa: E731
    out = dict(dgamma=rstd * (S2 - mean * S1), dbeta=S1, coef=ex((p, q, r)))
    mag = dict(dgamma=rstd * (S2.abs() + (mean * S1).abs()), dbeta=gstats[..., 0].abs().sum(0), coef=ex((p.abs(), mq, mr)))
    return out, mag


# dx from the kernel's fp32 table against autograd with the exact statistics: mean / rstd reach the kernel rounded to fp32 (1 each) and
# q ~ rstd^3 (3) * (S2 - mean S1) (1), r's second term carries mean once more (1); + the table's own rounding (1): 6, plus 2
K_BN_DX = 6 + 2

BN_CHANNELS = [(5, 0), (300, 0), (6, 7), (250, 20)]
BN_SIZE, BN_LOW = (4, 6, 2), (2, 3, 1)  # (the upper channel range is an exact 2x upsampling: scale1 = 8)


def bn_finalize_cases():
    tr = [dict(train=1, N=N, ch=ch, mom=mom, run=run) for N in (1, 3) for ch in BN_CHANNELS for mom in (0.1, 0.3) for run in (1, 0)]
    return tr + [dict(train=0, N=3, ch=ch, mom=0.1, run=1) for ch in ((300, 0), (6, 7))]


def bn_finalize_inputs(c):
    N, (C0, C1) = c["N"], c["ch"]
    g = _gen(N, C0, C1, int(c["mom"] * 10), c["run"], c["train"])
    x0 = torch.randn(N, *BN_SIZE, C0, generator=g) * 0.7 + 0.3 * torch.randn(C0, generator=g)
    x0[..., 1] = 0.75  # a constant channel: the variance clamps to 0
    x1 = torch.randn(N, *BN_LOW, C1, generator=g) * 0.7 + 0.3 * torch.randn(C1, generator=g) if C1 else None
    C = C0 + C1
    st = lambda t: torch.stack((t.double().reshape(N, -1, t.shape[-1]).sum(1), (t.double() ** 2).reshape(N, -1, t.shape[-1]).sum(1)), -1)  # noqa: E731
    t = dict(N=N, C0=C0, C1=C1, x0=x0, x1=x1, stats0=st(x0), stats1=st(x1) if C1 else None, count=float(x0[0, ..., 0].numel()),
             gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g), eps=1e-5, train=c["train"], mom=c["mom"],
             rm=None, rv=None)
    if c["run"]:
        t["rm"], t["rv"] = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    return t


def bn_finalize_ref(t, wrong=None):
    return bn_finalize(t["stats0"], 1.0, t["stats1"], 8.0, t["N"], t["count"], t["gamma"], t["beta"], t["eps"], t["train"], t["mom"],
                       t["rm"], t["rv"], wrong)


def bn_finalize_wrongs(c):
    w = []
    if c["train"]:
        if c["run"]:
            w.append("biased")
        if c["N"] > 1:
            w.append("count_only")
        if c["ch"][1]:
            w.append("scale1_ignored")
    return w


def bn_bwd_cases():
    return [dict(train=tr, N=N, C=C) for tr in (1, 0) for N in (1, 3) for C in (5, 300)]


def bn_bwd_inputs(c):
    N, C = c["N"], c["C"]
    g = _gen(N, C, c["train"], 5)
    x = torch.randn(N, 48, C, generator=g) * 0.7 + 0.3 * torch.randn(C, generator=g)
    dg = torch.randn(N, 48, C, generator=g)
    gamma = torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    xd = x.double().reshape(-1, C)
    eps = f32_scalar(1e-5)
    mr64 = (torch.stack((xd.mean(0), (xd.var(0, unbiased=False) + eps).rsqrt()), -1) if c["train"]
            else torch.stack((rm.double(), (rv.double() + eps).rsqrt()), -1))
    gst = torch.stack((dg.double().sum(1), (dg.double() * x.double()).sum(1)), -1)
    return dict(N=N, C=C, x=x, dg=dg, gamma=gamma, rm=rm, rv=rv, mr64=mr64, mean_rstd=mr64.float(), gstats=gst, count=48.0,
                train=c["train"])


def bn_bwd_ref(t, wrong=None, exact=False):
    return bn_bwd_finalize(t["gstats"], t["mr64"] if exact else t["mean_rstd"], t["gamma"], t["N"], t["count"], t["train"], wrong)


def bn_bwd_autograd(t):
    """(dx (N, V, C), dgamma, dbeta) of F.batch_norm in float64 with the exact statistics"""
    import torch.nn.functional as F

    x = t["x"].double().permute(0, 2, 1).contiguous().requires_grad_(True)  # (N, C, V)
    ga = t["gamma"].double().requires_grad_(True)
    be = torch.zeros(t["C"], dtype=F64, requires_grad=True)
    y = F.batch_norm(x, t["rm"].double().clone(), t["rv"].double().clone(), ga, be, bool(t["train"]), 0.1, f32_scalar(1e-5))
    y.backward(t["dg"].double().permute(0, 2, 1))
    return x.grad.permute(0, 2, 1).contiguous(), ga.grad, be.grad


def bn_bwd_wrongs(c):
    return (["count_only"] if c["N"] > 1 else []) if c["train"] else ["eval_not_zeroed"]


def bias_table(bias, N):
    return torch.stack((torch.ones_like(bias), bias), -1).double().unsqueeze(0).expand(N, -1, -1).contiguous()


def bias_grad(stats):
    return stats[..., 0].sum(0), stats[..., 0].abs().sum(0)


BIAS_CASES = [(3, 300), (1, 1)]


def bias_inputs(N, C):
    g = _gen(N, C, 3)
    return dict(bias=torch.randn(C, generator=g), stats=torch.randn(N, C, 2, generator=g, dtype=F64))


K_MUL = 1 + 2  # one product
MUL_SIZES = [1, 255, 257, 4099]


def mul_inputs(n):
    g = _gen(n, 11)
    return torch.randn(n, generator=g), (torch.rand(n, generator=g) > 0.3).float() / 0.7  # (a dropout mask, scaled)


def mul(a, b):
    return a.double() * b.double(), (a.double() * b.double()).abs()


# ---- activations (csrc/u3d_act.hip): 0 none, 1 ReLU, 2 LeakyReLU(slope), 3 ELU ---------------------------------------------------
ACT_MODES = [(0, 0.0), (1, 0.0), (2, 0.01), (2, 0.1), (3, 0.0)]
# roundings of f itself: none / ReLU select; LeakyReLU one product; ELU expm1f, documented at <= 1 ulp = 2 half-ulp roundings
ACT_ROUNDINGS = {0: 0, 1: 0, 2: 1, 3: 2}
K_ACT_FWD = {m: r + 2 for m, r in ACT_ROUNDINGS.items()}
# g * f'(y): one product, ELU one more for y + 1
K_ACT_BWD = {0: 1 + 2, 1: 1 + 2, 2: 1 + 2, 3: 2 + 2}


def _slope(slope, wrong):
    s = f32_scalar(slope)
    if wrong == "slope_swapped":
        s = f32_scalar({0.01: 0.1, 0.1: 0.01}[slope])
    return s


def act_f(x, mode, slope):
    if mode == 1:
        return x.clamp_min(0.0)
    if mode == 2:
        return torch.where(x > 0, x, slope * x)
    if mode == 3:
        return torch.where(x > 0, x, torch.expm1(x))
    return x.clone()


def act_fwd(x, mode, slope, wrong=None):
    y = act_f(x.double(), mode, _slope(slope, wrong))
    return y, y.abs()


def act_bwd(gr, y, mode, slope, wrong=None):
    """out = g * f'(.) through the OUTPUT y: 1 for y > 0, else 0 / slope / y + 1.  wrong: df_one_at_zero | slope_swapped"""
    gr, y = gr.double(), y.double()
    one = torch.ones_like(y)
    low, mlow = {0: (one, one), 1: (0 * one, 0 * one), 2: (_slope(slope, wrong) * one,) * 2, 3: (y + 1.0, y.abs() + 1.0)}[mode]
    pos = (y >= 0) if wrong == "df_one_at_zero" else (y > 0)
    return gr * torch.where(pos, one, low), gr.abs() * torch.where(pos, one, mlow)


def act_wrongs(mode, slope, bwd):
    w = ["slope_swapped"] if mode == 2 else []
    if bwd and mode in (1, 2):  # (ELU: y + 1 = 1 at y == 0, the conventions agree)
        w.append("df_one_at_zero")
    return w


ACT_SIZES = [1, 4099]
ACT_SPECIALS = [0.0, -0.0, 1e-30, -1e-30, -20.0, -100.0, 100.0]


def act_inputs(n, mode):
    g = _gen(n, mode, 21)
    x = torch.randn(n, generator=g)
    if n >= 3 * len(ACT_SPECIALS):
        x[torch.randperm(n, generator=g)[:3 * len(ACT_SPECIALS)]] = torch.tensor(ACT_SPECIALS * 3)
    else:
        x[0] = 0.0
    return x, torch.randn(n, generator=g)


def affine_add_act_K(mode, add):
    return 1 + (1 if add else 0) + ACT_ROUNDINGS[mode] + 2  # fmaf (1) [+ add (1)] + f


def affine_add_act(z, affine, add, mode, slope, wrong=None):
    """out = f(a z + b [+ add]).  The error of the pre-activation v (pre + 1 roundings' worth of sum |terms|) passes through f with at
    most sup |f'| over the interval it can lie in; f's own roundings scale with |f(v)|.  wrong: slope_swapped | coef_row0"""
    z = z.double()
    N, V, C = z.shape
    ab = affine.double()
    if wrong == "coef_row0":
        ab = ab[0:1].expand_as(ab)
    a, b = ab[..., 0].view(N, 1, C), ab[..., 1].view(N, 1, C)
    v, mpre, pre = a * z + b, (a * z).abs() + b.abs(), 1
    if add is not None:
        v, mpre, pre = v + add.double(), mpre + add.double().abs(), 2
    s = _slope(slope, wrong)
    hi = v + (pre + 1) * U32 * mpre
    one = torch.ones_like(v)
    sup = {0: one, 1: (hi > 0).double(), 2: torch.where(hi > 0, one, s * one), 3: torch.where(hi > 0, one, torch.exp(hi))}[mode]
    y = act_f(v, mode, s)
    K = affine_add_act_K(mode, add is not None)
    return y, ((pre + 1) * mpre * sup + (ACT_ROUNDINGS[mode] + 1) * y.abs()) / K


AFFINE_SHAPES = [(3, 5, 7), (2, 33, 24)]


def affine_cases():
    return [dict(shape=s, add=a, mode=m, slope=sl) for s in AFFINE_SHAPES for a in (1, 0) for m, sl in ACT_MODES]


def affine_inputs(c):
    """voxel 0 of every (n, c): z on a 1/8 lattice, a on a 1/4 lattice, b = -a z (an exact product) => the pre-activation is exactly 0
    there (with `add`: on the even channels, whose add is 0)"""
    N, V, C = c["shape"]
    g = _gen(N, V, C, c["add"], c["mode"], int(c["slope"] * 100))
    z = torch.randn(N, V, C, generator=g)
    z[:, 0, :] = torch.round(z[:, 0, :] * 8) / 8
    a = torch.round(torch.randn(N, C, generator=g) * 4) / 4
    a[a == 0] = 0.25
    aff = torch.stack((a, -a * z[:, 0, :]), -1).contiguous()
    add = None
    if c["add"]:
        add = torch.randn(N, V, C, generator=g)
        add[:, 0, ::2] = 0.0
    return dict(z=z, affine=aff, add=add)


def affine_wrongs(c):
    return (["coef_row0"] if c["shape"][0] > 1 else []) + (["slope_swapped"] if c["mode"] == 2 else [])


def pair_stats(a, b, wrong=None):
    """the INCREMENT of stats (N, C, 2): (sum_v a, sum_v a b).  wrong: drop_last"""
    a, b = a.double(), b.double()
    if wrong == "drop_last":
        a, b = a[:, :-1], b[:, :-1]
    return torch.stack((a.sum(1), (a * b).sum(1)), -1), torch.stack((a.abs().sum(1), (a * b).abs().sum(1)), -1)


def pair_stats_K(V):
    """launcher of csrc/u3d_act.hip: splits = min(128, ceil(V / 1024)) blocks per sample, 4 voxel rows per block; a thread's chain is
    ceil(per / 4) fmaf / add steps (one rounding each), the four rows are added in float64"""
    splits = min(128, -(-V // 1024))
    per = -(-V // splits)
    return -(-per // 4) + 2


PAIR_C, PAIR_V = [7, 70, 128], [1, 3, 1025, 5000]


def pair_stats_inputs(C, V, N=2):
    g = _gen(C, V, 31)
    return dict(a=torch.randn(N, V, C, generator=g), b=torch.randn(N, V, C, generator=g),
                init=torch.randn(N, C, 2, generator=g, dtype=F64))
