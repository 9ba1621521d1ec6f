"""float64 reference of the normalisation kernels (csrc/norm_act.hip) and the case generator of tests/test_norm_edges_gpu.py.

CPU only, pure torch.  Every quantity exists twice:

  reference64(c)   closed forms in float64 (statistics, forward, backward, fused pool) -- no autograd, so that
                   tests/test_norm_oracle_cpu.py can hold them against float64 autograd as an independent check;
  reference32(c)   the same case through torch's own float32 CPU ops (batch / instance / group norm, leaky_relu,
                   max_pool, autograd).  Its distance to reference64 is ``e32``, the yardstick of the tolerance rule.

A case ``c`` is a dict of CPU fp32 tensors and settings made by ``make_case``; ``case(name)`` builds (once) a case of the
matrix ``SPECS``.  Tensors are [N, C, D, H, W]; kind is "bn" (statistics per channel over N, S), "in" (per n, c), "gn" (per
n and group of ``cg`` consecutive channels) or "none" (activation only).  Per-group vectors are flat in the kernels' order:
[C] for "bn", [N * C / cg] otherwise.

Two input conditions are established here and verified by the CPU test, never on the GPU:
  kink margin  no pre-activation within KINK_ULPS * 2^-24 * (max|x*sc| + |mean*sc| + |beta| [+ max|r|]) of 0 (sc = gamma * rstd,
               maxima per statistics group): offending inputs are nudged away (at most NUDGE_CAP of a case);
  pool ties    windows whose two largest float64 values differ by less than TIE_REL relative (and are not equal) are excepted
               from the exact comparison of the argmax codes (at most TIE_CAP of a case); exact ties are not.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

import oracle_kit as kit
from oracle_kit import ceil2          # noqa: F401  (re-exported: other files round their floors with it)

F64, F32 = torch.float64, torch.float32
EPS = float(torch.tensor(1e-5, dtype=F32))       # the kernels receive eps as a float
KINK_ULPS = 16.0
NUDGE_CAP = 1e-3
TIE_REL = 1e-5
TIE_CAP = 5e-3
CONST = -3.0 / 64.0                              # value of the constant channel (exact in fp32; its mean is exact too)
KIND_OF = {"mean": "stat", "rstd": "stat", "run_mean": "stat", "run_var": "stat", "y": "act", "pooled": "act", "dx": "dx",
           "dr": "dx", "dgamma": "sum", "dbeta": "sum", "s1": "sum", "s2": "sum", "csum": "sum"}


def f32(v):
    return float(torch.tensor(v, dtype=F32))


EACH = ("rstd", "run_var")      # positive per-group quantities: every group relative to its OWN reference value, so that one
                                # group with a large value (a constant channel: rstd = eps^-1/2) does not hide the others


def rel(a, ref, each=False):
    """|a - ref|max / |ref|max, or with ``each`` the largest per-element relative error."""
    if each:
        return ((a.double() - ref).abs() / ref.abs()).max().item()
    return kit.rel(a, ref)


# ---------------------------------------------------------------------------------------------------------------------
# statistics groups
# ---------------------------------------------------------------------------------------------------------------------
def _gred(t, kind, cg, how):
    """``how`` ("mean" / "amax") over each statistics group of t [N, C, D, H, W]; broadcastable against t."""
    N, C = t.shape[:2]
    if kind == "bn":
        return getattr(t, how)((0, 2, 3, 4), keepdim=True)
    v = getattr(t.reshape(N, C // cg, -1), how)(2)
    return v.repeat_interleave(cg, 1).reshape(N, C, 1, 1, 1)


def flat(b, kind, cg=1):
    """Broadcast form ([1 or N, C, 1, 1, 1]) -> the flat per-group vector."""
    return b.reshape(-1) if kind == "bn" else b.reshape(b.shape[0], -1)[:, ::cg].reshape(-1)


def bcast(v, kind, cg, N, C):
    if kind == "bn":
        return v.reshape(1, C, 1, 1, 1)
    return v.reshape(N, C // cg).repeat_interleave(cg, 1).reshape(N, C, 1, 1, 1)


def group_elems(shape, kind, cg=1):
    N, C, D, H, W = shape
    return N * D * H * W if kind == "bn" else cg * D * H * W


def _chan(v, C, default):
    return torch.full((1, C, 1, 1, 1), default, dtype=F64) if v is None else v.double().reshape(1, C, 1, 1, 1)


def stats64(x, kind, cg=1):
    """(mean, biased variance, rstd) per group in broadcast form, two-pass in float64."""
    xd = x.double()
    if kind == "none":
        z = torch.zeros((1, x.shape[1], 1, 1, 1), dtype=F64)
        return z, z + 1.0 - EPS, z + 1.0
    m = _gred(xd, kind, cg, "mean")
    var = _gred((xd - m) ** 2, kind, cg, "mean")
    return m, var, (var + EPS).rsqrt()


def running64(mean, var, E, rm, rv, momentum):
    """BatchNorm's running buffers after one step (unbiased variance); ``momentum`` is the fp32 value the kernel gets."""
    m = f32(momentum)
    unb = var * E / (E - 1.0) if E > 1 else var
    return (1.0 - m) * rm.double() + m * mean, (1.0 - m) * rv.double() + m * unb


def tile_partials(x, T, per_sample):
    """The (sum, sumsq) partials a conv epilogue with T tiles per image would leave (float64 sums rounded to fp32), in
    mis_norm_stats_finalize's two layouts: [N*C, T, 2] (per_sample) or [C, N*T, 2]."""
    N, C = x.shape[:2]
    v = x.double().reshape(N, C, T, -1)
    p = torch.stack((v.sum(3), (v * v).sum(3)), 3)                  # [N, C, T, 2]
    if per_sample:
        return p.reshape(N * C, T, 2).float().contiguous()
    return p.permute(1, 0, 2, 3).reshape(C, N * T, 2).float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# 2x max-pool: windows, first maximum wins
# ---------------------------------------------------------------------------------------------------------------------
def _windows(y):
    """[N, C, Do, Ho, Wo, pz*4]: the elements of each window in code order dz*4 + dy*2 + dx (pz = 1 when D == 1)."""
    N, C, D, H, W = y.shape
    pz = 2 if D > 1 else 1
    w = y.reshape(N, C, D // pz, pz, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7)
    return w.reshape(N, C, D // pz, H // 2, W // 2, pz * 4)


def pool_first(y):
    """(pooled, codes uint8 [N, C, Do, Ho, Wo]) with the FIRST maximal element of a window."""
    w = _windows(y)
    best = w.max(-1, keepdim=True).values
    pos = torch.arange(w.shape[-1]).expand_as(w)
    codes = torch.where(w == best, pos, torch.full_like(pos, 99)).min(-1).values
    return best.squeeze(-1), codes.to(torch.uint8)


def near_ties(y):
    """Windows whose two largest values differ, but by less than TIE_REL relative."""
    top = _windows(y.double()).topk(2, -1).values
    gap = top[..., 0] - top[..., 1]
    return (gap > 0) & (gap < TIE_REL * top.abs().max(-1).values)


def unpool(dpool, codes, shape):
    """The max-pool's backward: dpool scattered to the element each code names; [N, C, D, H, W]."""
    N, C, D, H, W = shape
    pz = 2 if D > 1 else 1
    hit = torch.arange(pz * 4).reshape(1, 1, 1, 1, 1, -1) == codes.long().unsqueeze(-1)
    w = hit.to(dpool.dtype) * dpool.unsqueeze(-1)
    w = w.reshape(N, C, D // pz, H // 2, W // 2, pz, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7)
    return w.reshape(N, C, D, H, W)


# ---------------------------------------------------------------------------------------------------------------------
# float64 closed forms
# ---------------------------------------------------------------------------------------------------------------------
def _pre64(c):
    """xhat, rstd, gamma, pre-activation z and the kink margin delta, all float64 in broadcast form."""
    x = c["x"].double()
    N, C = x.shape[:2]
    kind, cg = c["kind"], c["cg"]
    m, var, rstd = stats64(c["x"], kind, cg)
    xh = (x - m) * rstd
    ga, be = _chan(c["gamma"], C, 1.0), _chan(c["beta"], C, 0.0)
    z = xh * ga + be
    rmax = 0.0
    if c["r"] is not None and c["res"] == "pre":
        z = z + c["r"].double()
        rmax = c["r"].abs().max().item()
    sc = ga * rstd
    gk = "in" if kind == "none" else kind
    delta = KINK_ULPS * 2.0 ** -24 * (_gred((x * sc).abs().expand_as(x), gk, cg, "amax")
                                     + _gred((m * sc).abs().expand_as(x), gk, cg, "amax")
                                     + _gred(be.abs().expand_as(x), gk, cg, "amax") + rmax)
    return dict(m=m, var=var, rstd=rstd, xh=xh, ga=ga, be=be, z=z, sc=sc, delta=delta)


def reference64(c):
    """Every quantity of the case in float64: dict of tensors (per-group vectors flat)."""
    x = c["x"]
    N, C = x.shape[:2]
    kind, cg, slope = c["kind"], c["cg"], f32(c["slope"])      # the kernels receive the slope as a float
    p = _pre64(c)
    z, xh, ga, rstd = p["z"], p["xh"], p["ga"], p["rstd"]
    out = {}
    if kind != "none":
        out["mean"], out["rstd"], out["var"] = flat(p["m"], kind, cg), flat(rstd, kind, cg), flat(p["var"], kind, cg)
        if c["rm"] is not None:
            out["run_mean"], out["run_var"] = running64(out["mean"], out["var"], group_elems(x.shape, kind, cg), c["rm"],
                                                        c["rv"], c["momentum"])
    a = torch.where(z > 0, z, z * slope)
    if c["r"] is not None and c["res"] == "post":
        a = a + c["r"].double()
    y = a * c["mask"].double() if c["mask"] is not None else a
    out["y"] = y
    if c["dpool"] is not None:
        out["pooled"], out["codes"] = pool_first(y)
        out["near"] = near_ties(y)
    g = c["da"].double() if c["da"] is not None else torch.zeros_like(y)
    if c["dpool"] is not None:
        g = g + unpool(c["dpool"].double(), out["codes"], x.shape)
    if c["mask"] is not None:
        g = g * c["mask"].double()
    dz = g * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if c["r"] is not None:
        out["dr"] = g if c["res"] == "post" else dz
    if kind == "none":
        out["dx"] = dz
        return out
    dxh = dz * ga
    out["dx"] = rstd * (dxh - _gred(dxh, kind, cg, "mean") - xh * _gred(dxh * xh, kind, cg, "mean"))
    if c["gamma"] is not None:
        out["dgamma"], out["dbeta"] = (dz * xh).sum((0, 2, 3, 4)), dz.sum((0, 2, 3, 4))
    if cg == 1:             # what mis_norm_act_bwd_sums returns: the group means of dz and dz * xhat (gamma not folded in)
        out["s1"], out["s2"] = flat(_gred(dz, kind, 1, "mean"), kind), flat(_gred(dz * xh, kind, 1, "mean"), kind)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the same through torch's float32 CPU ops
# ---------------------------------------------------------------------------------------------------------------------
def _norm32(c, x, gamma, beta, rm=None, rv=None):
    kind = c["kind"]
    if kind == "bn":
        return F.batch_norm(x, rm, rv, gamma, beta, True, f32(c["momentum"]), EPS)    # the fp32 value the kernel gets
    if kind == "in":
        return F.instance_norm(x, weight=gamma, bias=beta, eps=EPS)
    if kind == "gn":
        # the per-channel affine as ops of its own: F.group_norm's fused backward forms dgamma as (sum dy*x - mean * sum dy)
        # * rstd, which cancels (e32 of dgamma 3e-5 .. 8e-5 on the conditioning cases, 1e-6 this way): a tighter yardstick
        z = F.group_norm(x, x.shape[1] // c["cg"], None, None, EPS)
        return z * gamma.reshape(1, -1, 1, 1, 1) + beta.reshape(1, -1, 1, 1, 1)
    return x


def _act32(c, z, r):
    if r is not None and c["res"] == "pre":
        z = z + r
    a = F.leaky_relu(z, f32(c["slope"]))
    if r is not None and c["res"] == "post":
        a = a + r
    return a * c["mask"] if c["mask"] is not None else a


def reference_torch(c, codes=None, dtype=F32):
    """reference64's quantities from torch's ops and autograd in ``dtype`` (as float64 tensors): float32 gives the yardstick
    e32, float64 the independent check of the closed forms.  ``codes``: the argmax codes the pool gradient is scattered
    through (an input of mis_norm_act_bwd_pool; the float64 oracle's)."""
    c = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    x = c["x"].clone().requires_grad_(True)
    N, C, D, H, W = x.shape
    kind, cg = c["kind"], c["cg"]
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    gamma, beta, r = leaf(c["gamma"]), leaf(c["beta"]), leaf(c["r"])
    out = {}
    with torch.no_grad():
        if kind == "bn":
            _, m, rs = torch.native_batch_norm(c["x"], None, None, None, None, True, 0.0, EPS)
        elif kind == "in":
            _, m, rs = torch.native_batch_norm(c["x"].reshape(1, N * C, D, H, W), None, None, None, None, True, 0.0, EPS)
        elif kind == "gn":
            # a group is contiguous in NCDHW: batch-norm statistics of the [1, N*G, cg*S] view (double accumulation; the
            # fp32 cascade of native_group_norm is off by up to 2e-6 in the mean -- again the tighter yardstick)
            _, m, rs = torch.native_batch_norm(c["x"].reshape(1, N * C // cg, cg * D, H, W), None, None, None, None, True,
                                               0.0, EPS)
        if kind != "none":
            out["mean"], out["rstd"] = m.reshape(-1), rs.reshape(-1)
    rm = rv = None
    if c["rm"] is not None:
        rm, rv = c["rm"].clone(), c["rv"].clone()
    y = _act32(c, _norm32(c, x, gamma, beta, rm, rv), r)
    if rm is not None:
        out["run_mean"], out["run_var"] = rm, rv
    out["y"] = y.detach()
    if c["dpool"] is not None:
        out["pooled"] = (F.max_pool3d(out["y"], 2) if D > 1 else F.max_pool2d(out["y"][:, :, 0], 2).unsqueeze(2))
    g = c["da"] if c["da"] is not None else torch.zeros_like(c["x"])
    if c["dpool"] is not None:
        g = g + unpool(c["dpool"], codes, x.shape)
    y.backward(g)
    out["dx"] = x.grad
    if r is not None:
        out["dr"] = r.grad
    if gamma is not None:
        out["dgamma"], out["dbeta"] = gamma.grad, beta.grad
    if cg == 1 and kind in ("bn", "in"):
        E = group_elems(x.shape, kind)
        if kind == "bn" and gamma is not None:
            out["s1"], out["s2"] = beta.grad / E, gamma.grad / E
        elif kind == "in" and gamma is None:
            # F.instance_norm is batch_norm on the [1, N*C, ...] view: with a unit affine there, autograd's gradients of
            # the affine are the per-(n, c) sums
            w, b = torch.ones(N * C, dtype=dtype, requires_grad=True), torch.zeros(N * C, dtype=dtype, requires_grad=True)
            z = F.batch_norm(c["x"].reshape(1, N * C, D, H, W), None, None, w, b, True, 0.0, EPS).reshape(x.shape)
            _act32(c, z, c["r"]).backward(g)
            out["s1"], out["s2"] = b.grad / E, w.grad / E
    return {k: v.detach().double() for k, v in out.items()}


def reference32(c, codes=None):
    return reference_torch(c, codes, F32)


def channel_sum(x, dtype):
    return x.to(dtype).sum((0, 2, 3, 4)).double()


def from_running(rv, dtype):
    return (rv.to(dtype) + EPS).rsqrt().double()


@functools.lru_cache(maxsize=None)
def channel_sum_input(N, S):
    """The gradient at a conv's output, [N, 5, ...]: every channel sum is of the order of sqrt(N*S), none cancels to ~0."""
    g = torch.Generator().manual_seed(1000 * N + S)
    return torch.randn(_shape(N, 5, S), generator=g) + 0.25


@functools.lru_cache(maxsize=None)
def running_input(C):
    g = torch.Generator().manual_seed(C)
    return 0.3 * torch.randn(C, generator=g), 0.05 + 2.0 * torch.rand(C, generator=g)


CHANNEL_SUM_CASES = [(N, S) for N in (1, 3) for S in (4, 16388)]
RUNNING_CASES = (1, 255, 257)


def extra_e32():
    """(label, quantity, e32) of the cases outside SPECS."""
    for N, S in CHANNEL_SUM_CASES:
        x = channel_sum_input(N, S)
        yield f"csum-N{N}-S{S}", "csum", rel(channel_sum(x, F32), channel_sum(x, F64))
    for C in RUNNING_CASES:
        rv = running_input(C)[1]
        yield f"running-C{C}", "rstd", rel(from_running(rv, F32), from_running(rv, F64), True)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _nudge(c):
    """Move inputs whose pre-activation is within the kink margin away from 0; returns the number of elements moved."""
    moved = torch.zeros(c["x"].shape, dtype=torch.bool)
    for _ in range(20):
        p = _pre64(c)
        bad = p["z"].abs() < p["delta"]
        if not bad.any():
            return int(moved.sum())
        sc = p["sc"].expand_as(bad)
        assert (sc[bad] != 0).all(), "gamma = 0 needs |beta| above the margin"
        sign = torch.where(p["z"] < 0, -1.0, 1.0) * torch.sign(sc)
        step = sign * 4.0 * p["delta"] / sc.abs().clamp_min(1e-300)
        c["x"] = torch.where(bad, c["x"].double() + step, c["x"].double()).float()
        moved |= bad
    raise AssertionError("kink margin not reached")


def undecided(c):
    """Elements still within the kink margin (must be none)."""
    p = _pre64(c)
    return int((p["z"].abs() < p["delta"]).sum())


def make_case(name, kind, shape, cg=1, ratio=0.0, slope=0.01, affine=True, special=False, res=None, drop_p=0.0, pool=False,
              running=False, momentum=0.1, seed=0):
    N, C, D, H, W = shape
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{seed}".encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    gk = "in" if kind == "none" else kind

    def tie(t):                                        # one value per statistics group, [N, C, 1, 1, 1]
        t = t[:1].expand(N, C) if gk == "bn" else t[:, ::cg].repeat_interleave(cg, 1)
        return t.reshape(N, C, 1, 1, 1)
    sig = tie(0.5 + 1.5 * torch.rand(N, C, generator=g))
    sgn = tie(torch.where(torch.rand(N, C, generator=g) < 0.5, -1.0, 1.0))
    x = sgn * ratio * sig + sig * rn(*shape)
    if D * H * W <= 3 and gk == "in":
        # dx of a group of two elements is (dz0 - dz1)/2 * eps/(var + eps), of three elements one free direction plus such
        # a term: with var >> eps mostly cancellation (e32 3e-4 / 7e-6, which would become the floor of every dx in the
        # matrix); at std 2^-8, var is of the order of eps and the groups are as well conditioned as the larger ones
        x = x / 256.0
    gamma = beta = None
    if affine and kind != "none":
        gamma = 1.0 + 0.3 * rn(C)
        gamma = torch.where(gamma.abs() < 0.25, torch.full_like(gamma, 0.25), gamma)
        beta = 0.2 * rn(C)
    if special:
        assert gamma is not None and C >= 3 * cg
        x[:, :cg] = CONST                              # variance exactly 0 in every group that holds channel 0
        beta[:cg] = torch.tensor([0.15, -0.25])[:cg]    # the constant channels' pre-activation IS beta
        gamma[cg], gamma[cg + 1], beta[cg + 1] = -0.7, 0.0, 0.35
    c = dict(name=name, kind=kind, cg=cg, slope=slope, res=res, drop_p=drop_p, momentum=momentum, ratio=ratio, x=x,
             gamma=gamma, beta=beta, r=None, mask=None, da=rn(*shape), dpool=None, rm=None, rv=None)
    if res:
        c["r"] = 0.7 * rn(*shape)
    if drop_p > 0:
        c["mask"] = (torch.rand(*shape, generator=g) >= drop_p).float() / (1.0 - drop_p)
    if pool:
        c["dpool"] = rn(N, C, D // 2 if D > 1 else 1, H // 2, W // 2)
    if running:
        c["rm"], c["rv"] = 0.3 * rn(C), 0.5 + torch.rand(C, generator=g)
    c["nudged"] = _nudge(c)
    return c


SPECS = {}


def _spec(group, name, **kw):
    assert name not in SPECS, name
    SPECS[name] = dict(kw, group=group)


def _shape(N, C, S):
    known = {2: (1, 1, 2), 3: (1, 1, 3), 4: (1, 2, 2), 6: (1, 2, 3), 27: (3, 3, 3), 125: (5, 5, 5), 1001: (7, 11, 13),
             1024: (4, 16, 16), 4100: (1, 25, 164), 16384: (16, 32, 32), 16388: (1, 17, 964), 49156: (1, 12289, 4),
             524292: (3, 43691, 4)}
    assert known[S][0] * known[S][1] * known[S][2] == S
    return (N, C) + known[S]


def _build_matrix():
    # split geometry: every S for every kind; N in {1, 3}, C in {2, 5, 16} (GroupNorm, cg = 2: {2, 16, 32})
    for kind in ("bn", "in", "gn"):
        cs = (2, 16, 32) if kind == "gn" else (2, 5, 16)
        for S in (4, 1024, 4100, 16384, 16388, 49156):
            for N, C in ((3, cs[1]), (1, cs[2])) if S <= 4100 else ((3, cs[0]), (1, cs[1])):
                _spec("geometry", f"{kind}-S{S}-N{N}-C{C}", kind=kind, shape=_shape(N, C, S), cg=2 if kind == "gn" else 1,
                      slope=0.0 if kind != "bn" else 0.01, affine=kind != "in" or C == 5, running=kind == "bn",
                      drop_p=0.3 if N == 3 else 0.0)
        _spec("geometry", f"{kind}-S4-N1-C{cs[0]}", kind=kind, shape=_shape(1, cs[0], 4), cg=2 if kind == "gn" else 1,
              affine=kind != "in", running=kind == "bn")
    _spec("geometry", "in-S524292-N1-C2", kind="in", shape=_shape(1, 2, 524292), slope=0.0, affine=False)
    # scalar path (S % 4 != 0): BatchNorm, InstanceNorm (no affine there) and no normalisation
    for kind in ("bn", "in", "none"):
        for S in (2, 3, 6, 27, 125, 1001):
            _spec("scalar", f"{kind}-S{S}", kind=kind, shape=_shape(3, 5, S), slope=0.01 if kind == "bn" else 0.0,
                  affine=kind == "bn", running=kind == "bn")
    # conditioning: mean / std of every group, without and with the three special channels (the constant channel's
    # rstd = eps^-1/2 makes its dx the largest of the tensor, which would hide the other channels' if it were always there)
    for kind, C, cg in (("bn", 6, 1), ("in", 6, 1), ("gn", 8, 2)):
        for ratio in (0, 4, 32):
            for special in (False, True):
                _spec("conditioning", f"{kind}-ratio{ratio}" + ("-special" if special else ""), kind=kind,
                      shape=_shape(2, C, 16388), cg=cg, ratio=float(ratio), special=special,
                      slope=0.01 if kind == "bn" else 0.0, running=kind == "bn")
    # BatchNorm bookkeeping
    for mom in (0.1, 0.3):
        _spec("bookkeeping", f"bn-momentum{mom}", kind="bn", shape=(3, 5, 1, 12, 20), running=True, momentum=mom, ratio=1.0)
    # residual forms
    for kind in ("bn", "in"):
        for res in ("pre", "post"):
            _spec("residual", f"{kind}-{res}", kind=kind, shape=_shape(2, 3, 16388), res=res, affine=kind == "bn")
    # fused pool
    for shape in ((2, 3, 1, 2, 8), (1, 2, 1, 514, 8), (2, 2, 2, 4, 16), (1, 2, 6, 10, 24)):
        for kind, slope in (("bn", 0.01), ("in", 0.0)):
            for p in (0.0, 0.3):
                _spec("pool", f"{kind}-{'x'.join(map(str, shape))}-p{p}", kind=kind, shape=shape, slope=slope,
                      affine=kind == "bn", drop_p=p, pool=True)
    # mis_norm_act_bwd_sums
    for kind in ("bn", "in"):
        for S in (1024, 16388):
            _spec("sums", f"{kind}-S{S}", kind=kind, shape=_shape(3, 5, S), affine=kind == "bn",
                  slope=0.01 if kind == "bn" else 0.0)
    # every entry point with all operands as slices (the residual / pool / sums entry points reuse their cases above)
    for kind, C, cg in (("bn", 3, 1), ("in", 3, 1), ("gn", 4, 2)):
        _spec("strides", f"{kind}", kind=kind, shape=(2, C, 2, 6, 10), cg=cg, affine=kind != "in", running=kind == "bn",
              drop_p=0.3, slope=0.01)
    # partials for mis_norm_stats_finalize: np = T (per sample) or N * T (batch), 8 elements per tile
    for np_ in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1029):
        _spec("finalize", f"in-np{np_}", kind="in", shape=(2, 3, 1, np_, 8), affine=False, tiles=np_)
        for N in (1, 3):
            if np_ % N == 0:
                _spec("finalize", f"bn-np{np_}-N{N}", kind="bn", shape=(N, 3, 1, np_ // N, 8), running=True, tiles=np_ // N,
                      momentum=0.3 if N == 3 else 0.1)
    for ratio in (4, 32):
        _spec("finalize", f"in-np257-ratio{ratio}", kind="in", shape=(2, 3, 1, 257, 8), affine=False, tiles=257,
              ratio=float(ratio))
        _spec("finalize", f"bn-np1029-N3-ratio{ratio}", kind="bn", shape=(3, 3, 1, 343, 8), running=True, tiles=343,
              ratio=float(ratio))


_build_matrix()


def names(group):
    return [n for n, s in SPECS.items() if s["group"] == group]


@functools.lru_cache(maxsize=None)
def case(name):
    kw = {k: v for k, v in SPECS[name].items() if k not in ("group", "tiles")}
    return make_case(name, **kw)


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 reference, fp32 reference, e32 per quantity) of a matrix case; computed once, never modified."""
    c = case(name)
    r64 = reference64(c)
    r32 = reference32(c, r64.get("codes"))
    e32 = {k: rel(r32[k], r64[k], k in EACH) for k in r32}
    return r64, r32, e32


# The ``stat`` rule of tests/test_norm_edges_gpu.py (its K and FLOOR["stat"], measured there): kept here because
# tests/test_conv_edges_gpu.py holds the statistics of the split Winograd forward to the same rule.
K = 6.0
FLOOR_STAT = 1.2e-7


def finalize_factor(mean64, var64):
    """Conditioning of one-pass statistics from fp32 partials: the factor rstd and running_var get per group in
    mis_norm_stats_finalize's tests (tests/test_norm_edges_gpu.py; tests/test_conv_edges_gpu.py holds the split Winograd
    forward's to it too)."""
    return 1.0 + mean64 ** 2 / (var64 + EPS)
