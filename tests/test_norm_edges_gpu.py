"""The normalisation kernels (csrc/norm_act.hip) against the float64 oracle of tests/norm_oracle.py at their edges: the
split geometry of the reductions (S from one float4 unit to the 32-split cap, ragged last split), the scalar path
(S % 4 != 0), mis_norm_stats_finalize around its 64 / 256-thread switch and at every remainder of its unrolled loop,
batch-strided views of every operand, ill-conditioned inputs (mean / std up to 32, a constant channel, gamma < 0,
gamma = 0), BatchNorm's running statistics, the residual forms, the fused max-pool (argmax codes, first maximum wins),
mis_channel_sum, mis_norm_stats_from_running, mis_norm_act_bwd_sums and the refusals.

Every output is pre-filled with NaN and must come back finite; a strided operand is a channel slice of a wider buffer
(NaN around an input, a sentinel around an output, which must survive); a reference of exactly 0 must be met exactly.
The apply kernels always run on the statistics the HIP statistics pass produced for the same case (end to end).

Tolerance (the rule of test_loss_tails_gpu.py and F64_K of test_parity_gpu.py), per compared tensor:

    |hip - f64|_max <= max(K * e32, FLOOR) * |f64|_max,    K = 6

e32 = error of torch's fp32 CPU evaluation of the same case and quantity against float64 (norm_oracle.reference32);
FLOOR = the largest e32 of the whole matrix for that kind of quantity (test_norm_oracle_cpu.py recomputes the four).
The inputs keep every pre-activation a stated margin away from the ReLU kink (norm_oracle: KINK_ULPS), so a flipped
activation is a failure, and argmax codes are compared exactly except in windows whose two largest float64 values differ
by less than 1e-5 relative (none in this matrix); exact ties are compared.

One derived exception: mis_norm_stats_finalize reads partial sums that are fp32 by contract.  One-pass ss/E - m^2 from
values rounded at 2^-24 is off by that rounding times (1 + mean^2 / (var + eps)), so rstd and running_var get this factor
per group, from the oracle.  It is 1 on the centred cases: a dropped or mis-indexed partial still fails.  The stand-alone
mis_norm_stats reads the data itself, keeps double partials, and gets no factor.

Measured on an MI355X (this file's own run; `MIS_NORM_STATS=<file>` writes every figure as JSON):

    entry points (mis_norm_* / mis_*)      kind  e32 (fp32 torch vs f64)  HIP (max)  worst HIP / tolerance (case; "floor": K * e32 < FLOOR there)
    stats / fwd_g / bwd_g, split geometry  act   4.2e-09 .. 1.8e-07   1.03e-07   0.17  (bn-S1024-N3-C5 y)
    stats / fwd_g / bwd_g, split geometry  dx    5.1e-08 .. 2.5e-07   1.47e-07   0.28  (bn-S4-N1-C2 dx)
    stats / fwd_g / bwd_g, split geometry  stat  7.8e-09 .. 9.5e-08   5.71e-08   0.17  (bn-S4-N1-C16 mean)
    stats / fwd_g / bwd_g, split geometry  sum   2.0e-08 .. 2.6e-06   4.38e-07   0.04  (bn-S16388-N1-C5 dbeta)
    stats / fwd / bwd, S % 4 != 0          act   0.0e+00 .. 9.7e-08   9.11e-08   0.15  (bn-S1001 y; floor)
    stats / fwd / bwd, S % 4 != 0          dx    0.0e+00 .. 1.1e-07   1.08e-07   0.21  (in-S3 dx)
    stats / fwd / bwd, S % 4 != 0          stat  5.2e-09 .. 9.1e-08   5.15e-08   0.17  (bn-S6 rstd)
    stats / fwd / bwd, S % 4 != 0          sum   2.9e-08 .. 3.1e-07   8.24e-08   0.01  (bn-S6 dgamma; floor)
    stats / fwd_g / bwd_g, mean/std 0..32  act   6.0e-08 .. 4.8e-07   5.29e-07   0.22  (gn-ratio32 y)
    stats / fwd_g / bwd_g, mean/std 0..32  dx    9.0e-08 .. 1.5e-07   1.48e-07   0.23  (in-ratio0 dx)
    stats / fwd_g / bwd_g, mean/std 0..32  stat  3.7e-09 .. 1.1e-07   5.58e-08   0.17  (bn-ratio4 mean)
    stats / fwd_g / bwd_g, mean/std 0..32  sum   6.5e-08 .. 2.6e-06   2.11e-06   0.23  (in-ratio32-special dgamma)
    stats / fwd_g / bwd_g, slices          act   5.4e-08 .. 1.1e-07   9.30e-08   0.14  (gn y)
    stats / fwd_g / bwd_g, slices          dx    9.9e-08 .. 1.4e-07   1.05e-07   0.17  (in dx)
    stats / fwd_g / bwd_g, slices          stat  1.1e-08 .. 7.3e-08   4.13e-08   0.17  (bn rstd)
    stats / fwd_g / bwd_g, slices          sum   6.8e-08 .. 2.5e-07   1.12e-07   0.02  (gn dgamma; floor)
    BatchNorm bookkeeping                  act   7.2e-08 .. 7.5e-08   7.16e-08   0.12  (bn-momentum0.3 y; floor)
    BatchNorm bookkeeping                  dx    6.8e-08 .. 9.1e-08   7.62e-08   0.19  (bn-momentum0.3 dx)
    BatchNorm bookkeeping                  stat  1.5e-08 .. 8.6e-08   5.18e-08   0.17  (bn-momentum0.3 rstd)
    BatchNorm bookkeeping                  sum   7.2e-08 .. 2.1e-07   7.60e-08   0.01  (bn-momentum0.3 dbeta; floor)
    norm_res_act_fwd / bwd                 act   6.6e-08 .. 9.2e-08   7.99e-08   0.13  (in-post y; floor)
    norm_res_act_fwd / bwd                 dx    0.0e+00 .. 1.4e-07   9.51e-08   0.17  (in-pre dx)
    norm_res_act_fwd / bwd                 stat  8.8e-09 .. 6.2e-08   5.54e-08   0.17  (bn-pre mean)
    norm_res_act_fwd / bwd                 sum   5.3e-07 .. 5.7e-06   6.95e-07   0.06  (bn-post dgamma; floor)
    norm_act_fwd_pool / bwd_pool           act   3.9e-08 .. 1.0e-07   1.03e-07   0.17  (bn-1x2x1x514x8-p0.3 y)
    norm_act_fwd_pool / bwd_pool           dx    6.5e-08 .. 1.6e-07   1.66e-07   0.22  (bn-1x2x1x514x8-p0.3 dx)
    norm_act_fwd_pool / bwd_pool           stat  1.2e-08 .. 5.4e-08   4.78e-08   0.17  (in-2x2x2x4x16-p0.0 mean)
    norm_act_fwd_pool / bwd_pool           sum   1.7e-08 .. 1.3e-06   4.22e-07   0.07  (bn-1x2x6x10x24-p0.3 dgamma; floor)
    norm_act_bwd_sums                      sum   1.5e-07 .. 2.5e-06   2.94e-07   0.03  (in-S16388 s2; floor)
    norm_stats_finalize                    stat  4.3e-09 .. 9.2e-08   2.61e-06   0.75  (in-np257 mean; floor)
    channel_sum                            sum   3.7e-08 .. 1.1e-07   7.97e-08   0.01  (csum-N1-S16388 csum; floor)
    norm_stats_from_running                stat  2.1e-08 .. 4.8e-08   8.81e-08   0.31  (running-C255 rstd)

    kind: stat = mean / rstd / running buffers, act = y / pooled, dx = dx / dr, sum = dgamma / dbeta / group sums / channel sums.
    Every tensor is within 1.7 x its own e32 (K = 6 is never needed); the one ratio near 1 is the mean of the finalize path,
    9e-8 of a group mean that is itself 0.01 standard deviations (fp32 partials; e32 there is 2e-8, so the floor decides).
    No argmax code differs from the oracle's.  147 cases, 4.8 s wall (146 without the split-count test: 4.78 s).

    FLOOR: stat 1.2e-7 (running_mean, bn-ratio0), act 6.1e-7 (y at mean/std 32), dx 2.6e-7 (in-S4-N1-C2),
    sum 5.8e-6 (dbeta of bn-pre: a channel sum that nearly cancels).

mis_norm_stats at an offset ([2, C, 16388] inputs, two ragged splits), before (the parent commit's library under this file:
float2 partials between stats_partial_kernel and stats_final_kernel) and after (double2 partials; the final stage uses them
where mean^2 > 3 var and the fp32-rounded sums -- the parent's arithmetic, bit for bit -- below that, where they are within
fp32 noise).  rstd is the worst group relative to its own value; y and dgamma are what the apply kernels make of it:

    mean/std  quantity     before                tolerance            after
    4         rstd         2.4e-7 .. 7.6e-7      2.8e-7 .. 4.7e-7     4.6e-8 .. 5.4e-8
    4         y            1.6e-7 .. 7.4e-7      6.1e-7 .. 9.6e-7     8.5e-8 .. 1.4e-7
    32        rstd         1.9e-5 .. 4.4e-5      2.4e-7 .. 4.5e-7     4.0e-8 .. 5.6e-8
    32        running_var  4.7e-6 .. 1.2e-5      3.6e-7 .. 4.8e-7     2.3e-8 .. 4.0e-8
    32        y            1.7e-5 .. 3.5e-5      1.1e-6 .. 2.9e-6     1.7e-7 .. 5.3e-7
    32        dgamma       1.3e-5 .. 7.2e-5      5.8e-6 .. 9.4e-6     3.9e-7 .. 2.1e-6
    32        dx           8.6e-8 .. 1.7e-5      4.7e-7 .. 9.2e-7     4.8e-8 .. 1.5e-7

    (range over BatchNorm / InstanceNorm / GroupNorm, with and without the special channels; e32 of rstd is 4e-8 .. 8e-8 throughout.)
    Before, all six mean/std 32 cases fail and four of the six at mean/std 4 (rstd; y for InstanceNorm); the mean/std 0 cases
    pass.  After, all eighteen pass.  The finalize path (fp32 partials by contract) measures rstd 2.6e-6 at mean/std 32 under
    its factor of 1025.
"""
import functools

import pytest
import torch

import norm_oracle as no
import oracle_kit as kit
from oracle_kit import NAN, SENT

pytestmark = pytest.mark.gpu

K = no.K
FLOOR = {"stat": no.FLOOR_STAT,     # largest e32 of mean / rstd / running statistics: 1.11e-7 (running_mean, bn-ratio0)
         "act": 6.1e-7,       # of y / pooled: 6.02e-7 (in-np257-ratio32: mean / std 32)
         "dx": 2.6e-7,        # of dx / dr: 2.54e-7 (in-S4-N1-C2)
         "sum": 5.8e-6}       # of dgamma / dbeta / group sums / channel sums: 5.70e-6 (dbeta of bn-pre)
LEAD, TRAIL = 1, 2            # channels of the wider buffer before / after a slice
_in, _out = functools.partial(kit.place, lead=LEAD, trail=TRAIL), functools.partial(kit.Out, lead=LEAD, trail=TRAIL)
STATS = []


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not STATS:
        return
    for (test, key), r in kit.worst_rows(((test, key), cid, e32, ehip, max(e32, FLOOR[no.KIND_OF[key]] / K) * factor)
                                         for test, cid, key, e32, ehip, factor in STATS):
        print(f"\n[norm edges] {test:12s} {key:8s} e32 {r['lo']:.2e} .. {r['hi']:.2e}  hip max {r['hip']:.2e}  "
              f"worst hip/max(e32, floor/K) {r['ratio']:.2f} ({r['at']})", end="")
    print()
    kit.report(STATS, "MIS_NORM_STATS")


# ---------------------------------------------------------------------------------------------------------------------
# placement and comparison
# ---------------------------------------------------------------------------------------------------------------------
class _Check:
    def __init__(self, test, name):
        self.test, self.name = test, name
        self.r64, _, self.e32 = no.references(name) if name in no.SPECS else ({}, None, {})
        self.gate = kit.Gate(K, FLOOR, stats=STATS)

    def __call__(self, key, got, ref=None, e32=None, factor=None):
        ref = self.r64[key] if ref is None else ref
        e32 = self.e32[key] if e32 is None else e32
        got = got.detach().cpu().double().reshape(ref.shape)
        self.gate.finite(got, (self.name, key))
        self.gate.zero_ok((got[ref == 0] == 0).all(), (self.name, key))
        scale = ref.abs() if key in no.EACH else ref.abs().max()     # rstd / running_var: each group on its own scale
        err = (got - ref).abs()
        ehip = (err / scale).max().item() if scale.max().item() > 0 else 0.0
        fmax, ok = 1.0, None
        if factor is not None:                      # per-group conditioning factor (mis_norm_stats_finalize only)
            assert key in no.EACH
            fmax = factor.max().item()
            ok = bool((err <= max(K * e32, FLOOR[no.KIND_OF[key]]) * factor * scale).all())
        tol = self.gate.judge(self.name, key, no.KIND_OF[key], "max", e32, ehip, fmax, ok=ok,
                              row=(self.test, self.name, key, e32, ehip, fmax))
        print(f"[{self.test} {self.name}] {key:8s} |f64|max {scale.max().item():.3e} e32 {e32:.2e} hip {ehip:.2e} tol {tol:.2e}")

    def done(self):
        self.gate.done(self.name)


# ---------------------------------------------------------------------------------------------------------------------
# statistics -> forward -> backward of one case, every tensor against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _hip_stats(c, xv, chk=None):
    """(mean, rstd) of the HIP statistics pass for the case, compared when ``chk``; BatchNorm with running buffers also
    checks them and the batch counter."""
    ops = _ops()
    N, C = c["x"].shape[:2]
    kind, cg = c["kind"], c["cg"]
    if kind == "none":
        return torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    G = C if kind == "bn" else N * C // cg
    mean, rstd = kit.nan(G), kit.nan(G)
    if kind == "gn":
        ops.group_norm_stats(xv, cg, 1e-5, mean, rstd)
    elif c["rm"] is not None:
        rm, rv = c["rm"].cuda(), c["rv"].cuda()
        nbt = torch.tensor([41], dtype=torch.int64, device="cuda")
        ops.norm_stats(xv, False, 1e-5, mean, rstd, rm, rv, nbt, momentum=c["momentum"])
        assert nbt.item() == 42
        if chk:
            chk("run_mean", rm)
            chk("run_var", rv)
    else:
        ops.norm_stats(xv, kind != "bn", 1e-5, mean, rstd)
    if chk:
        chk("mean", mean)
        chk("rstd", rstd)
    return mean, rstd


def _run(test, name, layout):
    ops = _ops()
    c = no.case(name)
    chk = _Check(test, name)
    r64 = chk.r64
    shape = tuple(c["x"].shape)
    N, C, D, H, W = shape
    kind, cg, slope, p = c["kind"], c["cg"], c["slope"], c["drop_p"]
    per_sample = kind in ("in", "gn")
    xv = _in(c["x"], layout)
    mean, rstd = _hip_stats(c, xv, chk)
    gamma = None if c["gamma"] is None else c["gamma"].cuda()
    beta = None if c["beta"] is None else c["beta"].cuda()
    mask = None if c["mask"] is None else c["mask"].cuda()      # the explicit mask stays contiguous
    y = _out(shape, layout)
    rv = _in(c["r"], layout)
    post = c["res"] == "post"
    pooled = idx = None
    if c["r"] is not None:
        ops.norm_res_act_fwd(xv, rv, y.v, per_sample, mean, rstd, gamma, beta, slope, post=post)
    elif c["dpool"] is not None:
        pooled = _out(tuple(c["dpool"].shape), layout)
        idx = torch.full((c["dpool"].numel(),), 255, dtype=torch.uint8, device="cuda")
        ops.norm_act_fwd_pool(xv, y.v, pooled.v, idx, per_sample, mean, rstd, gamma, beta, slope, drop_p=p, drop_mask=mask)
    else:
        ops.norm_act_fwd(xv, y.v, per_sample, mean, rstd, gamma, beta, slope, drop_p=p, drop_mask=mask, cg=cg)
    chk("y", y.v)
    assert y.untouched()
    if pooled is not None:
        chk("pooled", pooled.v)
        assert pooled.untouched()
        differ = idx.cpu().reshape(r64["codes"].shape) != r64["codes"]
        assert not (differ & ~r64["near"]).any(), (name, "argmax codes", int(differ.sum()))

    dav = _in(c["da"], layout)
    dx = _out(shape, layout)
    dg = db = None
    if gamma is not None:
        dg, db = kit.nan(C), kit.nan(C)
    if c["r"] is not None:
        dr = _out(shape, layout)
        ops.norm_res_act_bwd(xv, rv, dav, dx.v, dr.v, False, per_sample, mean, rstd, gamma, beta, slope, dgamma=dg, dbeta=db,
                             post=post)
        chk("dr", dr.v)
        assert dr.untouched()
        once = dr.v.clone()
        ops.norm_res_act_bwd(xv, rv, dav, dx.v, dr.v, True, per_sample, mean, rstd, gamma, beta, slope, dgamma=dg, dbeta=db,
                             post=post)
        assert torch.equal(dr.v, once + once) and dr.untouched()       # accumulated: exactly twice the written gradient
    elif c["dpool"] is not None:
        codes = r64["codes"].reshape(-1).cuda()                 # the oracle's codes: the backward is judged on its own
        dpv = _in(c["dpool"], layout)
        ops.norm_act_bwd_pool(xv, dav, dpv, codes, dx.v, per_sample, mean, rstd, gamma, beta, slope, drop_p=p, drop_mask=mask,
                              dgamma=dg, dbeta=db)
    else:
        ops.norm_act_bwd(xv, dav, dx.v, per_sample, mean, rstd, gamma, beta, slope, drop_p=p, drop_mask=mask, dgamma=dg,
                         dbeta=db, cg=cg, no_norm=kind == "none")
    chk("dx", dx.v)
    assert dx.untouched()
    if dg is not None:
        chk("dgamma", dg)
        chk("dbeta", db)
    chk.done()
    return c, xv, dav, mean, rstd, gamma, beta, mask, dg, db


def test_split_counts_the_geometry_cases_rely_on():
    """The split count of a (group, chunk) is not visible in any result (one split computes the same sums, only slower); it
    is visible in mis_norm_workspace_bytes: P = ceil(S / 16384) up to 32 partials per (group, chunk), double2 for the
    statistics pass or float2 plus one float2 per group for the backward, whichever is larger."""
    from mis_hip import lib
    L = lib.load()
    for S, P in ((4, 1), (1024, 1), (4100, 1), (16384, 1), (16388, 2), (49156, 4), (524292, 32), (40 * 16384, 32)):
        for N, C, per_sample in ((1, 2, 1), (3, 5, 0), (3, 5, 1)):
            G = N * C if per_sample else C
            parts = N * C * P
            assert L.mis_norm_workspace_bytes(N, C, S, per_sample) == max(parts * 16, (parts + G) * 8), (S, P, N, C)


@pytest.mark.parametrize("name", no.names("geometry"))
def test_split_geometry(name):
    """S = 4 .. 524292: pick_P = 1, 2 (ragged: 2049 + 2048 units), 4 and the cap of 32; BatchNorm, InstanceNorm (with the
    per-channel affine at C = 5: gn_bwd_group / gn_bwd_affine at cg = 1) and GroupNorm (cg = 2); dropout mask at N = 3."""
    _run("geometry", name, "dense")


@pytest.mark.parametrize("name", no.names("scalar"))
def test_scalar_path(name):
    """S % 4 != 0 (S = 1001: four rounds of the 256 threads per InstanceNorm group), x / y / da / dx batch-strided."""
    _run("scalar", name, "slice")


@pytest.mark.parametrize("name", no.names("conditioning"))
def test_conditioning(name):
    """mean / std of every group 0, 4 or 32, plus a constant channel (variance exactly 0), gamma < 0, and gamma = 0 with
    beta != 0: HIP statistics through HIP apply under the plain rule."""
    _run("conditioning", name, "dense")


@pytest.mark.parametrize("name", no.names("strides"))
def test_every_operand_a_channel_slice(name):
    """mis_norm_stats / group statistics, mis_norm_act_fwd_g and mis_norm_act_bwd_g with x, y, da, dx as slices (x_bs != C*S,
    16-byte aligned offsets) and a contiguous explicit dropout mask; the result equals the dense call bit for bit."""
    ops = _ops()
    c, xv, dav, mean, rstd, gamma, beta, mask, dg, db = _run("strides", name, "slice")
    per_sample = c["kind"] != "bn"
    shape = tuple(c["x"].shape)
    assert xv.stride(0) != shape[1] * xv[0, 0].numel() and xv.data_ptr() % 16 == 0
    y1, y2 = _out(shape, "slice"), _out(shape, "dense")
    for xin, y in ((xv, y1), (c["x"].cuda(), y2)):
        ops.norm_act_fwd(xin, y.v, per_sample, mean, rstd, gamma, beta, c["slope"], drop_p=c["drop_p"], drop_mask=mask,
                         cg=c["cg"])
    assert torch.equal(y1.v, y2.v)
    d2 = _out(shape, "dense")
    dg2, db2 = (None, None) if gamma is None else (kit.nan(shape[1]), kit.nan(shape[1]))
    ops.norm_act_bwd(c["x"].cuda(), c["da"].cuda(), d2.v, per_sample, mean, rstd, gamma, beta, c["slope"], drop_p=c["drop_p"],
                     drop_mask=mask, dgamma=dg2, dbeta=db2, cg=c["cg"])
    d1 = _out(shape, "slice")
    ops.norm_act_bwd(xv, dav, d1.v, per_sample, mean, rstd, gamma, beta, c["slope"], drop_p=c["drop_p"], drop_mask=mask,
                     dgamma=dg, dbeta=db, cg=c["cg"])
    assert torch.equal(d1.v, d2.v) and d1.untouched()
    if gamma is not None:
        assert torch.equal(dg, dg2) and torch.equal(db, db2)


@pytest.mark.parametrize("name", no.names("bookkeeping"))
def test_batchnorm_bookkeeping(name):
    """Momentum 0.1 / 0.3 on non-trivial running buffers (compared in _hip_stats, with the counter 41 -> 42), and
    accumulate_affine: dgamma / dbeta are added to what the buffers hold."""
    ops = _ops()
    c, xv, dav, mean, rstd, gamma, beta, mask, dg, db = _run("bookkeeping", name, "dense")
    C = c["x"].shape[1]
    g0, b0 = torch.linspace(-3.0, 5.0, C, device="cuda"), torch.linspace(7.0, -2.0, C, device="cuda")
    ag, ab = g0.clone(), b0.clone()
    dx = _out(tuple(c["x"].shape), "dense")
    ops.norm_act_bwd(xv, dav, dx.v, False, mean, rstd, gamma, beta, c["slope"], dgamma=ag, dbeta=ab, accumulate_affine=True)
    assert torch.equal(ag, g0 + dg) and torch.equal(ab, b0 + db)
    assert not torch.equal(ag, dg)


@pytest.mark.parametrize("name", no.names("residual"))
def test_residual_forms(name):
    """mis_norm_res_act_fwd / bwd, y = act(norm(x) + r) and y = act(norm(x)) + r, at S = 16388 (two ragged splits), every
    operand a slice; dr written, then accumulated (in _run)."""
    _run("residual", name, "slice")


@pytest.mark.parametrize("name", no.names("pool"))
def test_fused_pool(name):
    """mis_norm_act_fwd_pool (y, pooled, argmax codes) and mis_norm_act_bwd_pool (da + the pool's scatter of dpool through
    the oracle's codes) against the oracle; y, pooled, da, dpool, dx as slices; 2-D and 3-D; a second block with one live
    thread (514 rows); with and without the explicit mask."""
    _run("pool", name, "slice")


@pytest.mark.parametrize("name", no.names("sums"))
def test_backward_sums(name):
    """mis_norm_act_bwd_sums: the group means (sum dz / E, sum dz * xhat / E), with dgamma / dbeta for BatchNorm."""
    ops = _ops()
    c = no.case(name)
    chk = _Check("sums", name)
    N, C = c["x"].shape[:2]
    per_sample = c["kind"] == "in"
    xv, dav = _in(c["x"], "slice"), _in(c["da"], "slice")
    mean, rstd = _hip_stats(c, xv)
    G = N * C if per_sample else C
    sums = torch.full((G, 2), NAN, device="cuda")
    gamma = None if per_sample else c["gamma"].cuda()
    beta = None if per_sample else c["beta"].cuda()
    dg, db = (None, None) if per_sample else (kit.nan(C), kit.nan(C))
    ops.norm_act_bwd_sums(xv, dav, per_sample, mean, rstd, gamma, beta, c["slope"], sums, dgamma=dg, dbeta=db)
    chk("s1", sums[:, 0])
    chk("s2", sums[:, 1])
    if dg is not None:
        chk("dgamma", dg)
        chk("dbeta", db)
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# mis_norm_stats_finalize: fp32 per-tile partials from the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", no.names("finalize"))
def test_stats_finalize(name):
    """np = tiles (per sample) or N * tiles (batch) partials per group around the 64 / 256-thread switch (np > 256) and at
    every remainder of the 4x unrolled loop; running statistics included.  rstd and running_var carry the conditioning
    factor 1 + mean^2 / (var + eps) per group (see the module docstring); it is 1 on the centred cases."""
    ops = _ops()
    c = no.case(name)
    chk = _Check("finalize", name)
    r64 = chk.r64
    N, C, D, H, W = c["x"].shape
    T = no.SPECS[name]["tiles"]
    per_sample = c["kind"] == "in"
    part = no.tile_partials(c["x"], T, per_sample).cuda()
    G = N * C if per_sample else C
    mean, rstd = kit.nan(G), kit.nan(G)
    factor = no.finalize_factor(r64["mean"], r64["var"])
    if c["ratio"] == 0 and no.group_elems(c["x"].shape, c["kind"]) >= 2000:     # (a group of 8 .. 520 values has a sample mean)
        assert factor.max().item() < 1.01
    if per_sample:
        ops.norm_stats_finalize(part, N, C, D * H * W, T, True, 1e-5, mean, rstd)
    else:
        rm, rv = c["rm"].cuda(), c["rv"].cuda()
        nbt = torch.tensor([7], dtype=torch.int64, device="cuda")
        ops.norm_stats_finalize(part, N, C, D * H * W, T, False, 1e-5, mean, rstd, rm, rv, nbt, momentum=c["momentum"])
        assert nbt.item() == 8
        chk("run_mean", rm)
        chk("run_var", rv, factor=factor)
    chk("mean", mean)
    chk("rstd", rstd, factor=factor)
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# mis_channel_sum, mis_norm_stats_from_running
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S", no.CHANNEL_SUM_CASES)
def test_channel_sum(N, S):
    """The conv-bias gradient: one unit and two ragged splits, N = 1 / 3, a batch-strided operand, plain and accumulating."""
    ops = _ops()
    x = no.channel_sum_input(N, S)
    ref, r32 = no.channel_sum(x, torch.float64), no.channel_sum(x, torch.float32)
    chk = _Check("channel_sum", f"csum-N{N}-S{S}")
    xv = _in(x, "slice")
    out = kit.nan(x.shape[1])
    ops.channel_sum(xv, out)
    chk("csum", out, ref, no.rel(r32, ref))
    dense = kit.nan(x.shape[1])
    ops.channel_sum(x.cuda(), dense)
    assert torch.equal(out, dense)
    acc0 = torch.linspace(-40.0, 90.0, x.shape[1], device="cuda")
    acc = acc0.clone()
    ops.channel_sum(xv, acc, accumulate=True)
    assert torch.equal(acc, acc0 + out) and not torch.equal(acc, out)
    chk.done()


@pytest.mark.parametrize("C", no.RUNNING_CASES)
def test_stats_from_running(C):
    """Eval-mode BatchNorm: mean = running_mean bit for bit, rstd = 1 / sqrt(running_var + eps); C around one 256-thread block."""
    ops = _ops()
    rm, rv = no.running_input(C)
    ref, r32 = no.from_running(rv, torch.float64), no.from_running(rv, torch.float32)
    buf = torch.full((2, C + 3), SENT, device="cuda")
    mean, rstd = buf[0, :C], buf[1, :C]
    mean.fill_(NAN), rstd.fill_(NAN)
    ops.norm_stats_from_running(rm.cuda(), rv.cuda(), 1e-5, mean, rstd)
    assert torch.equal(mean.cpu(), rm) and (buf[:, C:] == SENT).all()
    chk = _Check("from_running", f"running-C{C}")
    chk("rstd", rstd, ref, no.rel(r32, ref))
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: the documented status, nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def _operands(shape, misaligned=False):
    N, C, D, H, W = shape
    n = N * C * D * H * W
    if misaligned:
        x = torch.full((n + 4,), 0.5, device="cuda")[1:1 + n].view(shape)
        assert x.data_ptr() % 16 == 4
    else:
        x = torch.full(shape, 0.5, device="cuda")
    outs = [torch.full(shape, NAN, device="cuda") for _ in range(2)]
    stat = [kit.nan(N * C) for _ in range(4)]
    return x, outs, stat


def _all_nan(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in ts)


@pytest.mark.parametrize("what", ["dropout", "cg", "pool"])
def test_scalar_path_refuses_dropout_groupnorm_and_pool_gradient(what):
    ops = _ops()
    shape = (2, 4, 1, 3, 3) if what != "pool" else (2, 4, 1, 2, 3)
    x, (y, dx), (mean, rstd, dg, db) = _operands(shape)
    mean.fill_(0.0), rstd.fill_(1.0)
    mask = torch.ones(shape, device="cuda")
    da = torch.ones(shape, device="cuda")
    with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
        if what == "dropout":
            ops.norm_act_fwd(x, y, True, mean, rstd, None, None, 0.0, drop_p=0.3, drop_mask=mask)
        elif what == "cg":
            ops.norm_act_fwd(x, y, True, mean, rstd, None, None, 0.0, cg=2)
        else:
            dpool = torch.ones((2, 4, 1, 1, 1), device="cuda")
            idx = torch.zeros(dpool.numel(), dtype=torch.uint8, device="cuda")
            ops.norm_act_bwd_pool(x, da, dpool, idx, dx, True, mean, rstd, None, None, 0.0)
    if what != "pool":
        with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
            ops.norm_act_bwd(x, da, dx, True, mean, rstd, None, None, 0.0, **(dict(drop_p=0.3, drop_mask=mask)
                                                                               if what == "dropout" else dict(cg=2)))
    assert _all_nan(y, dx)


def test_vector_path_refuses_a_misaligned_x():
    ops = _ops()
    shape = (2, 3, 1, 4, 8)
    x, (y, dx), (mean, rstd, dg, db) = _operands(shape, misaligned=True)
    da = torch.ones(shape, device="cuda")
    calls = [lambda: ops.norm_stats(x, True, 1e-5, mean, rstd),
             lambda: ops.norm_act_fwd(x, y, True, mean, rstd, None, None, 0.0),
             lambda: ops.norm_act_bwd(x, da, dx, True, mean, rstd, None, None, 0.0),
             lambda: ops.channel_sum(x, dg[:3]),
             lambda: ops.norm_act_bwd_sums(x, da, True, mean, rstd, None, None, 0.0, torch.full((6, 2), NAN, device="cuda"))]
    for call in calls:
        with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
            call()
    assert _all_nan(y, dx, mean, rstd, dg)


@pytest.mark.parametrize("shape", [(2, 3, 1, 4, 8), (2, 3, 1, 3, 3)])
def test_batch_stride_below_one_image_and_short_workspace(shape):
    """x_bs < C*S is MIS_ERR_ARG on both paths; a workspace one byte short of mis_norm_workspace_bytes is
    MIS_ERR_WORKSPACE (the wrappers of mis_hip.ops cannot express either: straight through the C ABI)."""
    from mis_hip import lib
    L = lib.load()
    N, C, D, H, W = shape
    S = D * H * W
    x, (y, dx), (mean, rstd, dg, db) = _operands(shape)
    da = torch.ones(shape, device="cuda")
    sums = torch.full((N * C, 2), NAN, device="cuda")
    nb = L.mis_norm_workspace_bytes(N, C, S, 1)
    assert nb >= (N * C * 2) * 8
    ws = torch.full((nb // 4 + 4,), NAN, device="cuda")
    p, sp = lib.ptr, lib.stream_ptr()
    short = (C * S - 4) if S % 4 == 0 else (C * S - 1)
    ARG, WORKSPACE = -1, -4
    assert L.mis_norm_stats(p(x), short, N, C, S, 1, 1e-5, p(mean), p(rstd), None, None, None, 0.1, p(ws), nb, sp) == ARG
    assert L.mis_norm_act_fwd_g(p(x), short, p(y), C * S, N, C, S, 1, 1, p(mean), p(rstd), None, None, 0.0, 0.0, 0, None,
                                None, sp) == ARG
    assert L.mis_norm_act_bwd_g(p(x), short, p(da), C * S, p(dx), C * S, N, C, S, 1, 1, 0, p(mean), p(rstd), None, None, 0.0,
                                0.0, 0, None, None, None, None, 0, p(ws), nb, sp) == ARG
    if S % 4 == 0:
        assert L.mis_channel_sum(p(x), short, N, C, S, p(dg), 0, p(ws), nb, sp) == ARG
        assert L.mis_norm_stats(p(x), C * S, N, C, S, 1, 1e-5, p(mean), p(rstd), None, None, None, 0.1, p(ws), nb - 1,
                                sp) == WORKSPACE
        mean.fill_(0.0), rstd.fill_(1.0)
        assert L.mis_norm_act_bwd_g(p(x), C * S, p(da), C * S, p(dx), C * S, N, C, S, 1, 1, 0, p(mean), p(rstd), None, None,
                                    0.0, 0.0, 0, None, None, None, None, 0, p(ws), nb - 1, sp) == WORKSPACE
        assert L.mis_norm_act_bwd_sums(p(x), C * S, p(da), C * S, N, C, S, 1, p(mean), p(rstd), None, None, 0.0, p(sums),
                                       None, None, 0, p(ws), nb - 1, sp) == WORKSPACE
        nb0 = L.mis_norm_workspace_bytes(N, C, S, 0)
        assert L.mis_channel_sum(p(x), C * S, N, C, S, p(dg), 0, p(ws), nb0 - 1, sp) == WORKSPACE
        assert L.mis_norm_res_act_bwd(p(x), C * S, p(da), C * S, p(da), C * S, p(dx), C * S, p(y), C * S, 0, N, C, S, 1,
                                      p(mean), p(rstd), None, None, 0.0, None, None, 0, 0, p(ws), nb - 1, sp) == WORKSPACE
        mean.fill_(NAN), rstd.fill_(NAN)
    assert _all_nan(y, dx, mean, rstd, dg, sums, ws)
