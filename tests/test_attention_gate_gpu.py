"""The grid attention gate and integer up-sampling kernels (csrc/attention_gate.hip, include/mis_hip_attention_gate.h) on the
device, every entry point against the float64 oracle (tests/attention_unet_oracle.py) under the rule of
tests/test_norm_edges_gpu.py:

    |hip - f64|max <= max(K * e32, FLOOR[kind]) * |f64|max      per output tensor, K = 6

e32 = torch's own fp32 CPU operators on the same case against float64 (attention_gate_cases.py computes it with the case);
FLOOR = the largest e32 of the whole matrix for that kind of quantity (tests/test_attention_unet_cpu.py recomputes the five).
Outputs are pre-filled with NaN and must come back finite.  In the ``slice`` layout every 5-D operand is a channel slice of a
wider buffer: NaN around the inputs, a sentinel around the outputs that must survive.  The inputs keep every theta + phi 1/64
from the ReLU kink (the sums are exact in fp32) and the psi pre-activations within +-8 (attention_gate_cases.map_case asserts
both).  An accumulating call stores fl(base + gradient): it is held to the same bound on the gradient plus one fp32 rounding
of the stored sum, |hip - (base + f64)|max <= tolerance * |f64|max + 2^-24 * |base + f64|max (``base`` is seeded with the
case and exact in fp32).  Every backward runs twice and must return the same bits.

Measured on an MI355X (this file's own run; `MIS_ATTN_GATE_STATS=<file>` writes every figure as JSON):

    entry points             output    kind  e32 (fp32 torch vs f64)  HIP (max)  worst HIP / tolerance (case; "floor": K * e32 < FLOOR there)
    mis_attn_gate_map_*      att       att   3.84e-08 .. 1.42e-07     1.42e-07   0.19 (map-Ci4-24x24x24-dense)
                             df        dx    4.59e-08 .. 2.10e-07     2.10e-07   0.17 (map-Ci1-3x5x7-dense)
                             dpsi_w    sum   2.37e-08 .. 4.04e-07     4.65e-07   0.25 (map-Ci1-3x5x7-dense)
                             dpsi_b    sum   2.01e-08 .. 7.97e-07     3.72e-07   0.26 (map-Ci32-2x1x3-dense)
                             dphi_b    sum   4.59e-08 .. 3.25e-07     2.45e-07   0.17 (map-Ci1-3x5x7-dense, floor)
                             dpsi_w+ / dpsi_b+ / dphi_b+ (accumulating)          0.23 / 0.21 / 0.09
    mis_attn_gate_apply_*    y         act   4.23e-08 .. 1.36e-07     1.36e-07   0.17 (apply-C1-1x1x1-dense)
                             dx        dx    5.29e-08 .. 1.12e-07     8.84e-08   0.17 (apply-C5-2x1x3-dense)
                             datt      dx    3.04e-08 .. 3.03e-07     1.59e-07   0.42 (apply-C32-1x1x1-dense, floor)
                             dx+ (accumulating)                                  0.07
    mis_upsample_int_*       up        act   4.54e-09 .. 1.58e-07     1.19e-07   0.23 (up4-K4-4x2x6)
                             upT       upT   9.92e-08 .. 2.46e-06     1.62e-07   0.05 (up2-K2-2x1x3, floor)
                             upT+ (accumulating)                                 0.02

e32 here is from the GPU machine's run of the CPU operators (32 threads); FLOOR is from one thread (the CPU test).  The adjoint's
e32 is torch's scatter order over up to 16^3 outputs per cell; the kernel's wave tree stays at 1.6e-7.  510 figures, 63 tests.
"""
import functools

import pytest
import torch

import attention_gate_cases as ac
import oracle_kit as kit
from oracle_kit import NAN, SENT

pytestmark = pytest.mark.gpu

K = 6.0
FLOOR = {"att": 1.5e-7,       # largest e32 of the attention maps: 1.42e-7 (map-Ci128-2x1x3)
         "act": 1.6e-7,       # of y / the up-sampled tensors: 1.58e-7 (up8-K4-1x1x1)
         "dx": 3.1e-7,        # of dx / datt / df: 3.03e-7 (datt of apply-C5-1x1x1)
         "sum": 7.8e-7,       # of dpsi_w / dpsi_b / dphi_b: 7.74e-7 (dpsi_w of map-Ci1-3x5x7)
         "upT": 2.5e-6}       # of the up-sampling adjoint: 2.46e-6 (up8-K2-4x2x6)
LEAD, TRAIL = 1, 2            # channels of the wider buffer before / after a slice
_out = functools.partial(kit.Out, lead=LEAD, trail=TRAIL)
STATS = []
LAYOUTS = ("dense", "slice")


def _ops():
    from mis_hip import ops
    return ops


def _in(t, layout):
    """the fp32 device copy of an input; ``slice``: the 5-D tensors inside a wider buffer of NaN"""
    return kit.place(t.float().contiguous(), layout if t.dim() == 5 else "dense", LEAD, TRAIL)


def _check(label, out, hip, ref, e32, base=None):
    """``base``: what an accumulating call found in the output (float64 of the fp32 values)"""
    hip = hip.detach().cpu().double()
    assert tuple(hip.shape) == tuple(ref.shape), (label, out, hip.shape, ref.shape)
    gate = kit.Gate(K, FLOOR)
    gate.finite(hip, (label, out))
    kind = ac.KIND_OF[out.split("+")[0]]
    if base is None:
        err = float((hip - ref).abs().max() / ref.abs().max())
    else:
        rounding = 2.0 ** -24 * float((base + ref).abs().max())
        err = max(float((hip - (base + ref)).abs().max()) - rounding, 0.0) / float(ref.abs().max())
    tol = gate.judge(label, out, kind, "max", e32, err)
    STATS.append(dict(case=label, out=out, kind=kind, e32=e32, hip=err, tol=tol, floor=K * e32 < FLOOR[kind]))
    print(f"[attention gate] {label:28s} {out:10s} e32 {e32:.2e}  hip {err:.2e}  hip / tolerance {err / tol:.2f}")
    gate.done(label)


@pytest.fixture(scope="module", autouse=True)
def _stats_file():
    yield
    kit.report(STATS, "MIS_ATTN_GATE_STATS")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ci,grid", ac.MAP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"Ci{v}")
def test_gate_map_forward_and_backward(ci, grid, layout):
    ops, c = _ops(), ac.map_case(ci, grid)
    label = f"map-Ci{ci}-{'x'.join(map(str, grid))}-{layout}"
    i = c["in"]
    theta, phi = _in(i["theta"], layout), _in(i["phi"], layout)
    psi_w, psi_b = i["psi_w"].float().cuda(), i["psi_b"].float().cuda()
    abuf = _out(c["att"].shape, layout)
    att = abuf.v
    ops.attn_gate_map_fwd(theta, phi, psi_w, psi_b, att)
    _check(label, "att", att, c["att"], c["e32"]["att"])
    assert abuf.untouched(), "sentinel overwritten"
    # backward from the oracle's maps (rounded to fp32), so that the two directions are judged separately
    datt, att_in = _in(i["datt"], layout), _in(c["att"], layout)
    runs = []
    for accumulate in (False, True, False):
        base_w, base_b, base_p = (i[k].float().double() for k in ("dw0", "db0", "dp0"))
        fbuf = _out(c["df"].shape, layout)
        df = fbuf.v
        dw = base_w.float().cuda() if accumulate else torch.full((ac.G, ci), NAN, device="cuda")
        db = base_b.float().cuda() if accumulate else torch.full((ac.G,), NAN, device="cuda")
        dp = base_p.float().cuda() if accumulate else torch.full((ac.G * ci,), NAN, device="cuda")
        ops.attn_gate_map_bwd(datt, att_in, theta, phi, psi_w, df, dw, db, dp, accumulate=accumulate)
        torch.cuda.synchronize()
        assert fbuf.untouched(), "sentinel overwritten"
        if accumulate:
            _check(label, "dpsi_w+", dw, c["dpsi_w"], c["e32"]["dpsi_w"], base_w)
            _check(label, "dpsi_b+", db, c["dpsi_b"], c["e32"]["dpsi_b"], base_b)
            _check(label, "dphi_b+", dp, c["dphi_b"], c["e32"]["dphi_b"], base_p)
        else:
            _check(label, "df", df, c["df"], c["e32"]["df"])
            _check(label, "dpsi_w", dw, c["dpsi_w"], c["e32"]["dpsi_w"])
            _check(label, "dpsi_b", db, c["dpsi_b"], c["e32"]["dpsi_b"])
            _check(label, "dphi_b", dp, c["dphi_b"], c["e32"]["dphi_b"])
            # the ReLU mask is exact: theta + phi is exact in fp32 and never zero
            assert torch.equal(df.cpu() != 0, c["df"] != 0)
            runs.append((df.clone(), dw.clone(), db.clone(), dp.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), label


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ch,grid", ac.APPLY_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"C{v}")
def test_gate_apply_forward_and_backward(ch, grid, layout):
    ops, c = _ops(), ac.apply_case(ch, grid)
    label = f"apply-C{ch}-{'x'.join(map(str, grid))}-{layout}"
    i = c["in"]
    x, att = _in(i["x"], layout), _in(i["att"], layout)
    ybuf = _out(c["y"].shape, layout)
    y = ybuf.v
    ops.attn_gate_apply_fwd(x, att, y)
    _check(label, "y", y, c["y"], c["e32"]["y"])
    assert ybuf.untouched(), "sentinel overwritten"
    dy = _in(i["dy"], layout)
    runs = []
    for accumulate in (False, True, False):
        xbuf = _out(c["dx"].shape, layout, fill=i["dx0"] if accumulate else None)
        dx = xbuf.v
        abuf = _out(c["datt"].shape, layout)
        datt = abuf.v
        ops.attn_gate_apply_bwd(dy, x, att, dx, datt, accumulate=accumulate)
        torch.cuda.synchronize()
        assert xbuf.untouched(), "sentinel overwritten"
        assert abuf.untouched(), "sentinel overwritten"
        if accumulate:
            _check(label, "dx+", dx, c["dx"], c["e32"]["dx"], i["dx0"].float().double())
        else:
            _check(label, "dx", dx, c["dx"], c["e32"]["dx"])
            runs.append((dx.clone(), datt.clone()))
        _check(label, "datt", datt, c["datt"], c["e32"]["datt"])
    for a, b in zip(*runs):
        assert torch.equal(a, b), label


@pytest.mark.parametrize("s,k,grid", ac.UP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_upsample_int_into_a_slice_and_its_adjoint(s, k, grid):
    """The output goes into channels K .. 2K of a [N, 4K] buffer (the deep-supervision layout); the rest must keep the sentinel."""
    ops, c = _ops(), ac.up_case(s, k, grid)
    label = f"up{s}-K{k}-{'x'.join(map(str, grid))}"
    i = c["in"]
    x = i["x"].float().cuda()
    wide = torch.full((ac.N, 4 * k) + tuple(c["up"].shape[2:]), SENT, device="cuda")
    y = wide[:, k:2 * k]
    y.fill_(NAN)
    ops.upsample_int_fwd(x, y, s)
    _check(label, "up", y, c["up"], c["e32"]["up"])
    assert bool((wide[:, :k] == SENT).all()) and bool((wide[:, 2 * k:] == SENT).all())
    gwide = torch.full_like(wide, NAN)
    gwide[:, k:2 * k] = i["dy"].float().cuda()
    dy = gwide[:, k:2 * k]
    runs = []
    for accumulate in (False, True, False):
        dx = i["dx0"].float().cuda() if accumulate else torch.full(tuple(x.shape), NAN, device="cuda")
        ops.upsample_int_bwd(dy, dx, s, accumulate=accumulate)
        torch.cuda.synchronize()
        if accumulate:
            _check(label, "upT+", dx, c["upT"], c["e32"]["upT"], i["dx0"].float().double())
        else:
            _check(label, "upT", dx, c["upT"], c["e32"]["upT"])
            runs.append(dx.clone())
    assert torch.equal(*runs), label


def test_refusals_return_an_error_and_leave_the_output_untouched():
    from mis_hip import lib
    ops, L = _ops(), lib.load()
    P, st = lib.ptr, lib.stream_ptr
    x = torch.randn(2, 4, 4, 4, 4, device="cuda")
    att = torch.rand(2, 2, 2, 2, 2, device="cuda")
    y = torch.full((2, 8, 4, 4, 4), NAN, device="cuda")
    dx = torch.full_like(x, NAN)
    datt = torch.full_like(att, NAN)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    S, s = 64, 8
    # fine != 2 x coarse
    assert L.mis_attn_gate_apply_fwd(P(x), 4 * S, P(att), 2 * s, P(y), 8 * S, 2, 2, 4, 4, 4, 4, 2, 2, 1, st()) == -2
    assert L.mis_attn_gate_apply_fwd(P(x), 4 * S, P(att), 2 * s, P(y), 8 * S, 2, 2, 4, 4, 4, 4, 1, 2, 2, st()) == -2
    assert L.mis_attn_gate_apply_bwd(P(y), 8 * S, P(x), 4 * S, P(att), 2 * s, P(dx), 4 * S, P(datt), 2 * s, P(ws), ws.numel(),
                                     2, 2, 4, 4, 4, 4, 2, 1, 2, 0, st()) == -2
    # C or Ci of 0, more gates than a launch holds, a workspace that is too small
    assert L.mis_attn_gate_apply_fwd(P(x), 4 * S, P(att), 2 * s, P(y), 8 * S, 2, 2, 0, 4, 4, 4, 2, 2, 2, st()) == -1
    assert L.mis_attn_gate_apply_fwd(P(x), 4 * S, P(att), 2 * s, P(y), 8 * S, 2, 5, 4, 4, 4, 4, 2, 2, 2, st()) == -2
    assert L.mis_attn_gate_apply_bwd(P(y), 8 * S, P(x), 4 * S, P(att), 2 * s, P(dx), 4 * S, P(datt), 2 * s, P(ws), 16,
                                     2, 2, 4, 4, 4, 4, 2, 2, 2, 0, st()) == -4
    theta = torch.randn(2, 8, 2, 2, 2, device="cuda")
    psi_w, psi_b = torch.randn(2, 4, device="cuda"), torch.randn(2, device="cuda")
    a_out = torch.full((2, 2, 2, 2, 2), NAN, device="cuda")
    df, dw, db = torch.full_like(theta, NAN), torch.full_like(psi_w, NAN), torch.full_like(psi_b, NAN)
    assert L.mis_attn_gate_map_fwd(P(theta), 8 * s, P(theta), 8 * s, P(psi_w), P(psi_b), P(a_out), 2 * s, 2, 2, 0, 2, 2, 2, st()) == -1
    assert L.mis_attn_gate_map_bwd(P(att), 2 * s, P(att), 2 * s, P(theta), 8 * s, P(theta), 8 * s, P(psi_w), P(df), 8 * s, P(dw),
                                   P(db), None, P(ws), ws.numel(), 2, 2, 0, 2, 2, 2, 0, st()) == -1
    # a batch stride below the operand's size
    assert L.mis_attn_gate_map_fwd(P(theta), 8 * s - 1, P(theta), 8 * s, P(psi_w), P(psi_b), P(a_out), 2 * s, 2, 2, 4, 2, 2, 2,
                                   st()) == -1
    # mismatched G: the maps say 2 gates, the gated tensor / the psi parameters another number
    with pytest.raises(RuntimeError, match="MIS_ERR_ARG"):
        ops.attn_gate_apply_fwd(x, att, torch.full((2, 12, 4, 4, 4), NAN, device="cuda"))
    with pytest.raises(RuntimeError, match="MIS_ERR_ARG"):
        ops.attn_gate_apply_bwd(torch.randn(2, 12, 4, 4, 4, device="cuda"), x, att, dx, datt)
    with pytest.raises(RuntimeError, match="MIS_ERR_ARG"):
        ops.attn_gate_map_fwd(theta, theta, torch.randn(4, 2, device="cuda"), torch.randn(4, device="cuda"), a_out)
    # a scale outside {2, 4, 8}
    c = torch.randn(2, 2, 2, 2, 2, device="cuda")
    for sc in (1, 3, 16):
        up = torch.full((2, 2, 2 * sc, 2 * sc, 2 * sc), NAN, device="cuda")
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            ops.upsample_int_fwd(c, up, sc)
        dc = torch.full_like(c, NAN)
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            ops.upsample_int_bwd(torch.randn_like(up), dc, sc)
        assert bool(torch.isnan(up).all()) and bool(torch.isnan(dc).all())
    torch.cuda.synchronize()
    for t in (y, dx, datt, a_out, df, dw, db):
        assert bool(torch.isnan(t).all())
